#!/bin/bash
# One parametrised GPU job (round 6: replaces the one-off tools/job_r0*.sh of rounds 4-5; the ones a profiles/ file cites by name are kept).
#   /usr/local/graft/bin/gpurun --timeout 2700 -- 'bash tools/job.sh <job> [args]'       (several jobs: 'bash tools/job.sh a; bash tools/job.sh b')
# Everything is written under gpurun_out/ (merged back by gpurun); copy what should be judged into profiles/.
#
#   tests [pytest args]        the -m gpu suite with --durations=0                      -> gpurun_out/tests.log
#   train-tests                tests/test_train_gpu.py                                   -> gpurun_out/train_tests.log
#   train-time [lib ...]       tools/time_train.py at SB 4 x 4096 (+ each libdiner_hip_<lib>.so, alternating twice)  -> gpurun_out/train_time.log
#   train-prof [rays] [obj]    rocprofv3 kernel trace of the training step (tools/prof_train.sh)
#   train-pmc [rays] [obj]     HBM bytes / MfmaUtil per kernel of the training step (tools/pmc_train.sh)
#   l512-prof [rows]           phase timer of lin512_body (needs libdiner_hip_l512prof.so: build_variant('l512prof', ['DINER_L512_PROF']))
#   bench [bench args]         bench.py (default --gpus 1 --steps 20 --warmup 5 --full) -> bench_line.json in the output folder + a digest on stdout
#   profile <tag> [bench args] rocprofv3 stats + PMC passes of the bench (tools/profile_round.sh)
#   objective-time [args]      tools/time_objective.py: calc_losses against the torch expression of the objective, alternating (stdout; keep it as profiles/objective_step_ab.txt)
#   many-views-time [args]     tools/time_many_views.py --both: NV = 1, 2, 3, 4, 6, 8, 16 on the view-grouped and the forced-generic route, alternating (stdout; keep it under profiles/)
#   sampler-info-time [args]   tools/time_sampler_info.py: the sampler's plain entry against its info entry, alternating, and one 800 x 600 predict_surface_prior (stdout)
#   cull-time [args]           tools/time_cull.py: an 800 x 600 K = 128 frame with and without cull_empty, alternating, at the scene's own and at half the focal length (stdout; keep it as profiles/cull_frame_ab.txt)
#   geometry-time [args]       tools/time_geometry.py: an 800 x 600 K = 128 frame through predict_geometry and through predict_image(return_alpha=True), alternating, and the two geometry kernels on their own (stdout)
#   surface-time [args]        tools/time_surface.py: a 256^3 colour volume fused from sixteen 800 x 600 views (one call / sixteen), count + extract on it, and one 800 x 600 mesh_from_sources (stdout)
#   raycast-time [args]        tools/time_raycast.py: that 256^3 volume cast back into one and into sixteen 800 x 600 cameras, with and without the brick mask, and the brick build alone (stdout)
#   cloud-time [args]          tools/time_cloud.py: grid build, nearest neighbour in input and in own-grid order and the sums on 1 M x 1 M and 7.7 M x 5 M points, one child a size, and scipy's k-d tree on the host (stdout)
#   optim-time [args]          tools/time_optim.py --loop: DeviceAdam.step against torch.optim.Adam (default and fused=True), alternating windows, and the whole fit step against the loop on torch's optimiser (stdout; keep it as profiles/optim_step_ab.txt)
#   encoder-time [args]        tools/time_encoder.py: the trunk at 4 x 800x600 and 16 x 400x300 on the torch / MIOpen route and the device route, alternating; peak memory, the first call of each in a fresh process, the device route's launches one by one (stdout)
#   mvs-time [args]            tools/time_mvs.py: the matching stage's entries and the whole coarse_to_fine at the DTU stage shapes and a 256 x 320 image, kernels against the torch restatement on the device, alternating; peak memory (stdout; keep it as profiles/mvs_time_ab.txt)
#   costreg-time [args]        tools/time_costreg.py: CostRegNet on the three DTU stage volumes at base 8, kernels against the torch / MIOpen route, alternating; peak memory, the eleven launches one by one against their bounds, and the whole coarse_to_fine with the real regulariser (stdout; keep it as profiles/costreg_time_ab.txt)
#   fmt-time [args]            tools/time_fmt.py: FMT_with_pathway, the FMT alone and the pathway alone at the DTU shape (stage 1 of 128 x 160, five views), kernels against the torch route, alternating; peak memory, each launch against its bound, and coarse_to_fine with the module in front (stdout; keep it as profiles/fmt_time_ab.txt)
#   smoke                      __graft_entry__.smoke()
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}" || exit 1
mkdir -p gpurun_out
export TMPDIR=/tmp
job=$1; shift
case "$job" in
  tests)
    timeout 2400 python -m pytest tests -m gpu -q --durations=0 "$@" > gpurun_out/tests.log 2>&1; echo "rc=$?" >> gpurun_out/tests.log
    tail -60 gpurun_out/tests.log ;;
  train-tests)
    timeout 1500 python -m pytest tests/test_train_gpu.py -x -q --durations=0 "$@" > gpurun_out/train_tests.log 2>&1; echo "rc=$?" >> gpurun_out/train_tests.log
    tail -5 gpurun_out/train_tests.log ;;
  train-time)
    : > gpurun_out/train_time.log
    for rep in 1 2; do
      for lib in "" "$@"; do
        if [ -n "$lib" ]; then export DINER_AMD_LIB=$PWD/diner_amd/libdiner_hip_$lib.so; else unset DINER_AMD_LIB; fi
        echo "== lib ${lib:-default} (rep $rep)" >> gpurun_out/train_time.log
        timeout 600 python tools/time_train.py --objects 4 --rays 4096 >> gpurun_out/train_time.log 2>&1
      done
      [ $# -eq 0 ] && break
    done
    unset DINER_AMD_LIB
    grep -v amdgpu.ids gpurun_out/train_time.log ;;
  train-prof) bash tools/prof_train.sh "${1:-4096}" "${2:-4}" 2>&1 | tail -8; head -30 "gpurun_out/prof_train_${2:-4}x${1:-4096}/stats.md" ;;
  train-pmc) bash tools/pmc_train.sh "${1:-4096}" "${2:-4}" 2>&1 | tail -25 ;;
  l512-prof)
    DINER_AMD_LIB=$PWD/diner_amd/libdiner_hip_l512prof.so timeout 600 python tools/prof_l512.py "$@" > gpurun_out/prof_l512.log 2>&1
    grep -v amdgpu.ids gpurun_out/prof_l512.log ;;
  bench)
    [ $# -eq 0 ] && set -- --gpus 1 --steps 20 --warmup 5 --full
    ( time python bench.py "$@" ) > gpurun_out/bench_line.json 2> gpurun_out/bench_stderr.log; echo "rc=$?" >> gpurun_out/bench_stderr.log
    tail -5 gpurun_out/bench_stderr.log
    python - <<'PY'
import json
l = json.loads(open("gpurun_out/bench_line.json").read().strip().splitlines()[-1])
print({k: l.get(k) for k in ("value", "ms_per_step", "fallback_launches", "energy")})
print("encode", l.get("encode"))
t = l.get("train") or {}
print("train", {k: t.get(k) for k in ("ms_per_step", "forward_ms", "backward_ms", "host_enqueue_ms", "tflops_fp32_equivalent", "frac", "peak_memory_gib", "batched")})
c = l.get("cpu_baseline") or {}
print("cpu", {k: c.get(k) for k in ("value", "cores", "host_cores", "host_threads")})
print("modes", {k: (v["rays_per_s"], v["fallback_launches"], v["roofline"]["frac"]) for k, v in (l.get("modes") or {}).items()})
print("configs", {k[:28] + k[-8:]: (v["rays_per_s"], v["fallback_launches"], v["roofline"]["frac"]) for k, v in (l.get("configs") or {}).items()})
print("roofline", l["roofline"]["frac"], l["roofline"]["avg_launch_ms"])
PY
    ;;
  profile) bash tools/profile_round.sh "$@" ;;
  objective-time)
    timeout 900 python tools/time_objective.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  many-views-time)
    timeout 1100 python tools/time_many_views.py --both --nvs 1,2,3,4,6,8,16 "$@" 2>&1 | grep -v amdgpu.ids ;;
  sampler-info-time)
    timeout 300 python tools/time_sampler_info.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  cull-time)
    timeout 500 python tools/time_cull.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  geometry-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_geometry.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  surface-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_surface.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  raycast-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_raycast.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  cloud-time)
    set -o pipefail
    timeout -k 10 1500 python tools/time_cloud.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  optim-time)
    set -o pipefail
    timeout -k 10 900 python tools/time_optim.py --loop "$@" 2>&1 | grep -v amdgpu.ids ;;
  encoder-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_encoder.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  mvs-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_mvs.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  costreg-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_costreg.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  fmt-time)
    set -o pipefail
    timeout -k 10 500 python tools/time_fmt.py "$@" 2>&1 | grep -v amdgpu.ids ;;
  smoke) python __graft_entry__.py smoke ;;
  *) echo "unknown job '$job' (see the header of tools/job.sh)"; exit 2 ;;
esac
