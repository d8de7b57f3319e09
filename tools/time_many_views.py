"""Frame time of renders with 1 to 16 source views through the drop-in modules (the reference's PixelNeRF takes any number of
views, pixelnerf.py:67; here four run on the fused kernels, any other number on the same kernels over groups of four views, and
-- with --generic -- on the generic exact-fp32 path, so that both routes can be timed from one build).

    python tools/time_many_views.py [--frames 3] [--warmup 1] [--size 256] [--ray-batch 16384] [--no-prof] [--generic] [--nvs 4,6,8,16]
    python tools/time_many_views.py --both        # every view count on both routes, alternating, ratios to the four-view frame

One size x size frame of the seeded synthetic scene (make_scene(nv=NV), seed 0) at K = 128, n_candidates = 1000, n_gaussian = 48 through
PixelNeRF / NeRFRendererDGS and diner_amd.render.predict_image, with NV = 4, 6, 8 and 16 (--nvs), each in a child process of its own;
`path` of a run is fused4 (four views), grouped (view groups) or generic.  Unless
--no-prof, every child runs under `rocprofv3 --kernel-trace --stats` and its kernel time is split into the sampler, the generic inputs,
the GEMMs of the generic MLP, the fused field kernels and the rest.  Timed with device events around each frame; median of --frames frames
after --warmup.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NVS = (4, 6, 8, 16)
K, N_CAND, G = 128, 1000, 48
GROUPS = (("sampler", ("k_sample_depthguided",)), ("inputs", ("k_generic_inputs",)), ("gemm", ("k_gemm",)),
          ("fused", ("k_field_pre", "k_field_post", "k_field_views")))


def child(args):
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import ops
    from diner_amd.render import predict_image
    from diner_amd.synthetic import make_scene, make_mlp_state_dict, build_modules
    dev = torch.device("cuda", 0)
    W = H = args.size
    sc = make_scene(W, H, nv=args.nv, seed=0)
    normals = ops.depth2normal(sc["depths"].to(dev), sc["src_intrinsics"].to(dev))
    nerf, R = build_modules(sc, make_mlp_state_dict(), dev, normals=normals)
    tE, tK = sc["target_extrinsics"][None].to(dev), sc["target_intrinsics"][None].to(dev)
    ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=False)
    times = []
    with torch.no_grad():
        for i in range(args.warmup + args.frames):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            rgb, depth = predict_image(nerf, ren, tE, tK, W, H, sc["znear"], sc["zfar"], ray_batch_size=args.ray_batch, seed=1000 + i)
            ev1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(ev0.elapsed_time(ev1))
            assert torch.isfinite(rgb).all() and torch.isfinite(depth).all()
    ms = sorted(times)[len(times) // 2]
    path = "fused4" if not nerf.is_generic() else ("grouped" if nerf.is_view_grouped() else "generic")
    assert (path == "generic") == isinstance(nerf.hip_mlp(), ops.GenericMlp)
    print(json.dumps(dict(nv=args.nv, path=path, ms=round(ms, 2), frames=sorted(times),
                          rays_per_s=round(W * H / (ms * 1e-3)))), flush=True)


def split(stats_csv, frames_total):
    """kernel ms per frame by group, from a rocprofv3 kernel_stats.csv (every frame of the run, warm-up included)."""
    out = {name: 0.0 for name, _ in GROUPS}
    out["other"] = 0.0
    for r in csv.DictReader(open(stats_csv)):
        ms = float(r["TotalDurationNs"]) * 1e-6 / frames_total
        for name, keys in GROUPS:
            if any(k in r["Name"] for k in keys):
                out[name] += ms
                break
        else:
            out["other"] += ms
    return {k: round(v, 2) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nv", type=int, default=0, help="(child) one view count")
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ray-batch", type=int, default=16384)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--timeout", type=int, default=600, help="seconds per child")
    ap.add_argument("--generic", action="store_true", help="force the generic exact-fp32 route for view counts other than four")
    ap.add_argument("--both", action="store_true", help="each view count on the view-grouped and on the forced-generic route, alternating")
    ap.add_argument("--nvs", default=",".join(str(n) for n in NVS), help="view counts, comma-separated")
    args = ap.parse_args()
    if args.generic:
        os.environ["DINER_AMD_VIEW_GROUPS"] = "0"          # PixelNeRF.is_view_grouped() (inherited by the children)
    if args.nv:
        return child(args)
    nvs = tuple(int(n) for n in args.nvs.split(","))
    if args.both:
        return both(args, nvs)
    res = dict(tool="time_many_views", size=args.size, K=K, n_cand=N_CAND, G=G, frames=args.frames, ray_batch=args.ray_batch,
               forced_generic=bool(args.generic), runs={})
    for nv in nvs:
        cmd = [sys.executable, os.path.abspath(__file__), "--nv", str(nv), "--frames", str(args.frames), "--warmup", str(args.warmup),
               "--size", str(args.size), "--ray-batch", str(args.ray_batch)]
        with tempfile.TemporaryDirectory() as tmp:
            if not args.no_prof:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", f"nv{nv}", "--"] + cmd
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"NV={nv}: child exited with {p.returncode}")
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            run = json.loads(line)
            if not args.no_prof:
                stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                if stats:
                    run["kernel_ms_per_frame"] = split(stats[0], args.frames + args.warmup)
                else:
                    sys.stderr.write(f"NV={nv}: no kernel_stats.csv under the rocprofv3 output: "
                                     f"{sorted(glob.glob(os.path.join(tmp, '**'), recursive=True))[:20]}\n{p.stderr[-1500:]}\n")
        res["runs"][f"nv{nv}"] = run
        print(f"NV={nv}: {run}", file=sys.stderr, flush=True)
    if "nv4" in res["runs"]:
        base = res["runs"]["nv4"]["ms"]
        res["ratio_vs_nv4"] = {k: round(v["ms"] / base, 2) for k, v in res["runs"].items()}
    print(json.dumps(res), flush=True)


def both(args, nvs):
    """Every view count on the view-grouped route and on the forced-generic route, one child each, alternating (no profiler): frame
    times, the ratio of the two and the ratio of either to the four-view fused frame of the same run."""
    res = dict(tool="time_many_views", mode="both", size=args.size, K=K, n_cand=N_CAND, G=G, frames=args.frames, ray_batch=args.ray_batch, runs={})
    for nv in nvs:
        for route in ("grouped", "generic"):
            if nv == 4 and route == "generic":
                continue
            env = dict(os.environ, DINER_AMD_VIEW_GROUPS="0" if route == "generic" else "1")
            cmd = [sys.executable, os.path.abspath(__file__), "--nv", str(nv), "--frames", str(args.frames), "--warmup", str(args.warmup),
                   "--size", str(args.size), "--ray-batch", str(args.ray_batch)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, env=env)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"NV={nv} {route}: child exited with {p.returncode}")
            run = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            assert run["path"] == ("fused4" if nv == 4 else route), run
            res["runs"][f"nv{nv}_{run['path']}"] = run
            print(f"NV={nv} {route}: {run}", file=sys.stderr, flush=True)
    base = res["runs"].get("nv4_fused4", {}).get("ms")
    res["table"] = {}
    for nv in nvs:
        a, b = res["runs"].get(f"nv{nv}_grouped"), res["runs"].get(f"nv{nv}_generic")
        if a and b:
            res["table"][f"nv{nv}"] = dict(grouped_ms=a["ms"], generic_ms=b["ms"], generic_over_grouped=round(b["ms"] / a["ms"], 2),
                                           grouped_over_nv4=round(a["ms"] / base, 2) if base else None,
                                           generic_over_nv4=round(b["ms"] / base, 2) if base else None)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
