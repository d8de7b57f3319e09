"""What the sampler's info outputs cost: the plain entry against the info entry (diner_sample_depthguided_long_f32 /
diner_sample_depthguided_info_long_f32), and one frame of diner_amd.render.predict_surface_prior.

    python tools/time_sampler_info.py [--rays 4096] [--reps 20] [--rounds 3] [--size 800x600]

Per launch of --rays rays of the seeded synthetic scene (seed 0, four views, in-kernel noise) at K = 128 / 1000 candidates (the bounded
kernels) and K = 1024 / 4096 candidates (the wide kernels), n_gaussian = 3 K / 8: HIP events around each launch, median of --reps, plain
and info alternating over --rounds rounds (the median of each round is reported).  Then one 800 x 600 predict_surface_prior at
K = 40 / 1000 candidates after one warm-up frame.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((128, 1000), (1024, 4096))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", default="800x600")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import ops
    from diner_amd.render import predict_surface_prior
    from diner_amd.synthetic import make_scene, make_mlp_state_dict, build_modules
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    sc = make_scene(W, H, seed=0)
    normals = ops.depth2normal(sc["depths"].to(dev), sc["src_intrinsics"].to(dev))
    nerf, _ = build_modules(sc, make_mlp_state_dict(), dev, normals=normals)
    tE, tK = sc["target_extrinsics"][None].to(dev), sc["target_intrinsics"][None].to(dev)
    scene = nerf.hip_scene(0)
    rays = ops.gen_rays(tE, tK, W, H, sc["znear"], sc["zfar"], dev)[0]
    rays = rays[torch.linspace(0, W * H - 1, args.rays, device=dev).long()].contiguous()

    def median_ms(fn):
        times = []
        for _ in range(args.reps):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            fn()
            ev1.record()
            torch.cuda.synchronize()
            times.append(ev0.elapsed_time(ev1))
        return sorted(times)[len(times) // 2]

    res = dict(tool="time_sampler_info", rays=args.rays, reps=args.reps, launches={})
    for K, n_cand in CONFIGS:
        G = 3 * K // 8
        plain = lambda: ops.sample_depthguided_long(scene, rays, K, n_cand, G, seed=1)
        info = lambda: ops.sample_depthguided_long(scene, rays, K, n_cand, G, seed=1, want_info=True)
        plain(), info()
        torch.cuda.synchronize()
        rounds = [(round(median_ms(plain), 4), round(median_ms(info), 4)) for _ in range(args.rounds)]
        res["launches"][f"K{K}_c{n_cand}"] = dict(plain_ms=[r[0] for r in rounds], info_ms=[r[1] for r in rounds])
    frames = []
    for i in range(2):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        hit, depth, dstd = predict_surface_prior(nerf, tE, tK, W, H, sc["znear"], sc["zfar"], seed=1000 + i)
        ev1.record()
        torch.cuda.synchronize()
        frames.append(round(ev0.elapsed_time(ev1), 3))
    assert torch.isfinite(depth).all() and (hit >= 0).all()
    res["surface_prior"] = dict(size=args.size, K=40, n_cand=1000, warmup_ms=frames[0], ms=frames[1], hit_share=round(float((hit > 0).float().mean()), 4))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
