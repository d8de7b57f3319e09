"""What empty-ray culling saves, and what it costs where nothing is empty: diner_amd.render.predict_image with and without
cull_empty on the seeded synthetic scene.

    python tools/time_cull.py [--size 800x600] [--samples 128] [--rounds 3]

Scene: seed 0, four views, --size, K = --samples (n_gaussian = 3 K / 8), 1000 candidates, in-kernel noise, white background.  Two
target focal settings: the scene's own (almost every ray meets a surface) and x 0.5 (the object fills a quarter of the frame).  Per
setting one warm-up frame each way, then plain and culled frames alternating over --rounds rounds: HIP events around the whole
predict_image call (ray generation, host enqueue, the culled path's read-back inside), then once more each way with
ops.profile_enable() for the points the field kernels processed.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="800x600")
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import ops
    from diner_amd.render import predict_image, predict_surface_prior
    from diner_amd.synthetic import make_scene, make_mlp_state_dict, build_modules
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    K = args.samples
    G = 3 * K // 8
    sc = make_scene(W, H, seed=0)
    normals = ops.depth2normal(sc["depths"].to(dev), sc["src_intrinsics"].to(dev))
    nerf, R = build_modules(sc, make_mlp_state_dict(), dev, normals=normals)
    ren = R(n_samples=K, n_depth_candidates=1000, n_gaussian=G, white_bkgd=True)
    tE = sc["target_extrinsics"][None].to(dev)

    def frame(tK, cull, seed):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        rgb, depth = predict_image(nerf, ren, tE, tK, W, H, sc["znear"], sc["zfar"], seed=seed, cull_empty=cull)
        ev1.record()
        torch.cuda.synchronize()
        assert torch.isfinite(rgb).all()
        return round(ev0.elapsed_time(ev1), 2)

    res = dict(tool="time_cull", size=args.size, K=K, G=G, n_cand=1000, settings={})
    for name, scale in (("own_focal", 1.0), ("half_focal", 0.5)):
        tK = sc["target_intrinsics"].clone()
        tK[0, 0] *= scale
        tK[1, 1] *= scale
        tK = tK[None].to(dev)
        hit = predict_surface_prior(nerf, tE, tK, W, H, sc["znear"], sc["zfar"], K, 1000, G, seed=7)[0]
        frame(tK, False, 7), frame(tK, True, 7)
        plain_ms, culled_ms = [], []
        for r in range(args.rounds):
            plain_ms.append(frame(tK, False, 100 + r))
            culled_ms.append(frame(tK, True, 100 + r))
        points = {}
        ops.profile_enable()
        try:
            for cull in (False, True):
                ops.profile_collect()
                frame(tK, cull, 7)
                points["culled" if cull else "plain"] = ops.profile_collect()["points"]
        finally:
            ops.profile_enable(False)
        res["settings"][name] = dict(live_share=round(float((hit > 0).float().mean()), 4), plain_ms=plain_ms, culled_ms=culled_ms,
                                     points=points)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
