"""Frame time of long-ray renders through the drop-in modules (create_prediction_folder.py --nsamples, :20, :43-47).

    python tools/time_long_rays.py [--frames 3] [--warmup 1] [--ray-batch 4096]

One 800x600 frame of the seeded synthetic scene (bench.py's, seed 0) through PixelNeRF / NeRFRendererDGS and
diner_amd.render.predict_image at (K, n_candidates) = (128, 1000), (512, 1000), (512, 4096), (1024, 4096), n_gaussian =
15 K / 40 as the reference sets it.  Timed with device events around each frame; median of --frames frames after --warmup.
Prints one JSON line: ms per frame per configuration and the ratios against K = 128."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ((128, 1000), (512, 1000), (512, 4096), (1024, 4096))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ray-batch", type=int, default=4096)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import ops
    from diner_amd.render import predict_image
    from diner_amd.synthetic import make_scene, make_mlp_state_dict, build_modules
    dev = torch.device("cuda", 0)
    W, H = args.width, args.height
    sc = make_scene(W, H, seed=0)
    normals = ops.depth2normal(sc["depths"].to(dev), sc["src_intrinsics"].to(dev))
    nerf, R = build_modules(sc, make_mlp_state_dict(), dev, normals=normals)
    tE, tK = sc["target_extrinsics"][None].to(dev), sc["target_intrinsics"][None].to(dev)
    out = dict(tool="time_long_rays", W=W, H=H, frames=args.frames, ray_batch=args.ray_batch, precision="f16x3", ms={})
    for K, n_cand in CONFIGS:
        ren = R(n_samples=40, n_depth_candidates=n_cand, n_gaussian=15, white_bkgd=False)
        ren.n_samples, ren.n_gaussian = K, int(15 * K / 40)                # create_prediction_folder.py:44-47
        times = []
        for i in range(args.warmup + args.frames):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            rgb, depth = predict_image(nerf, ren, tE, tK, W, H, sc["znear"], sc["zfar"], ray_batch_size=args.ray_batch, seed=1000 + i)
            ev1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(ev0.elapsed_time(ev1))
            assert torch.isfinite(rgb).all() and torch.isfinite(depth).all()
        out["ms"][f"K{K}_c{n_cand}"] = sorted(times)[len(times) // 2]
        print(f"K={K} n_cand={n_cand}: {sorted(times)} ms", file=sys.stderr, flush=True)
    base = out["ms"]["K128_c1000"]
    out["ratio_vs_K128"] = {k: round(v / base, 3) for k, v in out["ms"].items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
