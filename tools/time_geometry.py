"""What the geometry of a frame costs: diner_amd.render.predict_geometry against predict_image(return_alpha=True) on the seeded
synthetic scene, and the two kernels of geometry.hip on their own.

    python tools/time_geometry.py [--size 800x600] [--samples 128] [--rounds 3] [--views 4]

Scene: seed 0, four source views, --size, K = --samples (n_gaussian = 3 K / 8), 1000 candidates, in-kernel noise, white background.  One
warm-up frame each way, then predict_image and predict_geometry frames alternating over --rounds rounds: HIP events around the whole
call (ray generation, host enqueue, the map assembly and depth2normal inside).  Then the two kernels alone, through the C entries on
preallocated outputs: diner_ray_geometry_f32 on a frame's worth of weights (size x K) as ONE launch and as the frame runs it (one
launch per 8192 rays, HIP events around the whole series: with launch gaps), and diner_depth_consistency_f32 on --views z-depth maps
of --size; each the median of 20 timed calls after 3 warm-up calls.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="800x600")
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--views", type=int, default=4)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import ops
    from diner_amd.render import predict_geometry, predict_image
    from diner_amd.synthetic import make_scene, make_mlp_state_dict, build_modules
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    K = args.samples
    G = 3 * K // 8
    sc = make_scene(W, H, seed=0)
    normals = ops.depth2normal(sc["depths"].to(dev), sc["src_intrinsics"].to(dev))
    nerf, R = build_modules(sc, make_mlp_state_dict(), dev, normals=normals)
    ren = R(n_samples=K, n_depth_candidates=1000, n_gaussian=G, white_bkgd=True)
    tE, tK = sc["target_extrinsics"][None].to(dev), sc["target_intrinsics"][None].to(dev)

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        out = fn()
        ev1.record()
        torch.cuda.synchronize()
        return round(ev0.elapsed_time(ev1), 3), out

    def image(seed):
        return timed(lambda: predict_image(nerf, ren, tE, tK, W, H, sc["znear"], sc["zfar"], seed=seed, return_alpha=True))

    def geometry(seed):
        return timed(lambda: predict_geometry(nerf, ren, tE, tK, W, H, sc["znear"], sc["zfar"], seed=seed))

    (_, img), (_, geo) = image(7), geometry(7)
    assert torch.equal(img[0], geo["rgb"]) and torch.equal(img[1], geo["depth"]) and torch.equal(img[2], geo["alpha"])
    image_ms, geometry_ms = [], []
    for r in range(args.rounds):
        image_ms.append(image(100 + r)[0])
        geometry_ms.append(geometry(100 + r)[0])

    def median_ms(fn, warm=3, n=20):
        for _ in range(warm):
            fn()
        return round(statistics.median(timed(fn)[0] for _ in range(n)), 4)

    # the kernels alone: the C entries on preallocated outputs, no tensor allocation or host camera conversion inside the timed region
    import ctypes as C
    from diner_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=dev).manual_seed(0)
    n_rays = W * H
    w = torch.rand(n_rays, K, device=dev, generator=g) / K
    z = torch.sort(torch.rand(n_rays, K, device=dev, generator=g) + 0.5, dim=1).values
    rays = ops.gen_rays(tE, tK, W, H, sc["znear"], sc["zfar"], dev)[0]
    fwd = (C.c_float * 3)(*tE[0, 2, :3].cpu().tolist())
    o_med, o_mean, o_zd = (torch.empty(n_rays, device=dev) for _ in range(3))
    o_idx = torch.empty(n_rays, device=dev, dtype=torch.int32)
    o_pts = torch.empty(n_rays, 3, device=dev)

    def ray_launch(r0, r1):
        _lib.check(lib.diner_ray_geometry_f32(w[r0:r1].data_ptr(), z[r0:r1].data_ptr(), rays[r0:r1].data_ptr(), r1 - r0, K, 0.5, 1e-3, fwd, 0,
                                              o_med[r0:r1].data_ptr(), o_idx[r0:r1].data_ptr(), o_mean[r0:r1].data_ptr(),
                                              o_zd[r0:r1].data_ptr(), o_pts[r0:r1].data_ptr(), st))

    def ray_kernel_batches():               # as the frame runs it: one launch per 8192 rays
        for r0 in range(0, n_rays, 8192):
            ray_launch(r0, min(n_rays, r0 + 8192))

    V = args.views
    maps = geo["zdepth"][:, 0].expand(V, -1, -1).contiguous()
    Ev = tE.cpu().float().expand(V, -1, -1).contiguous()
    Kv = tK.cpu().float().expand(V, -1, -1).contiguous()
    o_cnt = torch.empty(V, H, W, device=dev, dtype=torch.int32)
    o_avg = torch.empty(V, H, W, device=dev)

    def consistency_kernel():
        _lib.check(lib.diner_depth_consistency_f32(maps.data_ptr(), Kv.data_ptr(), Ev.data_ptr(), V, H, W, 1.0, 0.01, o_cnt.data_ptr(),
                                                   o_avg.data_ptr(), st))

    res = dict(tool="time_geometry", size=args.size, K=K, G=G, n_cand=1000, valid_share=round(float(geo["valid"].float().mean()), 4),
               predict_image_alpha_ms=image_ms, predict_geometry_ms=geometry_ms,
               ray_geometry_one_launch_ms=median_ms(lambda: ray_launch(0, n_rays)),
               ray_geometry_batched_ms=median_ms(ray_kernel_batches), ray_geometry_batches=(n_rays + 8191) // 8192,
               depth_consistency_ms=median_ms(consistency_kernel), depth_consistency_views=V)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
