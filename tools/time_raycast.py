"""What an image of the fused volume costs: the kernels of raycast.hip on their own.

    python tools/time_raycast.py [--dim 256] [--size 800x600] [--views 16] [--reps 20]

Scene: tools/time_surface.py's -- an analytic sphere of radius 0.25 at the origin seen by --views cameras on a tilted ring of radius 1,
fused (carving) into a --dim^3 volume with colour planes.  The volume is then cast back into the first camera and into all of them
(--size pixels each, step voxel / 2, zfar 2, every output wanted).  Through the C entries on preallocated buffers, HIP events around
each call, the median of --reps timed calls after 3 warm-up calls:
  - diner_tsdf_raycast_f32 without and with the brick mask, one view and --views views a call;
  - diner_tsdf_bricks alone.
samples_per_ray is the number of lattice samples the plain march evaluates on an average ray -- from the first lattice index inside the
box to the terminating one (or the last inside the box), counted in torch from the cameras and the kernel's own depth map, without the
few samples the kernel adds on either side for its rounding -- and taps_per_s that many samples x 16 taps (8 tsdf, 8 wsum) per second
of the plain call.  The brick mask changes which samples are looked at, not the maps: the two paths' outputs are compared bit for bit.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def samples_per_ray(E, Kmat, W, H, origin, voxel, n, step, zfar, zdepth):
    """Lattice samples from the box entry to termination per ray, averaged over the rays of every view: -> (mean, share of hits)."""
    import torch
    dev = zdepth.device
    E, Kmat = E.to(dev, torch.float64), Kmat.to(dev, torch.float64)
    x = (torch.arange(W, device=dev, dtype=torch.float64) + 0.5 - Kmat[0, 2]) / Kmat[0, 0]
    y = (torch.arange(H, device=dev, dtype=torch.float64) + 0.5 - Kmat[1, 2]) / Kmat[1, 1]
    dc = torch.stack((x.view(1, W).expand(H, W), y.view(H, 1).expand(H, W), torch.ones(H, W, device=dev, dtype=torch.float64)), dim=-1)
    dz = step / dc.norm(dim=-1)
    lo = torch.tensor(origin, device=dev, dtype=torch.float64)
    hi = lo + (n - 1) * voxel
    total = 0.0
    for v in range(E.shape[0]):
        R, t = E[v, :3, :3], E[v, :3, 3]
        eye = -R.T @ t
        dw = dc @ R
        ta, tb = (lo - eye) / dw, (hi - eye) / dw
        z_in = torch.minimum(ta, tb).amax(dim=-1).clamp(min=0.0)
        z_out = torch.maximum(ta, tb).amin(dim=-1).clamp(max=zfar)
        zd = zdepth[v].to(torch.float64)
        last = torch.where(zd > 0, zd, z_out)
        count = (torch.ceil(last / dz) - torch.ceil(z_in / dz) + 1).clamp(min=0.0)
        total += float(torch.where(z_out > z_in, count, torch.zeros_like(count)).mean())
    return total / E.shape[0], float((zdepth > 0).double().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--size", default="800x600")
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import _lib
    from time_surface import ring_cameras, sphere_maps
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    n, V = args.dim, args.views
    E, Kmat = ring_cameras(V, 1.125 * W, W, H)
    depth, color = sphere_maps(E, Kmat, W, H, 0.25, dev)
    Kv = Kmat[None].expand(V, -1, -1).contiguous()
    voxel = 0.8 / n
    o = (-0.4 + 0.013, -0.4 + 0.007, -0.4 + 0.003)
    origin = (C.c_float * 3)(*o)
    tsdf = torch.ones(n, n, n, device=dev)
    wsum = torch.zeros(n, n, n, device=dev)
    color4 = torch.zeros(4, n, n, n, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.diner_tsdf_integrate_f32(tsdf.data_ptr(), wsum.data_ptr(), color4.data_ptr(), n, n, n, origin, voxel, 3.0 * voxel,
                                            depth.data_ptr(), None, color.data_ptr(), Kv.data_ptr(), E.data_ptr(), V, H, W, 1, 0.0, st))
    del depth, color
    bricks = torch.zeros(lib.diner_tsdf_bricks_bytes(n, n, n), dtype=torch.uint8, device=dev)
    step, zfar = 0.5 * voxel, 2.0
    outs = {b: (torch.empty(V, H, W, device=dev), torch.empty(V, 3, H, W, device=dev), torch.empty(V, 3, H, W, device=dev),
                torch.empty(V, H, W, device=dev)) for b in (False, True)}

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    def median_ms(fn, warm=3):
        for _ in range(warm):
            fn()
        return round(statistics.median(timed(fn) for _ in range(args.reps)), 4)

    def build():
        _lib.check(lib.diner_tsdf_bricks(tsdf.data_ptr(), wsum.data_ptr(), n, n, n, 0.0, bricks.data_ptr(), st))

    def cast(views, use_bricks):
        z, nrm, rgb, wgt = outs[use_bricks]
        _lib.check(lib.diner_tsdf_raycast_f32(tsdf.data_ptr(), wsum.data_ptr(), color4.data_ptr(), n, n, n, origin, voxel,
                                              bricks.data_ptr() if use_bricks else None, Kv.data_ptr(), E.data_ptr(), views, H, W, 0.0, zfar,
                                              step, 0.0, z.data_ptr(), nrm.data_ptr(), rgb.data_ptr(), wgt.data_ptr(), st))

    build()
    res = dict(tool="time_raycast", dim=n, size=args.size, views=V, reps=args.reps, step_voxels=0.5, zfar=zfar,
               bricks=int(bricks.numel()), bricks_live=int(bricks.sum()), bricks_ms=median_ms(build))
    for views in sorted({1, V}):
        plain_ms = median_ms(lambda: cast(views, False))
        quick_ms = median_ms(lambda: cast(views, True))
        same = all(torch.equal(a[:views].view(torch.int32), b[:views].view(torch.int32)) for a, b in zip(outs[False], outs[True]))
        per_ray, hit_share = samples_per_ray(E[:views], Kmat, W, H, o, voxel, n, step, zfar, outs[False][0][:views])
        rays = views * H * W
        res[f"views_{views}"] = dict(plain_ms=plain_ms, bricks_ms=quick_ms, speedup=round(plain_ms / quick_ms, 2), same_bits=same,
                                     hit_share=round(hit_share, 4), samples_per_ray=round(per_ray, 1),
                                     taps_per_s=round(per_ray * rays * 16 / (plain_ms * 1e-3), -6),
                                     rays_per_s_plain=round(rays / (plain_ms * 1e-3), -3), rays_per_s_bricks=round(rays / (quick_ms * 1e-3), -3))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
