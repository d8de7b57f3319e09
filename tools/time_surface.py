"""What a mesh costs: the kernels of surface.hip on their own, and diner_amd.surface.mesh_from_sources end to end.

    python tools/time_surface.py [--dim 256] [--size 800x600] [--views 16] [--reps 20]

Scene for the kernels: an analytic sphere of radius 0.25 at the origin seen by --views cameras on a tilted ring of radius 1 (--size
depth and colour maps), fused into a --dim^3 volume with colour planes.  Through the C entries on preallocated buffers, HIP events
around each call, the median of --reps timed calls after 3 warm-up calls:
  - diner_tsdf_integrate_f32 with all views in ONE call, and as one call per view (events around the whole series);
  - diner_surface_count, and diner_surface_extract_f32 (which reads the counts back: one host synchronisation inside the events).
Each comes with the bytes the kernels must move and the GB/s that makes:
  integrate: 2 x 4 B x 6 planes per voxel and call (read + write tsdf, wsum and the four colour planes) + the maps once (16 B / pixel);
  count:     8 B / voxel (tsdf, wsum);   extract: 8 B / voxel + the 4 B / voxel cell -> vertex map written and read once + the outputs.
Then mesh_from_sources on the seeded synthetic scene of --size (four source views, default voxel: the longest side / 256), events
around the whole call -- box, allocation, fusion, counting, read-back, extraction.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ring_cameras(V, f, W, H):
    """V world->camera matrices (V,4,4) on a ring of radius 1 tilted by 0.3 rad, looking at the origin, and one intrinsics (3,3)."""
    import torch
    E = torch.zeros(V, 4, 4)
    for v in range(V):
        a = 2.0 * math.pi * v / V
        eye = torch.tensor([math.cos(a) * math.cos(0.3), math.sin(a) * math.cos(0.3), math.sin(0.3) * (1 if v % 2 else -1)])
        eye = eye / eye.norm()
        fw = -eye
        right = torch.linalg.cross(fw, torch.tensor([0.0, 0.0, 1.0]))
        right = right / right.norm()
        down = torch.linalg.cross(fw, right)
        R = torch.stack((right, down, fw))
        E[v, :3, :3], E[v, :3, 3], E[v, 3, 3] = R, -R @ eye, 1.0
    Kmat = torch.tensor([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    return E, Kmat


def sphere_maps(E, Kmat, W, H, radius, dev):
    """z-depth (V,H,W), 0 off the sphere, and colour (V,3,H,W) = 0.5 + 0.5 normal of the sphere at the origin, on `dev`."""
    import torch
    E, Kmat = E.to(dev), Kmat.to(dev)
    x = (torch.arange(W, device=dev) + 0.5 - Kmat[0, 2]) / Kmat[0, 0]
    y = (torch.arange(H, device=dev) + 0.5 - Kmat[1, 2]) / Kmat[1, 1]
    dc = torch.stack((x.view(1, W).expand(H, W), y.view(H, 1).expand(H, W), torch.ones(H, W, device=dev)), dim=-1)
    depth, color = [], []
    for v in range(E.shape[0]):
        R, t = E[v, :3, :3], E[v, :3, 3]
        eye = -R.T @ t
        dw = dc @ R
        a, b, c = (dw * dw).sum(-1), 2.0 * (dw @ eye), eye @ eye - radius * radius
        disc = b * b - 4 * a * c
        hit = disc > 0
        s = torch.where(hit, (-b - disc.clamp(min=0).sqrt()) / (2 * a), torch.zeros_like(a))
        n = (eye + s[..., None] * dw) / radius
        depth.append(s)
        color.append(torch.where(hit[None], 0.5 + 0.5 * n.permute(2, 0, 1), torch.zeros(3, H, W, device=dev)))
    return torch.stack(depth).contiguous(), torch.stack(color).contiguous()


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
    from diner_amd.surface import mesh_from_sources
    from diner_amd.synthetic import make_scene
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    W, H = (int(v) for v in args.size.split("x"))
    n, V = args.dim, args.views
    E, Kmat = ring_cameras(V, 1.125 * W, W, H)
    depth, color = sphere_maps(E, Kmat, W, H, 0.25, dev)
    Kv = Kmat[None].expand(V, -1, -1).contiguous()
    voxel = 0.8 / n
    trunc = 3.0 * voxel
    origin = (C.c_float * 3)(-0.4 + 0.013, -0.4 + 0.007, -0.4 + 0.003)
    tsdf = torch.ones(n, n, n, device=dev)
    wsum = torch.zeros(n, n, n, device=dev)
    color4 = torch.zeros(4, n, n, n, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        out = fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1), out

    def median_ms(fn, warm=3):
        for _ in range(warm):
            fn()
        return round(statistics.median(timed(fn)[0] for _ in range(args.reps)), 4)

    def integrate(v0, v1):
        _lib.check(lib.diner_tsdf_integrate_f32(tsdf.data_ptr(), wsum.data_ptr(), color4.data_ptr(), n, n, n, origin, voxel, trunc,
                                                depth[v0:v1].data_ptr(), None, color[v0:v1].data_ptr(), Kv[v0:v1].data_ptr(),
                                                E[v0:v1].data_ptr(), v1 - v0, H, W, 1, 0.0, st))

    def one_call():
        integrate(0, V)

    def per_view_calls():
        for v in range(V):
            integrate(v, v + 1)

    n_vox = n ** 3
    map_bytes = V * H * W * 16
    one_ms = median_ms(one_call)
    per_view_ms = median_ms(per_view_calls)
    # a clean volume for the extraction: exactly one pass over the views
    tsdf.fill_(1.0)
    wsum.zero_()
    color4.zero_()
    one_call()
    ws = torch.empty(lib.diner_surface_workspace_bytes(n, n, n), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)

    def count():
        _lib.check(lib.diner_surface_count(tsdf.data_ptr(), wsum.data_ptr(), n, n, n, 0.0, ws.data_ptr(), counts.data_ptr(), st))

    count()
    nv, nq = counts.tolist()
    verts, normals, rgb = (torch.empty(nv, 3, device=dev) for _ in range(3))
    faces = torch.empty(2 * nq, 3, device=dev, dtype=torch.int32)

    def extract():
        _lib.check(lib.diner_surface_extract_f32(tsdf.data_ptr(), wsum.data_ptr(), color4.data_ptr(), n, n, n, origin, voxel, 0.0,
                                                 ws.data_ptr(), nv, nq, verts.data_ptr(), normals.data_ptr(), rgb.data_ptr(),
                                                 faces.data_ptr(), st))

    count_ms = median_ms(count)
    extract_ms = median_ms(extract)
    r = (verts.norm(dim=1) - 0.25).abs().max().item() / voxel if nv else float("nan")

    def gbs(nbytes, ms):
        return round(nbytes / (ms * 1e-3) / 1e9, 1)

    integrate_bytes, per_view_bytes = 48 * n_vox + map_bytes, 48 * n_vox * V + map_bytes
    count_bytes = 8 * n_vox
    extract_bytes = 16 * n_vox + nv * 36 + nq * 24
    res = dict(tool="time_surface", dim=n, size=args.size, views=V, reps=args.reps,
               integrate_one_call_ms=one_ms, integrate_one_call_bytes=integrate_bytes, integrate_one_call_gbs=gbs(integrate_bytes, one_ms),
               integrate_per_view_calls_ms=per_view_ms, integrate_per_view_calls_bytes=per_view_bytes,
               integrate_per_view_calls_gbs=gbs(per_view_bytes, per_view_ms),
               vertices=nv, quads=nq, radius_error_voxels=round(r, 3),
               count_ms=count_ms, count_bytes=count_bytes, count_gbs=gbs(count_bytes, count_ms),
               extract_ms=extract_ms, extract_bytes=extract_bytes, extract_gbs=gbs(extract_bytes, extract_ms))
    del tsdf, wsum, color4, ws
    torch.cuda.empty_cache()

    # mesh_from_sources end to end on the synthetic scene's four source views
    sc = make_scene(W, H, seed=0, latent=False)
    g = torch.Generator().manual_seed(0)
    nvs = sc["depths"].shape[0]
    batch = dict(src_depths=sc["depths"][None].to(dev), src_rgbs=torch.rand(1, nvs, 3, H, W, generator=g).to(dev),
                 src_intrinsics=sc["src_intrinsics"][None], src_extrinsics=sc["src_extrinsics"][None])
    mesh_from_sources(batch)
    ms, meshes = [], None
    for _ in range(5):
        t, meshes = timed(lambda: mesh_from_sources(batch))
        ms.append(round(t, 3))
    mesh, vol = meshes
    res.update(mesh_from_sources_ms=ms, mesh_from_sources_median_ms=statistics.median(ms), mesh_from_sources_dims=list(vol.dims),
               mesh_from_sources_vertices=int(mesh.vertices.shape[0]), mesh_from_sources_triangles=int(mesh.faces.shape[0]))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
