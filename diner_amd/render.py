"""Image harness: the MI355X counterpart of DINER.predict_imgs_from_batch (reference src/models/diner.py:72-97).

The reference renders one target image by splitting its H*W rays into batches of `ray_batch_size` and calling
`renderer.forward` on each (diner.py:85-92).  Rays are independent, so here the row-major ray list is additionally
sharded into contiguous ranges across the GPUs of a node (one process per GPU, torch.distributed; backend "nccl" is
RCCL on ROCm), each rank renders its range with the HIP kernels, and ONE gather of the packed (rgb, depth) tiles
(16 B/ray) brings the image to rank 0.  There is no other collective on the data path: scene state and MLP weights
are replicated (every rank runs `encode` itself).
"""
import contextlib

import torch

from diner_amd import noise as _noise
from src.util.cam_geometry import gen_rays


def shard_range(n, rank, world):
    """Contiguous, balanced partition of range(n): rank r gets [lo, hi)."""
    per = (n + world - 1) // world
    lo = min(n, rank * per)
    return lo, min(n, lo + per)


def host_staged(group=None):
    """True when the process group cannot move device memory itself: backend "gloo" (ranks that share one GPU -- RCCL
    refuses two ranks on one device --, or a box without RCCL).  The two collectives of the path (tile gather, 8-byte seed
    broadcast) then go through pinned host buffers; with "nccl" (= RCCL) they run on device tensors over xGMI."""
    import torch.distributed as dist
    return "nccl" not in str(dist.get_backend(group))


def gather_tiles(local, n_total, rank, world, group=None, force=False):
    """Gather per-rank (n_r, C) tiles (contiguous ray ranges, see shard_range) to rank 0 -> (n_total, C) or None.

    Uses equal-size padded buffers so that a single gather collective suffices.  `force`: go through the collective even with one rank
    (bench.py --force-dist: exercises RCCL on a 1-GPU box)."""
    if world == 1 and not force:
        return local
    import torch.distributed as dist
    per = (n_total + world - 1) // world
    dev = local.device
    staged = local.is_cuda and host_staged(group)
    if staged:                       # 16 B/ray through pinned host memory (7.7 MB per 800x600 frame over all ranks)
        buf = torch.zeros(per, local.shape[1], dtype=local.dtype).pin_memory()
        buf[:local.shape[0]].copy_(local, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
    else:
        buf = local
        if local.shape[0] != per:
            buf = torch.zeros(per, local.shape[1], device=dev, dtype=local.dtype)
            buf[:local.shape[0]] = local
    out = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
    dist.gather(buf.contiguous(), out, dst=0, group=group)
    if rank != 0:
        return None
    full = torch.cat(out, dim=0)[:n_total]
    return full.to(dev, non_blocking=False) if staged else full


@torch.no_grad()
def predict_surface_prior(nerf, target_extrinsics, target_intrinsics, W, H, znear, zfar, n_samples=40, n_candidates=1000,
                          n_gaussian=15, depth_diff_max=0.05, ray_batch_size=8192, seed=None):
    """The depth-guided sampler's view of the (SB) target views: what the source depth maps alone say about every target pixel, without
    the MLP.  -> hit (SB,1,H,W), the depth maps' probability 1 - prod(1 - L) that the pixel's ray meets a surface; depth (SB,1,H,W) and
    depth_std (SB,1,H,W), mean and sigma of the likelihood-weighted gaussian the sampler draws its n_gaussian samples from (both 0 where
    hit is 0).  Needs the depth, std and normal maps of the scene last passed to nerf.encode() only; the latent and the MLP handle are
    not touched.  Rays, batches and the frame's noise key as in predict_image (one process): the maps do not depend on ray_batch_size,
    and on the noise only through the candidate jitter (1 / n_candidates of the depth range).  `seed` None: drawn from torch's global
    CPU generator.  Noise injected with diner_amd.noise.inject is sliced per batch as in predict_image."""
    from diner_amd import ops
    SB = target_extrinsics.shape[0]
    dev = nerf.encoder.depths.device
    rays = ops.gen_rays(target_extrinsics, target_intrinsics, W, H, znear, zfar, dev)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    inj = _noise.current()
    out = torch.empty(SB, H * W, 3, device=dev, dtype=torch.float32)
    for sb in range(SB):
        scene = nerf.hip_scene(sb)
        for r0 in range(0, H * W, ray_batch_size):
            r1 = min(H * W, r0 + ray_batch_size)
            nz = None if inj is None else tuple(None if t is None else t[sb, r0:r1] for t in inj)
            # the key renderer.forward uses for object sb under noise.keyed(seed, r0)
            info = ops.sample_depthguided_long(scene, rays[sb, r0:r1].contiguous(), n_samples, n_candidates, n_gaussian, depth_diff_max,
                                               noise=nz, seed=seed + 0x9E3779B97F4A7C15 * sb, ray_index0=r0, want_info=True)[1]
            out[sb, r0:r1] = torch.stack((info.sum_O, info.prior_depth, info.prior_std), dim=-1)
    out = out.view(SB, H, W, 3).permute(0, 3, 1, 2)
    return out[:, 0:1].contiguous(), out[:, 1:2].contiguous(), out[:, 2:3].contiguous()


CULL_BUFFER_BYTES = 1 << 30      # bound of the frame-level live-ray buffers of render_live_rays; a larger frame goes in chunks of rays


@torch.no_grad()
def render_live_rays(scene, mlp, rays, sample, n_samples, white_bkgd, n_aux=0, cull_below=0.0, ray_batch_size=8192,
                     rank=0, world=1, group=None):
    """Empty-ray culling for one object: render only the rays the source depth maps put a surface on.  rays (N,8): a frame's (or a
    call's) ray list; sample(r0, r1) -> (z (r1-r0, K), SamplerInfo) of rays[r0:r1] (ops.sample_depthguided_long(want_info=True) under
    the caller's noise key); K = n_samples.  -> (N, 4 + n_aux) rows [rgb, depth (, alpha (, depth_var))] on rank 0, None elsewhere.

    A ray is LIVE iff not (sum_O <= cull_below): sum_O is the depth maps' probability that the ray meets a surface, the reference's
    ray_mask (nerf_renderer.py:182) at cull_below = 0; a NaN is live.  Live rays are compacted in frame order (ops.compact_live), the
    live list is rendered by ops.render in batches of ray_batch_size -- a live ray's values are those of the plain frame, since a ray's
    result does not depend on the launch it is in -- and ops.expand_live puts them back.  A dead ray gets the compositor's values at
    zero density (ops.background_row) WITHOUT running the MLP.  That is an approximation of the reference, which evaluates the MLP on K
    stratified samples of such a ray too: wherever the network returns density away from every surface the depth maps know, the plain
    frame shows it and the culled frame does not.

    One host synchronisation (the 4-byte live count) per chunk: the whole list when the live buffers fit CULL_BUFFER_BYTES, else
    chunks of rays that do.  A chunk without a live ray launches no field kernel.  With world > 1 every rank compacts the whole list
    (the sampler is well under 1 % of a frame), renders shard_range(n_live, rank, world) of the live list and gather_tiles brings the
    live tiles to rank 0: the load is balanced over live rays, not over pixels."""
    from diner_amd import ops
    N, K, C = int(rays.shape[0]), int(n_samples), 4 + int(n_aux)
    dev = rays.device
    bg = ops.background_row(white_bkgd, n_aux, dev)
    out = torch.empty(N, C, device=dev, dtype=torch.float32) if rank == 0 else None
    chunk = max(1, min(N, CULL_BUFFER_BYTES // (4 * K + 40)))
    for c0 in range(0, N, chunk):
        c1 = min(N, c0 + chunk)
        rays_live = torch.empty(c1 - c0, 8, device=dev, dtype=torch.float32)
        z_live = torch.empty(c1 - c0, K, device=dev, dtype=torch.float32)
        live_idx = torch.empty(c1 - c0, device=dev, dtype=torch.int32)
        n_live_dev = torch.zeros(1, device=dev, dtype=torch.int32)
        slots = []
        for r0 in range(c0, c1, ray_batch_size):
            r1 = min(c1, r0 + ray_batch_size)
            z, info = sample(r0, r1)
            slots.append(ops.compact_live(info, cull_below, rays[r0:r1], z, r0, rays_live, z_live, live_idx, n_live_dev)[0])
        n_live = int(n_live_dev.item())                       # the one read-back
        lo, hi = shard_range(n_live, rank, world)
        tiles = []
        for a in range(lo, hi, ray_batch_size):
            b = min(hi, a + ray_batch_size)
            _, rgb, depth, *aux = ops.render(scene, mlp, rays_live[a:b], z_live[a:b], white_bkgd, want_aux=n_aux > 0)
            tiles.append(torch.cat((rgb, depth.unsqueeze(-1)) + tuple(t.unsqueeze(-1) for t in aux[:n_aux]), dim=-1))
        local = torch.cat(tiles, dim=0) if tiles else torch.zeros(0, C, device=dev)
        full = gather_tiles(local, n_live, rank, world, group) if n_live > 0 else local
        if rank == 0:
            slot = torch.cat(slots) if len(slots) > 1 else slots[0]
            out[c0:c1] = ops.expand_live(full, slot, bg, n_tiles=n_live)
    return out


def _predict_image_culled(nerf, renderer, rays, SB, n_rays, ray_batch_size, rank, world, group, seed, return_alpha, cull_below):
    """predict_image(cull_empty=True) per object: -> (n_rays, SB * C) tiles in predict_image's layout on rank 0, None elsewhere."""
    from diner_amd import ops
    renderer._check_model(nerf)
    K, n_cand, G = int(renderer.n_samples), int(renderer.n_depth_candidates), int(renderer.n_gaussian)
    assert K >= G
    mlp = nerf.hip_mlp()
    inj = _noise.current()
    per_object = []
    for sb in range(SB):
        scene = nerf.hip_scene(sb)

        def sample(r0, r1, sb=sb, scene=scene):
            nz = None if inj is None else tuple(None if t is None else t[sb, r0:r1] for t in inj)
            # the key renderer.forward uses for object sb under noise.keyed(seed, r0)
            return ops.sample_depthguided_long(scene, rays[sb, r0:r1], K, n_cand, G, 0.05, noise=nz,
                                               seed=seed + 0x9E3779B97F4A7C15 * sb, ray_index0=r0, want_info=True)

        per_object.append(render_live_rays(scene, mlp, rays[sb], sample, K, renderer.white_bkgd, n_aux=1 if return_alpha else 0,
                                           cull_below=cull_below, ray_batch_size=ray_batch_size, rank=rank, world=world, group=group))
    if rank != 0:
        return None
    return torch.stack(per_object, dim=1).reshape(n_rays, -1)


@torch.no_grad()
def predict_image(nerf, renderer, target_extrinsics, target_intrinsics, W, H, znear, zfar, ray_batch_size=8192,
                  rank=0, world=1, group=None, seed=None, return_alpha=False, cull_empty=False, cull_below=0.0):
    """Render the (SB) target views described by target_extrinsics (SB,4,4) / target_intrinsics (SB,3,3) of the
    scene last passed to nerf.encode().  Returns rgb (SB,3,H,W), depth (SB,1,H,W) on rank 0 (None elsewhere); with return_alpha also
    the opacity map alpha (SB,1,H,W) (renderer.forward(want_alpha=True): one more channel in the gathered tiles, 20 B/ray).
    Same ray order (row-major pixels, centres at +0.5) and output layout as diner.py:79-92.  Noise injected with
    diner_amd.noise.inject for the whole (SB, H*W, .) ray list is handed to every batch as the matching slice (parity
    tests); without injection the sampler draws in-kernel Philox noise keyed by (`seed`, position of the ray in the frame):
    the image does not depend on ray_batch_size or on the number of ranks.  `seed` None: drawn from torch's global CPU
    generator on rank 0 and, with more than one rank, broadcast (8 bytes) so that all shards belong to the same frame.

    cull_empty (off by default; HIP devices only): render only the rays the source depth maps put a surface on -- see render_live_rays.
    Per object the info sampler runs over the frame in ray batches (same noise key and injected-noise slices as the plain call), the
    live rays (not (sum_O <= cull_below)) are compacted, the live list is rendered in batches of ray_batch_size and expanded into the
    frame; every other pixel gets the compositor's values at zero density (rgb 1 with white_bkgd else 0, depth 0, alpha 0) without
    running the MLP.  This approximates the reference, which evaluates the MLP on K stratified samples of such rays as well; at the
    live pixels the frame is the plain frame bit for bit.  One host read-back (the live count) per object and frame.  With more than
    one rank every rank samples and compacts the whole frame and renders its share of the LIVE list.  With cull_empty False the
    function runs exactly the code it ran before the option existed."""
    SB = target_extrinsics.shape[0]
    dev = target_extrinsics.device
    znear = torch.as_tensor(znear, device=dev, dtype=torch.float32).expand(SB)
    zfar = torch.as_tensor(zfar, device=dev, dtype=torch.float32).expand(SB)
    if cull_empty and dev.type != "cuda":
        raise RuntimeError("diner_amd: predict_image(cull_empty=True) runs on a HIP device; there is no CPU fallback")
    lo, hi = (0, H * W) if cull_empty else shard_range(H * W, rank, world)     # culling: every rank compacts the whole frame
    if dev.type == "cuda":         # this rank's ray range only, generated on the device (diner_gen_rays_f32)
        from diner_amd import ops
        rays = ops.gen_rays(target_extrinsics, target_intrinsics, W, H, znear, zfar, dev, ray0=lo, n_rays=hi - lo)
        base = lo
    else:                          # host tensors (gloo tests): the reference's torch ops
        rays = gen_rays(target_extrinsics, target_intrinsics, W, H, znear, zfar).view(SB, H * W, 8)
        base = 0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if world > 1:
            import torch.distributed as dist
            on_dev = dev.type == "cuda" and not host_staged(group)
            t = torch.tensor([seed], dtype=torch.int64, device=dev if on_dev else "cpu")
            dist.broadcast(t, src=0, group=group)
            seed = int(t.item())
    C = 5 if return_alpha else 4
    if cull_empty:
        full = _predict_image_culled(nerf, renderer, rays, SB, H * W, ray_batch_size, rank, world, group, seed, return_alpha, cull_below)
    else:
        tiles = []
        inj = _noise.current()
        for r0 in range(lo, hi, ray_batch_size):
            r1 = min(hi, r0 + ray_batch_size)
            rb = rays[:, r0 - base:r1 - base].contiguous()
            ctx = contextlib.nullcontext() if inj is None else _noise.inject(*(None if t is None else t[:, r0:r1] for t in inj))
            with ctx, _noise.keyed(seed, r0):
                out = renderer.forward(model=nerf, rays=rb, want_alpha=True) if return_alpha else renderer.forward(model=nerf, rays=rb)
            parts = (out.fine.rgb, out.fine.depth.unsqueeze(-1)) + ((out.fine.alpha.unsqueeze(-1),) if return_alpha else ())
            tiles.append(torch.cat(parts, dim=-1))                                              # (SB, b, C)
        local = torch.cat(tiles, dim=1) if tiles else torch.zeros(SB, 0, C, device=dev)
        full = gather_tiles(local.permute(1, 0, 2).reshape(hi - lo, SB * C), H * W, rank, world, group)
    if full is None:
        return (None, None, None) if return_alpha else (None, None)
    full = full.view(H, W, SB, C).permute(2, 3, 0, 1)                                       # (SB,C,H,W)
    if return_alpha:
        return full[:, :3].contiguous(), full[:, 3:4].contiguous(), full[:, 4:5].contiguous()
    return full[:, :3].contiguous(), full[:, 3:4].contiguous()


GEOMETRY_MAPS = ("depth", "alpha", "depth_var", "depth_median", "depth_mean", "zdepth")


@torch.no_grad()
def predict_geometry(nerf, renderer, target_extrinsics, target_intrinsics, W, H, znear, zfar, ray_batch_size=8192, seed=None,
                     quantile=0.5, alpha_min=1e-3, point_depth="median"):
    """predict_image with the geometry of the rendered surface (one process; HIP devices only).  Same rays, ray order, batches and frame
    noise key as predict_image: rgb (SB,3,H,W), depth and alpha (SB,1,H,W) are predict_image(return_alpha=True)'s of the same seed bit
    for bit.  -> dict of maps: rgb; depth (the reference's sum_k w_k z_k, a distance along the ray), alpha, depth_var; depth_median (the
    sample depth at which the accumulated weight crosses `quantile` of the opacity), depth_mean (depth / alpha), both along the ray;
    zdepth (SB,1,H,W), the camera-z depth of the surface point -- the unit of the source depth maps and of depth2normal --; points
    (SB,3,H,W), the world-space surface point o + t d with t the median (point_depth "median") or the mean ("mean"); valid (SB,1,H,W)
    bool, alpha > alpha_min as ops.ray_geometry decides it (an invalid pixel has 0 in depth_median, depth_mean, zdepth and points); and
    normals (SB,3,H,W) = ops.depth2normal(zdepth, target_intrinsics): camera-frame normals with the reference's hole rule (an invalid
    pixel is a hole), the convention of the normal maps the encoder receives; and extrinsics, the target_extrinsics of the call (what
    diner_amd.geometry.point_cloud needs to turn the normals into the world frame).  Injected noise is sliced per batch as in predict_image."""
    from diner_amd import ops
    SB = target_extrinsics.shape[0]
    dev = target_extrinsics.device
    if dev.type != "cuda":
        raise RuntimeError("diner_amd: predict_geometry runs on a HIP device; there is no CPU fallback")
    znear = torch.as_tensor(znear, device=dev, dtype=torch.float32).expand(SB)
    zfar = torch.as_tensor(zfar, device=dev, dtype=torch.float32).expand(SB)
    rays = ops.gen_rays(target_extrinsics, target_intrinsics, W, H, znear, zfar, dev)
    cam_fwd = target_extrinsics.detach().to("cpu", torch.float32)[:, 2, :3].contiguous()
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    tiles = []
    inj = _noise.current()
    for r0 in range(0, H * W, ray_batch_size):
        r1 = min(H * W, r0 + ray_batch_size)
        rb = rays[:, r0:r1].contiguous()
        ctx = contextlib.nullcontext() if inj is None else _noise.inject(*(None if t is None else t[:, r0:r1] for t in inj))
        with ctx, _noise.keyed(seed, r0):
            f = renderer.forward_geometry(nerf, rb, cam_fwd=cam_fwd, quantile=quantile, alpha_min=alpha_min, point_depth=point_depth).fine
        tiles.append(torch.cat((f.rgb,) + tuple(f[k].unsqueeze(-1) for k in GEOMETRY_MAPS) + (f.points, f.median_idx.unsqueeze(-1).float()),
                               dim=-1))                                                  # (SB, b, 13)
    C = 3 + len(GEOMETRY_MAPS) + 4
    full = (torch.cat(tiles, dim=1) if tiles else torch.zeros(SB, 0, C, device=dev)).view(SB, H, W, C).permute(0, 3, 1, 2)
    out = {"rgb": full[:, :3].contiguous()}
    for i, k in enumerate(GEOMETRY_MAPS):
        out[k] = full[:, 3 + i:4 + i].contiguous()
    out["points"] = full[:, 9:12].contiguous()
    out["valid"] = full[:, 12:13] >= 0
    out["extrinsics"] = target_extrinsics
    out["normals"] = ops.depth2normal(out["zdepth"], target_intrinsics.to(dev)) if H * W > 0 else torch.zeros(SB, 3, H, W, device=dev)
    return out
