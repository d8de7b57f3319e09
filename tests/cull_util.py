"""Shared by tests/test_cull_cpu.py and tests/test_cull_gpu.py (empty-ray culling): the Python reference of the stream compaction, and
the seeded test scene with the oracle's verdict on each of its rays.  No GPU is touched here."""
import functools
import types

import numpy as np
import torch

from oracle import diner_oracle as O
from tests.helpers import oracle_setup, SAT_L

W, H, SCENE_SEED, N_CAND = 48, 40, 3, 1000
NOISE_SEED = 20261018


# ------------------------------------------------------------------------------------------------------ the compaction, in Python
def ref_compact(stats, threshold, rays, z, ray_index0, n_live, rays_out, z_out, live_idx):
    """What diner_compact_live_f32 does, one ray at a time, on CPU tensors; rays_out / z_out / live_idx (capacity rows) are written in
    place.  -> (slot (NR) int32, the advanced counter)."""
    cap = rays_out.shape[0]
    NR = z.shape[0]
    slot = torch.full((NR,), -1, dtype=torch.int32)
    s = stats[:, 1].tolist()
    thr = float(np.float32(threshold))
    for i in range(NR):
        if s[i] <= thr:                     # dead; a NaN compares false and is live
            continue
        if n_live < cap:
            rays_out[n_live] = rays[i]
            z_out[n_live] = z[i]
            live_idx[n_live] = ray_index0 + i
            slot[i] = n_live
        n_live += 1
    return slot, n_live


def ref_expand(tiles, slot, bg):
    """out[i] = slot[i] < 0 ? bg : tiles[slot[i]] as an indexing expression."""
    s = slot.long()
    return torch.where((s >= 0)[:, None], tiles[s.clamp(min=0)], bg[None].expand(s.shape[0], -1)) if tiles.shape[0] else \
        bg[None].expand(s.shape[0], -1).clone()


def bits(t):
    """float32 / int32 tensor -> its bytes as int32 (NaN-safe equality)."""
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------- the test scene
def reference_mask_any(scene, rays, z_cand, depth_diff_max=0.05):
    """(NR,) bool: the reference's candidate mask (nerf_renderer.py:121-124: a depth-map texel with non-zero sigma within depth_diff_max
    of the candidate, facing the ray) is true for some candidate in some view.  The same operations, in the same order, as the oracle's
    point_likelihood evaluates before any erf."""
    NR, n_cand = z_cand.shape
    xyz = rays[:, None, :3] + z_cand.unsqueeze(-1) * rays[:, None, 3:6]
    xyz_cam = O.world_to_cam(scene, xyz.reshape(-1, 3))
    dirs_cam = O.rot3(scene.poses[:, :3, :3], rays[:, 3:6])
    pd = dirs_cam.repeat_interleave(n_cand, dim=-2).transpose(-2, -1)
    uv = O.project_uv(scene, xyz_cam)
    ref_d, ref_s, ref_n = O.index_depth(scene, uv), O.index_depth_std(scene, uv), O.index_normal(scene, uv)
    ref_z = xyz_cam[..., 2:].permute(0, 2, 1)
    cosd = ((pd[:, 0:1] * ref_n[:, 0:1] + pd[:, 1:2] * ref_n[:, 1:2]) + pd[:, 2:3] * ref_n[:, 2:3])
    mask = (ref_s != 0) & ((ref_d - ref_z).abs() < depth_diff_max) & (cosd <= 0)
    return mask.any(dim=0).reshape(NR, n_cand).any(dim=-1)


def classify(scene, rays, noise_coarse):
    """The oracle's verdict per ray.  empty: its ray_mask (nerf_renderer.py:182) is false; pinned_dead: the candidate mask is false for
    every candidate and view (no erf involved); pinned_live: the largest likelihood is >= SAT_L, the spread between two erf
    implementations (tests/helpers.py); unpinned: neither."""
    zc = O.sample_coarse(rays, noise_coarse.shape[1], noise_coarse)
    L, Oq = O.point_likelihood(scene, rays, zc)
    dead = ~reference_mask_any(scene, rays, zc)
    live = L.max(dim=-1).values >= SAT_L
    assert not (dead & live).any() and (L[dead] == 0).all()
    return types.SimpleNamespace(empty=~(Oq != 0).any(-1), pinned_dead=dead, pinned_live=live, unpinned=~dead & ~live, sum_O=Oq.sum(-1))


def half_focal(Kt):
    """The target intrinsics with the two focal entries halved: the object fills a quarter of the frame."""
    Kt = Kt.clone()
    Kt[0, 0] *= 0.5
    Kt[1, 1] *= 0.5
    return Kt


def frame_noise(n_rays, K, G, seed=NOISE_SEED, n_cand=N_CAND):
    """(coarse (1,n,n_cand), gauss (1,n,G), fill (1,n,K)) for one object's frame, from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, n_rays, n_cand, generator=g), torch.randn(1, n_rays, G, generator=g), torch.rand(1, n_rays, K, generator=g))


@functools.lru_cache(maxsize=None)
def scene_case(nv=4, w=W, h=H, focal_scale=0.5, n_cand=N_CAND):
    """The seeded scene of the culling tests: -> namespace(sc, scene (oracle), msd, Kt, rays (h*w,8) from O.gen_rays, coarse: the
    candidate jitter (h*w,n_cand) of frame_noise, verdict: classify(...))."""
    kw = {} if nv == 4 else {"nv": nv}
    sc, scene, _, msd, _ = oracle_setup(w, h, SCENE_SEED, **kw)
    Kt = half_focal(sc["target_intrinsics"]) if focal_scale == 0.5 else sc["target_intrinsics"].clone()
    rays = O.gen_rays(sc["target_extrinsics"], Kt, w, h, sc["znear"], sc["zfar"])
    coarse = frame_noise(w * h, 40, 15, n_cand=n_cand)[0][0]
    return types.SimpleNamespace(sc=sc, scene=scene, msd=msd, Kt=Kt, rays=rays, coarse=coarse, verdict=classify(scene, rays, coarse),
                                 w=w, h=h)
