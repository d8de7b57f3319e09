"""CPU: geometry from renders (diner_ray_geometry_f32 / diner_depth_consistency_f32, diner_amd.geometry) -- the entries are declared,
exported, bound and refuse bad arguments before any device work; the PLY writer round-trips bit for bit; point_cloud keeps row-major
order and its thresholds; the Python wrappers check their arguments before touching a device; and the numpy restatements that the GPU
tests compare against are fit for purpose: the share of rays / pixels they must leave undecided stays under 5 %, and on the analytic
plane scene they count what the construction says."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import geometry_util as G
from tests.helpers import ROOT

ENTRIES = ("diner_ray_geometry_f32", "diner_depth_consistency_f32")


def test_entries_declared_exported_and_bound():
    from diner_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6
    assert "geometry.hip" in build.SOURCES


def test_entries_refuse_bad_arguments_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(16)                 # never dereferenced: the checks run before any device work
    fwd = (C.c_float * 3)(0.0, 0.0, 1.0)

    def ray(w=p, NR=4, K=8, q=0.5, amin=1e-3, cam=fwd, mode=0, zd=p):
        return lib.diner_ray_geometry_f32(w, p, p, NR, K, q, amin, cam, mode, p, p, p, zd, p, None)

    for kw, what in ((dict(w=None), b"null"), (dict(NR=0), b"NR"), (dict(K=0), b"K ="), (dict(K=1025), b"K ="), (dict(q=0.0), b"quantile"),
                     (dict(q=1.5), b"quantile"), (dict(q=float("nan")), b"quantile"), (dict(amin=-1.0), b"alpha_min"),
                     (dict(amin=float("nan")), b"alpha_min"), (dict(mode=2), b"point_mode"), (dict(cam=None), b"cam_fwd")):
        assert ray(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())

    def cons(d=p, Km=p, N=3, H=4, W=4, px=1.0, rel=0.01):
        return lib.diner_depth_consistency_f32(d, Km, p, N, H, W, px, rel, p, p, None)

    for kw, what in ((dict(d=None), b"null"), (dict(Km=None), b"null"), (dict(N=1), b"views"), (dict(N=17), b"views"), (dict(H=0), b"size"),
                     (dict(W=0), b"size"), (dict(H=1 << 20, W=1 << 20), b"size"), (dict(px=-1.0), b"threshold"),
                     (dict(rel=float("nan")), b"threshold")):
        assert cons(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())


def test_python_surface_is_off_by_default_and_checks_before_the_device():
    from diner_amd import evaluate, geometry, ops, render
    from src.models.nerf_renderer import NeRFRendererDGS
    assert inspect.signature(evaluate.write_prediction_folder).parameters["write_geometry"].default is False
    sig = inspect.signature(render.predict_geometry).parameters
    assert (sig["quantile"].default, sig["alpha_min"].default, sig["point_depth"].default) == (0.5, 1e-3, "median")
    sig = inspect.signature(ops.ray_geometry).parameters
    assert (sig["cam_fwd"].default, sig["quantile"].default, sig["alpha_min"].default, sig["point_depth"].default) == (None, 0.5, 1e-3, "median")
    sig = inspect.signature(ops.depth_consistency).parameters
    assert (sig["px_thr"].default, sig["rel_thr"].default) == (1.0, 0.01)
    assert inspect.signature(geometry.fuse_views).parameters["min_views"].default == 2
    assert hasattr(NeRFRendererDGS, "forward_geometry")
    w, z, rays = torch.zeros(5, 8), torch.zeros(5, 8), torch.zeros(5, 8)
    for kw, exc in ((dict(point_depth="mode"), ValueError), (dict(quantile=0.0), ValueError), (dict(quantile=1.01), ValueError),
                    (dict(alpha_min=-0.1), ValueError), (dict(cam_fwd=torch.zeros(4)), ValueError), ({}, RuntimeError)):
        with pytest.raises(exc):
            ops.ray_geometry(w, z, rays, **kw)                      # CPU tensors: the last one is the "no CPU fallback" error
    with pytest.raises(ValueError):
        ops.ray_geometry(w, torch.zeros(5, 9), rays)
    with pytest.raises(ValueError):
        ops.ray_geometry(torch.zeros(5, 1025), torch.zeros(5, 1025), rays)
    d, Km, E = torch.ones(3, 4, 5), torch.eye(3).repeat(3, 1, 1), torch.eye(4).repeat(3, 1, 1)
    for args, exc in (((d[:1], Km[:1], E[:1]), ValueError), ((d, Km[:2], E), ValueError), ((d, Km, E[:, :3]), ValueError),
                      ((d[0], Km, E), ValueError), ((torch.ones(17, 2, 2), torch.eye(3).repeat(17, 1, 1), torch.eye(4).repeat(17, 1, 1)), ValueError),
                      ((d, Km, E), RuntimeError)):
        with pytest.raises(exc):
            ops.depth_consistency(*args)
    with pytest.raises(ValueError):
        ops.depth_consistency(d, Km, E, px_thr=-1.0)
    with pytest.raises(RuntimeError):
        render.predict_geometry(None, None, E[:1], Km[:1], 4, 4, 0.5, 2.0)
    with pytest.raises(ValueError):
        geometry.fuse_views(None, None, E[:1], Km[:1], 4, 4, 0.5, 2.0)


# ----------------------------------------------------------------------------------------------------------------------- PLY
@pytest.mark.parametrize("M", [0, 1, 257])
@pytest.mark.parametrize("with_rgb,with_normals", [(False, False), (True, False), (False, True), (True, True)])
def test_ply_round_trip_is_bit_exact(tmp_path, M, with_rgb, with_normals):
    from diner_amd.geometry import read_ply, write_ply
    g = np.random.default_rng(M)
    xyz = g.normal(size=(M, 3)).astype(np.float32)
    if M:
        xyz[0] = [np.float32("nan"), np.float32("inf"), -0.0]
    rgb = g.integers(0, 256, (M, 3)).astype(np.uint8) if with_rgb else None
    nrm = g.normal(size=(M, 3)).astype(np.float32) if with_normals else None
    path = tmp_path / "cloud.ply"
    write_ply(path, torch.from_numpy(xyz), None if rgb is None else torch.from_numpy(rgb), nrm)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {M}"]
    want = ["property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] if with_normals else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_rgb else []
    assert head[3:-1] == want and head[-1] == ""
    assert len(raw) == raw.index(b"end_header\n") + 11 + M * (12 + 12 * with_normals + 3 * with_rgb)
    x2, c2, n2 = read_ply(path)
    assert x2.dtype == np.float32 and x2.shape == (M, 3) and x2.tobytes() == xyz.tobytes()
    assert (c2 is None) == (rgb is None) and (n2 is None) == (nrm is None)
    if with_rgb:
        assert c2.dtype == np.uint8 and c2.tobytes() == rgb.tobytes()
    if with_normals:
        assert n2.dtype == np.float32 and n2.tobytes() == nrm.tobytes()


def test_ply_refuses_wrong_columns(tmp_path):
    from diner_amd.geometry import write_ply
    with pytest.raises(ValueError):
        write_ply(tmp_path / "a.ply", np.zeros((3, 3)))                                         # float64
    with pytest.raises(ValueError):
        write_ply(tmp_path / "a.ply", np.zeros((3, 3), np.float32), rgb=np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError):
        write_ply(tmp_path / "a.ply", np.zeros((3, 3), np.float32), normals=np.zeros((3, 2), np.float32))


# --------------------------------------------------------------------------------------------------------------- point_cloud
def test_point_cloud_row_major_order_and_thresholds():
    from diner_amd.geometry import point_cloud
    SB, H, W = 2, 3, 4
    n = SB * H * W
    ids = torch.arange(n, dtype=torch.float32).view(SB, 1, H, W)
    geo = {"points": torch.cat((ids, ids + 0.25, ids + 0.5), dim=1), "rgb": (ids % 7 / 7.0).expand(-1, 3, -1, -1).contiguous(),
           "alpha": torch.full((SB, 1, H, W), 0.9), "depth_var": torch.zeros(SB, 1, H, W), "valid": torch.ones(SB, 1, H, W, dtype=torch.bool),
           "normals": torch.zeros(SB, 3, H, W), "extrinsics": torch.eye(4).repeat(SB, 1, 1)}
    geo["normals"][:, 2] = -1.0
    geo["extrinsics"][1, :3, :3] = torch.tensor([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])      # a quarter turn about z
    geo["normals"][1, 0], geo["normals"][1, 2] = 1.0, 0.0                                                     # camera +x in view 1
    geo["alpha"][0, 0, 1, 2] = 0.4              # below min_alpha
    geo["alpha"][0, 0, 2, 0] = 0.5              # at min_alpha: kept
    geo["valid"][1, 0, 0, 3] = False
    geo["depth_var"][1, 0, 2, 2] = 0.04         # std 0.2
    xyz, rgb, nrm = point_cloud(geo)
    kept = [i for i in range(n) if i not in (1 * W + 2, H * W + 3)]
    assert xyz[:, 0].tolist() == [float(i) for i in kept] and xyz.shape == (n - 2, 3) and torch.equal(xyz[:, 2], xyz[:, 0] + 0.5)
    assert rgb.dtype == torch.uint8 and rgb[:, 0].tolist() == [int(np.float32(np.float32(i % 7) / np.float32(7.0)) * np.float32(255.0) + np.float32(0.5))
                                                               for i in kept]
    first = len([i for i in kept if i < H * W])
    assert (nrm[:first] == torch.tensor([0.0, 0.0, -1.0])).all()
    assert torch.allclose(nrm[first:], torch.tensor([0.0, 1.0, 0.0]))        # R^T e_x = row 0 of R
    x2 = point_cloud(geo, max_depth_std=0.1)[0]
    assert x2.shape[0] == n - 3 and float(H * W + 2 * W + 2) not in x2[:, 0].tolist()
    assert point_cloud(geo, max_depth_std=0.2)[0].shape[0] == n - 2
    keep = torch.zeros(SB, 1, H, W, dtype=torch.bool)
    keep[1, 0, 1] = True
    assert point_cloud(geo, keep=keep)[0][:, 0].tolist() == [float(H * W + W + j) for j in range(W)]
    assert point_cloud(geo, min_alpha=0.95)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        point_cloud(geo, keep=keep.float())


# ------------------------------------------------------------------------------------------------------ the restatements themselves
@pytest.mark.parametrize("K", G.K_LIST)
def test_ray_restatement_leaves_few_rays_undecided(K):
    case = G.ray_case(K)
    assert case.NR % 4 != 0 and case.w.dtype == np.float32 and (np.diff(case.z, axis=1) >= 0).all()
    for q in G.quantiles_for(K):
        ref = G.ref_ray_geometry(case.w, case.z, case.rays, case.fwd, q, G.ALPHA_MIN, 0)
        amb = G.ambiguous_rays(ref, case.w, G.ALPHA_MIN)
        rnd = slice(0, G.NR_RANDOM)
        n_valid = int(ref.valid[rnd].sum())
        share = float((amb[rnd] & ref.valid[rnd]).sum()) / n_valid
        tol, gap = G.ray_tolerances(case, q, 0, ~amb)
        print(f"K={K} q={q}: {n_valid} of {G.NR_RANDOM} random rays valid, undecided share {share:.3f}, f32-f64 gap {gap}")
        assert n_valid >= 0.8 * G.NR_RANDOM and (~ref.valid[rnd]).sum() >= 1
        assert share <= 0.05
        # the hand-made rays: exact in any summation order (dyadic weights)
        h = case.hand
        if "tie" in h and q == 0.5:
            assert ref.idx[h["tie"]] == 1
        assert ref.idx[h["spike"]] == K // 2 and ref.depth_median[h["spike"]] == case.z[h["spike"], K // 2]
        assert ref.idx[h["below_alpha_min"]] == -1 and ref.idx[h["at_alpha_min"]] == -1 and ref.idx[h["above_alpha_min"]] == 0
        assert ref.points[h["below_alpha_min"]].tolist() == [0, 0, 0] and ref.zdepth[h["at_alpha_min"]] == 0
        if "negative_last" in h:
            assert ref.valid[h["negative_last"]] and 0 <= ref.idx[h["negative_last"]] <= K // 2


def test_consistency_restatement_counts_what_the_plane_scene_says():
    px_thr, rel_thr = 1.0, 0.01
    clean = G.consistency_scene(3, perturb=False)
    ref0 = G.ref_depth_consistency(clean.depth, clean.K, clean.E, px_thr, rel_thr)
    assert (clean.depth > 0).all()
    seen_by_all = ref0.geom[0, 1] & ref0.geom[0, 2]
    assert seen_by_all.sum() > 0.3 * clean.W * clean.H
    assert (ref0.count[0][seen_by_all] == 2).all()                           # a plane agrees with itself
    assert (ref0.count == ref0.geom.sum(axis=1)).all()
    assert not ref0.geom[2, 0].all() and not ref0.geom[0, 2].all()           # view 2 sees plane the others do not
    # not zero: the z-depth of a tilted plane is not linear in the pixel coordinates (its inverse is), so the bilinear lookup is off by
    # the second-order term -- two decades below the thresholds
    assert np.nanmax(ref0.dist) < 1e-2 * px_thr and np.nanmax(ref0.rel) < 1e-2 * rel_thr
    assert np.allclose(ref0.avg, clean.depth.astype(np.float32), rtol=1e-2 * rel_thr)

    sc = G.consistency_scene(3)
    ref = G.ref_depth_consistency(sc.depth, sc.K, sc.E, px_thr, rel_thr)
    assert (ref.count[1][sc.patch] == 0).all(), "the scaled patch agrees with nobody"
    assert (ref.count[1][sc.hole] == 0).all() and (ref.avg[1][sc.hole] == 0).all()
    assert not ref.geom[1][:, sc.hole[0], sc.hole[1]].any()
    # view 0: pixels whose taps in view 1 stay clear of the patch and the hole keep the clean count; some lose view 1
    changed = ref.count[0] != ref0.count[0]
    assert 0 < changed.sum() < 0.15 * sc.W * sc.H and (ref.count[0][changed] == ref0.count[0][changed] - 1).all()
    bands = G.consistency_bands(sc, px_thr, rel_thr)
    share = bands.fragile.sum() / (sc.depth != 0).sum()
    print(f"gaps: dist {bands.gap_dist:.3e} px, rel {bands.gap_rel:.3e}, texel {bands.gap_px:.3e}, avg {bands.gap_avg:.3e}; "
          f"undecided share {share:.4f}")
    assert share <= 0.05
    assert (bands.r32.count == bands.r64.count)[~bands.fragile].all()


@pytest.mark.parametrize("N", [2, 16])
def test_consistency_restatement_small_scenes(N):
    sc = G.consistency_scene(N, 16, 12)
    ref = G.ref_depth_consistency(sc.depth, sc.K, sc.E, 1.0, 0.01)
    assert ref.count.max() <= N - 1 and ref.count.max() >= 1
    bands = G.consistency_bands(sc, 1.0, 0.01)
    assert (bands.r32.count == bands.r64.count)[~bands.fragile].all()
    # N = 2: the cap of the three-camera scene.  N = 16 repeats four cameras: a border pixel re-projects onto the image edge of its twin
    # view, where rounding decides whether a tap is inside -- the border pixels (52 of 192) may be undecided, no interior pixel is
    interior = np.zeros(sc.depth.shape, dtype=bool)
    interior[:, 1:-1, 1:-1] = True
    share = bands.fragile.sum() / (sc.depth != 0).sum()
    print(f"N={N}: undecided share {share:.4f}, interior {int((bands.fragile & interior).sum())}")
    assert not (bands.fragile & interior).any() if N == 16 else share <= 0.05
