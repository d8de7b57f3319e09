"""CPU: ray-casting the TSDF volume (raycast.hip, TsdfVolume.raycast) -- the entries are declared, exported, bound and refuse bad
arguments before any device work; the Python layer is off by default and checks its arguments before touching a device; and the numpy
restatement the GPU tests compare against (tests/raycast_util.py) is fit for purpose.

The last three tests exercise the restatement alone: they cannot fail without the feature.  They show that the definition is one
fp32 can carry -- the rays whose outcome it may decide the other way stay under 2 % of a view -- that it finds the sphere, and that
leaving out the samples of 0-bricks changes no bit.  The first three do fail without it, and so does every test of
tests/test_raycast_gpu.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import raycast_util as RU
from tests import surface_util as S
from tests.helpers import ROOT

ENTRIES = ("diner_tsdf_raycast_f32", "diner_tsdf_bricks", "diner_tsdf_bricks_bytes")


def test_entries_declared_exported_and_bound():
    from diner_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "raycast.hip" in build.SOURCES
    assert lib.diner_tsdf_bricks_bytes(16, 16, 16) == 8 and lib.diner_tsdf_bricks_bytes(17, 13, 9) == 2 * 2 * 1
    assert lib.diner_tsdf_bricks_bytes(2, 2, 2) == 1 and lib.diner_tsdf_bricks_bytes(67, 33, 31) == 9 * 4 * 4
    assert lib.diner_tsdf_bricks_bytes(1, 16, 16) == 0 and lib.diner_tsdf_bricks_bytes(16, 1025, 16) == 0


REFUSALS = ((dict(V=0), b"views"), (dict(V=17), b"views"), (dict(dims=(1, 8, 8)), b"dimension"), (dict(dims=(8, 1025, 8)), b"dimension"),
            (dict(voxel=0.0), b"voxel"), (dict(voxel=-1.0), b"voxel"), (dict(step=0.0), b"step"), (dict(step=-0.1), b"step"),
            (dict(step=float("inf")), b"step"), (dict(step=float("nan")), b"step"), (dict(zfar=float("inf")), b"zfar"),
            (dict(zfar=float("nan")), b"zfar"), (dict(znear=1.0, zfar=1.0), b"zfar"), (dict(znear=2.0, zfar=1.0), b"zfar"),
            (dict(znear=-0.1), b"znear"), (dict(step=1e-7, zfar=1.0), b"samples"), (dict(color4=None), b"rgb_out"),
            (dict(tsdf=None), b"null"), (dict(wsum=None), b"null"), (dict(zdepth=None), b"null"), (dict(Km=None), b"null"),
            (dict(E=None), b"null"), (dict(origin=None), b"null"))


def raycast_entry(lib, ptrs, cams, **kw):
    """diner_tsdf_raycast_f32 with one argument changed: ptrs = (tsdf, wsum, color4, zdepth, normal, rgb, weight), cams = (Km, E)."""
    a = dict(tsdf=ptrs[0], wsum=ptrs[1], color4=ptrs[2], zdepth=ptrs[3], normal=ptrs[4], rgb=ptrs[5], weight=ptrs[6], Km=cams[0],
             E=cams[1], origin=(C.c_float * 3)(0.0, 0.0, 0.0), dims=(8, 8, 8), voxel=0.1, V=1, znear=0.0, zfar=2.0, step=0.05)
    a.update(kw)
    return lib.diner_tsdf_raycast_f32(a["tsdf"], a["wsum"], a["color4"], *a["dims"], a["origin"], a["voxel"], None, a["Km"], a["E"], a["V"],
                                      4, 4, a["znear"], a["zfar"], a["step"], 0.0, a["zdepth"], a["normal"], a["rgb"], a["weight"], None)


def host_cameras():
    Km = (C.c_float * (9 * 16))()
    E = (C.c_float * (16 * 16))()
    for v in range(16):
        Km[9 * v], Km[9 * v + 4], Km[9 * v + 8], Km[9 * v + 2], Km[9 * v + 5] = 4.0, 4.0, 1.0, 2.0, 2.0
        for a in range(4):
            E[16 * v + 5 * a] = 1.0
    return Km, E


def test_entries_refuse_bad_arguments_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(16)                 # never dereferenced: the checks run before any device work
    for kw, what in REFUSALS:
        assert raycast_entry(lib, (p,) * 7, host_cameras(), **kw) == _lib.E_INVALID and what in lib.diner_last_error(), \
            (kw, lib.diner_last_error())
    # a camera without a focal length has no finite number of samples on a ray
    Km, E = host_cameras()
    Km[0] = 0.0
    assert raycast_entry(lib, (p,) * 7, (Km, E)) == _lib.E_INVALID and b"samples" in lib.diner_last_error()
    for dims, what in (((1, 8, 8), b"dimension"), ((8, 8, 2048), b"dimension")):
        assert lib.diner_tsdf_bricks(p, p, *dims, 0.0, p, None) == _lib.E_INVALID and what in lib.diner_last_error()
    assert lib.diner_tsdf_bricks(p, p, 8, 8, 8, 0.0, None, None) == _lib.E_INVALID and b"null" in lib.diner_last_error()
    assert lib.diner_tsdf_bricks(p, p, 8, 8, 8, float("nan"), p, None) == _lib.E_INVALID and b"min_weight" in lib.diner_last_error()


def test_python_layer_is_opt_in_and_checks_before_the_device():
    from diner_amd import evaluate, ops, surface
    assert inspect.signature(evaluate.write_prediction_folder).parameters["write_volume_view"].default is False
    sig = inspect.signature(surface.sources_through_volume).parameters
    assert sig["carve"].default is False and inspect.signature(surface.mesh_from_sources).parameters["carve"].default is True
    sig = inspect.signature(surface.TsdfVolume.raycast).parameters
    assert sig["zfar"].default is None and sig["step"].default is None and sig["znear"].default == 0.0 and sig["accelerate"].default is True
    t = torch.ones(8, 8, 8)
    Km, E = torch.eye(3)[None], torch.eye(4)[None]
    ok = dict(W=4, H=4, znear=0.0, zfar=2.0, step=0.05)
    for kw, exc in ((dict(step=0.0), ValueError), (dict(step=float("inf")), ValueError), (dict(zfar=float("inf")), ValueError),
                    (dict(zfar=0.0), ValueError), (dict(znear=-1.0), ValueError), (dict(W=0), ValueError), ({}, RuntimeError)):
        with pytest.raises(exc):
            ops.tsdf_raycast(t, t, None, (0, 0, 0), 0.1, Km, E, **{**ok, **kw})
    with pytest.raises(ValueError):
        ops.tsdf_raycast(t, t, None, (0, 0, 0), 0.1, Km.expand(17, -1, -1), E.expand(17, -1, -1), **ok)
    with pytest.raises(ValueError):
        ops.tsdf_raycast(t, t, None, (0, 0, 0), 0.1, Km, E, bricks=torch.zeros(2, 2, 2, dtype=torch.uint8), **ok)
    with pytest.raises(ValueError):
        ops.tsdf_raycast(t, t[:4], None, (0, 0, 0), 0.1, Km, E, **ok)
    with pytest.raises(ValueError):
        ops.tsdf_bricks(t, t[:4])
    with pytest.raises(RuntimeError):
        ops.tsdf_bricks(t, t)
    with pytest.raises(RuntimeError):
        surface.sources_through_volume({}, device="cpu")


# ------------------------------------------------------------------------------------------------- the restatement alone
@pytest.mark.parametrize("n,carve,step_voxels", RU.MAIN_CASES)
def test_restatement_band_is_small(n, carve, step_voxels):
    p = RU.cast_pair(n, carve, step_voxels)
    per_view = p.band.reshape(3, -1).mean(axis=1)
    both = p.r64.hit & p.r32.hit & ~p.band
    gap = float(np.abs(p.r32.zdepth.astype(np.float64) - p.r64.zdepth)[both].max())
    print(f"n={n} carve={carve} step={step_voxels} voxel: band {p.band.sum(axis=(1, 2)).tolist()} of {S.CAM_W * S.CAM_H} rays a view, "
          f"hits {p.r64.hit.sum(axis=(1, 2)).tolist()}, ended from behind {p.r64.behind.sum(axis=(1, 2)).tolist()}, depth gap {gap:.2e}")
    assert (per_view <= 0.02).all()
    assert (p.r64.hit.sum(axis=(1, 2)) > 300).all()
    assert (p.r64.zdepth[~p.r64.hit] == 0).all() and (p.r64.zdepth[p.r64.hit] > 0).all()
    if not carve:                       # the "solid met out of unknown space is a miss" rule is exercised
        assert (p.r64.behind.sum(axis=(1, 2)) >= 14).all()


@pytest.mark.parametrize("n,step_voxels", [(16, 0.5), (16, 1.0), (24, 0.5), (24, 1.0)])
def test_restatement_finds_the_carved_sphere(n, step_voxels):
    p = RU.cast_pair(n, True, step_voxels)
    for v, eye in enumerate((S.EYES[0], S.EYES[4], RU.NOVEL_EYE)):
        d, _, _ = S.sphere_maps(S.look_at(eye), p.K[v].astype(np.float64), S.CAM_W, S.CAM_H)
        m = p.r64.hit[v] & (d > 0)
        err = np.abs(p.r64.zdepth[v] - d)[m] / p.vol.voxel
        print(f"n={n} step={step_voxels} view {v}: {int(m.sum())} common hits, error mean {err.mean():.3f} max {err.max():.3f} voxel")
        assert err.mean() < 0.5


def test_restatement_with_and_without_a_brick_mask():
    """A volume of several bricks an axis, most of them 0: the restatement that never looks at a sample of a 0-brick gives the bits of
    the one that looks at every sample, in float32 and in float64."""
    dims, voxel, origin = (67, 33, 31), 0.03, (-1.0, -0.49, -0.46)
    t = S.sphere_tsdf(dims, origin, voxel, 0.4, 0.09)
    w = np.ones_like(t)
    bricks = RU.ref_bricks(t, w)
    assert bricks.shape == (4, 4, 9) and 0 < int(bricks.sum()) < bricks.size
    Kmat, E = RU.cameras(((1.6, 0.2, 0.1), (-0.8, 0.1, 0.05)))             # outside the volume, and inside it (in free space)
    for dtype in (np.float32, np.float64):
        a = RU.ref_raycast(t, w, None, origin, voxel, Kmat, E, S.CAM_H, S.CAM_W, 0.0, 3.0, 0.015, dtype=dtype)
        b = RU.ref_raycast(t, w, None, origin, voxel, Kmat, E, S.CAM_H, S.CAM_W, 0.0, 3.0, 0.015, bricks=bricks, dtype=dtype)
        assert a.hit.sum() > 300
        for k in ("zdepth", "normal", "weight", "hit", "n_term"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
