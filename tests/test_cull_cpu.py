"""CPU: empty-ray culling (diner_compact_live_f32 / diner_expand_live_f32, predict_image(cull_empty=...)) -- the entries are declared,
exported and bound, the option is off by default, the Python reference of the compaction that the GPU tests compare against agrees
with a numpy one-liner, and the seeded test scene is fit for purpose: the oracle calls a large share of its rays empty and pins all
but a few of them one way or the other."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import cull_util as U
from tests.helpers import ROOT

ENTRIES = ("diner_compact_live_workspace_bytes", "diner_compact_live_f32", "diner_expand_live_f32")


def test_entries_declared_exported_and_bound():
    from diner_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6
    assert "cull.hip" in build.SOURCES
    assert lib.diner_compact_live_workspace_bytes(1) == 4 and lib.diner_compact_live_workspace_bytes(257) == 8
    assert lib.diner_compact_live_workspace_bytes(0) == 0 and lib.diner_compact_live_workspace_bytes(1 << 31) == 0


def test_entries_refuse_bad_arguments_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(16)                 # never dereferenced: the checks run before any device work

    def compact(stats=p, NR=4, K=8, r0=0, cap=4, rays_out=p, n_live=p, ws=p):
        return lib.diner_compact_live_f32(stats, 0.0, p, p, NR, K, r0, cap, rays_out, p, p, p, n_live, ws, None)

    for kw, what in ((dict(stats=None), b"null"), (dict(n_live=None), b"null"), (dict(ws=None), b"null"), (dict(NR=0), b"NR"),
                     (dict(K=0), b"K"), (dict(K=1025), b"K"), (dict(cap=-1), b"capacity"), (dict(rays_out=None), b"null output"),
                     (dict(r0=-1), b"ray ind"), (dict(r0=(1 << 31) - 2), b"ray ind")):
        assert compact(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())

    def expand(tiles=p, n=3, slot=p, bg=p, N=4, Cc=4, out=p):
        return lib.diner_expand_live_f32(tiles, n, slot, bg, N, Cc, out, None)

    for kw, what in ((dict(slot=None), b"null"), (dict(bg=None), b"null"), (dict(out=None), b"null"), (dict(tiles=None), b"tile"),
                     (dict(n=-1), b"tile"), (dict(N=0), b"N"), (dict(Cc=0), b"C ="), (dict(Cc=9), b"C =")):
        assert expand(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())


def test_culling_is_off_by_default():
    from diner_amd import evaluate, render, sweep
    from src.models.nerf_renderer import NeRFRendererDGS
    sig = inspect.signature(render.predict_image).parameters
    assert sig["cull_empty"].default is False and sig["cull_below"].default == 0.0
    assert inspect.signature(evaluate.write_prediction_folder).parameters["cull_empty"].default is False
    assert inspect.signature(sweep.create_cam_sweep).parameters["cull_empty"].default is False
    ren = NeRFRendererDGS()
    assert ren.cull_empty is False and ren.cull_below == 0.0
    ren.cull_empty = True                                   # a plain attribute, like white_bkgd
    assert ren.cull_empty is True and NeRFRendererDGS.cull_empty is False


@pytest.mark.parametrize("NR,K,cap,threshold", [(1, 1, 1, 0.0), (257, 5, 257, 0.0), (1000, 8, 1000, 0.5), (300, 4, 40, 0.0)])
def test_python_reference_compaction_agrees_with_numpy(NR, K, cap, threshold):
    g = torch.Generator().manual_seed(NR + K)
    stats = torch.rand(NR, 4, generator=g)
    stats[torch.rand(NR, generator=g) < 0.5, 1] = 0.0
    if NR > 2:
        stats[1, 1], stats[2, 1] = float("nan"), float("inf")
    rays, z = torch.randn(NR, 8, generator=g), torch.randn(NR, K, generator=g)
    ro, zo, li = torch.full((cap, 8), -7.0), torch.full((cap, K), -7.0), torch.full((cap,), -7, dtype=torch.int32)
    slot, n = U.ref_compact(stats, threshold, rays, z, 11, 3, ro, zo, li)
    keep = np.flatnonzero(~(stats[:, 1].numpy() <= np.float32(threshold)))               # the one-liner
    assert n == 3 + len(keep)
    fit = keep[:max(0, cap - 3)]
    assert np.array_equal(ro[3:3 + len(fit)].numpy(), rays.numpy()[fit]) and np.array_equal(zo[3:3 + len(fit)].numpy(), z.numpy()[fit])
    assert np.array_equal(li[3:3 + len(fit)].numpy(), fit + 11)
    assert (ro[:3] == -7).all() and (ro[3 + len(fit):] == -7).all() and (li[3 + len(fit):] == -7).all()
    want = np.full(NR, -1, dtype=np.int32)
    want[fit] = 3 + np.arange(len(fit))
    assert np.array_equal(slot.numpy(), want)
    if NR > 2:
        assert 1 in keep and 2 in keep                       # NaN and +inf are live
    # the expansion's indexing expression
    tiles, bg = torch.randn(cap, 5, generator=g), torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0])
    out = U.ref_expand(tiles, slot, bg).numpy()
    assert np.array_equal(out[want >= 0], tiles.numpy()[want[want >= 0]]) and (out[want < 0] == bg.numpy()).all()


@pytest.mark.parametrize("nv", [4, 6])
def test_scene_is_fit_for_purpose(nv):
    """Half the focal length on the seeded 48 x 40 scene: 20 % .. 80 % of the 1920 rays empty, at most 1 % of them unpinned."""
    case = U.scene_case(nv)
    v = case.verdict
    n = case.rays.shape[0]
    assert n == 1920
    empty, unpinned = int(v.empty.sum()), int(v.unpinned.sum())
    print(f"NV={nv}: {empty} of {n} rays empty, pinned dead {int(v.pinned_dead.sum())}, pinned live {int(v.pinned_live.sum())}, "
          f"unpinned {unpinned}")
    assert 0.2 * n <= empty <= 0.8 * n
    assert unpinned <= 0.01 * n
    assert (v.empty[v.pinned_dead]).all() and not v.empty[v.pinned_live].any()
