"""CPU: scoring clouds and meshes (cloud.hip, diner_amd.cloudmetrics, evaluate_geometry_folder) -- the entries are declared, exported,
bound and refuse bad arguments before any device work; the Python layers check their arguments before touching a device; the CLI
without --geometry is what it was; and the numpy restatement the GPU tests compare against (tests/cloud_util.py) is fit for purpose.

The last two tests exercise the restatement alone: they cannot fail without the feature.  They show that its exhaustive float32
search agrees with an independent k-d tree (scipy, when it imports) and that it reproduces scores computed by hand.  The first three do
fail without the feature, and so does every test of tests/test_cloud_gpu.py."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import cloud_util as CU
from tests.helpers import ROOT

ENTRIES = ("diner_cloud_grid_bytes", "diner_cloud_grid_order_offset", "diner_cloud_grid_build_f32", "diner_cloud_nearest_f32",
           "diner_cloud_reduce_workspace_bytes", "diner_cloud_reduce_f32")


def test_entries_declared_exported_and_bound():
    from diner_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "cloud.hip" in build.SOURCES
    assert lib.diner_cloud_grid_bytes(1000, 4, 5, 6) >= 1000 * 4 + 4 * 5 * 6 * 4
    assert lib.diner_cloud_grid_bytes(1000, 1024, 1024, 64) > 0 and lib.diner_cloud_grid_bytes(1, 1, 1, 1) > 0
    for dims in ((0, 4, 4), (4, 1025, 4), (4, 4, 0), (1024, 1024, 65), (512, 512, 512)):     # a 0 or 1025 side, more than 2^26 cells
        assert lib.diner_cloud_grid_bytes(1000, *dims) == 0, dims
    assert lib.diner_cloud_grid_bytes(0, 4, 4, 4) == 0 and lib.diner_cloud_grid_bytes(2 ** 31, 4, 4, 4) == 0
    at = lib.diner_cloud_grid_order_offset(1000, 4, 5, 6)
    assert at % 16 == 0 and 0 < at < lib.diner_cloud_grid_bytes(1000, 4, 5, 6)
    assert lib.diner_cloud_reduce_workspace_bytes(0) == 0 and lib.diner_cloud_reduce_workspace_bytes(3000) > 0


INF, NAN = float("inf"), float("nan")
BOX_REFUSALS = ((dict(NB=0), b"NB"), (dict(NB=2 ** 31), b"NB"), (dict(lo=(NAN, 0.0, 0.0)), b"lo"), (dict(lo=(0.0, INF, 0.0)), b"lo"),
                (dict(lo=None), b"lo"), (dict(h=0.0), b"cell"), (dict(h=-1.0), b"cell"), (dict(h=INF), b"cell"), (dict(h=NAN), b"cell"),
                (dict(dims=(0, 4, 4)), b"dims"), (dict(dims=(4, 1025, 4)), b"dims"), (dict(dims=(1024, 1024, 65)), b"dims"),
                (dict(xyz_b=None), b"null"), (dict(ws=None), b"null"), (dict(ws=C.c_void_p(24)), b"aligned"))
NEAREST_REFUSALS = BOX_REFUSALS + ((dict(NA=0), b"NA"), (dict(NA=-3), b"NA"), (dict(max_dist=0.0), b"max_dist"),
                                   (dict(max_dist=-1.0), b"max_dist"), (dict(max_dist=NAN), b"max_dist"), (dict(xyz_a=None), b"null"),
                                   (dict(d2=None), b"null"), (dict(idx=None), b"null"))
REDUCE_REFUSALS = ((dict(n=0), b"n ="), (dict(max_dist=0.0), b"max_dist"), (dict(max_dist=NAN), b"max_dist"), (dict(T=-1), b"T ="),
                   (dict(T=9), b"T ="), (dict(T=2, taus=(0.1, NAN)), b"threshold"), (dict(T=2, taus=(-0.1, 0.2)), b"threshold"),
                   (dict(T=1, taus=None), b"null"), (dict(d2=None), b"null"), (dict(idx=None), b"null"), (dict(ws=None), b"null"),
                   (dict(out=None), b"null"), (dict(na=None), b"normals"), (dict(nb_rows=0), b"nb_rows"))


def _floats(v):
    return None if v is None else (C.c_float * len(v))(*v)


def grid_entry(lib, which, p, **kw):
    """The return code of diner_cloud_grid_build_f32 ("build") or diner_cloud_nearest_f32 ("nearest") with one argument changed; p: a
    pointer that is never dereferenced.  Only the entry asked for is called: the other one would run."""
    a = dict(xyz_b=p, NB=100, lo=(0.0, 0.0, 0.0), h=0.1, dims=(4, 4, 4), ws=p, xyz_a=p, NA=50, order=None, max_dist=INF, d2=p, idx=p)
    a.update(kw)
    if which == "build":
        return lib.diner_cloud_grid_build_f32(a["xyz_b"], a["NB"], _floats(a["lo"]), a["h"], *a["dims"], a["ws"], None)
    return lib.diner_cloud_nearest_f32(a["xyz_b"], a["NB"], _floats(a["lo"]), a["h"], *a["dims"], a["ws"], a["xyz_a"], a["NA"], a["order"],
                                       a["max_dist"], a["d2"], a["idx"], None)


def reduce_entry(lib, p, **kw):
    a = dict(d2=p, idx=p, n=100, max_dist=INF, taus=(0.1, 0.2), T=0, na=p, nb=p, nb_rows=10, ws=p, out=p)
    a.update(kw)
    return lib.diner_cloud_reduce_f32(a["d2"], a["idx"], a["n"], a["max_dist"], _floats(a["taus"]), a["T"], a["na"], a["nb"], a["nb_rows"],
                                      a["ws"], a["out"], None)


def test_entries_refuse_bad_arguments_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(16)                 # never dereferenced: the checks run before any device work
    for kw, what in BOX_REFUSALS:
        assert grid_entry(lib, "build", p, **kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())
    for kw, what in NEAREST_REFUSALS:
        assert grid_entry(lib, "nearest", p, **kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())
    for kw, what in REDUCE_REFUSALS:
        assert reduce_entry(lib, p, **kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())


def test_python_layers_check_before_the_device():
    from diner_amd import cloudmetrics as CM
    from diner_amd import evaluate, ops
    x = torch.zeros(10, 3)
    # ops: shapes, dtypes and sizes are ValueError, a CPU tensor that passes them is the missing-device RuntimeError
    for kw in (dict(xyz_b=torch.zeros(10, 2)), dict(xyz_b=torch.zeros(0, 3)), dict(xyz_b=x.double()), dict(lo=(0.0, NAN, 0.0)),
               dict(lo=(0.0, 0.0)), dict(cell=0.0), dict(cell=INF), dict(dims=(0, 1, 1)), dict(dims=(1025, 1, 1)), dict(dims=(512, 512, 512)),
               dict(dims=(4, 4))):
        with pytest.raises(ValueError):
            ops.cloud_grid(**{**dict(xyz_b=x, lo=(0.0, 0.0, 0.0), cell=0.1, dims=(4, 4, 4)), **kw})
    with pytest.raises(RuntimeError):
        ops.cloud_grid(x, (0.0, 0.0, 0.0), 0.1, (4, 4, 4))
    grid = ops.CloudGridData(x, torch.zeros(16, dtype=torch.uint8), (C.c_float * 3)(), 0.1, (4, 4, 4), torch.zeros(10, dtype=torch.int32))
    for kw in (dict(grid=None), dict(xyz_a=torch.zeros(3)), dict(xyz_a=x.double()), dict(max_dist=0.0), dict(max_dist=NAN),
               dict(order=torch.zeros(10, dtype=torch.int64)), dict(order=torch.zeros(9, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.cloud_nearest(**{**dict(grid=grid, xyz_a=x, max_dist=INF, order=None), **kw})
    with pytest.raises(RuntimeError):
        ops.cloud_nearest(grid, x)
    d2, idx = torch.zeros(10), torch.zeros(10, dtype=torch.int32)
    for kw in (dict(idx=idx[:5]), dict(idx=idx.long()), dict(d2=d2.double()), dict(max_dist=-1.0), dict(thresholds=(0.1,) * 9),
               dict(thresholds=(-0.1,)), dict(thresholds=(NAN,)), dict(normals_a=x), dict(normals_a=x[:5], normals_b=x),
               dict(normals_a=x, normals_b=torch.zeros(4, 2))):
        with pytest.raises(ValueError):
            ops.cloud_reduce(**{**dict(d2=d2, idx=idx), **kw})
    with pytest.raises(RuntimeError):
        ops.cloud_reduce(d2, idx)
    # cloudmetrics
    for kw in (dict(pred_xyz=torch.zeros(10, 4)), dict(gt_xyz=x.half()), dict(pred_xyz=x.numpy()), dict(max_dist=0.0), dict(thresholds=(-1.0,)),
               dict(pred_normals=torch.zeros(9, 3)), dict(bounds=((0, 0, 0), (1, 1))), dict(bounds=((1, 0, 0), (0, 1, 1))), dict(thin=0.0)):
        with pytest.raises(ValueError):
            CM.cloud_scores(**{**dict(pred_xyz=x, gt_xyz=x), **kw})
    for call in (lambda: CM.cloud_scores(x, x), lambda: CM.CloudGrid(x), lambda: CM.mesh_scores((x, x, None, None), x),
                 lambda: CM.write_error_ply(os.devnull, x, torch.zeros(10), 1.0)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    with pytest.raises(ValueError):
        CM.CloudGrid(torch.zeros(0, 3))
    # the choice of box: within the limits, no finer than max_dist / 2, a few points per cell of a surface
    cell, dims = CM.grid_box((0, 0, 0), (1, 1, 1), 7_700_000)
    assert max(dims) <= 1024 and dims[0] * dims[1] * dims[2] <= 2 ** 26 and 2e-4 < cell < 4e-3
    assert CM.grid_box((0, 0, 0), (1, 1, 1), 1000, max_dist=0.5)[0] >= 0.25
    assert CM.grid_box((0, 0, 0), (0, 0, 0), 1) == (1.0, (1, 1, 1)) and CM.grid_box((0, 0, 0), (1, 1, 1), 10, cell=1e-6)[1][0] <= 1024
    assert CM.threshold_key("fscore", 0.01) == "fscore@0.01" == CU.threshold_key("fscore", 0.01)
    # evaluate: argument errors and an empty folder come before the device
    sig = inspect.signature(evaluate.evaluate_geometry_folder).parameters
    assert sig["pred_suffix"].default == ".ply" and sig["gt_suffix"].default == "-gt.ply" and sig["max_dist"].default == INF
    assert sig["thresholds"].default == () and sig["thin"].default is None and sig["device"].default is None
    for kw in (dict(max_dist=0.0), dict(thresholds=(-1.0,)), dict(thin=-1.0)):
        with pytest.raises(ValueError):
            evaluate.evaluate_geometry_folder(ROOT, ROOT, **kw)
    with pytest.raises(FileNotFoundError):
        evaluate.evaluate_geometry_folder(os.path.join(ROOT, "include"), os.path.join(ROOT, "include"))


def test_cli_without_geometry_is_what_it_was(monkeypatch, tmp_path):
    from diner_amd import evaluate
    calls = []
    monkeypatch.setattr(evaluate, "evaluate_folder", lambda *a, **k: calls.append(("images", a, k)) or {"psnr": 1.0})
    monkeypatch.setattr(evaluate, "evaluate_geometry_folder", lambda *a, **k: calls.append(("geometry", a, k)) or {"chamfer": 2.0})
    evaluate.main(["--eval_path", str(tmp_path)])
    assert calls == [("images", (tmp_path / "visualizations", tmp_path), dict(show_tqdm=True))]
    calls.clear()
    (tmp_path / "visualizations").mkdir()
    evaluate.main(["--eval_path", str(tmp_path), "--geometry", "--max_dist", "0.5", "--threshold", "0.01", "--threshold", "0.02"])
    assert calls == [("geometry", (tmp_path / "visualizations", tmp_path), dict(max_dist=0.5, thresholds=[0.01, 0.02], thin=None))]
    args = evaluate._parser().parse_args(["--eval_path", "x"])
    assert args.geometry is False and args.max_dist == INF and args.threshold == [] and args.thin is None


# ------------------------------------------------------------------------------------------------- the restatement alone
def test_restatement_agrees_with_a_kd_tree():
    """Cannot fail without the feature: the exhaustive float32 search of tests/cloud_util.py against scipy's k-d tree (float64) on the
    test clouds -- the neighbour distance to 1e-6 relative."""
    spatial = pytest.importorskip("scipy.spatial")
    for name in ("sphere", "duplicates", "lattice", "na257"):
        a, b = CU.exactness_clouds()[name][:2]
        d2, idx = CU.exactness_reference(name, math.inf)
        d, _ = spatial.cKDTree(b.astype(np.float64)).query(a.astype(np.float64))
        assert (idx >= 0).all() and np.allclose(np.sqrt(d2.astype(np.float64)), d, rtol=1e-6, atol=1e-9), name
        d_cap, _ = spatial.cKDTree(b.astype(np.float64)).query(a.astype(np.float64), distance_upper_bound=0.03)
        d2c, idxc = CU.exactness_reference(name, 0.03)
        near_cap = np.abs(d - 0.03) < 1e-6
        assert ((idxc >= 0) == np.isfinite(d_cap))[~near_cap].all(), name


def test_restatement_reproduces_hand_computed_scores():
    """Cannot fail without the feature: two four-point clouds scored by hand.  pred -> gt distances 0, 0, 2 (a tie between gt 2 and 3:
    index 2), 4; gt -> pred 1, 0, 0, 2."""
    d2, idx = CU.ref_nearest(CU.HAND_PRED, CU.HAND_GT)
    assert d2.tolist() == [0.0, 0.0, 4.0, 16.0] and idx.tolist() == [2, 1, 2, 1]
    d2, idx = CU.ref_nearest(CU.HAND_GT, CU.HAND_PRED)
    assert d2.tolist() == [1.0, 0.0, 0.0, 4.0] and idx.tolist() == [0, 1, 0, 2]
    s = CU.ref_scores(CU.HAND_PRED, CU.HAND_GT)
    assert (s["accuracy"], s["completeness"], s["chamfer"]) == (1.5, 0.75, 1.125) and (s["matched_pred"], s["matched_gt"]) == (4, 4)
    assert (s["accuracy_median"], s["completeness_median"]) == (0.0, 0.0)
    s = CU.ref_scores(CU.HAND_PRED, CU.HAND_GT, max_dist=3.0, thresholds=(1.0,))
    assert s["accuracy"] == pytest.approx(2.0 / 3.0) and s["completeness"] == 0.75 and (s["matched_pred"], s["matched_gt"]) == (3, 4)
    assert (s["precision@1"], s["recall@1"]) == (0.5, 0.75) and s["fscore@1"] == pytest.approx(0.6)
    assert np.isinf(s["dist_pred"][3]) and s["dist_gt"].tolist() == [1.0, 0.0, 0.0, 2.0]
    # normals: |n . n'| over matched pairs, both directions
    n = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float32)
    s = CU.ref_scores(CU.HAND_PRED, CU.HAND_GT, pred_normals=n, gt_normals=n[::-1].copy())
    # pred i -> gt idx [2,1,2,1]: n_gt = n[::-1] -> rows [n1, n2, n1, n2]: dots 0, 0, 0, 0; gt -> pred [0,1,0,2]: gt normals n3,n2,n1,n0
    assert s["normal_consistency"] == pytest.approx(0.5 * (0.0 + (1.0 + 0.0 + 0.0 + 0.0) / 4.0))
    # bounds and thin: the point at x = 5 leaves; one point per unit cell, the smallest index
    assert CU.ref_kept(CU.HAND_PRED, bounds=((-1, -1, -1), (3, 3, 3))).tolist() == [0, 1, 2]
    assert CU.ref_kept(np.array([[0.1, 0.1, 0.1], [0.9, 0.2, 0.3], [1.1, 0, 0], [np.nan, 0, 0], [-0.1, 0, 0]], np.float32), thin=1.0).tolist() == [0, 2, 4]
    # nothing matched: nan scores, zero counts
    s = CU.ref_scores(CU.HAND_PRED + 100.0, CU.HAND_GT, max_dist=1.0, thresholds=(0.5,))
    assert math.isnan(s["accuracy"]) and math.isnan(s["chamfer"]) and s["matched_pred"] == 0 and s["precision@0.5"] == 0.0 and s["fscore@0.5"] == 0.0
