"""GPU: scoring clouds and meshes -- diner_cloud_grid_build_f32 / diner_cloud_nearest_f32 / diner_cloud_reduce_f32 through ops,
diner_amd.cloudmetrics and evaluate.evaluate_geometry_folder, against the numpy restatement of tests/cloud_util.py.

  1  exactness: np.array_equal on the bits of d2 and on idx against exhaustive search, per cloud and per cap;
  2  the grid's dims and the order in which the threads take the queries change no bit;
  3  two builds and two searches give the same bits; the grid's order is a permutation in cell order;
  4  the sums of cloud_reduce: counts equal, float64 sums to 1e-12 relative; nothing matched -> zeros, and nan scores;
  5  cloud_scores with bounds, thin and normals against the restatement; swapping the clouds swaps accuracy and completeness;
  6  a surface-nets sphere scored against analytic points;
  7  refusals leave sentinel-filled outputs untouched;
  8  evaluate_geometry_folder, write_error_ply, rendering untouched.

The largest search is 3000 queries against 2500 points."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from tests import cloud_util as CU
from tests import surface_util as S

pytestmark = pytest.mark.gpu
SEED = 20261019


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()              # a copy: the shared clouds are read-only


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def search(ops, a, b, lo, cell, dims, cap, order=None):
    grid = ops.cloud_grid(cuda(b), lo, cell, dims)
    d2, idx = ops.cloud_nearest(grid, cuda(a), cap, order=order)
    return d2.cpu().numpy(), idx.cpu().numpy()


def assert_same(got, ref, label):
    d2, idx = got
    rd2, ridx = ref
    wrong = np.nonzero((d2.view(np.int32) != rd2.view(np.int32)) | (idx != ridx))[0]
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and wrong.size == 0, \
        f"{label}: {wrong.size} of {idx.size} queries differ, first {wrong[:5].tolist()}: got {d2[wrong[:5]].tolist()} {idx[wrong[:5]].tolist()}, " \
        f"expected {rd2[wrong[:5]].tolist()} {ridx[wrong[:5]].tolist()}"


# -------------------------------------------------------------------------------------------------------------------- 1 exactness
@pytest.mark.parametrize("name", ["sphere", "duplicates", "lattice", "far", "one_target", "na1", "na63", "na64", "na65", "na257", "nonfinite"])
def test_nearest_equals_exhaustive_search(ops, name):
    a, b, lo, cell, dims = CU.exactness_clouds()[name]
    for cap in CU.CAPS:
        ref = CU.exactness_reference(name, cap)
        got = search(ops, a, b, lo, cell, dims, cap)
        print(f"{name}: NA {len(a)} NB {len(b)} grid {dims} cell {cell:g} cap {cap}: {int((ref[1] >= 0).sum())} matched")
        assert_same(got, ref, f"{name} cap {cap}")
    if name == "duplicates":
        assert (CU.exactness_reference(name, math.inf)[0][-300:] == 0).all()     # the tie rule is exercised: exact hits on doubled points
    if name == "nonfinite":
        d2, idx = CU.exactness_reference(name, math.inf)
        assert (idx[[0, 63, 64, 399]] == -1).all() and np.isinf(d2[[0, 63, 64, 399]]).all() and not np.isin(idx, [5, 17, 40, 899]).any()


# ------------------------------------------------------------------------------------------------------------ 2 cell independence
def test_dims_and_query_order_change_no_bit(ops):
    a, b = CU.exactness_clouds()["sphere"][:2]
    lo = b.min(axis=0)
    ta = cuda(a)
    own = ops.cloud_grid(ta, a.min(axis=0), 0.02, CU.box_of(a, 0.02)[2]).order                   # the queries in the cell order of their own grid
    shuffled = torch.from_numpy(np.random.default_rng(SEED).permutation(len(a)).astype(np.int32)).cuda()
    for cap in (math.inf, 0.03):
        ref = CU.exactness_reference("sphere", cap)
        outs = []
        # the last three cover the cloud in part only; 128 x 128 x 32 cells are 513 tiles of the scan: three passes over the tile sums
        for dims, cell in (((1, 1, 1), 1.0), ((3, 2, 5), 0.11), ((17, 9, 33), 0.017), ((128, 128, 32), 0.0045)):
            for order in (None, own, shuffled):
                got = search(ops, a, b, lo, cell, dims, cap, order=order)
                assert_same(got, ref, f"dims {dims} cap {cap} order {'no' if order is None else 'yes'}")
                outs.append(got)
        for got in outs[1:]:
            assert np.array_equal(got[0].view(np.int32), outs[0][0].view(np.int32)) and np.array_equal(got[1], outs[0][1])


# ------------------------------------------------------------------------------------------------------------- 3 reproducibility
def test_two_builds_give_the_same_bits(ops):
    a, b, lo, cell, dims = CU.exactness_clouds()["nonfinite"]
    tb, ta = cuda(b), cuda(a)
    runs = []
    for _ in range(2):
        grid = ops.cloud_grid(tb, lo, cell, dims)
        runs.append(ops.cloud_nearest(grid, ta, 0.03) + (grid.order.clone(),))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
    # the order: a permutation, sorted by cell, the non-finite points behind the last cell
    order = runs[0][2].cpu().numpy()
    assert order.dtype == np.int32 and np.array_equal(np.sort(order), np.arange(len(b)))
    ok = np.isfinite(b).all(axis=1)
    with np.errstate(invalid="ignore"):
        c = np.floor((b - lo) / np.float32(cell))
    c = np.stack([np.clip(c[:, k], 0, dims[k] - 1) for k in range(3)], axis=1)
    cells = np.where(ok, (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0], dims[0] * dims[1] * dims[2])
    assert (np.diff(cells[order]) >= 0).all() and set(order[-4:].tolist()) == {5, 17, 40, 899}
    assert np.array_equal(np.sort(runs[1][2].cpu().numpy()), np.arange(len(b)))


# ------------------------------------------------------------------------------------------------------------------------ 4 reduce
def test_reduce_against_restatement(ops):
    a, b, lo, cell, dims = CU.exactness_clouds()["sphere"]
    _, na = CU.sphere_cloud(3000, 1, with_normals=True)
    _, nb = CU.sphere_cloud(2500, 2, with_normals=True)
    taus = (0.005, 0.01, 0.02, 0.0, 0.5, 0.011, 0.012, 0.013)
    for cap, n_taus, normals in ((math.inf, 8, True), (0.03, 3, True), (0.012, 2, False), (0.001, 1, True), (1e-6, 2, True)):
        d2, idx = CU.exactness_reference("sphere", math.inf)                       # searched without a cap: the reduce applies it
        ref = CU.ref_reduce(d2, idx, cap, taus[:n_taus], na if normals else None, nb if normals else None)
        args = (cuda(d2), cuda(idx), cap, taus[:n_taus], cuda(na) if normals else None, cuda(nb) if normals else None)
        out = ops.cloud_reduce(*args)
        again = ops.cloud_reduce(*args)
        assert out.dtype == torch.float64 and tuple(out.shape) == (11,) and torch.equal(out.view(torch.int64), again.view(torch.int64))
        got = out.cpu().tolist()
        print(f"cap {cap}: matched {got[0]:.0f} of {len(d2)}, sum {got[1]:.17g} (numpy {ref['sum_dist']:.17g}), normals {got[2]:.17g} "
              f"({ref['sum_normal']:.17g}), counts {got[3:3 + n_taus]}")
        assert got[0] == ref["matched"] and got[3:3 + n_taus] == ref["counts"] and got[3 + n_taus:] == [0.0] * (8 - n_taus)
        assert got[1] == pytest.approx(ref["sum_dist"], rel=1e-12, abs=0.0) and got[2] == pytest.approx(ref["sum_normal"], rel=1e-12, abs=0.0)
        if cap == 1e-6:
            assert got[:3] == [0.0, 0.0, 0.0] and ref["matched"] == 0
    # unmatched entries (idx -1) never count, whatever their d2
    d2 = torch.tensor([0.0, 1.0, 4.0, float("inf"), float("nan")], device="cuda")
    idx = torch.tensor([0, -1, 3, -1, 2], dtype=torch.int32, device="cuda")
    assert ops.cloud_reduce(d2, idx, thresholds=(1.5,)).cpu().tolist()[:4] == [2.0, 2.0, 0.0, 1.0]


def test_scores_with_nothing_matched_are_nan(ops):
    from diner_amd import cloudmetrics as CM
    a, b = CU.exactness_clouds()["sphere"][:2]
    s = CM.cloud_scores(cuda(a + np.float32(10.0)), cuda(b), max_dist=0.5, thresholds=(0.1,))
    assert (s["matched_pred"], s["matched_gt"], s["n_pred"], s["n_gt"]) == (0, 0, 3000, 2500)
    for k in ("accuracy", "completeness", "chamfer", "accuracy_median", "completeness_median"):
        assert math.isnan(s[k]), k
    assert s["precision@0.1"] == s["recall@0.1"] == s["fscore@0.1"] == 0.0
    assert bool(torch.isinf(s["dist_pred"]).all()) and bool(torch.isinf(s["dist_gt"]).all())
    # a cloud that bounds empties scores nan as well, and is no error
    s = CM.cloud_scores(cuda(a), cuda(b), bounds=((5, 5, 5), (6, 6, 6)), thresholds=(0.1,))
    assert (s["n_pred"], s["n_gt"]) == (0, 0) and math.isnan(s["chamfer"]) and math.isnan(s["fscore@0.1"]) and s["dist_pred"].numel() == 0


# ------------------------------------------------------------------------------------------------------------------ 5 cloud_scores
SCORE_KEYS = ("accuracy", "completeness", "chamfer", "accuracy_median", "completeness_median", "normal_consistency")


def test_cloud_scores_against_restatement(ops):
    from diner_amd import cloudmetrics as CM
    a, na = CU.sphere_cloud(3000, 1, with_normals=True)
    b, nb = CU.sphere_cloud(2500, 2, with_normals=True)
    a, b = a.copy(), b.copy()
    a[7], b[11, 1] = np.nan, np.inf                                               # dropped, on both sides
    taus = (0.005, 0.01, 0.02)
    for kw in (dict(), dict(max_dist=0.015), dict(bounds=((-0.3, -0.3, -0.05), (0.3, 0.1, 0.3)), thin=0.02, max_dist=0.03), dict(thin=0.05)):
        ref = CU.ref_scores(a, b, thresholds=taus, pred_normals=na, gt_normals=nb, **kw)
        got = CM.cloud_scores(cuda(a), cuda(b), thresholds=taus, pred_normals=cuda(na), gt_normals=cuda(nb), **kw)
        swapped = CM.cloud_scores(cuda(b), cuda(a), thresholds=taus, pred_normals=cuda(nb), gt_normals=cuda(na), **kw)
        print(kw, {k: got[k] for k in ("n_pred", "n_gt", "matched_pred", "matched_gt") + SCORE_KEYS})
        assert ref["n_pred"] < 3000 and ref["n_gt"] < 2500
        for side in ("pred", "gt"):                                                # the same kept points, the same distances
            assert np.array_equal(got["index_" + side].cpu().numpy(), ref["index_" + side])
            assert np.allclose(got["dist_" + side].cpu().numpy(), ref["dist_" + side], rtol=1e-6, atol=0.0)     # inf where unmatched
        for k in ("n_pred", "n_gt", "matched_pred", "matched_gt"):
            assert got[k] == ref[k] and isinstance(got[k], int), k
        for k in SCORE_KEYS:
            assert isinstance(got[k], float) and got[k] == pytest.approx(ref[k], rel=1e-6, abs=0.0), k
        for t in taus:
            for name in ("precision", "recall", "fscore"):
                assert got[CU.threshold_key(name, t)] == ref[CU.threshold_key(name, t)], (name, t)
            assert swapped[CU.threshold_key("precision", t)] == got[CU.threshold_key("recall", t)]
        assert swapped["accuracy"] == got["completeness"] and swapped["completeness"] == got["accuracy"]
        assert swapped["accuracy_median"] == got["completeness_median"] and swapped["matched_pred"] == got["matched_gt"]
        assert torch.equal(bits(swapped["dist_gt"]), bits(got["dist_pred"]))
    # without one of the normal sets there is no normal_consistency; CloudGrid.nearest is the same search
    assert "normal_consistency" not in CM.cloud_scores(cuda(a), cuda(b), pred_normals=cuda(na))
    grid = CM.CloudGrid(cuda(b), max_dist=0.03)
    dist, idx = grid.nearest(cuda(a))
    rd2, ridx = CU.ref_nearest(a, b, 0.03)
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), ridx) and grid.n_finite == 2499
    assert np.allclose(dist.cpu().numpy(), np.sqrt(rd2), rtol=1e-6, atol=0.0) and grid.cell >= 0.015


# -------------------------------------------------------------------------------------------------------------------- 6 end to end
def fibonacci_sphere(n, radius):
    i = np.arange(n) + 0.5
    phi, theta = np.arccos(1.0 - 2.0 * i / n), math.pi * (1.0 + 5.0 ** 0.5) * i
    u = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    return (u * radius).astype(np.float32), u.astype(np.float32)


def test_mesh_scores_on_the_sphere(ops):
    """A 33^3 sphere TSDF, its surface-nets mesh scored against 4000 analytic points.  Surface-nets vertices lie within a cell of the
    zero crossing, so: accuracy < 1 voxel, completeness < 1 voxel + the spacing of the samples (sqrt(area / n)), F-score at 1 voxel
    > 0.99, normal consistency > 0.95.  The float64 restatement of surface nets (tests/surface_util.py) scored by tests/cloud_util.py
    gives accuracy 0.0055, completeness 0.0083 (voxel 0.025, spacing 0.014), F-score 1.0 and normal consistency 0.9994: no bound needed
    widening."""
    from diner_amd import cloudmetrics as CM
    from diner_amd.surface import Mesh
    dims, voxel, origin, radius = (33, 33, 33), 0.025, S.ORIGIN, S.RADIUS
    t = S.sphere_tsdf(dims, origin, voxel, radius, 3 * voxel)
    m = ops.surface_extract(cuda(t), cuda(np.ones_like(t)), None, origin, voxel)
    gt, gn = fibonacci_sphere(4000, radius)
    spacing = math.sqrt(4.0 * math.pi * radius * radius / 4000)
    s = CM.mesh_scores(Mesh(m.vertices, m.normals, None, m.faces), cuda(gt), thresholds=(voxel,), gt_normals=cuda(gn))
    r = S.ref_surface_nets(t, np.ones_like(t), None, origin, voxel)
    ref = CU.ref_scores(r.vertices.astype(np.float32), gt, thresholds=(voxel,), pred_normals=r.normals.astype(np.float32), gt_normals=gn)
    key = CU.threshold_key("fscore", voxel)
    print(f"{s['n_pred']} vertices: accuracy {s['accuracy']:.5f} ({ref['accuracy']:.5f}), completeness {s['completeness']:.5f} "
          f"({ref['completeness']:.5f}), fscore {s[key]:.4f} ({ref[key]:.4f}), normal consistency {s['normal_consistency']:.5f} "
          f"({ref['normal_consistency']:.5f}); voxel {voxel}, spacing {spacing:.4f}")
    assert s["n_pred"] == r.n_vertices > 1000 and s["n_gt"] == 4000
    assert ref["accuracy"] < voxel and ref["completeness"] < voxel + spacing and ref[key] > 0.99 and ref["normal_consistency"] > 0.95
    assert s["accuracy"] < voxel and s["completeness"] < voxel + spacing and s[key] > 0.99 and s["normal_consistency"] > 0.95


# ---------------------------------------------------------------------------------------------------------------------- 7 refusals
def test_refusals_touch_nothing(ops):
    from diner_amd import _lib
    from tests.test_cloud_cpu import BOX_REFUSALS, NEAREST_REFUSALS, REDUCE_REFUSALS, grid_entry, reduce_entry
    lib = _lib.load()
    b, a = cuda(CU.sphere_cloud(100, 1)), cuda(CU.sphere_cloud(50, 2))
    ws = torch.full((lib.diner_cloud_grid_bytes(100, 4, 4, 4),), 0x5a, dtype=torch.uint8, device="cuda")
    d2, idx = torch.full((50,), -7.0, device="cuda"), torch.full((50,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((11,), -7.0, dtype=torch.float64, device="cuda")
    rws = torch.full((lib.diner_cloud_reduce_workspace_bytes(50),), 0x5a, dtype=torch.uint8, device="cuda")
    nrm = torch.ones(100, 3, device="cuda")
    p = C.c_void_p(16)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    real = dict(xyz_b=ptr(b), ws=ptr(ws), xyz_a=ptr(a), d2=ptr(d2), idx=ptr(idx), lo=(-0.3, -0.3, -0.3), h=0.15)
    for kw, what in BOX_REFUSALS:
        assert grid_entry(lib, "build", p, **{**real, **kw}) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())
    for kw, what in NEAREST_REFUSALS:
        assert grid_entry(lib, "nearest", p, **{**real, **kw}) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())
    rreal = dict(d2=ptr(d2), idx=ptr(idx), n=50, na=ptr(nrm), nb=ptr(nrm), nb_rows=100, ws=ptr(rws), out=ptr(out))
    for kw, what in REDUCE_REFUSALS:
        assert reduce_entry(lib, p, **{**rreal, **kw}) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())
    torch.cuda.synchronize()
    assert bool((ws == 0x5a).all()) and bool((rws == 0x5a).all()) and bool((d2 == -7).all()) and bool((idx == -7).all()) and bool((out == -7).all())
    assert grid_entry(lib, "build", p, **real) == 0 and grid_entry(lib, "nearest", p, **real) == 0
    assert reduce_entry(lib, p, **rreal) == 0
    torch.cuda.synchronize()
    ref = CU.ref_nearest(a.cpu().numpy(), b.cpu().numpy())
    assert_same((d2.cpu().numpy(), idx.cpu().numpy()), ref, "after the refusals")
    assert out.cpu().tolist()[0] == 50.0 and out.cpu().tolist()[2] == 50.0 * 3.0


# ------------------------------------------------------------------------------------------------------------------ 8 Python layer
def test_geometry_folder_error_ply_and_rendering_untouched(ops, tmp_path):
    from diner_amd import cloudmetrics as CM
    from diner_amd import evaluate, noise
    from diner_amd.geometry import read_ply, write_ply
    from diner_amd.render import predict_image
    from diner_amd.surface import write_mesh_ply
    from tests.test_geometry_gpu import model
    case, nerf, ren, E, Kt = model()
    sc, w, h = case.sc, case.w, case.h

    def renders():
        rays = ops.gen_rays(E, Kt, w, h, sc["znear"], sc["zfar"], "cuda")[:, 100:900].contiguous()
        with torch.no_grad(), noise.keyed(SEED, 100):
            f = ren.forward(nerf, rays, want_alpha=True).fine
        return predict_image(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED), f

    before = renders()
    src = tmp_path / "visualizations"
    src.mkdir()
    kw = dict(max_dist=0.05, thresholds=(0.01, 0.02))
    expected = []
    for n, stem in enumerate(("view0", "view1")):
        pred, pn = CU.sphere_cloud(900 + 50 * n, 20 + n, with_normals=True)
        gt, gn = CU.sphere_cloud(800, 30 + n, sigma=0.0, with_normals=True)
        write_ply(src / f"{stem}.ply", pred, normals=pn if n == 0 else None)
        write_ply(src / f"{stem}-gt.ply", gt, normals=gn)
        row = {k: v for k, v in CM.cloud_scores(cuda(pred), cuda(gt), pred_normals=cuda(pn) if n == 0 else None,
                                                gt_normals=cuda(gn) if n == 0 else None, **kw).items() if isinstance(v, (int, float))}
        if n == 0:
            verts, vn = CU.sphere_cloud(500, 40, sigma=0.002, with_normals=True)
            write_mesh_ply(src / f"{stem}-mesh.ply", verts, vn, None, np.array([[0, 1, 2]], np.int32))
            ms = CM.mesh_scores((cuda(verts), cuda(vn), None, None), cuda(gt), gt_normals=cuda(gn), **kw)
            row.update({"mesh_" + k: v for k, v in ms.items() if isinstance(v, (int, float))})
        expected.append(row)
    avg = evaluate.evaluate_geometry_folder(src, tmp_path, **kw)
    report = json.load(open(tmp_path / evaluate.GEOMETRY_REPORT_FILENAME))
    assert [r.pop("path") for r in report] == [str(src / "view0.ply"), str(src / "view1.ply")]
    assert report == expected and "normal_consistency" in report[0] and "normal_consistency" not in report[1] and "mesh_chamfer" in report[0]
    assert json.load(open(tmp_path / evaluate.GEOMETRY_SCORE_FILENAME)) == avg
    assert avg["chamfer"] == float(np.mean([r["chamfer"] for r in expected])) and avg["mesh_chamfer"] == expected[0]["mesh_chamfer"]
    assert 0.0 < avg["chamfer"] < 0.05 and 0.0 < avg["fscore@0.02"] <= 1.0       # means run over matched distances: below max_dist
    evaluate.main(["--eval_path", str(tmp_path), "--geometry", "--max_dist", "0.05", "--threshold", "0.01", "--threshold", "0.02"])
    assert json.load(open(tmp_path / evaluate.GEOMETRY_SCORE_FILENAME)) == avg        # no images in the folder: the geometry alone

    # write_error_ply: the points come back, coloured through the depth images' colour map
    from diner_amd.imageio import _lut_u8
    pred = cuda(CU.sphere_cloud(300, 50))
    dist = torch.linspace(0.0, 0.02, 300, device="cuda")
    dist[-1] = float("inf")
    CM.write_error_ply(tmp_path / "err.ply", pred, dist, vmax=0.01)
    xyz, rgb, nrm = read_ply(tmp_path / "err.ply")
    lut = _lut_u8("viridis", pred.device).cpu().numpy()
    assert nrm is None and np.array_equal(xyz, pred.cpu().numpy()) and rgb.dtype == np.uint8
    assert (rgb[0] == lut[0]).all() and (rgb[-1] == lut[255]).all() and (rgb[200] == lut[255]).all() and (rgb[75] == lut[int(75 / 299 * 2 * 256)]).all()

    after = renders()
    for a_, b_ in zip(before[0], after[0]):
        assert torch.equal(a_, b_)
    for k in before[1]:
        assert torch.equal(bits(before[1][k]), bits(after[1][k])), k
