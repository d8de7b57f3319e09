"""Shared by tests/test_cloud_cpu.py and tests/test_cloud_gpu.py: the definition of correct for cloud.hip and diner_amd.cloudmetrics,
restated in numpy from include/diner_hip.h -- exhaustive search in float32 with the header's operation order and tie rule, chunked over
the queries; the sums and the scores in float64 -- and the seeded clouds the tests run on.  No GPU is touched here."""
import functools
import math

import numpy as np

RADIUS, SIGMA = 0.25, 0.01
CAPS = (math.inf, 0.5, 0.03, 0.001)           # no cap, larger than the box, a few cells, smaller than a cell
THIN_OFFSET = 1 << 20


# ------------------------------------------------------------------------------------------------------------------ the search
def ref_nearest(xyz_a, xyz_b, max_dist=math.inf, chunk=256):
    """diner_cloud_nearest_f32's definition by exhaustive search -> (d2 (NA,) float32, idx (NA,) int32)."""
    a = np.ascontiguousarray(xyz_a, dtype=np.float32)
    b = np.ascontiguousarray(xyz_b, dtype=np.float32)
    cap2 = np.float32(max_dist) * np.float32(max_dist)
    b_ok = np.isfinite(b).all(axis=1)
    d2_out = np.full(a.shape[0], np.inf, dtype=np.float32)
    idx_out = np.full(a.shape[0], -1, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for s in range(0, a.shape[0], chunk):
            q = a[s:s + chunk]
            d = b[None, :, :] - q[:, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            assert d2.dtype == np.float32
            valid = b_ok[None, :] & (d2 <= cap2) & np.isfinite(q).all(axis=1)[:, None]
            masked = np.where(valid, d2, np.float32(np.inf))
            j = np.argmin(masked, axis=1)                                    # the first of equal minima: the smallest index
            rows = np.arange(q.shape[0])
            j = np.where(np.isinf(masked[rows, j]), np.argmax(valid, axis=1), j)   # an overflowed d2 (inf) is a candidate too
            found = valid.any(axis=1)
            d2_out[s:s + chunk] = np.where(found, d2[rows, j], np.float32(np.inf))
            idx_out[s:s + chunk] = np.where(found, j, -1)
    return d2_out, idx_out


def ref_reduce(d2, idx, max_dist=math.inf, thresholds=(), normals_a=None, normals_b=None):
    """diner_cloud_reduce_f32's definition -> dict(matched int, sum_dist, sum_normal float64, counts [int per threshold])."""
    d2 = np.asarray(d2, dtype=np.float32)
    idx = np.asarray(idx)
    m = (idx >= 0) & (d2 <= np.float32(max_dist) * np.float32(max_dist))
    with np.errstate(over="ignore"):
        out = dict(matched=int(m.sum()), sum_dist=float(np.sqrt(d2[m].astype(np.float64)).sum()), sum_normal=0.0,
                   counts=[int((m & (d2 <= np.float32(t) * np.float32(t))).sum()) for t in thresholds])
    if normals_a is not None and normals_b is not None:
        na = np.asarray(normals_a, dtype=np.float32).astype(np.float64)[m]
        nb = np.asarray(normals_b, dtype=np.float32).astype(np.float64)[idx[m]]
        out["sum_normal"] = float(np.abs((na[:, 0] * nb[:, 0] + na[:, 1] * nb[:, 1]) + na[:, 2] * nb[:, 2]).sum())
    return out


# ------------------------------------------------------------------------------------------------------------------ the scores
def ref_kept(xyz, bounds=None, thin=None):
    """cloudmetrics.kept_points' definition -> sorted int64 indices."""
    xyz = np.asarray(xyz, dtype=np.float32)
    keep = np.isfinite(xyz).all(axis=1)
    if bounds is not None:
        lo, hi = np.asarray(bounds[0], dtype=np.float32), np.asarray(bounds[1], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            keep &= ((xyz >= lo) & (xyz <= hi)).all(axis=1)
    index = np.nonzero(keep)[0].astype(np.int64)
    if thin is not None and index.size:
        with np.errstate(over="ignore"):
            k = np.floor(xyz[index] / np.float32(thin))
        assert k.dtype == np.float32
        k = np.clip(k, -THIN_OFFSET, THIN_OFFSET - 1).astype(np.int64) + THIN_OFFSET
        key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
        _, first = np.unique(key, return_index=True)                      # the first occurrence: the smallest index
        index = index[np.sort(first)]
    return index


def lower_median(x):
    x = np.sort(np.asarray(x))
    return float(x[(x.size - 1) // 2]) if x.size else math.nan


def threshold_key(name, tau):
    return f"{name}@{float(tau):g}"


def ref_scores(pred, gt, max_dist=math.inf, thresholds=(), pred_normals=None, gt_normals=None, bounds=None, thin=None):
    """cloudmetrics.cloud_scores' definition, the scores in float64 from the float32 search."""
    pred, gt = np.asarray(pred, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    ip, ig = ref_kept(pred, bounds, thin), ref_kept(gt, bounds, thin)
    P, G = pred[ip], gt[ig]
    Pn = None if pred_normals is None else np.asarray(pred_normals, dtype=np.float32)[ip]
    Gn = None if gt_normals is None else np.asarray(gt_normals, dtype=np.float32)[ig]
    out = dict(n_pred=len(ip), n_gt=len(ig), index_pred=ip, index_gt=ig)
    nan = math.nan
    sides = {}
    for name, (A, B, An, Bn) in (("pred", (P, G, Pn, Gn)), ("gt", (G, P, Gn, Pn))):
        if len(A) and len(B):
            d2, idx = ref_nearest(A, B, max_dist)
        else:
            d2, idx = np.full(len(A), np.inf, np.float32), np.full(len(A), -1, np.int32)
        both = An is not None and Bn is not None
        r = ref_reduce(d2, idx, max_dist, thresholds, An if both else None, Bn if both else None)
        dist = np.sqrt(d2)
        sides[name] = (r, dist, lower_median(dist[idx >= 0]))
        out["dist_" + name] = dist
    (rp, _, med_p), (rg, _, med_g) = sides["pred"], sides["gt"]
    mp, mg = rp["matched"], rg["matched"]
    out.update(matched_pred=mp, matched_gt=mg, accuracy=rp["sum_dist"] / mp if mp else nan,
               completeness=rg["sum_dist"] / mg if mg else nan, accuracy_median=med_p, completeness_median=med_g)
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    for k, t in enumerate(thresholds):
        prec = rp["counts"][k] / len(ip) if len(ip) else nan
        rec = rg["counts"][k] / len(ig) if len(ig) else nan
        out[threshold_key("precision", t)], out[threshold_key("recall", t)] = prec, rec
        out[threshold_key("fscore", t)] = 2.0 * prec * rec / (prec + rec) if prec + rec > 0.0 else (nan if math.isnan(prec + rec) else 0.0)
    if Pn is not None and Gn is not None:
        out["normal_consistency"] = 0.5 * (rp["sum_normal"] / mp + rg["sum_normal"] / mg) if mp and mg else nan
    return out


# ------------------------------------------------------------------------------------------------------------------ the clouds
def sphere_cloud(n, seed, radius=RADIUS, sigma=SIGMA, with_normals=False):
    """n points on the sphere of `radius` at the origin, moved along their normals by N(0, sigma) -> (n,3) float32 [, normals]."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = (u * (radius + sigma * rng.standard_normal((n, 1)))).astype(np.float32)
    return (p, u.astype(np.float32)) if with_normals else p


def box_of(xyz_b, cell):
    """A box around the finite points of xyz_b cut into cells of size `cell`: -> (lo (3,) float32, cell, dims)."""
    b = np.asarray(xyz_b, dtype=np.float32)
    b = b[np.isfinite(b).all(axis=1)]
    lo = b.min(axis=0) if len(b) else np.zeros(3, np.float32)
    hi = b.max(axis=0) if len(b) else np.zeros(3, np.float32)
    dims = tuple(int(min(max(math.floor(float(e) / cell) + 1, 1), 1024)) for e in (hi - lo))
    return lo.astype(np.float32), float(np.float32(cell)), dims


@functools.lru_cache(maxsize=None)
def exactness_clouds():
    """name -> (xyz_a, xyz_b, lo, cell, dims): the clouds of the exactness test, each with the grid it is searched through."""
    out = {}
    a, b = sphere_cloud(3000, 1), sphere_cloud(2500, 2)
    out["sphere"] = (a, b, *box_of(b, 0.02))
    # every point twice, at shuffled places: equal distances must go to the smaller index
    rng = np.random.default_rng(3)
    half = sphere_cloud(600, 4)
    dup = np.concatenate([half, half])[rng.permutation(1200)]
    out["duplicates"] = (np.concatenate([sphere_cloud(500, 5), half[:300]]), dup, *box_of(dup, 0.03))
    # targets exactly on cell faces and corners, queries at cell centres and on faces: distances tie all the time
    lo, h, n = np.array([-0.5, 0.25, 1.0], np.float32), np.float32(0.125), 6
    ijk = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), np.arange(n + 1), indexing="ij"), -1).reshape(-1, 3)
    lattice = (lo + ijk.astype(np.float32) * h).astype(np.float32)
    centres = (lattice[(ijk < n).all(axis=1)] + np.float32(0.5) * h).astype(np.float32)
    on_faces = (lattice + np.array([0.5, 0.5, 0.0], np.float32) * h).astype(np.float32)
    out["lattice"] = (np.concatenate([centres, on_faces, lattice]), lattice[rng.permutation(len(lattice))], lo, float(h), (n, n, n))
    # queries far outside the box on each side (and near it), against the sphere
    far = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            for dist in (0.3, 1.0, 40.0, 1e6, 1e30):
                p = rng.uniform(-0.3, 0.3, size=(4, 3))
                p[:, axis] = sign * dist
                far.append(p)
    out["far"] = (np.concatenate(far).astype(np.float32), b, *box_of(b, 0.05))
    out["one_target"] = (sphere_cloud(200, 6), np.array([[0.1, -0.05, 0.2]], np.float32), np.array([0.1, -0.05, 0.2], np.float32), 0.05,
                         (1, 1, 1))
    for na in (1, 63, 64, 65, 257):
        out[f"na{na}"] = (sphere_cloud(na, 10 + na), b[:700], *box_of(b[:700], 0.04))
    # NaN and inf rows on both sides
    bad_b, bad_a = sphere_cloud(900, 7).copy(), sphere_cloud(400, 8).copy()
    bad_b[5] = np.nan
    bad_b[17, 1] = np.inf
    bad_b[40, 2] = -np.inf
    bad_b[899, 0] = np.nan
    bad_a[0, 0] = np.nan
    bad_a[63] = np.inf
    bad_a[64, 2] = -np.inf
    bad_a[399, 1] = np.nan
    out["nonfinite"] = (bad_a, bad_b, *box_of(bad_b, 0.03))
    return out


@functools.lru_cache(maxsize=None)
def exactness_reference(name, cap):
    a, b = exactness_clouds()[name][:2]
    return ref_nearest(a, b, cap)


# two four-point clouds whose scores are computed by hand in tests/test_cloud_cpu.py
HAND_PRED = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 0, 0]], np.float32)
HAND_GT = np.array([[0, 0, 1], [1, 0, 0], [0, 0, 0], [0, 2, 2]], np.float32)
