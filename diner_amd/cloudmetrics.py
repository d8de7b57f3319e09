"""Distance scores between point clouds and meshes on the device: accuracy (prediction -> ground truth), completeness (ground truth ->
prediction), their mean (Chamfer), precision / recall / F-score at distance thresholds and normal consistency -- the scores DTU is
evaluated with.  They rest on one primitive, the nearest neighbour between two clouds of millions of points, which cloud.hip answers
through a uniform grid with the bits of exhaustive search (ops.cloud_grid / cloud_nearest / cloud_reduce).

    s = cloud_scores(pred_xyz, gt_xyz, max_dist=20.0, thresholds=(1.0, 2.0))
    s["accuracy"], s["completeness"], s["chamfer"], s[threshold_key("fscore", 1.0)]

Everything runs on the HIP device the clouds live on; there is no CPU path.  Choosing a box and a cell size, the masks and the medians
are torch ops that run once per cloud; the searches and the sums are the kernels."""
import math

import numpy as np
import torch

POINTS_PER_CELL = 2.0            # what CloudGrid(cell=None) aims at in an occupied cell


def threshold_key(name, tau):
    """The key of a per-threshold score: threshold_key("fscore", 0.01) == "fscore@0.01"."""
    return f"{name}@{float(tau):g}"


def _check_points(who, name, xyz, normals=None, device=True):
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"diner_amd: {who} expects {name} (N,3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if xyz.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects {name} float32, got {xyz.dtype}")
    if normals is not None and (not torch.is_tensor(normals) or tuple(normals.shape) != tuple(xyz.shape) or normals.dtype != torch.float32):
        raise ValueError(f"diner_amd: {who} expects the normals of {name} float32 {tuple(xyz.shape)}")
    if device:
        _require_device(who, name, xyz, normals)


def _require_device(who, name, xyz, normals=None):
    if not xyz.is_cuda or (normals is not None and normals.device != xyz.device):
        raise RuntimeError(f"diner_amd: {who} expects {name} on a HIP device; there is no CPU fallback")


def _check_max_dist(who, max_dist):
    max_dist = float(max_dist)
    if not max_dist > 0.0:
        raise ValueError(f"diner_amd: {who} max_dist {max_dist} must be > 0 (inf: no cap)")
    return max_dist


def grid_box(lo, hi, n, cell=None, max_dist=math.inf):
    """The box CloudGrid puts around n points between the corners lo and hi: -> (cell, (Gx,Gy,Gz)).  cell=None aims at POINTS_PER_CELL
    points in an occupied cell of a SURFACE, whose area is taken as half the box's; the cell is then at least max_dist / 2 (a capped
    search stays within a few rings) and grows until the dims are within 1024 a side and 2^26 in all.  Host arithmetic only."""
    from .ops import CLOUD_MAX_CELLS, CLOUD_MAX_DIM
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    if cell is None:
        area = ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]
        cell = math.sqrt(area * POINTS_PER_CELL / max(int(n), 1))
        if not cell > 0.0:                                   # the points lie on a line, or are one point
            cell = max(ext) * POINTS_PER_CELL / max(int(n), 1)
        if not cell > 0.0:
            cell = 1.0
        if math.isfinite(max_dist):
            cell = max(cell, 0.5 * max_dist)
    cell = float(np.float32(cell))
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"diner_amd: CloudGrid cell size {cell} must be > 0 and finite")
    while True:
        dims = tuple(int(e / cell) + 1 for e in ext)
        if max(dims) <= CLOUD_MAX_DIM and dims[0] * dims[1] * dims[2] <= CLOUD_MAX_CELLS:
            return cell, dims
        cell = float(np.float32(cell * 1.1))


class CloudGrid:
    """A search structure over the cloud xyz (N,3) float32 on the HIP device: the box of its finite points, cut into cubic cells.
    cell: the cell size, None: grid_box's choice; max_dist: the cap the searches will mostly run with (it only steers that choice).
    .nearest(queries) answers from it; .data is the ops.CloudGridData, whose .order lists the cloud's own indices in cell order."""

    def __init__(self, xyz, cell=None, max_dist=math.inf):
        from . import ops
        _check_points("CloudGrid", "xyz", xyz, device=False)
        if xyz.shape[0] < 1:
            raise ValueError("diner_amd: CloudGrid needs at least one point")
        self.max_dist = _check_max_dist("CloudGrid", max_dist)
        if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
            raise ValueError(f"diner_amd: CloudGrid cell size {cell} must be > 0 and finite")
        _require_device("CloudGrid", "xyz", xyz)
        xyz = xyz.detach().contiguous()
        finite = torch.isfinite(xyz).all(dim=1)
        n = int(finite.sum())
        if n:
            pts = xyz if n == xyz.shape[0] else xyz[finite]
            lo, hi = pts.amin(dim=0).cpu().tolist(), pts.amax(dim=0).cpu().tolist()
        else:
            lo = hi = [0.0, 0.0, 0.0]
        self.n_finite = n
        self.cell, self.dims = grid_box(lo, hi, n, cell, self.max_dist)
        self.lo = tuple(lo)
        self.data = ops.cloud_grid(xyz, lo, self.cell, self.dims)

    def nearest(self, queries, max_dist=None):
        """-> (dist (NA,) float32 = sqrt(d2), idx (NA,) int64): the nearest point of the cloud within max_dist (None: the grid's) of
        every query; inf and -1 where there is none, and for a non-finite query.  Without a cap a query far from the cloud walks
        most of the grid: give one where outliers are expected."""
        from . import ops
        _check_points("CloudGrid.nearest", "queries", queries)
        d2, idx = ops.cloud_nearest(self.data, queries, self.max_dist if max_dist is None else max_dist)
        return torch.sqrt(d2), idx.to(torch.int64)


THIN_OFFSET = 1 << 20            # thin's lattice coordinates floor(p / s) are kept within +- 2^20 cells of the world origin


def kept_points(xyz, bounds=None, thin=None):
    """The rows of xyz (N,3) float32 that cloud_scores scores, as sorted int64 indices on xyz's device: the finite points, inside
    bounds = (lo, hi) (lo <= p <= hi on every axis, compared in fp32) when given, and -- thin = s -- of those one per cell of the lattice
    of size s anchored at the world origin (cell floor(p / s) in fp32 per axis), the one with the smallest index."""
    keep = torch.isfinite(xyz).all(dim=1)
    if bounds is not None:
        lo = torch.as_tensor(bounds[0], dtype=torch.float32).reshape(3).to(xyz.device)
        hi = torch.as_tensor(bounds[1], dtype=torch.float32).reshape(3).to(xyz.device)
        keep &= ((xyz >= lo) & (xyz <= hi)).all(dim=1)
    index = torch.nonzero(keep).reshape(-1)
    if thin is not None and index.numel():
        k = torch.floor(xyz[index] / torch.tensor(float(thin), dtype=torch.float32, device=xyz.device))
        k = k.clamp_(-THIN_OFFSET, THIN_OFFSET - 1).to(torch.int64) + THIN_OFFSET
        key = (k[:, 2] << 42) | (k[:, 1] << 21) | k[:, 0]
        uniq, inverse = torch.unique(key, return_inverse=True)
        first = torch.full((uniq.numel(),), index.numel(), dtype=torch.int64, device=xyz.device)
        first.scatter_reduce_(0, inverse, torch.arange(index.numel(), device=xyz.device), reduce="amin")
        index = index[torch.sort(first).values]
    return index


def _check_scores_args(who, pred_xyz, gt_xyz, max_dist, thresholds, pred_normals, gt_normals, bounds, thin):
    from .ops import CLOUD_MAX_THRESHOLDS
    _check_points(who, "pred_xyz", pred_xyz, pred_normals, device=False)
    _check_points(who, "gt_xyz", gt_xyz, gt_normals, device=False)
    max_dist = _check_max_dist(who, max_dist)
    taus = [float(t) for t in thresholds]
    if len(taus) > CLOUD_MAX_THRESHOLDS or not all(t >= 0.0 for t in taus):
        raise ValueError(f"diner_amd: {who} takes at most {CLOUD_MAX_THRESHOLDS} thresholds, each >= 0, got {taus}")
    if bounds is not None:
        b = np.asarray(bounds, dtype=np.float64)
        if b.shape != (2, 3) or not (b[0] <= b[1]).all():
            raise ValueError(f"diner_amd: {who} bounds must be (lo, hi) of three values each with lo <= hi, got {bounds}")
    if thin is not None and not (float(thin) > 0.0 and math.isfinite(float(thin))):
        raise ValueError(f"diner_amd: {who} thin {thin} must be > 0 and finite")
    _require_device(who, "pred_xyz", pred_xyz, pred_normals)
    _require_device(who, "gt_xyz", gt_xyz, gt_normals)
    if pred_xyz.device != gt_xyz.device:
        raise RuntimeError(f"diner_amd: {who} expects both clouds on one device, got {pred_xyz.device} and {gt_xyz.device}")
    return max_dist, taus


def _direction(grid, own, normals, grid_normals, max_dist, taus):
    """One direction of the scores: every point of the cloud of `own` against the cloud of `grid` -> (host sums of cloud_reduce, dist
    (N,) float32, median of the matched distances).  The threads take the queries in the cell order of their own grid, so that a
    wavefront walks the same cells: 1.8x (1 M against 1 M points) to 2.7x (7.7 M against 5 M) the rate of input order on clouds in no
    spatial order (tools/time_cloud.py)."""
    from . import ops
    d2, idx = ops.cloud_nearest(grid.data, own.data.xyz, max_dist, order=own.data.order)
    both = normals is not None and grid_normals is not None
    sums = ops.cloud_reduce(d2, idx, max_dist, taus, normals if both else None, grid_normals if both else None).cpu().tolist()
    dist = torch.sqrt(d2)
    matched = dist[idx >= 0]
    median = float(torch.median(matched)) if matched.numel() else math.nan
    return sums, dist, median


@torch.no_grad()
def cloud_scores(pred_xyz, gt_xyz, max_dist=math.inf, thresholds=(), pred_normals=None, gt_normals=None, bounds=None, thin=None):
    """Score the predicted cloud pred_xyz (NP,3) against the ground truth gt_xyz (NG,3), float32 on one HIP device -> dict:
      accuracy / completeness: the mean distance from a predicted point to its nearest ground-truth point / the other way round, over
        the MATCHED points only -- those with a neighbour within max_dist (DTU's rule: beyond it a distance is an outlier);
        chamfer their mean; accuracy_median / completeness_median the (lower) medians of the same distances;
      precision@t / recall@t / fscore@t (threshold_key) per threshold t: the share of ALL scored predicted / ground-truth points with a
        neighbour within t (and within max_dist) -- outliers do cost here -- and their harmonic mean;
      normal_consistency, when both normal sets (N,3) are given: the mean over the two directions of the mean |n . n'| over matched pairs;
      n_pred, n_gt: the points scored; matched_pred, matched_gt: those matched;
      dist_pred (n_pred,), dist_gt (n_gt,): the distances, float32 on the device, inf where unmatched; index_pred, index_gt: the rows
        of the inputs they belong to (int64, sorted).
    Scored are the finite points, inside bounds = (lo, hi) when given (the role of DTU's observation mask), thinned to one point per
    thin-sized cell when thin is given (kept_points).  A side with no matched point -- or no point -- scores nan; that is no error.
    The search is exact, so without a cap a point far from the other cloud walks most of that cloud's grid: clouds with outliers
    want a finite max_dist (DTU uses 20 mm), which also ends such a walk after a few rings."""
    max_dist, taus = _check_scores_args("cloud_scores", pred_xyz, gt_xyz, max_dist, thresholds, pred_normals, gt_normals, bounds, thin)
    dev = pred_xyz.device
    with torch.cuda.device(dev):
        ip, ig = kept_points(pred_xyz, bounds, thin), kept_points(gt_xyz, bounds, thin)
        P, G = pred_xyz[ip].contiguous(), gt_xyz[ig].contiguous()
        Pn = None if pred_normals is None else pred_normals[ip].contiguous()
        Gn = None if gt_normals is None else gt_normals[ig].contiguous()
        n_pred, n_gt = int(P.shape[0]), int(G.shape[0])
        out = {"n_pred": n_pred, "n_gt": n_gt, "index_pred": ip, "index_gt": ig}
        nan = math.nan
        if n_pred and n_gt:
            grid_p, grid_g = CloudGrid(P, max_dist=max_dist), CloudGrid(G, max_dist=max_dist)
            sp, dist_p, med_p = _direction(grid_g, grid_p, Pn, Gn, max_dist, taus)
            sg, dist_g, med_g = _direction(grid_p, grid_g, Gn, Pn, max_dist, taus)
        else:
            sp = sg = [0.0] * (3 + len(taus))
            dist_p = torch.full((n_pred,), math.inf, dtype=torch.float32, device=dev)
            dist_g = torch.full((n_gt,), math.inf, dtype=torch.float32, device=dev)
            med_p = med_g = nan
    mp, mg = int(sp[0]), int(sg[0])
    out["matched_pred"], out["matched_gt"] = mp, mg
    out["accuracy"] = sp[1] / mp if mp else nan
    out["completeness"] = sg[1] / mg if mg else nan
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["accuracy_median"], out["completeness_median"] = med_p, med_g
    for k, t in enumerate(taus):
        prec = sp[3 + k] / n_pred if n_pred else nan
        rec = sg[3 + k] / n_gt if n_gt else nan
        out[threshold_key("precision", t)], out[threshold_key("recall", t)] = prec, rec
        out[threshold_key("fscore", t)] = 2.0 * prec * rec / (prec + rec) if prec + rec > 0.0 else (nan if math.isnan(prec + rec) else 0.0)
    if Pn is not None and Gn is not None:
        out["normal_consistency"] = 0.5 * (sp[2] / mp + sg[2] / mg) if mp and mg else nan
    out["dist_pred"], out["dist_gt"] = dist_p, dist_g
    return out


def mesh_scores(mesh, gt_xyz, max_dist=math.inf, thresholds=(), gt_normals=None, bounds=None, thin=None):
    """cloud_scores of a surface.Mesh by its vertices, with the vertex normals as pred_normals: surface-nets vertices sit at voxel
    spacing, the resolution of the surface itself (triangle interiors are not sampled).  mesh: (vertices, normals, rgb, faces) with
    the first two float32 tensors on the HIP device (normals may be None)."""
    vertices, normals = mesh[0], mesh[1]
    return cloud_scores(vertices, gt_xyz, max_dist=max_dist, thresholds=thresholds, pred_normals=normals, gt_normals=gt_normals,
                        bounds=bounds, thin=thin)


def write_error_ply(path, xyz, dist, vmax, cmap="viridis"):
    """A cloud coloured by its distances (cloud_scores' dist_pred / dist_gt): xyz (N,3), dist (N,) float32 on the HIP device, 0 .. vmax
    through the colour map of the depth images (imageio), an unmatched point (inf) in the map's last colour; written with write_ply."""
    from . import _lib
    from .geometry import write_ply
    from .imageio import _lut_u8
    from .ops import _ptr, _stream, lib
    _check_points("write_error_ply", "xyz", xyz)
    if not torch.is_tensor(dist) or tuple(dist.shape) != (xyz.shape[0],) or dist.dtype != torch.float32 or dist.device != xyz.device:
        raise ValueError(f"diner_amd: write_error_ply expects dist float32 ({xyz.shape[0]},) on the cloud's device")
    if not (float(vmax) > 0.0 and math.isfinite(float(vmax))):
        raise ValueError(f"diner_amd: write_error_ply vmax {vmax} must be > 0 and finite")
    n = int(xyz.shape[0])
    rgb = torch.empty(n, 3, dtype=torch.uint8, device=xyz.device)
    if n:
        with torch.cuda.device(xyz.device):
            _lib.check(lib.diner_colormap_u8(_ptr(dist.contiguous()), n, _ptr(_lut_u8(cmap, xyz.device)), 0.0, float(vmax), _ptr(rgb),
                                             _stream()))
    write_ply(path, xyz, rgb)
