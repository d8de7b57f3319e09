"""Shared by tests/test_geometry_cpu.py and tests/test_geometry_gpu.py: numpy restatements of the two kernels of geometry.hip (written
from their definitions in include/diner_hip.h, evaluated in a dtype of the caller's choice: float64 is what the kernels are measured
against, float32 gives the error of the definition itself at the kernels' precision) and the seeded input generators.  No GPU is
touched here."""
import functools
import types

import numpy as np

F32_EPS = 2.0 ** -24
ALPHA_MIN = 1e-3
K_LIST = (1, 5, 64, 65, 256, 257, 1024)
NR_RANDOM = 67                         # not a multiple of the 4 rays of a workgroup
FAR = 2.0


def quantiles_for(K):
    """q = 0.5 everywhere; q = 0.9 up to K = 257 only: at K = 1024 the worst-case summation bound calls 12.7 % of these rays ambiguous."""
    return (0.5, 0.9) if K <= 257 else (0.5,)


# ------------------------------------------------------------------------------------------------------------------ ray geometry
def composite_f64(sigma, z, far):
    """float64 alpha compositing of densities (NR,K) at depths z (NR,K): w_k = alpha_k prod_{j<k} (1 - alpha_j + 1e-10)."""
    delta = np.concatenate((z[:, 1:], np.full((z.shape[0], 1), far)), axis=1) - z
    alpha = 1.0 - np.exp(-delta * np.maximum(sigma, 0.0))
    T = np.cumprod(1.0 - alpha + 1e-10, axis=1)
    T = np.concatenate((np.ones((z.shape[0], 1)), T[:, :-1]), axis=1)
    return alpha * T


def ray_case(K, seed=None):
    """Seeded rays for one K: NR_RANDOM random rays and the hand-made ones on top -> namespace(w, z (NR,K) float32, rays (NR,8) float32,
    fwd (3) float32, hand: name -> row).  The default seed is 3000 + K; over the seeds looked at the undecided share of the float64
    restatement (ambiguous_rays) is 0 - 2 % with an occasional 5 - 6 % (67 rays: one ray is 1.6 %), and tests/test_geometry_cpu.py
    asserts the 5 % cap for the seed in use."""
    g = np.random.default_rng(3000 + K if seed is None else seed)
    n = NR_RANDOM
    z = np.sort(g.uniform(0.5, FAR, (n, K)), axis=1).astype(np.float32)
    k = np.arange(K)[None, :]
    centre = g.uniform(0.1, 0.9, (n, 1)) * K
    width = g.uniform(0.6, 3.0, (n, 1))
    amp = 10.0 ** g.uniform(0.0, 3.0, (n, 1))
    floor = g.uniform(0.0, 0.05, (n, 1))
    sigma = amp * np.exp(-0.5 * ((k - centre) / width) ** 2) + floor
    sigma[g.permutation(n)[:max(1, n // 16)]] = 0.0                   # one ray in 16 has zero density
    w = composite_f64(sigma, z.astype(np.float64), FAR).astype(np.float32)

    hand, rows_w = {}, []
    zh = np.linspace(0.6, 1.9, K, dtype=np.float32)

    def add(name, vals):
        row = np.zeros(K, dtype=np.float32)
        row[:len(vals)] = vals
        hand[name] = n + len(rows_w)
        rows_w.append(row)

    a32 = np.float32(ALPHA_MIN)
    if K >= 3:
        add("tie", [0.25, 0.25, 0.5])                                 # c_1 = 0.5 = 0.5 A exactly: median_idx 1 at quantile 0.5
    spike = np.zeros(K, dtype=np.float32)
    spike[K // 2] = 0.75
    add("spike", spike)
    if K >= 2:
        neg = np.zeros(K, dtype=np.float32)
        neg[0], neg[K // 2], neg[-1] = 0.125, 0.5, -0.0625            # a negative last weight (a sample beyond far)
        add("negative_last", neg)
    add("below_alpha_min", [np.nextafter(a32, np.float32(0))])
    add("at_alpha_min", [a32])
    add("above_alpha_min", [np.nextafter(a32, np.float32(1))])
    w = np.concatenate((w, np.stack(rows_w)), axis=0)
    z = np.concatenate((z, np.repeat(zh[None], len(rows_w), axis=0)), axis=0)
    NR = w.shape[0]
    d = g.normal(size=(NR, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate((g.uniform(-1.0, 1.0, (NR, 3)), d, np.full((NR, 1), 0.5), np.full((NR, 1), FAR)), axis=1).astype(np.float32)
    fwd = g.normal(size=3)
    fwd = (fwd / np.linalg.norm(fwd)).astype(np.float32)
    return types.SimpleNamespace(w=w, z=z, rays=rays, fwd=fwd, hand=hand, K=K, NR=NR)


def ref_ray_geometry(w, z, rays, fwd, quantile, alpha_min, point_mode, dtype=np.float64):
    """diner_ray_geometry_f32's definition, evaluated in `dtype` with the sums in sample order.  quantile and alpha_min are the float32
    values the entry receives.  -> namespace(valid, idx (int32, -1 invalid), depth_median, depth_mean, zdepth, points, c, A, thr)."""
    w, z, rays, fwd = (np.asarray(a).astype(dtype) for a in (w, z, rays, fwd))
    q, amin = dtype(np.float32(quantile)), dtype(np.float32(alpha_min))
    NR, K = w.shape
    c = np.cumsum(w, axis=1, dtype=dtype)
    A = c[:, -1]
    valid = A > amin
    thr = q * A
    with np.errstate(invalid="ignore", divide="ignore"):
        ge = c >= thr[:, None]
        idx = np.where(valid, np.argmax(ge, axis=1), -1).astype(np.int32)
        d_med = np.where(valid, z[np.arange(NR), np.maximum(idx, 0)], 0).astype(dtype)
        wz = np.cumsum(w * z, axis=1, dtype=dtype)[:, -1]
        d_mean = np.where(valid, wz / A, 0).astype(dtype)
    t = d_med if point_mode == 0 else d_mean
    o, d = rays[:, :3], rays[:, 3:6]
    cosine = (d[:, 0] * fwd[0] + d[:, 1] * fwd[1]) + d[:, 2] * fwd[2]
    zdepth = np.where(valid, t * cosine, 0).astype(dtype)
    points = np.where(valid[:, None], o + t[:, None] * d, 0).astype(dtype)
    return types.SimpleNamespace(valid=valid, idx=idx, depth_median=d_med, depth_mean=d_mean, zdepth=zdepth, points=points, c=c, A=A,
                                 thr=thr)


def ambiguous_rays(ref, w, alpha_min):
    """(NR,) bool: rays whose index -- or validity -- the worst-case fp32 summation error could move: some |c_k - q A| (or |A - alpha_min|)
    is within 2 K 2^-24 sum_k |w_k| of the float64 restatement `ref`."""
    K = w.shape[1]
    bound = 2.0 * K * F32_EPS * np.abs(w.astype(np.float64)).sum(axis=1)
    near_idx = (np.abs(ref.c - ref.thr[:, None]) <= bound[:, None]).any(axis=1)
    near_valid = np.abs(ref.A - np.float64(np.float32(alpha_min))) <= bound
    return (near_idx & ref.valid) | near_valid


def ray_tolerances(case, quantile, point_mode, keep):
    """4 x the largest |float32 restatement - float64 restatement| over the rays `keep`, per float output: the tolerance of the kernel's
    depth_mean, zdepth and points against the float64 restatement on these inputs."""
    r64 = ref_ray_geometry(case.w, case.z, case.rays, case.fwd, quantile, ALPHA_MIN, point_mode, np.float64)
    r32 = ref_ray_geometry(case.w, case.z, case.rays, case.fwd, quantile, ALPHA_MIN, point_mode, np.float32)
    same = keep & r64.valid & r32.valid & (r64.idx == r32.idx)
    gap = {f: float(np.abs(getattr(r32, f).astype(np.float64) - getattr(r64, f))[same].max()) if same.any() else 0.0
           for f in ("depth_mean", "zdepth", "points")}
    return {f: 4.0 * v for f, v in gap.items()}, gap


# --------------------------------------------------------------------------------------------------------------- depth2normal
def ref_depth2normal_interior(zdepth, Kmat, dtype=np.float64):
    """depth2normal (prep.hip: point_at, raw_normal) on the interior pixels [1:-1, 1:-1] of a map without holes, in `dtype`:
    p(i,j) = ((j + 0.5 - cx) / fx z, (i + 0.5 - cy) / fy z, z), n = normalize(cross(p(i+1,j) - p(i-1,j), p(i,j+1) - p(i,j-1)))
    -> (3,H-2,W-2)."""
    zd = np.asarray(zdepth).astype(dtype)
    Kmat = np.asarray(Kmat).astype(dtype)
    H, W = zd.shape
    x = ((np.arange(W).astype(dtype) + dtype(0.5)) - Kmat[0, 2]) / Kmat[0, 0]
    y = ((np.arange(H).astype(dtype) + dtype(0.5)) - Kmat[1, 2]) / Kmat[1, 1]
    P = np.stack((x[None, :] * zd, y[:, None] * zd, zd), axis=0)
    v = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    h = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    c = np.stack((v[1] * h[2] - v[2] * h[1], v[2] * h[0] - v[0] * h[2], v[0] * h[1] - v[1] * h[0]), axis=0)
    nrm = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
    return c / nrm


# ------------------------------------------------------------------------------------------------------------- depth consistency
def look_at_camera(position, target, f, W, H, roll=0.0):
    """World->camera extrinsics (4,4) of a pinhole camera at `position` looking at `target` (+z forward, +y down) and intrinsics (3,3)
    with the principal point at the image centre; float64."""
    position, target = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fw = target - position
    fw /= np.linalg.norm(fw)
    right = np.cross(fw, np.array([0.0, -1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fw, right)
    cr, sr = np.cos(roll), np.sin(roll)
    R = np.stack((cr * right + sr * down, -sr * right + cr * down, fw), axis=0)
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ position
    return E, np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def plane_zdepth(E, Kmat, W, H, normal, offset):
    """float64 z-depth map (H,W) of the plane normal . X = offset seen by the camera; 0 where the pixel's ray does not meet it in front."""
    R, t = E[:3, :3], E[:3, 3]
    x = (np.arange(W) + 0.5 - Kmat[0, 2]) / Kmat[0, 0]
    y = (np.arange(H) + 0.5 - Kmat[1, 2]) / Kmat[1, 1]
    dirs = np.stack(np.broadcast_arrays(x[None, :], y[:, None], np.ones((H, W))), axis=-1)        # camera frame, z = 1
    n_c = R @ np.asarray(normal, dtype=np.float64)                    # n . R^T (d D - t) = offset
    D = (offset + n_c @ t) / (dirs @ n_c)
    return np.where(D > 0, D, 0.0)


PLANE_N, PLANE_D = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0]), 2.0


@functools.lru_cache(maxsize=None)
def consistency_scene(N=3, W=40, H=32, perturb=True):
    """N pinhole cameras looking at an analytic plane, z-depth maps in float64.  N = 3: the test scene -- view 1 carries a 6 x 6 patch
    scaled by 1.05 and a 4 x 4 hole of zeros (perturb), view 2 is turned far enough that part of the plane it sees lies outside its
    neighbours' images.  N = 2: its first two cameras.  Other N: four distinct cameras, repeated.
    -> namespace(depth (N,H,W) float64, K (N,3,3), E (N,4,4), patch, hole: (slice, slice) in view 1)."""
    f = 1.1 * W
    base = [look_at_camera((0.0, 0.0, 0.0), (0.0, 0.0, 2.0), f, W, H),
            look_at_camera((0.25, 0.05, 0.0), (0.05, 0.0, 2.0), f, W, H, roll=0.03),
            look_at_camera((-0.3, -0.1, 0.1), (0.55, 0.1, 2.0), f, W, H, roll=-0.05),
            look_at_camera((0.1, 0.3, -0.1), (0.0, -0.1, 2.0), f, W, H, roll=0.02)]
    cams = [base[n % 4] if N > 3 else base[n] for n in range(N)]
    E = np.stack([c[0] for c in cams])
    Km = np.stack([c[1] for c in cams])
    depth = np.stack([plane_zdepth(E[n], Km[n], W, H, PLANE_N, PLANE_D) for n in range(N)])
    patch = (slice(H // 4, H // 4 + 6), slice(W // 4, W // 4 + 6))
    hole = (slice(H // 2 + 2, H // 2 + 6), slice(W // 2 + 3, W // 2 + 7))
    if perturb and N == 3:
        depth[1][patch] *= 1.05
        depth[1][hole] = 0.0
    return types.SimpleNamespace(depth=depth, K=Km, E=E, patch=patch, hole=hole, N=N, W=W, H=H)


def _taps_ok(px, py, depth_s, W, H):
    """All four taps of the bilinear lookup at texel coordinates (px, py) inside the image and non-zero (NaN: not ok)."""
    with np.errstate(invalid="ignore"):
        inside = (px >= 0) & (px < W - 1) & (py >= 0) & (py < H - 1)
    x0 = np.where(inside, np.floor(px), 0).astype(np.int64)
    y0 = np.where(inside, np.floor(py), 0).astype(np.int64)
    x0, y0 = np.clip(x0, 0, max(W - 2, 0)), np.clip(y0, 0, max(H - 2, 0))
    if W < 2 or H < 2:
        return np.zeros(px.shape, dtype=bool), x0, y0
    nz = (depth_s[y0, x0] != 0) & (depth_s[y0, x0 + 1] != 0) & (depth_s[y0 + 1, x0] != 0) & (depth_s[y0 + 1, x0 + 1] != 0)
    return inside & nz, x0, y0


def ref_depth_consistency(depth, Kmat, E, px_thr, rel_thr, dtype=np.float64):
    """diner_depth_consistency_f32's definition in `dtype` (the inputs are rounded to float32 first: that is what the entry is given).
    -> namespace(count (N,H,W) int32, avg (N,H,W), and per ordered pair (N,N,H,W): geom (the pair reached the comparison), dist, rel,
    px, py (texel coordinates in s), zs)."""
    depth = np.asarray(depth).astype(np.float32).astype(dtype)
    Kmat, E = np.asarray(Kmat).astype(np.float32).astype(dtype), np.asarray(E).astype(np.float32).astype(dtype)
    px_thr, rel_thr = dtype(np.float32(px_thr)), dtype(np.float32(rel_thr))
    N, H, W = depth.shape
    half = dtype(0.5)
    uc = (np.arange(W).astype(dtype) + half)[None, :] * np.ones((H, 1), dtype=dtype)
    vc = (np.arange(H).astype(dtype) + half)[:, None] * np.ones((1, W), dtype=dtype)
    shape = (N, N, H, W)
    out = types.SimpleNamespace(geom=np.zeros(shape, dtype=bool), dist=np.full(shape, np.nan), rel=np.full(shape, np.nan),
                                px=np.full(shape, np.nan), py=np.full(shape, np.nan), zs=np.full(shape, np.nan))
    count = np.zeros((N, H, W), dtype=np.int32)
    total = depth.copy()

    def back(n, u, v, d):
        return np.stack(((u - Kmat[n, 0, 2]) / Kmat[n, 0, 0] * d, (v - Kmat[n, 1, 2]) / Kmat[n, 1, 1] * d, d), axis=0)

    def to_world(n, X):
        Y = X - E[n, :3, 3][:, None, None]
        R = E[n, :3, :3]
        return np.stack([(R[0, k] * Y[0] + R[1, k] * Y[1]) + R[2, k] * Y[2] for k in range(3)], axis=0)

    def to_cam(n, Xw):
        R, t = E[n, :3, :3], E[n, :3, 3]
        return np.stack([((R[k, 0] * Xw[0] + R[k, 1] * Xw[1]) + R[k, 2] * Xw[2]) + t[k] for k in range(3)], axis=0)

    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for r in range(N):
            D = depth[r]
            has = D != 0
            Xw = to_world(r, back(r, uc, vc, D))
            for s in range(N):
                if s == r:
                    continue
                Xs = to_cam(s, Xw)
                front = Xs[2] > 0
                u = Kmat[s, 0, 0] * (Xs[0] / Xs[2]) + Kmat[s, 0, 2]
                v = Kmat[s, 1, 1] * (Xs[1] / Xs[2]) + Kmat[s, 1, 2]
                px, py = u - half, v - half
                ok, x0, y0 = _taps_ok(px, py, depth[s], W, H)
                ax, ay = px - x0.astype(dtype), py - y0.astype(dtype)
                bx, by = dtype(1) - ax, dtype(1) - ay
                ds = depth[s]
                x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
                Ds = ((bx * by) * ds[y0, x0] + (ax * by) * ds[y0, x1]) + ((bx * ay) * ds[y1, x0] + (ax * ay) * ds[y1, x1])
                Xr = to_cam(r, to_world(s, back(s, u, v, Ds)))
                dr = Xr[2]
                u2 = Kmat[r, 0, 0] * (Xr[0] / dr) + Kmat[r, 0, 2]
                v2 = Kmat[r, 1, 1] * (Xr[1] / dr) + Kmat[r, 1, 2]
                du, dv = u2 - uc, v2 - vc
                dist = np.sqrt(du * du + dv * dv)
                rel = np.abs(dr - D) / D
                geom = has & front & ok
                good = geom & (dist < px_thr) & (rel < rel_thr)
                count[r] += good
                total[r] = np.where(good, total[r] + dr, total[r])
                out.geom[r, s], out.px[r, s], out.py[r, s], out.zs[r, s] = geom, px, py, Xs[2]
                out.dist[r, s] = np.where(geom, dist, np.nan)
                out.rel[r, s] = np.where(geom, rel, np.nan)
    out.count = count
    out.avg = np.where(depth != 0, total / (count + 1).astype(dtype), 0).astype(dtype)
    return out


def consistency_bands(scene, px_thr, rel_thr):
    """The float32 - float64 gap of the restatement on `scene` and what it leaves undecided.  -> namespace(r64, r32, gap_dist, gap_rel,
    gap_px, gap_avg, fragile (N,H,W) bool): a pixel is fragile -- left out of the count comparison -- if for some other view its dist or
    its relative difference lies within 4 x gap of its threshold, or 4 x gap_px (the gap of the texel coordinates) could change the tap
    rule's verdict or the sign test of z_s."""
    r64 = ref_depth_consistency(scene.depth, scene.K, scene.E, px_thr, rel_thr, np.float64)
    r32 = ref_depth_consistency(scene.depth, scene.K, scene.E, px_thr, rel_thr, np.float32)
    both = r64.geom & r32.geom

    def gap(a, b, m):
        return float(np.abs(a.astype(np.float64)[m] - b[m]).max()) if m.any() else 0.0

    g = types.SimpleNamespace(r64=r64, r32=r32, gap_dist=gap(r32.dist, r64.dist, both), gap_rel=gap(r32.rel, r64.rel, both),
                              gap_px=max(gap(r32.px, r64.px, both), gap(r32.py, r64.py, both)))
    agree = (r64.count == r32.count) & (scene.depth != 0)
    g.gap_avg = gap(r32.avg, r64.avg, agree)
    N, H, W = scene.depth.shape
    d32 = scene.depth.astype(np.float32)
    thr_px, thr_rel = np.float64(np.float32(px_thr)), np.float64(np.float32(rel_thr))
    fragile = np.zeros((N, H, W), dtype=bool)
    b = 4.0 * g.gap_px
    with np.errstate(invalid="ignore"):
        for r in range(N):
            for s in range(N):
                if s == r:
                    continue
                near = r64.geom[r, s] & ((np.abs(r64.dist[r, s] - thr_px) <= 4.0 * g.gap_dist) | (np.abs(r64.rel[r, s] - thr_rel) <= 4.0 * g.gap_rel))
                verdicts = [_taps_ok(r64.px[r, s] + sx * b, r64.py[r, s] + sy * b, d32[s], W, H)[0] for sx in (-1, 1) for sy in (-1, 1)]
                flips = np.any([v != verdicts[0] for v in verdicts[1:]], axis=0)
                sign = np.abs(r64.zs[r, s]) <= b
                fragile[r] |= (near | flips | sign) & (scene.depth[r] != 0)
    g.fragile = fragile
    return g


def ref_points_from_t(t, rays, fwd, dtype=np.float64):
    """The last step of the ray-geometry definition for a given depth t along the ray: -> (zdepth = t (d . fwd), points = o + t d)."""
    t, rays, fwd = (np.asarray(a).astype(dtype) for a in (t, rays, fwd))
    o, d = rays[:, :3], rays[:, 3:6]
    cosine = (d[:, 0] * fwd[0] + d[:, 1] * fwd[1]) + d[:, 2] * fwd[2]
    return t * cosine, o + t[:, None] * d


# ------------------------------------------------------------------------------------------- gen_rays and the way back to the pixel
def ref_gen_rays(E, Kmat, W, H, dtype=np.float64):
    """The rays of gen_rays (prep.hip, write_ray) in `dtype`: per pixel (i, j) of the row-major (H, W) list, origin -R^T t and direction
    R^T normalize(((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy, 1)) -> (H W, 6).  E, Kmat are rounded to float32 first: that is what the
    entry is given."""
    E, Kmat = np.asarray(E).astype(np.float32).astype(dtype), np.asarray(Kmat).astype(np.float32).astype(dtype)
    R, t = E[:3, :3], E[:3, 3]
    half = dtype(0.5)
    x = np.tile(((np.arange(W).astype(dtype) + half) - Kmat[0, 2]) / Kmat[0, 0], H)
    y = np.repeat(((np.arange(H).astype(dtype) + half) - Kmat[1, 2]) / Kmat[1, 1], W)
    nrm = np.sqrt((x * x + y * y) + dtype(1))
    dc = np.stack((x / nrm, y / nrm, dtype(1) / nrm), axis=1)
    d = np.stack([(R[0, k] * dc[:, 0] + R[1, k] * dc[:, 1]) + R[2, k] * dc[:, 2] for k in range(3)], axis=1)
    o = np.stack([-((R[0, k] * t[0] + R[1, k] * t[1]) + R[2, k] * t[2]) for k in range(3)])
    return np.concatenate((np.broadcast_to(o, d.shape), d), axis=1).astype(dtype)


def ref_round_trip(t, E, Kmat, W, H, dtype=np.float64):
    """Pixel -> ray (ref_gen_rays) -> point o + t d and zdepth t (d . row 2 of R) -> back through the camera, all in `dtype`:
    -> (u, v: the pixel coordinates the point projects to; dz: its camera z minus zdepth).  Exact arithmetic gives the pixel centres and
    0; float32 gives the error the chain has at the kernels' precision."""
    rays = ref_gen_rays(E, Kmat, W, H, dtype)
    E32, K32 = np.asarray(E).astype(np.float32).astype(dtype), np.asarray(Kmat).astype(np.float32).astype(dtype)
    zd, pts = ref_points_from_t(np.asarray(t).astype(dtype), np.concatenate((rays, rays[:, :2]), axis=1), E32[2, :3], dtype)
    R, tt = E32[:3, :3], E32[:3, 3]
    Xc = np.stack([((R[k, 0] * pts[:, 0] + R[k, 1] * pts[:, 1]) + R[k, 2] * pts[:, 2]) + tt[k] for k in range(3)], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):              # t = 0 (an invalid pixel) projects nowhere
        u = K32[0, 0] * (Xc[:, 0] / Xc[:, 2]) + K32[0, 2]
        v = K32[1, 1] * (Xc[:, 1] / Xc[:, 2]) + K32[1, 2]
    return u, v, Xc[:, 2] - zd
