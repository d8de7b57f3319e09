"""Shared by tests/test_surface_cpu.py and tests/test_surface_gpu.py: numpy restatements of the two definitions of surface.hip -- TSDF
integration and naive surface nets, written from include/diner_hip.h and evaluated in a dtype of the caller's choice: float64 is what
the kernels are measured against, float32 gives the error of the definition itself at the kernels' precision -- the mesh checks
(closed, oriented, Euler characteristic, signed volume) and the analytic scene builders.  No GPU is touched here."""
import functools
import types

import numpy as np

RADIUS = 0.25
EYES = ((1, .1, .05), (-1, .05, .1), (.1, 1, .05), (.05, -1, .1), (.1, .05, 1), (.05, .1, -1))
CAM_W, CAM_H, FOCAL = 40, 32, 45.0
VOXEL, ORIGIN, TRUNC = 0.05, (-0.387, -0.393, -0.397), 0.15
BAND_PX, BAND_TRUNC = 1e-4, 1e-4


# ------------------------------------------------------------------------------------------------------------------- the scene
def look_at(eye):
    """World->camera (4,4) float64 of a camera at `eye` looking at the origin: rows of R = right, down, forward; right = f x up with
    up = z, or y when |f_z| >= 0.9."""
    eye = np.asarray(eye, dtype=np.float64)
    f = -eye / np.linalg.norm(eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(f[2]) >= 0.9 else np.array([0.0, 0.0, 1.0])
    right = np.cross(f, up)
    right /= np.linalg.norm(right)
    down = np.cross(f, right)
    E = np.eye(4)
    E[:3, :3] = np.stack((right, down, f))
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def sphere_maps(E, Kmat, W, H, radius=RADIUS):
    """Analytic maps of the sphere of `radius` at the origin: z-depth (H,W) (0 off the sphere), colour (3,H,W) = 0.5 + 0.5 normal (0 off
    it) and the cosine between the normal and the ray back to the camera (H,W), all float64."""
    R, t = E[:3, :3], E[:3, 3]
    eye = -R.T @ t
    x = (np.arange(W) + 0.5 - Kmat[0, 2]) / Kmat[0, 0]
    y = (np.arange(H) + 0.5 - Kmat[1, 2]) / Kmat[1, 1]
    dc = np.stack(np.broadcast_arrays(x[None, :], y[:, None], np.ones((H, W))), axis=-1)          # camera frame, z = 1
    dw = dc @ R                                                                                     # R^T d per pixel
    a = (dw * dw).sum(-1)
    b = 2.0 * dw @ eye
    c = eye @ eye - radius * radius
    disc = b * b - 4 * a * c
    hit = disc > 0
    s = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)                      # the camera-z depth: d has z = 1
    P = eye + s[..., None] * dw
    n = P / radius
    depth = np.where(hit, s, 0.0)
    color = np.where(hit[None], 0.5 + 0.5 * np.moveaxis(n, -1, 0), 0.0)
    cosine = np.where(hit, -(n * dw).sum(-1) / np.sqrt(a), 0.0)
    return depth, color, cosine


@functools.lru_cache(maxsize=None)
def main_scene(n=16, N=6):
    """The main scene: the sphere seen by the six 40 x 32 cameras (N = 1: the first; N = 16: the six repeated, four dropped), and an n^3
    volume of voxel 0.8 / n -- 0.05 at n = 16 -- from the same origin, truncated at 3 voxels.
    -> namespace(depth (N,H,W), color (N,3,H,W), weight (N,H,W) float32; K (N,3,3), E (N,4,4) float32; origin, voxel, trunc, dims)."""
    Kmat = np.array([[FOCAL, 0.0, CAM_W / 2.0], [0.0, FOCAL, CAM_H / 2.0], [0.0, 0.0, 1.0]])
    ids = [i % 6 for i in range(N)]
    E = np.stack([look_at(EYES[i]) for i in ids])
    maps = [sphere_maps(E[v], Kmat, CAM_W, CAM_H) for v in range(N)]
    voxel = VOXEL * 16.0 / n
    return types.SimpleNamespace(depth=np.stack([m[0] for m in maps]).astype(np.float32),
                                 color=np.stack([m[1] for m in maps]).astype(np.float32),
                                 weight=np.stack([m[2] for m in maps]).astype(np.float32),
                                 K=np.repeat(Kmat[None], N, axis=0).astype(np.float32), E=E.astype(np.float32),
                                 origin=np.array(ORIGIN, dtype=np.float32), voxel=np.float32(voxel), trunc=np.float32(TRUNC * voxel / VOXEL),
                                 dims=(n, n, n), N=N, W=CAM_W, H=CAM_H)


def fresh_volume(dims, color=True, dtype=np.float32):
    Nx, Ny, Nz = dims
    return (np.ones((Nz, Ny, Nx), dtype=dtype), np.zeros((Nz, Ny, Nx), dtype=dtype),
            np.zeros((4, Nz, Ny, Nx), dtype=dtype) if color else None)


# ----------------------------------------------------------------------------------------------------------------- integration
def ref_integrate(tsdf, wsum, color4, origin, voxel, trunc, depth, weight, color, Kmat, E, carve, max_weight=0.0, dtype=np.float64):
    """diner_tsdf_integrate_f32's definition in `dtype`, every operation in the order the header gives (the inputs are the float32
    values the entry receives).  tsdf, wsum (Nz,Ny,Nx), color4 (4,Nz,Ny,Nx) | None are NOT modified.
    -> namespace(tsdf, wsum, color4, and per view (N,Nz,Ny,Nx): used (the view updated the voxel), painted (it updated the colour sums),
    edge (distance in pixels to the nearest pixel edge, inf where the voxel is behind the camera), cut (|sdf + trunc| and
    |sdf - trunc| / trunc, inf where there is no surface))."""
    f = np.asarray(tsdf).astype(dtype).copy()
    ws = np.asarray(wsum).astype(dtype).copy()
    c4 = None if color4 is None else np.asarray(color4).astype(dtype).copy()
    origin = np.asarray(origin, dtype=np.float32).astype(dtype)
    voxel, trunc, max_weight = dtype(np.float32(voxel)), dtype(np.float32(trunc)), dtype(np.float32(max_weight))
    depth = np.asarray(depth, dtype=np.float32)
    N, H, W = depth.shape
    Kmat, E = np.asarray(Kmat, dtype=np.float32).astype(dtype), np.asarray(E, dtype=np.float32).astype(dtype)
    Nz, Ny, Nx = f.shape
    p0 = (origin[0] + np.arange(Nx).astype(dtype) * voxel)[None, None, :]
    p1 = (origin[1] + np.arange(Ny).astype(dtype) * voxel)[None, :, None]
    p2 = (origin[2] + np.arange(Nz).astype(dtype) * voxel)[:, None, None]
    shape = (N, Nz, Ny, Nx)
    out = types.SimpleNamespace(used=np.zeros(shape, bool), painted=np.zeros(shape, bool), edge=np.full(shape, np.inf),
                                cut=np.full(shape, np.inf))
    one = dtype(1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for n in range(N):
            R, t = E[n, :3, :3], E[n, :3, 3]
            x = ((R[0, 0] * p0 + R[0, 1] * p1) + R[0, 2] * p2) + t[0]
            y = ((R[1, 0] * p0 + R[1, 1] * p1) + R[1, 2] * p2) + t[1]
            z = ((R[2, 0] * p0 + R[2, 1] * p1) + R[2, 2] * p2) + t[2]
            front = z > 0
            u = Kmat[n, 0, 0] * (x / z) + Kmat[n, 0, 2]
            v = Kmat[n, 1, 1] * (y / z) + Kmat[n, 1, 2]
            inside = front & (u >= 0) & (u < W) & (v >= 0) & (v < H)
            pj = np.where(inside, np.floor(u), 0).astype(np.int64)
            pi = np.where(inside, np.floor(v), 0).astype(np.int64)
            wp = (np.ones((H, W), np.float32) if weight is None else np.asarray(weight, dtype=np.float32)[n])[pi, pj].astype(dtype)
            D = depth[n][pi, pj].astype(dtype)
            sdf = D - z
            surface = D > 0
            hidden = surface & (sdf < -trunc)
            d = np.where(surface, np.minimum(one, sdf / trunc), one)
            use = inside & (wp > 0) & ((surface & ~hidden) | ((D == 0) & bool(carve)))
            wn = ws + wp
            f = np.where(use, (f * ws + d * wp) / wn, f)
            ws = np.where(use, np.minimum(wn, max_weight) if max_weight > 0 else wn, ws)
            paint = use & surface & (sdf <= trunc)
            if c4 is not None:
                cn = np.asarray(color, dtype=np.float32)[n].astype(dtype)
                for ch in range(3):
                    c4[ch] = np.where(paint, c4[ch] + wp * cn[ch][pi, pj], c4[ch])
                c4[3] = np.where(paint, c4[3] + wp, c4[3])
            out.used[n], out.painted[n] = use, paint
            eu = np.minimum(np.abs(u - np.round(u)), np.abs(v - np.round(v)))
            out.edge[n] = np.where(front, eu, np.inf)
            seen = inside & (wp > 0) & surface
            out.cut[n] = np.where(seen, np.minimum(np.abs(sdf + trunc), np.abs(sdf - trunc)) / trunc, np.inf)
    out.tsdf, out.wsum, out.color4 = f, ws, c4
    return out


def integration_band(r64, W, H):
    """(Nz,Ny,Nx) bool: the voxels some view's skip decision could go either way in fp32 -- within BAND_PX of a pixel edge (the image
    border is one) or within BAND_TRUNC trunc of the -trunc cut (or of the +trunc cut, which decides the colour sums)."""
    return ((r64.edge <= BAND_PX) | (r64.cut <= BAND_TRUNC)).any(axis=0)


# ---------------------------------------------------------------------------------------------------------------- surface nets
def ref_surface_nets(tsdf, wsum, color4, origin, voxel, min_weight=0.0, dtype=np.float64):
    """The mesh definition of diner_surface_extract_f32 in `dtype`.  Topology (ids, faces) depends on exact comparisons of the float32
    inputs only.  -> namespace(vertices, normals (nv,3), rgb (nv,3) | None, faces (2 nq,3) int32, cells (nv,3) int: i, j, k)."""
    t32, w32 = np.asarray(tsdf, dtype=np.float32), np.asarray(wsum, dtype=np.float32)
    Nz, Ny, Nx = t32.shape
    neg = t32 < 0                                   # an exact 0 and a NaN are positive
    seen = w32 > np.float32(min_weight)

    def corners(a):                                 # (8, Nz-1, Ny-1, Nx-1), corner c = x + 2 y + 4 z
        return np.stack([a[(c >> 2):Nz - 1 + (c >> 2), ((c >> 1) & 1):Ny - 1 + ((c >> 1) & 1), (c & 1):Nx - 1 + (c & 1)] for c in range(8)])

    n_neg = corners(neg).sum(axis=0)
    active = corners(seen).all(axis=0) & (n_neg > 0) & (n_neg < 8)
    kk, jj, ii = np.nonzero(active)                 # linear cell order, x fastest
    nv = len(ii)
    vid = np.full((Nz, Ny, Nx), -1, dtype=np.int64)
    vid[kk, jj, ii] = np.arange(nv)
    f = corners(t32)[:, kk, jj, ii].astype(dtype)   # (8, nv)
    zero, one = dtype(0), dtype(1)
    s = [np.zeros(nv, dtype=dtype) for _ in range(3)]
    cnt = np.zeros(nv, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for axis in range(3):
            step = 1 << axis
            for a in range(8):
                if a & step:
                    continue
                fa, fb = f[a], f[a + step]
                cross = (fa < 0) != (fb < 0)
                t = fa / (fa - fb)
                base = (dtype(a & 1), dtype((a >> 1) & 1), dtype(a >> 2))
                for ax in range(3):
                    s[ax] = np.where(cross, s[ax] + (t if ax == axis else base[ax]), s[ax])
                cnt = np.where(cross, cnt + one, cnt)
        m = [s[ax] / cnt for ax in range(3)]
        origin = np.asarray(origin, dtype=np.float32).astype(dtype)
        voxel = dtype(np.float32(voxel))
        cell = (ii.astype(dtype), jj.astype(dtype), kk.astype(dtype))
        vertices = np.stack([origin[ax] + voxel * (cell[ax] + m[ax]) for ax in range(3)], axis=1)

        def lerp(a, b, t):
            return a * (one - t) + b * t

        def tri(g):
            a0, a1, a2, a3 = lerp(g[0], g[1], m[0]), lerp(g[2], g[3], m[0]), lerp(g[4], g[5], m[0]), lerp(g[6], g[7], m[0])
            return lerp(lerp(a0, a1, m[1]), lerp(a2, a3, m[1]), m[2])

        def bil(d00, d10, d01, d11, p, q):
            return lerp(lerp(d00, d10, p), lerp(d01, d11, p), q)

        gx = bil(f[1] - f[0], f[3] - f[2], f[5] - f[4], f[7] - f[6], m[1], m[2])
        gy = bil(f[2] - f[0], f[3] - f[1], f[6] - f[4], f[7] - f[5], m[0], m[2])
        gz = bil(f[4] - f[0], f[5] - f[1], f[6] - f[2], f[7] - f[3], m[0], m[1])
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = ln > 0
        normals = np.stack([np.where(ok, g / ln, zero) for g in (gx, gy, gz)], axis=1)
        rgb = None
        if color4 is not None:
            c32 = np.asarray(color4, dtype=np.float32)
            den = tri(corners(c32[3])[:, kk, jj, ii].astype(dtype))
            okc = den > 0
            rgb = np.stack([np.where(okc, tri(corners(c32[ch])[:, kk, jj, ii].astype(dtype)) / den, zero) for ch in range(3)], axis=1)

    # quads: per grid sample in linear order, then the x-, y-, z-edge
    act = np.zeros((Nz + 1, Ny + 1, Nx + 1), dtype=bool)           # padded by one on the low side: act[k+1, j+1, i+1] = cell (i,j,k)
    act[1:Nz, 1:Ny, 1:Nx] = active
    quads = []
    for axis in range(3):
        ua, va = (axis + 1) % 3, (axis + 2) % 3
        sl_a = [slice(None)] * 3
        sl_b = [slice(None)] * 3
        dim = 2 - axis                                             # numpy axis of the grid axis (arrays are [k, j, i])
        sl_a[dim], sl_b[dim] = slice(0, -1), slice(1, None)
        na, nb = neg[tuple(sl_a)], neg[tuple(sl_b)]
        kq, jq, iq = np.nonzero(na != nb)
        for k, j, i in zip(kq, jq, iq):
            p = [i, j, k]

            def cell_at(du, dv):
                q = list(p)
                q[ua] -= du
                q[va] -= dv
                return q

            ring = [cell_at(1, 1), cell_at(0, 1), cell_at(0, 0), cell_at(1, 0)]       # counter-clockwise seen from +axis
            if not all(act[c[2] + 1, c[1] + 1, c[0] + 1] for c in ring):
                continue
            ids = [int(vid[c[2], c[1], c[0]]) for c in ring]
            if not neg[k, j, i]:
                ids = [ids[0], ids[3], ids[2], ids[1]]
            quads.append(((k * Ny + j) * Nx + i, axis, ids))
    quads.sort(key=lambda q: (q[0], q[1]))
    faces = np.array([tri_ for q in quads for tri_ in ((q[2][0], q[2][1], q[2][2]), (q[2][0], q[2][2], q[2][3]))], dtype=np.int32).reshape(-1, 3)
    return types.SimpleNamespace(vertices=vertices, normals=normals, rgb=rgb, faces=faces, cells=np.stack((ii, jj, kk), axis=1),
                                 n_vertices=nv, n_quads=len(quads))


# ------------------------------------------------------------------------------------------------------------------ mesh checks
def mesh_stats(vertices, faces):
    """-> namespace(euler (V - E + F with the quads' diagonals as edges), boundary_edges (undirected edges used once), bad_edges (used
    more than twice), directed_twice (directed edges used more than once), closed, oriented, volume (signed))."""
    vertices, faces = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    if len(faces) == 0:
        return types.SimpleNamespace(euler=len(vertices), boundary_edges=0, bad_edges=0, directed_twice=0, closed=False, oriented=True,
                                     volume=0.0, n_edges=0)
    d = np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]))
    _, dc = np.unique(d, axis=0, return_counts=True)
    _, uc = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    a, b, c = (vertices[faces[:, n]] for n in range(3))
    volume = float((a * np.cross(b, c)).sum() / 6.0)
    used = len(np.unique(faces))
    boundary, bad, twice = int((uc == 1).sum()), int((uc > 2).sum()), int((dc > 1).sum())
    return types.SimpleNamespace(euler=used - len(uc) + len(faces), boundary_edges=boundary, bad_edges=bad, directed_twice=twice,
                                 closed=boundary == 0 and bad == 0, oriented=twice == 0, volume=volume, n_edges=len(uc))


def sphere_tsdf(dims, origin, voxel, radius, trunc):
    """min(1, (|p| - radius) / trunc) clipped at -1, written straight into a (Nz,Ny,Nx) float32 volume."""
    Nx, Ny, Nz = dims
    x = origin[0] + np.arange(Nx) * voxel
    y = origin[1] + np.arange(Ny) * voxel
    z = origin[2] + np.arange(Nz) * voxel
    r = np.sqrt(x[None, None, :] ** 2 + y[None, :, None] ** 2 + z[:, None, None] ** 2)
    return np.clip((r - radius) / trunc, -1.0, 1.0).astype(np.float32)
