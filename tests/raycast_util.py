"""Shared by tests/test_raycast_cpu.py and tests/test_raycast_gpu.py: the numpy restatement of raycast.hip's two definitions -- the
ray-cast of a TSDF volume and its brick mask -- written from include/diner_hip.h and evaluated in a dtype of the caller's choice:
float64 is what the kernel is measured against, float32 gives the error of the definition itself at the kernel's precision
(tests/surface_util.py's convention).  The scenes come from tests/surface_util.py.  No GPU is touched here."""
import functools
import types

import numpy as np

from tests import surface_util as S

BAND_F = 1e-5                        # an observed sample with |f| <= BAND_F may fall on either side of 0 in fp32
NOVEL_EYE = (0.7, 0.6, 0.4)
MAX_SAMPLES = 1 << 20


def corners(a):
    """(Nz,Ny,Nx) -> (8, Nz-1, Ny-1, Nx-1): corner c = x + 2 y + 4 z of every cell."""
    Nz, Ny, Nx = a.shape
    return np.stack([a[(c >> 2):Nz - 1 + (c >> 2), ((c >> 1) & 1):Ny - 1 + ((c >> 1) & 1), (c & 1):Nx - 1 + (c & 1)] for c in range(8)])


def ref_bricks(tsdf, wsum, min_weight=0.0):
    """diner_tsdf_bricks: (nbz,nby,nbx) uint8, 1 iff some cell of the brick of 8^3 cells has 8 observed corners and a negative one."""
    t32, w32 = np.asarray(tsdf, dtype=np.float32), np.asarray(wsum, dtype=np.float32)
    live = corners(w32 > np.float32(min_weight)).all(axis=0) & corners(t32 < 0).any(axis=0)
    nb = [(n + 7) // 8 for n in live.shape]
    pad = np.zeros([8 * n for n in nb], dtype=bool)
    pad[:live.shape[0], :live.shape[1], :live.shape[2]] = live
    return pad.reshape(nb[0], 8, nb[1], 8, nb[2], 8).any(axis=(1, 3, 5)).astype(np.uint8)


def ref_raycast(tsdf, wsum, color4, origin, voxel, Kmat, E, H, W, znear, zfar, step, min_weight=0.0, bricks=None, dtype=np.float64,
                mark=None):
    """diner_tsdf_raycast_f32's definition in `dtype`, every operation in the order the header gives (the inputs are the float32 values
    the entry receives).  Kmat (V,3,3), E (V,4,4).  bricks (nbz,nby,nbx) or None: a sample whose cell lies in a 0-brick is not
    evaluated at all -- what the kernel's jumps amount to.
    -> namespace(zdepth (V,H,W), normal (V,3,H,W), rgb (V,3,H,W) | None, weight (V,H,W), hit (V,H,W) bool, n_term (V,H,W) int: the
    terminating lattice index or 0, small (V,H,W) bool: an observed sample up to termination had |f| <= BAND_F, behind (V,H,W) bool: the
    march ended at a negative sample whose predecessor was not observed, marked (V,H,W) bool: with mark (Nz,Ny,Nx) bool given, a
    corner of the cell of the terminating sample, of its predecessor or of the hit point is marked)."""
    t32, w32 = np.asarray(tsdf, dtype=np.float32), np.asarray(wsum, dtype=np.float32)
    Nz, Ny, Nx = t32.shape
    N = (Nx, Ny, Nz)
    seen_c = w32 > np.float32(min_weight)
    t = t32.astype(dtype)
    w = w32.astype(dtype)
    c4 = None if color4 is None else np.asarray(color4, dtype=np.float32).astype(dtype)
    origin = np.asarray(origin, dtype=np.float32).astype(dtype)
    voxel, znear, zfar, step = (dtype(np.float32(x)) for x in (voxel, znear, zfar, step))
    Kmat, E = np.asarray(Kmat, dtype=np.float32).astype(dtype), np.asarray(E, dtype=np.float32).astype(dtype)
    V = E.shape[0]
    one, zero, half = dtype(1), dtype(0), dtype(0.5)
    R, tr = E[:, :3, :3], E[:, :3, 3]
    col = np.arange(W).astype(dtype)[None, None, :]
    row = np.arange(H).astype(dtype)[None, :, None]
    full = (V, H, W)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dcx = np.broadcast_to(((col + half) - Kmat[:, 0, 2, None, None]) / Kmat[:, 0, 0, None, None], full)
        dcy = np.broadcast_to(((row + half) - Kmat[:, 1, 2, None, None]) / Kmat[:, 1, 1, None, None], full)
        eye = [-((R[:, 0, a] * tr[:, 0] + R[:, 1, a] * tr[:, 1]) + R[:, 2, a] * tr[:, 2])[:, None, None] for a in range(3)]
        dw = [(R[:, 0, a, None, None] * dcx + R[:, 1, a, None, None] * dcy) + R[:, 2, a, None, None] for a in range(3)]
        dz = step / np.sqrt((dcx * dcx + dcy * dcy) + one)
        n_all = int(np.floor(float(zfar) / float(dz.min()))) + 2
        assert n_all <= MAX_SAMPLES

        def lerp(a, b, wt):
            return a + wt * (b - a)

        def cell_of(z):
            g = [((eye[a] + z * dw[a]) - origin[a]) / voxel for a in range(3)]
            fl = [np.clip(np.nan_to_num(np.floor(g[a]), nan=0.0), 0, N[a] - 2) for a in range(3)]
            idx = [fl[a].astype(np.int64) for a in range(3)]
            m = [g[a] - fl[a].astype(dtype) for a in range(3)]
            ins = np.ones(full, dtype=bool)
            for a in range(3):
                ins &= (g[a] >= 0) & (g[a] <= dtype(N[a] - 1))
            return idx, m, ins

        def gather(plane, idx):
            i, j, k = idx
            return [plane[k + (c >> 2), j + ((c >> 1) & 1), i + (c & 1)] for c in range(8)]

        def tri(f, m):
            a0, a1, a2, a3 = lerp(f[0], f[1], m[0]), lerp(f[2], f[3], m[0]), lerp(f[4], f[5], m[0]), lerp(f[6], f[7], m[0])
            return lerp(lerp(a0, a1, m[1]), lerp(a2, a3, m[1]), m[2])

        def sample(n):
            """-> (observed, f, looked, z): looked = the sample is evaluated at all (always, without bricks)."""
            z = dtype(n) * dz
            idx, m, ins = cell_of(z)
            ins = ins & (z >= znear)
            obs = ins & np.all(gather(seen_c, idx), axis=0)
            f = tri(gather(t, idx), m)
            looked = np.ones(full, dtype=bool)
            if bricks is not None:
                looked = np.asarray(bricks)[idx[2] >> 3, idx[1] >> 3, idx[0] >> 3] != 0
            if mark is not None:
                touched[0] = np.any(gather(mark, idx), axis=0)
            return obs, f, looked, z

        touched = [np.zeros(full, dtype=bool)]
        marked = np.zeros(full, dtype=bool)
        alive = np.ones(full, dtype=bool)
        n_term = np.zeros(full, dtype=np.int64)
        f_n = np.zeros(full, dtype=dtype)
        small = np.zeros(full, dtype=bool)
        for n in range(1, n_all + 1):
            obs, f, looked, z = sample(n)
            alive &= z <= zfar
            if not alive.any():
                break
            use = alive & obs & looked
            small |= use & (np.abs(f) <= BAND_F)
            end = use & (f < 0)
            n_term = np.where(end, n, n_term)
            marked |= end & touched[0]
            f_n = np.where(end, f, f_n)
            alive &= ~end
        # the predecessor of the terminating sample, evaluated afresh (never through the brick mask); sample 0 is never observed
        hit = np.zeros(full, dtype=bool)
        f_p = np.zeros(full, dtype=dtype)
        for n in np.unique(n_term):
            if n < 2:
                continue
            obs, f, _, _ = sample(n - 1)
            sel = (n_term == n) & obs
            hit |= sel
            marked |= sel & touched[0]
            f_p = np.where(sel, f, f_p)
        z_p = (n_term - 1).astype(dtype) * dz
        zd = np.where(hit, z_p + dz * (f_p / (f_p - f_n)), zero)
        idx, m, _ = cell_of(zd)
        f = gather(t, idx)
        if mark is not None:
            marked |= hit & np.any(gather(mark, idx), axis=0)
        gx = lerp(lerp(f[1] - f[0], f[3] - f[2], m[1]), lerp(f[5] - f[4], f[7] - f[6], m[1]), m[2])
        gy = lerp(lerp(f[2] - f[0], f[3] - f[1], m[0]), lerp(f[6] - f[4], f[7] - f[5], m[0]), m[2])
        gz = lerp(lerp(f[4] - f[0], f[5] - f[1], m[0]), lerp(f[6] - f[2], f[7] - f[3], m[0]), m[1])
        ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = hit & (ln > 0)
        nw = [np.where(ok, g / ln, zero) for g in (gx, gy, gz)]
        normal = np.stack([np.where(ok, (R[:, a, 0, None, None] * nw[0] + R[:, a, 1, None, None] * nw[1]) + R[:, a, 2, None, None] * nw[2], zero)
                           for a in range(3)], axis=1)
        rgb = None
        if c4 is not None:
            den = tri(gather(c4[3], idx), m)
            okc = hit & (den > 0)
            rgb = np.stack([np.where(okc, tri(gather(c4[ch], idx), m) / den, zero) for ch in range(3)], axis=1)
        weight = np.where(hit, tri(gather(w, idx), m), zero)
    return types.SimpleNamespace(zdepth=zd, normal=normal, rgb=rgb, weight=weight, hit=hit, n_term=n_term, small=small,
                                 behind=(n_term > 0) & ~hit, marked=marked)


def raycast_band(r64, r32):
    """(V,H,W) bool: the rays whose outcome fp32 may decide the other way -- the float64 run saw |f| <= BAND_F at an observed sample up
    to termination, or the two runs disagree on hit / miss or on the terminating index."""
    return r64.small | (r64.hit != r32.hit) | (r64.n_term != r32.n_term)


# -------------------------------------------------------------------------------------------------------------------- the scenes
def cameras(eyes=None):
    """Source cameras 0 and 4 of the main scene and the novel camera: -> (K (3,3,3), E (3,4,4)) float32."""
    eyes = (S.EYES[0], S.EYES[4], NOVEL_EYE) if eyes is None else eyes
    Kmat = np.array([[S.FOCAL, 0.0, S.CAM_W / 2.0], [0.0, S.FOCAL, S.CAM_H / 2.0], [0.0, 0.0, 1.0]])
    E = np.stack([S.look_at(e) for e in eyes])
    return np.repeat(Kmat[None], len(eyes), axis=0).astype(np.float32), E.astype(np.float32)


def far_corner(E, origin, voxel, dims):
    """Per camera, the distance from the eye to the farthest corner of the volume's box: what zfar=None means."""
    E = np.asarray(E, dtype=np.float64)
    lo = np.asarray(origin, dtype=np.float64)
    hi = lo + (np.asarray(dims, dtype=np.float64) - 1) * float(voxel)
    box = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    eye = -np.einsum("vba,vb->va", E[:, :3, :3], E[:, :3, 3])
    return np.linalg.norm(box[None] - eye[:, None], axis=-1).max(axis=1)


@functools.lru_cache(maxsize=None)
def fused_scene(n=16, carve=True, dims=None):
    """The main scene (six views) fused with ref_integrate in float32 -- the volume the device would hold, up to its band -- into
    float32 planes of n^3 samples (or `dims`, from the same origin at the same voxel): -> namespace(tsdf, wsum, color4, origin, voxel,
    trunc, dims, sc).  Shared and never modified."""
    sc = S.main_scene(n, 6)
    dims = sc.dims if dims is None else dims
    t0, w0, c0 = S.fresh_volume(dims, True)
    r = S.ref_integrate(t0, w0, c0, sc.origin, sc.voxel, sc.trunc, sc.depth, None, sc.color, sc.K, sc.E, carve, dtype=np.float32)
    out = types.SimpleNamespace(tsdf=r.tsdf.astype(np.float32), wsum=r.wsum.astype(np.float32), color4=r.color4.astype(np.float32),
                                origin=sc.origin, voxel=float(sc.voxel), trunc=float(sc.trunc), dims=dims, sc=sc)
    for a in (out.tsdf, out.wsum, out.color4):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cast_pair(n=16, carve=True, step_voxels=0.5):
    """The restatement on fused_scene(n, carve) into the three cameras, zfar = 2, in float64 and float32, and the band: shared by the
    CPU and the GPU tests.  -> namespace(vol, K, E, zfar, step, r64, r32, band)."""
    vol = fused_scene(n, carve)
    Kmat, E = cameras()
    zfar, step = 2.0, step_voxels * vol.voxel
    args = (vol.tsdf, vol.wsum, vol.color4, vol.origin, vol.voxel, Kmat, E, S.CAM_H, S.CAM_W, 0.0, zfar, step)
    r64 = ref_raycast(*args)
    r32 = ref_raycast(*args, dtype=np.float32)
    return types.SimpleNamespace(vol=vol, K=Kmat, E=E, zfar=zfar, step=step, r64=r64, r32=r32, band=raycast_band(r64, r32))


MAIN_CASES = [(16, True, 0.5), (16, True, 1.0), (16, False, 0.5), (16, False, 1.0), (24, True, 0.5), (24, True, 1.0)]


PLANE_DIMS, PLANE_X0, PLANE_VOXEL, PLANE_ORIGIN = (12, 10, 9), 5.25, 0.1, (-0.55, -0.45, -0.4)


def plane_volume(dims=PLANE_DIMS, x0=PLANE_X0):
    """tsdf = (x0 - i) / 4, a linear ramp in x (free space below the plane i = x0, solid above) whose values float32 holds exactly,
    wsum = 1: -> (tsdf, wsum) float32."""
    Nx, Ny, Nz = dims
    t = np.broadcast_to(((x0 - np.arange(Nx)) / 4.0).astype(np.float32)[None, None, :], (Nz, Ny, Nx)).copy()
    return t, np.ones_like(t)
