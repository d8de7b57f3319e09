"""GPU: ray-casting the TSDF volume -- diner_tsdf_raycast_f32 / diner_tsdf_bricks through ops, TsdfVolume.raycast,
surface.sources_through_volume and evaluate.write_prediction_folder(write_volume_view=True).

  1  the kernel against the float64 restatement (tests/raycast_util.py) on the main scene: the hit mask equal outside the band the
     restatement cannot decide, zdepth / normal / rgb / weight at 4 x its float32 - float64 gap on common hits, misses exactly 0;
  2  with and without the brick mask: torch.equal on every output, and the mask equal to numpy's;
  3  V views in one call leave the bits of V single-view calls; 17 views through TsdfVolume.raycast;
  4  hand-made volumes: a plane, all-positive / all-unobserved / all-negative, znear, zfar, min_weight, NaN and exact-0 corners;
  5  refusals leave sentinel-filled outputs untouched;
  6  the Python layer, rendering untouched.

Every shape is 40 x 32 pixels on volumes of 2^3 .. 67 x 33 x 31."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import raycast_util as RU
from tests import surface_util as S

pytestmark = pytest.mark.gpu
SEED = 20261019
H, W = S.CAM_H, S.CAM_W


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()              # a copy: the shared scenes are read-only


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def cast(ops, tsdf, wsum, color4, origin, voxel, Kmat, E, zfar, step, znear=0.0, min_weight=0.0, bricks=False):
    """ops.tsdf_raycast on numpy planes; bricks True: with the device's own brick mask."""
    t, w, c4 = cuda(tsdf), cuda(wsum), cuda(color4)
    b = ops.tsdf_bricks(t, w, min_weight) if bricks else None
    return ops.tsdf_raycast(t, w, c4, origin, voxel, torch.from_numpy(np.asarray(Kmat)), torch.from_numpy(np.asarray(E)), W, H, znear, zfar,
                            step, min_weight=min_weight, bricks=b)


def same_bits(a, b):
    for x, y, name in zip(a, b, a._fields):
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(bits(x), bits(y)), name


def against_restatement(out, r64, r32, band, label):
    """The kernel's maps against the restatement's: hit mask outside the band, every quantity at 4 x gap on common hits, zeros."""
    z = out.zdepth.cpu().numpy()
    hit = z > 0
    ok = ~band
    line = f"{label}: band {int(band.sum())} of {band.size} rays, hits {int(r64.hit.sum())}"
    assert np.array_equal(hit[ok], r64.hit[ok]), line
    common = hit & r64.hit & r32.hit & ok
    pairs = [("zdepth", z, r64.zdepth, r32.zdepth, common), ("weight", out.weight.cpu().numpy(), r64.weight, r32.weight, common),
             ("normal", out.normal.cpu().numpy(), r64.normal, r32.normal, np.broadcast_to(common[:, None], r64.normal.shape))]
    if r64.rgb is not None:
        pairs.append(("rgb", out.rgb.cpu().numpy(), r64.rgb, r32.rgb, np.broadcast_to(common[:, None], r64.rgb.shape)))
    else:
        assert out.rgb is None
    for name, got, want, want32, m in pairs:
        gap = float(np.abs(want32.astype(np.float64) - want)[m].max())
        err = float(np.abs(got - want)[m].max())
        line += f"; {name} err {err:.3e} / tol {4 * gap:.3e} ({int((got[m] != want32[m]).sum())} values off the float32 restatement's)"
        miss = np.broadcast_to(~hit if got.ndim == 3 else ~hit[:, None], got.shape)
        assert (got[miss] == 0).all(), name                              # a miss is exactly 0 everywhere
    print(line)
    for name, got, want, want32, m in pairs:
        gap = float(np.abs(want32.astype(np.float64) - want)[m].max())
        assert float(np.abs(got - want)[m].max()) <= 4 * gap, line
    return line


# ------------------------------------------------------------------------------------------------------------------ 1 main scene
@pytest.mark.parametrize("n,carve,step_voxels", RU.MAIN_CASES)
def test_main_scene_against_restatement(ops, n, carve, step_voxels):
    p = RU.cast_pair(n, carve, step_voxels)
    v = p.vol
    assert p.band.reshape(3, -1).mean(axis=1).max() <= 0.02
    for use_bricks in (False, True):
        out = cast(ops, v.tsdf, v.wsum, v.color4, v.origin, v.voxel, p.K, p.E, p.zfar, p.step, bricks=use_bricks)
        against_restatement(out, p.r64, p.r32, p.band, f"n={n} carve={carve} step={step_voxels} voxel bricks={use_bricks}")
    if not carve:
        assert p.r64.behind.sum() > 0 and (out.zdepth.cpu().numpy()[p.r64.behind & ~p.band] == 0).all()


# -------------------------------------------------------------------------------------------------- 2 with and without the bricks
def sphere_67():
    dims, voxel, origin = (67, 33, 31), 0.03, (-1.0, -0.49, -0.46)
    t = S.sphere_tsdf(dims, origin, voxel, 0.4, 0.09)
    return t, np.ones_like(t), None, origin, voxel


def brick_cases():
    main = RU.fused_scene(16, True)
    unc = RU.fused_scene(16, False)
    big = RU.fused_scene(24, True)
    odd = RU.fused_scene(16, True, dims=(17, 13, 9))
    Kmat, E = RU.cameras()
    std = (Kmat, E, 2.0)
    cases = {"main": ((main.tsdf, main.wsum, main.color4, main.origin, main.voxel), std),
             "main uncarved": ((unc.tsdf, unc.wsum, unc.color4, unc.origin, unc.voxel), std),
             "24^3": ((big.tsdf, big.wsum, big.color4, big.origin, big.voxel), std),
             "17 x 13 x 9": ((odd.tsdf, odd.wsum, odd.color4, odd.origin, odd.voxel), std)}
    # 67 x 33 x 31, 9 x 4 x 4 bricks: a camera outside, one inside the volume (in free space), one most of whose rays pass the box by
    far = S.look_at((1.6, 0.2, 0.1))
    far[:3, 3] += np.array([0.9, 0.0, 0.0])                              # the camera moves sideways: the box leaves the image
    Ks, Es = RU.cameras(((1.6, 0.2, 0.1), (-0.8, 0.1, 0.05), (1.6, 0.2, 0.1)))
    Es[2] = far.astype(np.float32)
    cases["67 x 33 x 31"] = (sphere_67(), (Ks, Es, 3.0))
    return cases


@pytest.mark.parametrize("name", ["main", "main uncarved", "24^3", "17 x 13 x 9", "67 x 33 x 31"])
def test_bricks_change_no_bit(ops, name):
    (t, w, c4, origin, voxel), (Kmat, E, zfar) = brick_cases()[name]
    mask = ops.tsdf_bricks(cuda(t), cuda(w))
    ref = RU.ref_bricks(t, w)
    assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), ref)
    for step in (0.5 * voxel, voxel):
        plain = cast(ops, t, w, c4, origin, voxel, Kmat, E, zfar, step)
        quick = cast(ops, t, w, c4, origin, voxel, Kmat, E, zfar, step, bricks=True)
        same_bits(plain, quick)
        hits = (plain.zdepth > 0).sum(dim=(1, 2)).tolist()
        print(f"{name} step {step / voxel} voxel: bricks {int(ref.sum())} of {ref.size} live, hits a view {hits}")
        assert hits[0] > 100
    if name == "67 x 33 x 31":
        assert 0 < int(ref.sum()) < ref.size
        r64 = RU.ref_raycast(t, w, None, origin, voxel, Kmat, E, H, W, 0.0, zfar, voxel)
        r32 = RU.ref_raycast(t, w, None, origin, voxel, Kmat, E, H, W, 0.0, zfar, voxel, dtype=np.float32)
        against_restatement(quick, r64, r32, RU.raycast_band(r64, r32), name)
        assert r64.hit[1].sum() > 100 and 0 < r64.hit[2].sum() < 0.5 * r64.hit[0].sum()      # inside: hits; sideways: few
        # a mask of another min_weight is another mask
        w2 = w.copy()
        w2[:, :, 40:] = 0.5
        assert np.array_equal(ops.tsdf_bricks(cuda(t), cuda(w2), 0.75).cpu().numpy(), RU.ref_bricks(t, w2, 0.75))
        assert not np.array_equal(RU.ref_bricks(t, w2, 0.75), ref)


# ------------------------------------------------------------------------------------------------- 3 one call = V calls, bit for bit
def sixteen_cameras():
    eyes = list(S.EYES) + [RU.NOVEL_EYE] + [tuple(1.3 * c for c in e) for e in S.EYES] + [(-0.7, 0.6, -0.4), (0.5, -0.8, 0.3), (0.2, 0.3, 0.25)]
    return RU.cameras(tuple(eyes))


@pytest.mark.parametrize("V", [1, 3, 16])
def test_one_call_equals_single_view_calls(ops, V):
    v = RU.fused_scene(16, True)
    Kmat, E = sixteen_cameras()
    Kmat, E = Kmat[:V], E[:V]
    for use_bricks in (False, True):
        one = cast(ops, v.tsdf, v.wsum, v.color4, v.origin, v.voxel, Kmat, E, 2.5, 0.5 * v.voxel, bricks=use_bricks)
        assert one.zdepth.shape == (V, H, W) and one.normal.shape == (V, 3, H, W) and one.rgb.shape == (V, 3, H, W)
        for n in range(V):
            single = cast(ops, v.tsdf, v.wsum, v.color4, v.origin, v.voxel, Kmat[n:n + 1], E[n:n + 1], 2.5, 0.5 * v.voxel, bricks=use_bricks)
            same_bits(type(one)(*(x[n:n + 1] for x in one)), single)
    assert ((one.zdepth > 0).sum(dim=(1, 2)) > 0).all()


def test_seventeen_views_through_the_volume(ops):
    from diner_amd.surface import TsdfVolume
    v = RU.fused_scene(16, True)
    vol = TsdfVolume(v.origin, v.voxel, v.dims, trunc=v.trunc, device="cuda")
    vol.tsdf.copy_(cuda(v.tsdf)), vol.wsum.copy_(cuda(v.wsum)), vol.color4.copy_(cuda(v.color4))
    Kmat, E = sixteen_cameras()
    Kmat, E = np.concatenate((Kmat, Kmat[:1])), np.concatenate((E, E[3:4]))
    out = vol.raycast(torch.from_numpy(E), torch.from_numpy(Kmat), W, H)
    assert out["zdepth"].shape == (17, 1, H, W) and out["normal"].shape == (17, 3, H, W) and out["valid"].dtype == torch.bool
    for n in (0, 3, 15, 16):                                              # each launch's zfar is its farthest camera's: no bit changes
        single = vol.raycast(torch.from_numpy(E[n:n + 1]), torch.from_numpy(Kmat[0]), W, H, accelerate=False)
        for k in ("zdepth", "normal", "rgb", "weight", "points", "valid"):
            assert torch.equal(out[k][n:n + 1], single[k]), (n, k)
    assert torch.equal(out["zdepth"][16], out["zdepth"][3])


# ------------------------------------------------------------------------------------------------------------ 4 hand-made volumes
def plane_camera():
    return RU.cameras(((-1.2, 0.15, 0.1),))


def test_plane(ops):
    t, w = RU.plane_volume()
    Kmat, E = plane_camera()
    origin, voxel = RU.PLANE_ORIGIN, RU.PLANE_VOXEL
    args = (t, w, None, origin, voxel, Kmat, E)
    r64 = RU.ref_raycast(*args, H, W, 0.0, 3.0, 0.05)
    r32 = RU.ref_raycast(*args, H, W, 0.0, 3.0, 0.05, dtype=np.float32)
    band = RU.raycast_band(r64, r32)
    assert band.mean() <= 0.02 and r64.hit.sum() > 500
    for use_bricks in (False, True):
        out = cast(ops, *args, 3.0, 0.05, bricks=use_bricks)
        against_restatement(out, r64, r32, band, f"plane bricks={use_bricks}")
    # a trilinear interpolant of a linear field is exact: the depth is the plane's, the normal is R (-1, 0, 0)
    E64 = E[0].astype(np.float64)
    R, tr = E64[:3, :3], E64[:3, 3]
    eye = -R.T @ tr
    Kd = Kmat[0].astype(np.float64)
    x = (np.arange(W) + 0.5 - Kd[0, 2]) / Kd[0, 0]
    y = (np.arange(H) + 0.5 - Kd[1, 2]) / Kd[1, 1]
    dwx = R[0, 0] * x[None, :] + R[1, 0] * y[:, None] + R[2, 0]
    xp = float(np.float32(origin[0])) + RU.PLANE_X0 * float(np.float32(voxel))
    z_plane = (xp - eye[0]) / dwx
    m = r64.hit[0] & ~band[0]
    z = out.zdepth.cpu().numpy()[0]
    gap = float(np.abs(r32.zdepth.astype(np.float64) - r64.zdepth)[0][m].max())
    err = float(np.abs(z - z_plane)[m].max())
    nrm = out.normal.cpu().numpy()[0]
    gap_n = float(np.abs(r32.normal.astype(np.float64) - r64.normal)[0][:, m].max())
    err_n = float(np.abs(nrm - (-R[:, 0])[:, None, None])[:, m].max())
    print(f"plane: {int(m.sum())} hits, depth vs analytic err {err:.3e} / tol {4 * gap:.3e}; normal vs -R[:,0] err {err_n:.3e} / tol "
          f"{4 * gap_n:.3e}")
    assert err <= 4 * gap and err_n <= 4 * gap_n
    assert (out.weight.cpu().numpy()[0][m] == 1).all()


def test_volumes_without_a_surface_seen(ops):
    Kmat, E = plane_camera()
    origin, voxel = RU.PLANE_ORIGIN, RU.PLANE_VOXEL
    t, w = RU.plane_volume()

    def zeros(out):
        return all(float(x.abs().max()) == 0.0 for x in out if x is not None)

    def run(tt, ww, **kw):
        a = dict(zfar=3.0, step=0.05)
        a.update(kw)
        return [cast(ops, tt, ww, None, origin, voxel, Kmat, E, bricks=b, **a) for b in (False, True)]

    for label, tt, ww in (("all positive", np.ones_like(t), w), ("all unobserved", t, np.zeros_like(w)),
                          ("all negative", -np.ones_like(t), w)):        # the last: entered out of unknown space, never a hit
        for out in run(tt, ww):
            assert zeros(out), label
    one = np.ones((2, 2, 2), np.float32)
    for out in run(one, one) + run(-one, one):
        assert zeros(out)
    base = run(t, w)[0]
    zb = base.zdepth[base.zdepth > 0]
    assert zb.numel() > 500
    # znear beyond the surface: the first observed sample is negative; zfar short of it: the lattice runs out
    for out in run(t, w, znear=float(zb.max()) + 0.1) + run(t, w, zfar=float(zb.min()) - 0.1):
        assert zeros(out)
    # znear in front of the surface changes nothing
    for out in run(t, w, znear=float(zb.min()) - 0.2):
        same_bits(out, base)
    # min_weight above some corners' weight: the rays that end in those cells become misses, as the restatement says
    w2 = w.copy()
    w2[:, :4, :] = 0.5
    for out in run(t, w2, min_weight=0.75):
        r64 = RU.ref_raycast(t, w2, None, origin, voxel, Kmat, E, H, W, 0.0, 3.0, 0.05, min_weight=0.75)
        r32 = RU.ref_raycast(t, w2, None, origin, voxel, Kmat, E, H, W, 0.0, 3.0, 0.05, min_weight=0.75, dtype=np.float32)
        against_restatement(out, r64, r32, RU.raycast_band(r64, r32), "min_weight 0.75")
        lost = (base.zdepth > 0) & ~(out.zdepth > 0)
        assert int(lost.sum()) > 50 and not ((out.zdepth > 0) & ~(base.zdepth > 0)).any()
    for out in run(t, w2):
        same_bits(type(out)(out.zdepth, out.normal, None, None), type(out)(base.zdepth, base.normal, None, None))
    # a NaN corner and an exact-0 corner are positive: alone they end no march, and in free space they move no hit
    t3 = np.ones_like(t)
    t3[4, 5, 6], t3[3, 4, 5] = np.float32("nan"), 0.0
    for out in run(t3, w):
        assert zeros(out)
    t4 = t.copy()
    t4[4, 5, 1], t4[3, 4, 2] = np.float32("nan"), 0.0
    for out in run(t4, w):
        assert torch.equal(bits(out.zdepth), bits(base.zdepth))


# ---------------------------------------------------------------------------------------------------------------------- 5 refusals
def test_refusals_touch_nothing(ops):
    from diner_amd import _lib
    from tests.test_raycast_cpu import REFUSALS, host_cameras, raycast_entry
    lib = _lib.load()
    planes = [torch.ones(8, 8, 8, device="cuda"), torch.ones(8, 8, 8, device="cuda"), torch.zeros(4, 8, 8, 8, device="cuda")]
    outs = [torch.full(s, -7.0, device="cuda") for s in ((16, 4, 4), (16, 3, 4, 4), (16, 3, 4, 4), (16, 4, 4))]
    ptrs = tuple(C.c_void_p(x.data_ptr()) for x in planes + outs)
    for kw, what in REFUSALS:
        assert raycast_entry(lib, ptrs, host_cameras(), **kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())
    torch.cuda.synchronize()
    assert all(bool((x == -7).all()) for x in outs)
    assert raycast_entry(lib, ptrs, host_cameras(), V=16) == 0
    torch.cuda.synchronize()
    assert all(bool((x == 0).all()) for x in outs)                      # an all-positive volume: every ray a miss, every output written


# ------------------------------------------------------------------------------------------------------------------ 6 Python layer
def test_volume_raycast_on_the_sphere(ops):
    from diner_amd.geometry import backproject
    from diner_amd.surface import TsdfVolume
    sc = S.main_scene(16, 6)
    vol = TsdfVolume(sc.origin, float(sc.voxel), sc.dims, trunc=float(sc.trunc), device="cuda")
    vol.integrate(cuda(sc.depth)[:, None], torch.from_numpy(sc.K[0]), torch.from_numpy(sc.E), rgb=cuda(sc.color), carve=True)
    Kmat, E = RU.cameras()
    out = vol.raycast(torch.from_numpy(E).cuda(), torch.from_numpy(Kmat[0]), W, H)
    assert sorted(out) == ["extrinsics", "normal", "normals", "points", "rgb", "valid", "weight", "zdepth"]
    assert out["zdepth"].shape == out["weight"].shape == out["valid"].shape == (3, 1, H, W)
    assert out["normal"].shape == out["rgb"].shape == out["points"].shape == (3, 3, H, W) and out["normals"] is out["normal"]
    assert out["valid"].dtype == torch.bool and torch.equal(out["valid"], out["zdepth"] > 0)
    assert torch.equal(out["points"], backproject(out["zdepth"], torch.from_numpy(Kmat), torch.from_numpy(E)))
    plain = vol.raycast(torch.from_numpy(E), torch.from_numpy(Kmat), W, H, accelerate=False)
    for k in ("zdepth", "normal", "rgb", "weight"):
        assert torch.equal(bits(out[k]), bits(plain[k])), k
    z, nrm, valid = out["zdepth"].cpu().numpy()[:, 0], out["normal"].cpu().numpy(), out["valid"].cpu().numpy()[:, 0]
    x = (np.arange(W) + 0.5 - Kmat[0, 0, 2]) / Kmat[0, 0, 0]
    y = (np.arange(H) + 0.5 - Kmat[0, 1, 2]) / Kmat[0, 1, 1]
    for v, eye in enumerate((S.EYES[0], S.EYES[4], RU.NOVEL_EYE)):
        d, color, _ = S.sphere_maps(S.look_at(eye), Kmat[v].astype(np.float64), W, H)
        m = valid[v] & (d > 0)
        err = np.abs(z[v] - d)[m] / float(sc.voxel)
        dot = -(nrm[v, 0] * x[None, :] + nrm[v, 1] * y[:, None] + nrm[v, 2])          # normal . (-ray), the ray being d_c
        away = int((dot[valid[v]] <= 0).sum())
        cerr = np.abs(out["rgb"].cpu().numpy()[v] - color)[:, m].max()
        print(f"view {v}: {int(valid[v].sum())} hits, depth error mean {err.mean():.3f} max {err.max():.3f} voxel, colour error max "
              f"{cerr:.3f}, normals facing away {away}, min normal . (-ray) {dot[valid[v]].min():.4f}")
        assert m.sum() > 380 and err.mean() < 0.5
        assert np.abs(np.linalg.norm(nrm[v], axis=0)[valid[v]] - 1).max() < 1e-5
        # Camera 0 is left out of this one check: on 3 of its 408 hits -- grazing silhouette rays -- the float64 restatement itself gives
        # normal . (-ray) = -0.002 .. -0.07 (the gradient of the cell the interpolated depth falls in need not fall along the ray).
        if v > 0:
            assert (dot[valid[v]] > 0).all()
    vol_plain = TsdfVolume(sc.origin, float(sc.voxel), sc.dims, trunc=float(sc.trunc), color=False, device="cuda")
    vol_plain.integrate(cuda(sc.depth)[:, None], torch.from_numpy(sc.K[0]), torch.from_numpy(sc.E), carve=True)
    bare = vol_plain.raycast(torch.from_numpy(E), torch.from_numpy(Kmat), W, H)
    assert bare["rgb"] is None and torch.equal(bits(bare["zdepth"]), bits(out["zdepth"]))


def test_sources_through_volume(ops):
    """The main scene with a 6 x 6 block of view 0's depth zeroed.  With carve=True the block is filled from the other five views and its
    depths are the restatement chain's.  With the default carve=False it is NOT filled on this scene (the float64 chain fills 0 of its
    36 pixels, and at most 11 of 36 wherever the block is put): a hit needs an observed sample in front of the surface, and without
    carving the free space in front of the hole was observed by view 0 alone -- the other cameras see it next to the sphere, not on it.
    The default call is held to the definitions of `filled` and `agree` only."""
    from diner_amd.surface import sources_through_volume
    sc = S.main_scene(16, 6)
    depth = sc.depth.copy()
    rows, cols = slice(16, 22), slice(20, 26)
    assert (depth[0, rows, cols] > 0).all()
    depth[0, rows, cols] = 0.0
    batch = dict(src_depths=torch.from_numpy(depth)[None, :, None], src_rgbs=torch.from_numpy(sc.color)[None],
                 src_intrinsics=torch.from_numpy(sc.K)[None], src_extrinsics=torch.from_numpy(sc.E)[None])
    lo = np.asarray(sc.origin, dtype=np.float64)
    hi = lo + 15 * float(sc.voxel)
    block = np.zeros(depth.shape, dtype=bool)
    block[0, rows, cols] = True
    d_true, _, _ = S.sphere_maps(S.look_at(S.EYES[0]), sc.K[0].astype(np.float64), W, H)
    for carve in (True, None):
        kw = {} if carve is None else dict(carve=carve)
        out, vol = sources_through_volume(batch, bounds=(lo, hi), voxel=float(sc.voxel), trunc=float(sc.trunc), **kw)
        assert vol.dims == (16, 16, 16) and sorted(out) == ["agree", "filled", "src_depths", "src_normals"]
        assert out["src_depths"].shape == out["filled"].shape == out["agree"].shape == (6, 1, H, W)
        assert out["src_normals"].shape == (6, 3, H, W) and out["filled"].dtype == out["agree"].dtype == torch.bool
        z = out["src_depths"].cpu().numpy()[:, 0]
        filled, agree = out["filled"].cpu().numpy()[:, 0], out["agree"].cpu().numpy()[:, 0]
        assert not (filled & (depth != 0)).any() and np.array_equal(filled, (depth == 0) & (z > 0))
        assert np.array_equal(agree, (depth > 0) & (z > 0) & (np.abs(z - depth) <= np.float32(vol.trunc)))
        # the restatement chain on the volume sources_through_volume chose: ref_integrate, then ref_raycast with raycast's defaults
        t0, w0, c0 = S.fresh_volume(vol.dims, True)
        origin, voxel = vol.origin.numpy(), np.float32(vol.voxel)
        zfar = float(np.float32(RU.far_corner(sc.E, origin, voxel, vol.dims).max()))
        chain = {}
        for dtype in (np.float64, np.float32):
            r = S.ref_integrate(t0, w0, c0, origin, voxel, np.float32(vol.trunc), depth, None, sc.color, sc.K, sc.E, bool(carve), dtype=dtype)
            if dtype is np.float64:
                mark = S.integration_band(r, W, H)
            chain[dtype] = RU.ref_raycast(r.tsdf.astype(np.float32), r.wsum.astype(np.float32), None, origin, voxel, sc.K, sc.E, H, W, 0.0,
                                          zfar, 0.5 * float(voxel), dtype=dtype, mark=mark)
        r64, r32 = chain[np.float64], chain[np.float32]
        # the ray-cast's own band, capped as everywhere; and, on top of it, the rays that end in a cell with a voxel the INTEGRATION
        # cannot decide (surface_util.integration_band): a few voxels, each met by the rays of several views
        band = RU.raycast_band(r64, r32)
        assert band.reshape(6, -1).mean(axis=1).max() <= 0.02
        undecided = r64.marked | r32.marked
        ok = ~(band | undecided)
        hit = z > 0
        common = hit & r64.hit & r32.hit & ok
        gap = float(np.abs(r32.zdepth.astype(np.float64) - r64.zdepth)[common].max())
        err = float(np.abs(z - r64.zdepth)[common].max())
        sphere = np.abs(z[0] - d_true)[rows, cols][hit[0][rows, cols]] / float(voxel)
        rest = np.abs(z[0] - d_true)[hit[0] & ~block[0] & (d_true > 0)] / float(voxel)
        print(f"sources_through_volume carve={bool(carve)}: band {int(band.sum())} + {int((undecided & ~band).sum())} rays at {int(mark.sum())} "
              f"undecided voxels, of {band.size}; hits {int(hit.sum())}, filled {int(filled.sum())} ({int(filled[0, rows, cols].sum())} of 36 "
              f"in the block), agree {int(agree.sum())} of {int((depth > 0).sum())}; depth err {err:.3e} / tol {4 * gap:.3e}; against the "
              f"sphere: the block mean {sphere.mean() if sphere.size else float('nan'):.3f} max "
              f"{sphere.max() if sphere.size else float('nan'):.3f} voxel, the rest of view 0 mean {rest.mean():.3f}")
        assert np.array_equal(hit[ok], r64.hit[ok])
        assert err <= 4 * gap
        if carve:
            assert filled[0, rows, cols].all() and (common & block).sum() == 36      # filled from the other five views, all comparable


def test_volume_view_files_and_rendering_untouched(ops, tmp_path):
    from diner_amd import evaluate, noise
    from diner_amd.png import read_png
    from diner_amd.render import predict_image
    from diner_amd.surface import mesh_from_sources
    from tests.test_geometry_gpu import model
    case, nerf, ren, E, Kt = model()
    sc, w, h = case.sc, case.w, case.h

    def renders():
        rays = ops.gen_rays(E, Kt, w, h, sc["znear"], sc["zfar"], "cuda")[:, 100:900].contiguous()
        with torch.no_grad(), noise.keyed(SEED, 100):
            f = ren.forward(nerf, rays, want_alpha=True).fine
        return predict_image(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED), f

    before = renders()
    g = torch.Generator().manual_seed(3)
    nv = sc["depths"].shape[0]
    batch = dict(src_depths=sc["depths"][None], src_rgbs=torch.rand(1, nv, 3, h, w, generator=g), src_intrinsics=sc["src_intrinsics"][None],
                 src_extrinsics=sc["src_extrinsics"][None], target_rgb=torch.rand(1, 3, h, w, generator=g), sample_name=["view0"],
                 target_extrinsics=sc["target_extrinsics"][None], target_intrinsics=case.Kt[None])
    encode, nerf.encode = nerf.encode, lambda **kw: None               # the scene is injected, as everywhere in this suite
    import diner_amd.datasets as datasets
    orig, datasets.encode_args = datasets.encode_args, lambda b, dev: {}
    try:
        for name, kw in (("plain", {}), ("view", dict(write_volume_view=True)), ("both", dict(write_volume_view=True, write_mesh=True)),
                         ("mesh", dict(write_mesh=True))):
            torch.manual_seed(5)
            evaluate.write_prediction_folder(nerf, ren, [batch], str(tmp_path / name), sc["znear"], sc["zfar"], **kw)
    finally:
        datasets.encode_args = orig
        nerf.encode = encode
    files = {name: sorted(os.listdir(tmp_path / name)) for name in ("plain", "view", "both", "mesh")}
    extra = ["view0-vdepth.png", "view0-vnormal.png"]
    assert files["plain"] == ["view0-depth.png", "view0-gt.png", "view0-pred.png", "view0-ref.png"]
    assert files["view"] == sorted(files["plain"] + extra) and files["both"] == sorted(files["mesh"] + extra)
    for name, base in (("view", "plain"), ("both", "mesh"), ("both", "view")):
        for f in files[base]:
            assert open(tmp_path / base / f, "rb").read() == open(tmp_path / name / f, "rb").read(), (name, f)
    vd, vn = read_png(str(tmp_path / "view" / "view0-vdepth.png")), read_png(str(tmp_path / "view" / "view0-vnormal.png"))
    assert vd.shape == vn.shape == (h, w, 3)
    _, vol = mesh_from_sources(batch)
    view = vol.raycast(batch["target_extrinsics"][0:1], batch["target_intrinsics"][0:1], w, h)
    hit = view["valid"][0, 0].cpu().numpy()
    print(f"volume view of the culling scene: volume {vol.dims}, {int(hit.sum())} of {hit.size} pixels see the prior's surface")
    assert hit.sum() > 0 and (np.asarray(vn)[~hit] == 128).all()       # a miss has the normal 0: mid-grey

    after = renders()
    for a_, b_ in zip(before[0], after[0]):
        assert torch.equal(a_, b_)
    for k in before[1]:
        assert torch.equal(bits(before[1][k]), bits(after[1][k])), k
