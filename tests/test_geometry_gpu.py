"""GPU: geometry from renders -- diner_ray_geometry_f32 / diner_depth_consistency_f32 through ops, NeRFRendererDGS.forward_geometry,
render.predict_geometry, diner_amd.geometry and evaluate.write_prediction_folder(write_geometry=True).

  1  the ray reduction against the float64 restatement (tests/geometry_util.py): NR not a multiple of the workgroup's 4 rays, K in both
     per-lane layouts with a partial last lane, two quantiles, both point modes, the hand-made rays; median_idx exact on every ray
     the worst-case fp32 summation bound decides, depth_median bit-equal to z[idx], depth_mean / zdepth / points at 4 x the float32 -
     float64 gap of the restatement; single-output calls give the bits of the all-output call; bad arguments launch nothing;
  2  through the modules on the 48 x 40 culling scene: predict_geometry's colour, depth and opacity are predict_image's bits, forward is
     untouched by a forward_geometry call, the points re-project onto their pixel centres at their zdepth, the normals are
     depth2normal of the zdepth; a planted density spike on an analytic plane gives points on the plane and its normal;
  3  the consistency check against its restatement on three cameras looking at a plane (a scaled patch, a hole, a turned camera), on
     two cameras and on sixteen;
  4  fuse_views and write_prediction_folder(write_geometry=True) end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import cull_util as U
from tests import geometry_util as G

pytestmark = pytest.mark.gpu
K, NG, N_CAND, SEED = 40, 15, U.N_CAND, 20261019


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ----------------------------------------------------------------------------------------------------------------- 1 ray geometry
@pytest.mark.parametrize("Kz", G.K_LIST)
def test_ray_geometry_against_restatement(ops, Kz):
    case = G.ray_case(Kz)
    w, z, rays = cuda(case.w), cuda(case.z), cuda(case.rays)
    for q in G.quantiles_for(Kz):
        for mode, name in ((0, "median"), (1, "mean")):
            ref = G.ref_ray_geometry(case.w, case.z, case.rays, case.fwd, q, G.ALPHA_MIN, mode)
            amb = G.ambiguous_rays(ref, case.w, G.ALPHA_MIN)
            tol, gap = G.ray_tolerances(case, q, mode, ~amb)
            out = ops.ray_geometry(w, z, rays, cam_fwd=torch.from_numpy(case.fwd), quantile=q, alpha_min=G.ALPHA_MIN, point_depth=name)
            idx = out.median_idx.cpu().numpy()
            d_med, d_mean = out.depth_median.cpu().numpy(), out.depth_mean.cpu().numpy()
            zd, pts = out.zdepth.cpu().numpy(), out.points.cpu().numpy()
            ok = ~amb
            share = float((amb & ref.valid)[:G.NR_RANDOM].sum()) / float(ref.valid[:G.NR_RANDOM].sum())
            err = {f: float(np.abs(v.astype(np.float64) - getattr(ref, f))[ok & ref.valid].max())
                   for f, v in (("depth_mean", d_mean), ("zdepth", zd), ("points", pts))}
            print(f"K={Kz} q={q} {name}: left out {share:.3f}; err {err}; tolerance {tol}")
            assert idx.dtype == np.int32 and share <= 0.05
            assert np.array_equal(idx[ok], ref.idx[ok])
            # every ray, decided or not: the index is in range, the median is that sample's depth bit for bit, an invalid ray is 0 / -1
            valid = idx >= 0
            assert (idx[valid] < Kz).all() and np.array_equal(d_med[valid].view(np.int32), case.z[np.flatnonzero(valid), idx[valid]].view(np.int32))
            for a in (d_med, d_mean, zd, pts):
                assert (a[~valid].view(np.int32) == 0).all()
            assert (idx[~valid] == -1).all() and (~valid).sum() >= 3
            for f, v in (("depth_mean", d_mean), ("zdepth", zd), ("points", pts)):
                assert err[f] <= tol[f], (f, err[f], tol[f])
            # the hand-made rays are exact in any summation order
            h = case.hand
            if "tie" in h and q == 0.5:
                assert idx[h["tie"]] == 1
            assert idx[h["spike"]] == Kz // 2
            assert [idx[h[n]] for n in ("below_alpha_min", "at_alpha_min", "above_alpha_min")] == [-1, -1, 0]
            if "negative_last" in h:
                assert idx[h["negative_last"]] == ref.idx[h["negative_last"]] and valid[h["negative_last"]]
        # without cam_fwd: no zdepth, everything else the same bits
        plain = ops.ray_geometry(w, z, rays, quantile=q, alpha_min=G.ALPHA_MIN, point_depth="mean")
        assert plain.zdepth is None
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(plain, out) if a is not None)


@pytest.mark.parametrize("Kz", [65, 1024])
def test_single_output_calls_and_refusals(ops, Kz):
    from diner_amd import _lib
    lib = _lib.load()
    case = G.ray_case(Kz)
    w, z, rays = cuda(case.w), cuda(case.z), cuda(case.rays)
    fwd = (C.c_float * 3)(*case.fwd.tolist())
    NR = case.NR
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(outs, NR_=NR, K_=Kz, q=0.5, cam=fwd):
        return lib.diner_ray_geometry_f32(w.data_ptr(), z.data_ptr(), rays.data_ptr(), NR_, K_, q, G.ALPHA_MIN, cam, 0,
                                          *(None if o is None else C.c_void_p(o.data_ptr()) for o in outs), st)

    def fresh():
        return [torch.full((NR,), -7.0, device="cuda"), torch.full((NR,), -7, device="cuda", dtype=torch.int32),
                torch.full((NR,), -7.0, device="cuda"), torch.full((NR,), -7.0, device="cuda"), torch.full((NR, 3), -7.0, device="cuda")]

    full = fresh()
    assert call(full) == 0
    for i in range(5):
        one = fresh()
        assert call([o if j == i else None for j, o in enumerate(one)]) == 0
        assert torch.equal(bits(one[i]), bits(full[i])), i
        assert all((bits(o) == bits(fresh()[j])).all() for j, o in enumerate(one) if j != i)
    assert call([None] * 5) == 0                                        # nothing to write is not an error
    # refused calls launch nothing: the sentinels stay
    kept = fresh()
    for kw in (dict(NR_=0), dict(K_=0), dict(K_=1025), dict(q=0.0), dict(q=1.5), dict(cam=None)):
        assert call(kept, **kw) == _lib.E_INVALID, kw
    torch.cuda.synchronize()
    assert all((bits(o) == bits(f)).all() for o, f in zip(kept, fresh()))
    # empty input: no launch, empty outputs
    out = ops.ray_geometry(w[:0], z[:0], rays[:0], cam_fwd=case.fwd)
    assert out.points.shape == (0, 3) and out.median_idx.shape == (0,) and out.zdepth.shape == (0,)


# ------------------------------------------------------------------------------------------------------------ 2 through the modules
_MODELS = {}


def model():
    """(scene case, PixelNeRF on the device, renderer, E (1,4,4), Kt (1,3,3)) of the 48 x 40 culling scene, built once per process."""
    if not _MODELS:
        from diner_amd.synthetic import build_modules
        case = U.scene_case()
        nerf, R = build_modules(case.sc, case.msd, "cuda", normals=case.sc["normals"])
        ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=NG, white_bkgd=True)
        _MODELS["m"] = (case, nerf, ren, case.sc["target_extrinsics"][None].cuda(), case.Kt[None].cuda())
    return _MODELS["m"]


@pytest.fixture(scope="module")
def frame(ops):
    from diner_amd.render import predict_geometry
    case, nerf, ren, E, Kt = model()
    return predict_geometry(nerf, ren, E, Kt, case.w, case.h, case.sc["znear"], case.sc["zfar"], seed=SEED)


def test_predict_geometry_is_predict_image_plus_geometry(ops, frame):
    from diner_amd.render import predict_geometry, predict_image
    case, nerf, ren, E, Kt = model()
    sc, w, h = case.sc, case.w, case.h
    rgb, depth, alpha = predict_image(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED, return_alpha=True)
    assert torch.equal(frame["rgb"], rgb) and torch.equal(frame["depth"], depth) and torch.equal(frame["alpha"], alpha)
    shapes = {k: tuple(v.shape) for k, v in frame.items()}
    one, three = (1, 1, h, w), (1, 3, h, w)
    assert shapes == dict(rgb=three, depth=one, alpha=one, depth_var=one, depth_median=one, depth_mean=one, zdepth=one, points=three,
                          valid=one, normals=three, extrinsics=(1, 4, 4))
    assert frame["valid"].dtype == torch.bool
    n_valid = int(frame["valid"].sum())
    print(f"{n_valid} of {w * h} pixels valid")
    assert 0 < n_valid < w * h                                           # at least one valid and one invalid pixel
    # the kernel's A and the compositor's alpha are the same sum in two orders: they can part on a ray within rounding of alpha_min
    assert (frame["valid"] ^ (frame["alpha"] > 1e-3)).sum() <= 0.01 * w * h
    inv = ~frame["valid"]
    for k in ("depth_median", "depth_mean", "zdepth"):
        assert (frame[k][inv] == 0).all()
    assert (frame["points"][inv.expand(-1, 3, -1, -1)] == 0).all()
    # the frame does not depend on the batch size
    again = predict_geometry(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED, ray_batch_size=777)
    assert all(torch.equal(again[k], frame[k]) for k in ("rgb", "depth", "alpha", "depth_median", "zdepth", "points", "valid"))
    # normals: depth2normal of the returned zdepth, the convention of the encoder's normal maps
    assert torch.equal(bits(frame["normals"]), bits(ops.depth2normal(frame["zdepth"], Kt)))
    # the mean normalised by the opacity; the median is one of the samples between near and far
    v = frame["valid"]
    assert torch.allclose(frame["depth_mean"][v] * frame["alpha"][v], frame["depth"][v], rtol=1e-5, atol=1e-6)
    assert (frame["depth_median"][v] > 0).all() and (frame["zdepth"][v] > 0).all() and (frame["zdepth"][v] <= frame["depth_median"][v] * (1 + 1e-6)).all()
    mean_mode = predict_geometry(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED, point_depth="mean")
    assert torch.equal(mean_mode["depth_median"], frame["depth_median"]) and not torch.equal(mean_mode["points"], frame["points"])


def test_forward_is_untouched_by_forward_geometry(ops):
    from diner_amd import noise
    case, nerf, ren, E, Kt = model()
    rays = ops.gen_rays(E, Kt, case.w, case.h, case.sc["znear"], case.sc["zfar"], "cuda")[:, 100:900].contiguous()
    fwd = E[:, 2, :3].cpu()
    with torch.no_grad():
        with noise.keyed(SEED, 100):
            before = ren.forward(nerf, rays, want_alpha=True).fine
        with noise.keyed(SEED, 100):
            geo = ren.forward_geometry(nerf, rays, cam_fwd=fwd, want_weights=True).fine
        with noise.keyed(SEED, 100):
            after = ren.forward(nerf, rays, want_alpha=True).fine
            plain = ren.forward(nerf, rays).fine
    assert sorted(after.keys()) == sorted(before.keys()) == ["alpha", "depth", "depth_var", "rgb"] and sorted(plain.keys()) == ["depth", "rgb"]
    for k in before:
        assert torch.equal(bits(before[k]), bits(after[k])) and torch.equal(bits(before[k]), bits(geo[k])), k
    assert sorted(geo.keys()) == ["alpha", "depth", "depth_mean", "depth_median", "depth_var", "median_idx", "points", "rgb", "weights",
                                  "zdepth"]
    assert geo.points.shape == (1, 800, 3) and geo.median_idx.dtype == torch.int32 and geo.weights.shape == (1, 800, K)
    with torch.no_grad():
        assert "zdepth" not in ren.forward_geometry(nerf, rays).fine and "weights" not in ren.forward_geometry(nerf, rays).fine
        with pytest.raises(ValueError):
            ren.forward_geometry(nerf, rays, cam_fwd=torch.zeros(2, 3))
    assert nerf.needs_grad()
    with pytest.raises(ValueError):                                      # no gradient flows through the geometry: grad mode is refused
        ren.forward_geometry(nerf, rays, cam_fwd=fwd)


def test_points_reproject_onto_their_pixels(ops, frame):
    case, nerf, ren, E, Kt = model()
    w, h = case.w, case.h
    rays = ops.gen_rays(E, Kt, w, h, case.sc["znear"], case.sc["zfar"], "cuda")[0].cpu().numpy()
    E64, K64 = E[0].cpu().numpy().astype(np.float64), Kt[0].cpu().numpy().astype(np.float64)
    v = frame["valid"][0, 0].cpu().numpy().reshape(-1)
    t = frame["depth_median"][0, 0].cpu().numpy().reshape(-1)
    pts = frame["points"][0].cpu().numpy().reshape(3, -1).T
    zd = frame["zdepth"][0, 0].cpu().numpy().reshape(-1)
    fwd = E[0, 2, :3].cpu().numpy()
    # the measured tolerance: 4 x the float32 - float64 gap of the definition's last step on these rays and depths
    zd64, p64 = G.ref_points_from_t(t, rays, fwd, np.float64)
    zd32, p32 = G.ref_points_from_t(t, rays, fwd, np.float32)
    tol_p, tol_z = 4 * np.abs(p32 - p64)[v].max(), 4 * np.abs(zd32 - zd64)[v].max()
    err_p, err_z = np.abs(pts - p64)[v].max(), np.abs(zd - zd64)[v].max()
    print(f"points err {err_p:.3e} (tolerance {tol_p:.3e}), zdepth err {err_z:.3e} (tolerance {tol_z:.3e})")
    assert err_p <= tol_p and err_z <= tol_z
    # back through the target camera in float64: the pixel centre, and a camera z equal to zdepth.  Tolerance: 4 x the float32 - float64
    # gap of the whole chain restated -- gen_rays, o + t d, t (d . fwd), R p + t, the projection -- at these depths
    Xc = pts.astype(np.float64) @ E64[:3, :3].T + E64[:3, 3]
    u = K64[0, 0] * Xc[:, 0] / Xc[:, 2] + K64[0, 2]
    vv = K64[1, 1] * Xc[:, 1] / Xc[:, 2] + K64[1, 2]
    jj, ii = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    u64, v64, dz64 = G.ref_round_trip(t, E64, K64, w, h, np.float64)
    u32, v32, dz32 = G.ref_round_trip(t, E64, K64, w, h, np.float32)
    tol_px = 4 * max(np.abs(u32 - u64)[v].max(), np.abs(v32 - v64)[v].max())
    tol_zc = 4 * np.abs(dz32 - dz64)[v].max()
    err_px = max(np.abs(u - jj.reshape(-1))[v].max(), np.abs(vv - ii.reshape(-1))[v].max())
    err_zc = np.abs(Xc[:, 2] - zd)[v].max()
    print(f"camera z err {err_zc:.3e} (tolerance {tol_zc:.3e}), pixel err {err_px:.3e} (tolerance {tol_px:.3e})")
    assert (Xc[v, 2] > 0).all() and err_zc <= tol_zc and err_px <= tol_px


def test_planted_plane(ops):
    """A density spike on an analytic plane for every ray of a 24 x 20 camera, through ops.composite and ops.ray_geometry only."""
    W, H, Kz = 24, 20, 48
    E64, K64 = G.look_at_camera((0.2, -0.1, 0.0), (0.0, 0.0, 2.0), 30.0, W, H, roll=0.04)
    E, Kt = torch.from_numpy(E64).float()[None], torch.from_numpy(K64).float()[None]
    rays = ops.gen_rays(E, Kt, W, H, 0.5, 4.0, "cuda")[0]
    r = rays.cpu().numpy().astype(np.float64)
    t_hit = (G.PLANE_D - r[:, :3] @ G.PLANE_N) / (r[:, 3:6] @ G.PLANE_N)          # along the fp32 rays the kernel is given
    assert (t_hit > 0.6).all() and (t_hit < 3.9).all()
    g = np.random.default_rng(5)
    z = np.sort(g.uniform(0.5, 4.0, (W * H, Kz)), axis=1)
    k_hit = np.clip((z < t_hit[:, None]).sum(axis=1), 1, Kz - 2)
    z[np.arange(W * H), k_hit] = t_hit
    z = np.sort(z, axis=1).astype(np.float32)
    k_hit = np.argmin(np.abs(z - t_hit[:, None].astype(np.float32)), axis=1)
    field = np.zeros((W * H, Kz, 4), dtype=np.float32)
    field[..., :3] = 0.5
    field[np.arange(W * H), k_hit, 3] = 1e6                                       # opaque at the planted sample, empty elsewhere
    wts, rgb, depth, alpha, var = ops.composite(cuda(field), cuda(z), rays, False, want_weights=True, want_aux=True)
    fwd = E[0, 2, :3]
    geo = ops.ray_geometry(wts, cuda(z), rays, cam_fwd=fwd)
    assert np.array_equal(geo.median_idx.cpu().numpy(), k_hit)
    pts = geo.points.cpu().numpy().astype(np.float64)
    # on the plane up to the rounding of t (half an ulp), of t d and of o + t d: 4 roundings of magnitudes below |o| + t
    off = np.abs(pts @ G.PLANE_N - G.PLANE_D).max()
    tol_plane = 4 * G.F32_EPS * np.sqrt(3.0) * (np.abs(r[:, :3]).max() + t_hit.max())
    print(f"planted plane: offset {off:.3e} (tolerance {tol_plane:.3e})")
    assert off <= tol_plane
    # the interior normals against the plane's, at 4 x the float32 - float64 gap of the depth2normal restatement on the plane's z-depth
    zd_map = geo.zdepth.view(1, 1, H, W)
    normals = ops.depth2normal(zd_map, Kt.cuda())[0, :, 1:-1, 1:-1].cpu().numpy().astype(np.float64)
    exact = G.plane_zdepth(E64, K64, W, H, G.PLANE_N, G.PLANE_D)
    n64 = G.ref_depth2normal_interior(exact, K64, np.float64)
    n32 = G.ref_depth2normal_interior(exact.astype(np.float32), K64.astype(np.float32), np.float32)
    n_cam = E64[:3, :3] @ G.PLANE_N
    n_cam = -n_cam if n_cam[2] > 0 else n_cam
    gap = np.abs(n32.astype(np.float64) - n64).max()
    err = np.abs(normals - n_cam[:, None, None]).max()
    print(f"planted plane: normal err {err:.3e}, restatement gap {gap:.3e} (tolerance {4 * gap:.3e})")
    assert np.abs(n64 - n_cam[:, None, None]).max() < 1e-12
    assert err <= 4 * gap


# ------------------------------------------------------------------------------------------------------------------ 3 consistency
def run_consistency(ops, sc, px_thr, rel_thr):
    count, avg = ops.depth_consistency(cuda(sc.depth.astype(np.float32)), torch.from_numpy(sc.K).float(), torch.from_numpy(sc.E).float(),
                                       px_thr, rel_thr)
    assert count.dtype == torch.int32 and count.shape == avg.shape == sc.depth.shape
    return count.cpu().numpy(), avg.cpu().numpy()


def check_consistency(ops, sc, px_thr=1.0, rel_thr=0.01):
    bands = G.consistency_bands(sc, px_thr, rel_thr)
    count, avg = run_consistency(ops, sc, px_thr, rel_thr)
    ok = ~bands.fragile
    share = float(bands.fragile.sum()) / float((sc.depth != 0).sum())
    same = ok & (count == bands.r64.count)
    err = float(np.abs(avg.astype(np.float64) - bands.r64.avg)[same].max())
    print(f"N={sc.N}: left out {share:.4f}; count mismatches {int((count != bands.r64.count)[ok].sum())}; depth_avg err {err:.3e} "
          f"(tolerance {4 * bands.gap_avg:.3e}); gaps dist {bands.gap_dist:.2e} rel {bands.gap_rel:.2e}")
    assert np.array_equal(count[ok], bands.r64.count[ok])
    assert err <= 4 * bands.gap_avg
    hole = sc.depth == 0
    assert (count[hole] == 0).all() and (avg[hole].view(np.int32) == 0).all()
    return bands, count, avg, share


def test_consistency_three_cameras_on_a_plane(ops):
    sc = G.consistency_scene(3)
    bands, count, avg, share = check_consistency(ops, sc)
    assert share <= 0.05
    assert (count[1][sc.patch] == 0).all() and (count[1][sc.hole] == 0).all() and count.max() == 2
    assert 0 < (count[0] == 2).sum() < sc.W * sc.H
    # one output at a time: the same bits
    from diner_amd import _lib
    lib = _lib.load()
    d = cuda(sc.depth.astype(np.float32))
    Km, E = torch.from_numpy(sc.K).float().contiguous(), torch.from_numpy(sc.E).float().contiguous()
    c1 = torch.full(sc.depth.shape, -7, device="cuda", dtype=torch.int32)
    a1 = torch.full(sc.depth.shape, -7.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.diner_depth_consistency_f32(d.data_ptr(), Km.data_ptr(), E.data_ptr(), 3, sc.H, sc.W, 1.0, 0.01, c1.data_ptr(), None, st) == 0
    assert lib.diner_depth_consistency_f32(d.data_ptr(), Km.data_ptr(), E.data_ptr(), 3, sc.H, sc.W, 1.0, 0.01, None, a1.data_ptr(), st) == 0
    assert np.array_equal(c1.cpu().numpy(), count) and np.array_equal(a1.cpu().numpy().view(np.int32), avg.view(np.int32))
    # a looser and a tighter threshold pair move the counts the way the restatement says
    for px_thr, rel_thr in ((1.0, 0.1), (1e-4, 1e-6)):
        check_consistency(ops, sc, px_thr, rel_thr)
    # (N,1,H,W) is taken as well
    c4, a4 = ops.depth_consistency(d[:, None], Km, E)
    assert np.array_equal(c4.cpu().numpy(), count)


@pytest.mark.parametrize("N", [2, 16])
def test_consistency_two_and_sixteen_cameras(ops, N):
    sc = G.consistency_scene(N, 16, 12)
    bands, count, avg, share = check_consistency(ops, sc)
    assert count.max() >= 1 and count.max() <= N - 1
    # N = 2: the cap of the three-camera scene.  N = 16 repeats four cameras: a border pixel re-projects onto the image edge of its twin
    # view, where rounding decides whether a tap is inside -- exactly the 52 border pixels of 16 x 12 (27 %) may be left out, no interior one
    interior = np.zeros(sc.depth.shape, dtype=bool)
    interior[:, 1:-1, 1:-1] = True
    assert not (bands.fragile & interior).any() if N == 16 else share <= 0.05


# ------------------------------------------------------------------------------------------------------------------- 4 end to end
def test_fuse_views(ops, tmp_path):
    from diner_amd.geometry import backproject, fuse_views, point_cloud, read_ply, write_ply
    case, nerf, ren, E, Kt = model()
    sc, w, h = case.sc, case.w, case.h
    turn = torch.eye(4)
    a = 0.06
    turn[0, 0], turn[0, 2], turn[2, 0], turn[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    Es = torch.stack((E[0].cpu(), turn @ E[0].cpu(), turn.T @ E[0].cpu())).cuda()
    xyz, rgb, nrm, views = fuse_views(nerf, ren, Es, Kt[0], w, h, sc["znear"], sc["zfar"], min_views=1, seed=SEED)
    assert len(views) == 3 and xyz.dtype == torch.float32 and rgb.dtype == torch.uint8 and xyz.shape == rgb.shape == nrm.shape
    zd = torch.cat([g["zdepth"] for g in views])
    count, avg = ops.depth_consistency(zd, Kt.cpu().expand(3, -1, -1), Es)
    assert all(torch.equal(g["count"][0, 0], count[v]) and torch.equal(g["depth_avg"][0, 0], avg[v]) for v, g in enumerate(views))
    keep = count >= 1
    M = int(keep.sum())
    print(f"fuse_views: {M} of {3 * w * h} pixels kept, counts {[int((count == c).sum()) for c in range(3)]}")
    assert 0 < M < 3 * w * h and xyz.shape == (M, 3)
    pts = backproject(avg[:, None], Kt.cpu().expand(3, -1, -1), Es)
    assert torch.equal(xyz, pts.permute(0, 2, 3, 1)[keep])
    # a kept pixel's fused point is near the view's own surface point (the depths agree to rel_thr)
    own = torch.cat([g["points"] for g in views]).permute(0, 2, 3, 1)[keep]
    assert ((xyz - own).norm(dim=-1) <= 0.02 * float(sc["zfar"])).all()
    assert fuse_views(nerf, ren, Es, Kt[0], w, h, sc["znear"], sc["zfar"], min_views=3, seed=SEED)[0].shape[0] == 0     # of 2 others
    # a single view's cloud, through the writer
    x1, c1, n1 = point_cloud(views[0])
    m = views[0]["valid"] & (views[0]["alpha"] >= 0.5)
    assert x1.shape[0] == int(m.sum()) > 0 and torch.equal(x1, views[0]["points"].permute(0, 2, 3, 1)[m[:, 0]])
    write_ply(tmp_path / "v0.ply", x1, c1, n1)
    x2, c2, n2 = read_ply(tmp_path / "v0.ply")
    assert x2.tobytes() == x1.cpu().numpy().tobytes() and c2.tobytes() == c1.cpu().numpy().tobytes() and n2.tobytes() == n1.cpu().numpy().tobytes()


def test_write_prediction_folder_with_geometry(ops, tmp_path):
    from diner_amd.datasets import DTUSamples, collate
    from diner_amd.evaluate import write_prediction_folder
    from diner_amd.geometry import read_ply
    from diner_amd.png import read_png
    from diner_amd.synthetic import make_mlp_state_dict
    from src.util.import_helper import import_obj
    from tests.helpers import GOLD
    from tests.test_boundary_cpu import build_nerf
    tree = os.path.join(GOLD, "dtu_tiny")
    ds = DTUSamples(tree, "val", scan_list=os.path.join(tree, "scan_list.txt"))
    torch.manual_seed(0)
    nerf = build_nerf().cuda().eval()
    nerf.mlp_fine.load_state_dict(make_mlp_state_dict())
    ren = import_obj("src.models.nerf_renderer.NeRFRendererDGS")(n_samples=64, n_gaussian=24, n_depth_candidates=1000, white_bkgd=False)
    batch = collate([ds[17]])
    torch.manual_seed(1)
    geo = write_prediction_folder(nerf, ren, [batch], str(tmp_path / "geo"), ds.znear, ds.zfar, write_geometry=True)
    stem = geo["sample_name"][0]
    assert set(os.listdir(tmp_path / "geo")) == {stem + s for s in ("-pred.png", "-depth.png", "-ref.png", "-gt.png", "-zdepth.png", "-normal.png",
                                                                    ".ply")}
    # the colour and the depth written are predict_image's of the same frame seed (the scene is still encoded; encode draws nothing)
    from diner_amd.imageio import depth_to_uint8, to_uint8
    from diner_amd.render import predict_image
    H, W = batch["target_rgb"].shape[-2:]
    torch.manual_seed(1)
    rgb, depth = predict_image(nerf, ren, batch["target_extrinsics"].cuda(), batch["target_intrinsics"].cuda(), W, H, ds.znear, ds.zfar)
    assert np.array_equal(read_png(tmp_path / "geo" / (stem + "-pred.png")), to_uint8(rgb[0]).cpu().numpy())
    assert np.array_equal(read_png(tmp_path / "geo" / (stem + "-depth.png")), depth_to_uint8(depth[0]).cpu().numpy())
    pred = read_png(tmp_path / "geo" / (stem + "-pred.png"))
    assert read_png(tmp_path / "geo" / (stem + "-normal.png")).shape == pred.shape
    assert read_png(tmp_path / "geo" / (stem + "-zdepth.png")).shape == pred.shape
    xyz, rgb, nrm = read_ply(tmp_path / "geo" / (stem + ".ply"))
    assert xyz.shape[0] > 0 and rgb.shape == xyz.shape and nrm.shape == xyz.shape and np.isfinite(xyz).all()
