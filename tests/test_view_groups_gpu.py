"""GPU: scenes with 1 to 16 source views on the FUSED field kernels, four views at a time (the *_views entries of the C ABI: the
view-group instances k_field_views_h3n / k_field_views_f32, one launch per group of up to four cameras, each adding (1 / NV) x the sum
over its live views into the same hand-over; one unchanged post kernel).  Bar: 1e-4 max-norm-relative on rays whose samples are the
reference's.

  1. G23 (the reference's renderer.forward at NV = 6, 8, 16): ops.render with a HipMlp in f16x3 and fp32; no fall-back in f16x3;
  2. NV = 1, 2, 3, 5, 7 against the oracle (pinned bit-exact to the reference): partial groups, a single live view;
  3. duplicated views: G8's four views given twice is torch.equal to the four-view entries (1 / 8 is a power of two); NV = 4 through
     the new entries is the old entries;
  4. dead columns: the spare columns of a partial group never reach the result (NaN behind the maps; the duplicated camera as only source);
  5. the range fall-back inside a render at NV = 6 (G20 variant b's hot latent): gated exact pass over all groups, equal to fp32 mode;
  6. the drop-in modules at NV = 6: no-grad forward view-grouped, grad mode on the generic path;
  7. DINER_PRECISION_F16 at NV = 6 is refused."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, max_norm_rel
from tests.test_many_views_cpu import nv_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ("f16x3", "fp32")


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def hip_scene(ops, sc, views=None):
    """HipScene of the scene dict; views: a list of source-view indices (repeats allowed) to build the scene from."""
    K = sc["src_intrinsics"]
    pick = (lambda t: t) if views is None else (lambda t: t[torch.as_tensor(views)])
    return ops.HipScene(pick(sc["latent"]).cuda(), pick(sc["depths"]).cuda(), pick(sc["depths_std"]).cuda(), pick(sc["normals"]).cuda(),
                        pick(sc["src_extrinsics"]), pick(K[:, [0, 1], [0, 1]]), pick(K[:, :2, -1]), sc["image_shape"], sc["feature_padding"])


def hip_mlp(ops, msd):
    return ops.HipMlp({k: v.cuda() for k, v in msd.items()})


def errs(rgb, depth, ref_rgb, ref_d, same):
    e_rgb = ((rgb.cpu() - ref_rgb).abs().max(-1).values / ref_rgb.abs().max())[same].max().item()
    e_d = ((depth.cpu() - ref_d).abs() / ref_d.abs().max())[same].max().item()
    return e_rgb, e_d


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("nv", [6, 8, 16])
def test_render_many_views_against_reference(ops, nv):
    from diner_amd.synthetic import make_mlp_state_dict
    g = load("g23_many_views.npz")
    sc, scene, w, rs, noises = nv_inputs(g, nv)
    K, G, n_cand = int(g["K"]), int(g["G"]), int(g["n_cand"])
    hs, hm = hip_scene(ops, sc), hip_mlp(ops, make_mlp_state_dict())
    nc, ng, nf = (t.cuda() for t in noises[K])
    r = rs.cuda()
    z = ops.sample_depthguided_long(hs, r, K, n_cand, G, 0.05, noise=(nc, ng, nf))
    same = torch.isclose(z.cpu(), T(g[f"z_{nv}_{K}"]), rtol=3e-6, atol=1e-7).all(-1)
    ref_rgb, ref_d = T(g[f"rgb_{nv}"]), T(g[f"depth_{nv}"])
    for prec in PRECISIONS:
        hm.fallback_launches(reset=True)
        _, rgb, depth = ops.render(hs, hm, r, z, False, precision=prec)
        fb = hm.fallback_launches(reset=True)
        e_rgb, e_d = errs(rgb, depth, ref_rgb, ref_d, same)
        print(f"view groups NV={nv} [{prec}]: {int(same.sum())}/{rs.shape[0]} rays with the reference's samples, rgb {e_rgb:.2e}, "
              f"depth {e_d:.2e}, fall-back launches {fb}")
        assert int((~same).sum()) == 0 and e_rgb < TOL and e_d < TOL
        assert fb == 0


# ---------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("nv", [1, 2, 3, 5, 7])
def test_partial_groups_against_oracle(ops, nv):
    W = H = 32
    K, G, n_cand, NR = 64, 24, 1000, 320
    sc, scene, w, msd, rays = oracle_setup(W, H, 2300 + nv, nv=nv)
    hs, hm = hip_scene(ops, sc), hip_mlp(ops, msd)
    gen = torch.Generator().manual_seed(2310 + nv)
    sel = torch.randperm(W * H, generator=gen)[:NR].sort().values
    rs = rays[sel].contiguous()
    nc, ng, nf = torch.rand(NR, n_cand, generator=gen), torch.randn(NR, G, generator=gen), torch.rand(NR, K, generator=gen)
    ref = O.render(scene, w, rs, K, n_cand, G, False, nc, ng, nf)
    r = rs.cuda()
    z = ops.sample_depthguided_long(hs, r, K, n_cand, G, 0.05, noise=(nc.cuda(), ng.cuda(), nf.cuda()))
    same = torch.isclose(z.cpu(), ref["z"], rtol=3e-6, atol=1e-7).all(-1)
    assert int(same.sum()) >= NR - 3
    for prec in PRECISIONS:
        hm.fallback_launches(reset=True)
        _, rgb, depth = ops.render(hs, hm, r, z, False, precision=prec)
        e_rgb, e_d = errs(rgb, depth, ref["rgb"], ref["depth"], same)
        print(f"view groups NV={nv} [{prec}]: {int(same.sum())}/{NR} rays with the oracle's samples, rgb {e_rgb:.2e}, depth {e_d:.2e}")
        assert e_rgb < TOL and e_d < TOL
        assert hm.fallback_launches(reset=True) == 0
    # the field at explicit points goes the same way
    zz = z[:40]
    xyz = (r[:40, None, :3] + zz[..., None] * r[:40, None, 3:6]).reshape(-1, 3)
    dirs = r[:40, None, 3:6].expand(-1, K, -1).reshape(-1, 3).contiguous()
    for prec in PRECISIONS:
        assert max_norm_rel(ops.field_from_points(hs, hm, xyz, dirs, precision=prec).view(40, K, 4),
                            ops.field_from_rays(hs, hm, r[:40].contiguous(), zz.contiguous(), precision=prec)) < 1e-5, prec


# ---------------------------------------------------------------------------------------------------------------------- 3
def _g8(ops):
    g = load("g8_render_cfg1.npz")
    W, H, K = int(g["W"]), int(g["H"]), int(g["K"])
    sc, scene, w, msd, rays = oracle_setup(W, H, int(g["seed"]))
    z = T(g["z"])[::4].contiguous().cuda()
    r = rays.cuda()[::4].contiguous()
    return sc, msd, r, z, K


def _views_call(ops, entry, hs, hm, r, z, prec):
    """One of the *_views entries called directly (ops routes four-view scenes to the four-view entries)."""
    from diner_amd import _lib
    NR, K = z.shape
    hs.prepare(hm)
    out = torch.empty(NR, K, 4, device=r.device)
    ws = torch.empty(ops.lib.diner_field_views_workspace_bytes(NR * K), dtype=torch.uint8, device=r.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "rays":
        _lib.check(ops.lib.diner_field_from_rays_views_f32(hs.ref, hm.handle, C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr()), NR, K, prec,
                                                           C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), st))
    else:
        xyz = (r[:, None, :3] + z[..., None] * r[:, None, 3:6]).reshape(-1, 3).contiguous()
        dirs = r[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3).contiguous()
        _lib.check(ops.lib.diner_field_from_points_views_f32(hs.ref, hm.handle, C.c_void_p(xyz.data_ptr()), C.c_void_p(dirs.data_ptr()), NR * K,
                                                             prec, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), st))
    return out


def test_duplicated_views_equal_the_four_view_entries(ops):
    sc, msd, r, z, K = _g8(ops)
    h4, h8, hm = hip_scene(ops, sc), hip_scene(ops, sc, views=[0, 1, 2, 3, 0, 1, 2, 3]), hip_mlp(ops, msd)
    assert (h4.nv, h8.nv) == (4, 8)
    for prec in PRECISIONS:
        f4 = ops.field_from_rays(h4, hm, r, z, precision=prec)
        f8 = ops.field_from_rays(h8, hm, r, z, precision=prec)
        assert torch.isfinite(f4).all() and torch.equal(f4, f8), prec
        code = ops.PRECISION_NAMES[prec]
        assert torch.equal(_views_call(ops, "rays", h4, hm, r, z, code), f4), prec       # NV = 4 through the new entries
        xyz = (r[:, None, :3] + z[..., None] * r[:, None, 3:6]).reshape(-1, 3).contiguous()
        dirs = r[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3).contiguous()
        assert torch.equal(_views_call(ops, "points", h4, hm, r, z, code).view(-1, 4), ops.field_from_points(h4, hm, xyz, dirs, precision=prec)), prec
        w4, rgb4, d4 = ops.render(h4, hm, r, z, False, want_weights=True, precision=prec)
        w8, rgb8, d8 = ops.render(h8, hm, r, z, False, want_weights=True, precision=prec)
        assert torch.equal(rgb4, rgb8) and torch.equal(d4, d8) and torch.equal(w4, w8), prec
    assert hm.fallback_launches(reset=True) == 0


# ---------------------------------------------------------------------------------------------------------------------- 4
def test_dead_columns_never_reach_the_result(ops):
    sc, msd, r, z, K = _g8(ops)
    hm = hip_mlp(ops, msd)
    # (a) NV = 5: the second group has one live view and three dead columns.  The scene's maps are views into LARGER buffers whose tails --
    #     where views 5..7 of the group would lie -- hold NaN: what a dead column that addressed "its" view would read.
    views = [0, 1, 2, 3, 2]
    ref5 = {p: ops.field_from_rays(hip_scene(ops, sc, views=views), hm, r, z, precision=p) for p in PRECISIONS}
    h5 = hip_scene(ops, sc, views=views)
    for name in ("latent_cl", "depth", "depth_std", "normals"):
        t = getattr(h5, name)
        big = torch.full((8,) + tuple(t.shape[1:]), float("nan"), device=t.device)
        big[:5] = t
        setattr(h5, name, big[:5])
        setattr(h5.struct, name, big.data_ptr())
    h5.prepare(hm)
    # the projected maps keep the plane stride NV Hf Wf 512: the poisoned tail lies behind the LAST plane, where the dead columns of the
    # last group of plane 2 would read; planes 0 and 1 are followed by the next plane's live views
    flat = torch.full((h5.latent_proj.numel() + 3 * h5.Hf * h5.Wf * 512,), float("nan"), device="cuda")
    flat[:h5.latent_proj.numel()] = h5.latent_proj
    h5.latent_proj = flat
    h5.struct.latent_proj = flat.data_ptr()
    for p in PRECISIONS:
        f = ops.field_from_rays(h5, hm, r, z, precision=p)
        assert torch.isfinite(f).all() and torch.equal(f, ref5[p]), p
    # (b) one source view: three dead columns that recompute it.  The mean of one view is the view itself, so NV = 1 is NV = 2 of the same
    #     view (x + x and the scales 1 and 1 / 2 are exact; three and four equal terms round at 3 x): bit for bit in the exact kernels,
    #     whose waves run the same instructions per view.  In the f16x3 kernel the projected taps of column group g enter the accumulation
    #     chain at a step that depends on g, so the same view in two columns differs by fp32 rounding: held to 1e-5 there.
    f1 = {p: ops.field_from_rays(hip_scene(ops, sc, views=[1]), hm, r, z, precision=p) for p in PRECISIONS}
    h2 = hip_scene(ops, sc, views=[1, 1])
    for p in PRECISIONS:
        f2 = ops.field_from_rays(h2, hm, r, z, precision=p)
        assert torch.isfinite(f1[p]).all() and torch.isfinite(f2).all()
        e = max_norm_rel(f2, f1[p])
        print(f"one view against the same view twice [{p}]: {e:.2e}")
        assert torch.equal(f2, f1[p]) if p == "fp32" else e < 1e-5, p
    assert max_norm_rel(f1["f16x3"], f1["fp32"]) < 1e-5
    assert hm.fallback_launches(reset=True) == 0


# ---------------------------------------------------------------------------------------------------------------------- 5
def test_range_fallback_inside_a_render_nv6(ops):
    from tests.test_hip_parity import _g20_inputs
    g, sc, msd = _g20_inputs("b")
    hs, hm = hip_scene(ops, sc, views=[0, 1, 2, 3, 0, 1]), hip_mlp(ops, msd)
    assert hs.nv == 6 and hm.h3_ok
    rays, z = T(g["rays"]).cuda(), T(g["z"]).cuda()
    hm.fallback_launches(reset=True)
    exact = ops.render(hs, hm, rays, z, False, want_weights=True, precision="fp32")
    assert hm.fallback_launches(reset=True) == 0
    split = ops.render(hs, hm, rays, z, False, want_weights=True, precision="f16x3")
    fb = hm.fallback_launches(reset=True)
    print(f"G20 b at NV = 6: fall-back launches {fb}")
    assert fb > 0, "activations beyond the fp16 range did not raise the range flag inside a view-grouped render"
    # bit for bit -- compared as bit patterns: a few rays of this scene are not finite in the reference's own compositor (G20 variant b), and
    # torch.equal calls a NaN unequal to itself
    for a, b in zip(split, exact):
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    assert int((~torch.isfinite(exact[1]).all(-1)).sum()) <= 4


# ---------------------------------------------------------------------------------------------------------------------- 6
def test_modules_view_grouped_nv6(ops):
    from diner_amd import noise
    from diner_amd.synthetic import build_modules, make_mlp_state_dict
    nv = 6
    g = load("g23_many_views.npz")
    sc, scene, w, rs, noises = nv_inputs(g, nv)
    K, G, n_cand = int(g["K"]), int(g["G"]), int(g["n_cand"])
    nerf, R = build_modules(sc, make_mlp_state_dict(), "cuda", normals=sc["normals"])
    assert nerf.is_generic() and nerf.is_view_grouped()
    assert isinstance(nerf.hip_mlp(), ops.HipMlp)
    assert isinstance(nerf.mlp_fine.hip_mlp(nv=nv), ops.GenericMlp)          # the explicit-matrix route stays generic
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=False)
    nc, ng, nf = (t[None].cuda() for t in noises[K])
    r = rs.cuda()[None]
    with noise.inject(nc, ng, nf), torch.no_grad():
        out = ren.forward(nerf, r)
        z = ren.fill_up_uniform_samples(ren.sample_depthguided(r, nerf, K, n_cand, n_gaussian=G), r)[0]
    same = torch.isclose(z.cpu(), T(g[f"z_{nv}_{K}"]), rtol=3e-6, atol=1e-7).all(-1)
    e_rgb, e_d = errs(out.fine.rgb[0], out.fine.depth[0], T(g[f"rgb_{nv}"]), T(g[f"depth_{nv}"]), same)
    print(f"modules NV={nv} view-grouped: rgb {e_rgb:.2e}, depth {e_d:.2e}")
    assert int((~same).sum()) == 0 and e_rgb < TOL and e_d < TOL
    # ... and it is what ops.render gives with the packed handle (test 1)
    _, rgb, depth = ops.render(nerf.hip_scene(0), nerf.hip_mlp(), r[0], z, False)
    assert torch.equal(rgb, out.fine.rgb[0]) and torch.equal(depth, out.fine.depth[0])
    # grad mode: the generic path, with gradients
    nerf.train()
    xyz = (r[0, :8, None, :3] + z[:8, :, None] * r[0, :8, None, 3:6]).reshape(1, -1, 3)
    dirs = r[0, :8, None, 3:6].expand(-1, K, -1).reshape(1, -1, 3).contiguous()
    f = nerf.forward(xyz, dirs)
    assert f.requires_grad
    f.square().mean().backward()
    gw = nerf.mlp_fine.lin_out.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and float(gw.abs().max()) > 0
    with torch.no_grad():
        f_ng = nerf.forward(xyz, dirs)
    assert max_norm_rel(f_ng, f.detach()) < TOL


# ---------------------------------------------------------------------------------------------------------------------- 7
def test_plain_fp16_refused_for_other_view_counts(ops):
    from diner_amd import _lib
    sc, msd, r, z, K = _g8(ops)
    h6, hm = hip_scene(ops, sc, views=[0, 1, 2, 3, 0, 1]), hip_mlp(ops, msd)
    h6.prepare(hm)
    NR = z.shape[0]
    out = torch.empty(NR, K, 4, device="cuda")
    ws = torch.empty(ops.lib.diner_field_views_workspace_bytes(NR * K), dtype=torch.uint8, device="cuda")
    rc = ops.lib.diner_field_from_rays_views_f32(h6.ref, hm.handle, C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr()), NR, K, ops.PRECISION_F16,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), None)
    msg = ops.lib.diner_last_error()
    assert rc == _lib.E_UNSUPPORTED and b"f16x3" in msg and b"fp32" in msg, (rc, msg)
    with pytest.raises(RuntimeError, match="f16x3"):
        ops.field_from_rays(h6, hm, r, z, precision="f16")
