"""GPU: scenes with 5 to 16 source views (DINER_MAX_VIEWS) on the NV-generic route -- the wide-scene instances of the depth-guided
sampler (one wave per ray and one workgroup per ray), of diner_index_f32 and of the generic inputs and their adjoint, the generic exact-fp32
MLP -- through ops, the drop-in modules and training.

  1. the sampler against the reference (tests/golden/g23_many_views.npz) at NV = 6, 8, 16 (K = 64) and at K = 320 (NV = 8);
  2. duplicated views: the 4-view G8 scene given twice as an 8-view scene picks exactly what the 4-view kernel picks (the likelihood is a
     maximum over views), and its field on the generic path agrees with the 4-view fused kernel;
  3. NeRFRendererDGS.forward through the drop-in modules against the reference's colours and depths at NV = 6, 8, 16;
  4. a grad-mode step at NV = 6 through PixelNeRF.forward against the reference's autograd;
  5. a 128 x 128 frame at NV = 16 over many generic launches against the oracle;
  6. the index lookups at NV = 6 against the oracle, and 17 views refused by HipScene."""
import numpy as np
import pytest
import torch

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, sha, selection_diff, SAT_L, max_norm_rel
from tests.test_many_views_cpu import nv_inputs

pytestmark = pytest.mark.gpu
TOL = 1e-4
# rays of G23 whose unfilled pick set differs from the reference's: candidates within SAT_L of the cut-off (the erf-boundary classes A / B
# of DESIGN.md section 2), pinned per (NV, K)
MAX_DIFF = {(6, 64): 0, (8, 64): 0, (16, 64): 0, (8, 320): 4}


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def hip_scene(ops, sc, rep=1):
    K = sc["src_intrinsics"]
    cat = lambda t: torch.cat([t] * rep) if rep > 1 else t
    return ops.HipScene(cat(sc["latent"]).cuda(), cat(sc["depths"]).cuda(), cat(sc["depths_std"]).cuda(), cat(sc["normals"]).cuda(),
                        cat(sc["src_extrinsics"]), cat(K[:, [0, 1], [0, 1]]), cat(K[:, :2, -1]), sc["image_shape"], sc["feature_padding"])


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("nv,K", [(6, 64), (8, 64), (16, 64), (8, 320)])
def test_sampler_many_views_against_reference(ops, nv, K):
    g = load("g23_many_views.npz")
    sc, scene, w, rs, noises = nv_inputs(g, nv)
    nc, ng, nf = noises[K]
    n_cand, G, NR = int(g["n_cand"]), ng.shape[1], rs.shape[0]
    hs = hip_scene(ops, sc)
    z, zu = ops.sample_depthguided_long(hs, rs.cuda(), K, n_cand, G, 0.05, noise=(nc.cuda(), ng.cuda(), nf.cuda()), want_unfilled=True)
    z, zu = z.cpu(), zu.cpu()
    if K <= 256:                      # the bounded entry runs the same wave-per-ray instance
        zb, zub = ops.sample_depthguided(hs, rs.cuda(), K, n_cand, G, 0.05, noise=(nc.cuda(), ng.cuda(), nf.cuda()), want_unfilled=True)
        assert torch.equal(zb.cpu(), z) and torch.equal(zub.cpu(), zu)
    ref_u = T(g[f"z_unfilled_{nv}_{K}"])
    _, aux = O.sample_depthguided(scene, rs, K, n_cand, G, nc, ng, return_aux=True)
    bad, worst = selection_diff(ref_u[:, :K - G].sort(-1).values, zu[:, :K - G].sort(-1).values, aux["L"], aux["z_cand"], K - G)
    print(f"NV={nv} K={K}: {len(bad)}/{NR} rays with a different pick set, worst distance to the cut-off {worst:.1e}")
    assert worst < SAT_L and len(bad) <= MAX_DIFF[(nv, K)]
    cond = aux["O"].sum(-1) >= 1e-2
    assert torch.allclose(zu[cond, K - G:], ref_u[cond, K - G:], rtol=3e-6, atol=1e-7)
    assert torch.equal(O.fill_up_uniform_samples(zu, rs, nf), z)


# ---------------------------------------------------------------------------------------------------------------------- 2
def test_duplicated_views_match_four_view_kernels(ops):
    g = load("g8_render_cfg1.npz")
    W, H, K, G, n_cand = (int(g[k]) for k in ("W", "H", "K", "G", "n_cand"))
    sc, scene, w, msd, rays = oracle_setup(W, H, int(g["seed"]))
    h4, h8 = hip_scene(ops, sc), hip_scene(ops, sc, rep=2)
    assert (h4.nv, h8.nv) == (4, 8)
    rc = rays.cuda()
    gen = torch.Generator().manual_seed(2308)
    for (k, gg, nc_) in ((K, G, n_cand), (320, 120, 1000)):
        noise = (torch.rand(W * H, nc_, generator=gen).cuda(), torch.randn(W * H, gg, generator=gen).cuda(),
                 torch.rand(W * H, k, generator=gen).cuda())
        for nz, seed in ((noise, 0), (None, 99)):
            a = ops.sample_depthguided_long(h4, rc, k, nc_, gg, 0.05, noise=nz, seed=seed, want_unfilled=True)
            b = ops.sample_depthguided_long(h8, rc, k, nc_, gg, 0.05, noise=nz, seed=seed, want_unfilled=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (k, nz is None)
    # the field at the G8 samples: 8-view generic exact fp32 against the 4-view fused kernel (default precision)
    z = T(g["z"])[::4].contiguous().cuda()
    r = rc[::4].contiguous()
    xyz = (r[:, None, :3] + z[..., None] * r[:, None, 3:6]).reshape(-1, 3)
    dirs = r[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3).contiguous()
    msd_c = {k_: v.cuda() for k_, v in msd.items()}
    f4 = ops.field_from_points(h4, ops.HipMlp(msd_c), xyz, dirs)
    gm = ops.GenericMlp(msd_c, combine_layer=3)
    f8 = ops.field_generic(h8, gm, xyz=xyz, viewdirs=dirs)
    f4g = ops.field_generic(h4, gm, xyz=xyz, viewdirs=dirs)
    e, e_gen = max_norm_rel(f8.cpu(), f4.cpu()), max_norm_rel(f8.cpu(), f4g.cpu())
    print(f"duplicated views: field 8-view generic vs 4-view fused {e:.2e}, vs 4-view generic {e_gen:.2e}")
    assert e < 1e-5 and e_gen < 1e-5
    # the index lookups: every view of the 8-view scene is its original
    uv = (torch.rand(8, 300, 2, generator=gen) * 2.4 - 1.2).cuda()
    for mode in range(4):
        o8 = ops.index(h8, mode, uv)
        assert torch.equal(o8[:4], ops.index(h4, mode, uv[:4])) and torch.equal(o8[4:], ops.index(h4, mode, uv[4:])), mode


# ---------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("nv", [6, 8, 16])
def test_renderer_forward_many_views_against_reference(ops, nv):
    from diner_amd import noise
    from diner_amd.synthetic import build_modules
    g = load("g23_many_views.npz")
    sc, scene, w, rs, noises = nv_inputs(g, nv)
    K, G, n_cand = int(g["K"]), int(g["G"]), int(g["n_cand"])
    nerf, R = build_modules(sc, O_msd(), "cuda", normals=sc["normals"])
    assert nerf.is_generic()
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=False)
    nc, ng, nf = (t[None].cuda() for t in noises[K])
    r = rs.cuda()[None]
    with noise.inject(nc, ng, nf), torch.no_grad():
        out = ren.forward(nerf, r)
        z = ren.fill_up_uniform_samples(ren.sample_depthguided(r, nerf, K, n_cand, n_gaussian=G), r)[0]
    same = torch.isclose(z.cpu(), T(g[f"z_{nv}_{K}"]), rtol=3e-6, atol=1e-7).all(-1)
    ref_rgb, ref_d = T(g[f"rgb_{nv}"]), T(g[f"depth_{nv}"])
    e_rgb = ((out.fine.rgb[0].cpu() - ref_rgb).abs().max(-1).values / ref_rgb.abs().max())[same].max().item()
    e_d = ((out.fine.depth[0].cpu() - ref_d).abs() / ref_d.abs().max())[same].max().item()
    print(f"renderer.forward NV={nv}: {int(same.sum())}/{rs.shape[0]} rays with the reference's samples, rgb {e_rgb:.2e}, depth {e_d:.2e}")
    assert int((~same).sum()) <= MAX_DIFF[(nv, K)] and e_rgb < TOL and e_d < TOL


def O_msd():
    from diner_amd.synthetic import make_mlp_state_dict
    return make_mlp_state_dict()


# ---------------------------------------------------------------------------------------------------------------------- 4
def test_training_step_nv6_against_reference_autograd(ops):
    from diner_amd import train
    from diner_amd.synthetic import build_modules, realistic_mlp_state_dict
    g = load("g23_many_views.npz")
    W, H, nv, K = int(g["W"]), int(g["H"]), int(g["nv_t"]), int(g["K_t"])
    sc, _, _, _, rays = oracle_setup(W, H, int(g["scene_seed"]), nv=nv)
    rsd = realistic_mlp_state_dict(int(g["mlp_seed"]))
    assert sha(*[rsd[k] for k in sorted(rsd)]) == str(g["t_mlp_sha"])
    nerf, _ = build_modules(sc, rsd, "cuda", normals=sc["normals"])
    nerf.train()
    nerf.encoder.latent = nerf.encoder.latent.detach().requires_grad_(True)
    rs = T(g["t_rays"])
    assert torch.allclose(rays[T(g["t_ray_idx"])], rs, rtol=0, atol=1e-6)
    r, z = rs.cuda(), T(g["t_z"]).cuda()
    xyz = (r[:, None, :3] + z[..., None] * r[:, None, 3:6]).reshape(1, -1, 3)
    dirs = r[:, None, 3:6].expand(-1, K, -1).reshape(1, -1, 3).contiguous()
    field = nerf.forward(xyz, dirs)[0].view(rs.shape[0], K, 4)
    assert field.requires_grad
    rgb, _ = train.composite_train(field, z, r, False)
    loss = torch.nn.functional.mse_loss(rgb, T(g["t_target"]).cuda())
    loss.backward()
    gp = dict(nerf.mlp_fine.named_parameters())
    tx = T(g["t_g_lat_texels"])
    gl = nerf.encoder.latent.grad[0].cpu()[tx[:, 0], :, tx[:, 1], tx[:, 2]]
    errs = {"loss": abs(loss.item() - float(g["t_loss"])) / abs(float(g["t_loss"])),
            "rgb": max_norm_rel(rgb.detach().cpu(), T(g["t_rgb"])),
            "lin_out.weight": max_norm_rel(gp["lin_out.weight"].grad.cpu(), T(g["t_g_lin_out_w"])),
            "lin_out.bias": max_norm_rel(gp["lin_out.bias"].grad.cpu(), T(g["t_g_lin_out_b"])),
            "blocks.0.fc_0.weight": ((gp["blocks.0.fc_0.weight"].grad.cpu()[::8] - T(g["t_g_fc0_w_rows8"])).abs().max()
                                     / float(g["t_g_fc0_w_absmax"])).item(),
            "blocks.0.fc_0.bias": max_norm_rel(gp["blocks.0.fc_0.bias"].grad.cpu(), T(g["t_g_fc0_b"])),
            "latent": ((gl - T(g["t_g_lat"])).abs().max() / float(g["t_g_lat_absmax"])).item()}
    print("training step NV=6 vs the reference's autograd: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert int((nerf.encoder.latent.grad[0].abs().sum(1) != 0).sum()) == int(g["t_g_lat_nonzero_texels"])
    for k, v in errs.items():
        assert v < TOL, (k, v)


# ---------------------------------------------------------------------------------------------------------------------- 5
def test_frame_128_nv16_over_many_generic_launches(ops, monkeypatch):
    W = H = 128
    nv, K, G, n_cand = 16, 64, 24, 1000
    sc, scene, w, msd, rays = oracle_setup(W, H, 1623, nv=nv)
    hs = hip_scene(ops, sc)
    gm = ops.GenericMlp({k: v.cuda() for k, v in msd.items()}, combine_layer=3)
    gen = torch.Generator().manual_seed(1624)
    nc, ng, nf = torch.rand(W * H, n_cand, generator=gen), torch.randn(W * H, G, generator=gen), torch.rand(W * H, K, generator=gen)
    rc = rays.cuda()
    z = ops.sample_depthguided_long(hs, rc, K, n_cand, G, 0.05, noise=(nc.cuda(), ng.cuda(), nf.cuda()))
    monkeypatch.setattr(ops, "GENERIC_POINTS_PER_LAUNCH", 1 << 16)        # 16384 points per launch at NV = 16: 64 launches
    assert ops.generic_points_per_launch(nv) == 1 << 14
    field = ops.field_generic(hs, gm, rays=rc, z=z)
    _, rgb, depth = ops.composite(field.view(W * H, K, 4), z, rc, False, want_weights=False)
    assert torch.isfinite(rgb).all() and torch.isfinite(depth).all()
    sub = torch.randperm(W * H, generator=gen)[:48].sort().values
    ref = O.render(scene, w, rays[sub].contiguous(), K, n_cand, G, False, nc[sub], ng[sub], nf[sub])
    same = torch.isclose(z[sub].cpu(), ref["z"], rtol=3e-6, atol=1e-7).all(-1)
    e_rgb = ((rgb[sub].cpu() - ref["rgb"]).abs().max(-1).values / ref["rgb"].abs().max())[same].max().item()
    e_d = ((depth[sub].cpu() - ref["depth"]).abs() / ref["depth"].abs().max())[same].max().item()
    print(f"128x128 NV=16: {int(same.sum())}/48 rays with the oracle's samples, rgb {e_rgb:.2e}, depth {e_d:.2e}")
    assert int(same.sum()) >= 46 and e_rgb < TOL and e_d < TOL


# ---------------------------------------------------------------------------------------------------------------------- 6
def test_index_many_views_against_oracle(ops):
    sc, scene, _, _, _ = oracle_setup(40, 48, 7, nv=6, bg_std_zero=True)
    hs = hip_scene(ops, sc)
    uv = torch.rand(6, 500, 2, generator=torch.Generator().manual_seed(66)) * 2.6 - 1.3
    uv[:, :40] = uv[:, :40] * 6
    got = [ops.index(hs, m, uv.cuda()).cpu() for m in range(4)]
    ref = [O.index_latent(scene, uv), O.index_depth(scene, uv), O.index_depth_std(scene, uv), O.index_normal(scene, uv)]
    for m in range(4):
        assert got[m].shape == ref[m].shape
        assert ((got[m] - ref[m]).abs().max() / ref[m].abs().max().clamp(min=1e-30)).item() < 1e-5, m


def test_hip_scene_refuses_17_views(ops):
    sc, *_ = oracle_setup(16, 16, 3, nv=17)
    with pytest.raises(ValueError, match="1 to 16 source views"):
        hip_scene(ops, sc)
