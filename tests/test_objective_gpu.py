"""The training objective on the device (diner_amd.objective, csrc/objective.hip, k_gen_rays_at of prep.hip) against fixture G25 (the
reference's MSELoss / AntibiasLoss / autograd in float32 and float64, and the patch rule), against the contiguous ray entry, and end to
end against the same training step assembled from the pieces that existed before.

test_objective_matches_reference_g25 prints, per case, the kernel's distance from the reference's float64 values next to the
reference's own float32-versus-float64 spread (the yardstick); DESIGN.md section 8b quotes a run."""
import numpy as np
import pytest
import torch

from tests.helpers import load, max_norm_rel
from tests.test_objective_cpu import g25_cases, g25_patches, host_objective

pytestmark = pytest.mark.gpu
TOL_ROUTES = 1e-5        # tests/test_train_gpu.py: two routes of the same step (one node per object against one node for the objects)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- 1a: the patch of the step -------------------------------------------------------------------------------------------------------
def test_sample_patch_matches_g25():
    from diner_amd import objective
    for (H, W, s), fg, u, centres, pix, flags in g25_patches():
        p, c, f = objective.sample_patch(dev(fg), s, u=dev(u))
        assert p.dtype == torch.int32 and tuple(p.shape) == (fg.shape[0], s * s)
        assert np.array_equal(c.cpu().numpy(), centres), (H, W, s, c.cpu().numpy(), centres)
        assert np.array_equal(p.cpu().numpy(), pix), (H, W, s)
        assert np.array_equal(f.cpu().numpy(), flags), (H, W, s)


def test_sample_patch_philox_draws():
    from diner_amd import objective
    (H, W, s), fg, _, _, _, _ = next(iter(g25_patches()))
    n = 4096
    mask = dev(fg[0])[None].expand(n, -1, -1).contiguous()
    p1, c1, f1 = objective.sample_patch(mask, s, seed=7, step=3)
    p2, c2, f2 = objective.sample_patch(mask, s, seed=7, step=3)
    assert torch.equal(p1, p2) and torch.equal(c1, c2) and torch.equal(f1, f2)
    _, c3, _ = objective.sample_patch(mask, s, seed=7, step=4)
    assert not torch.equal(c1, c3)
    pad = (s + 1) // 2
    w = fg[0].copy()
    w[:pad] = 0
    w[-pad:] = 0
    w[:, :pad] = 0
    w[:, -pad:] = 0
    c = c1.cpu().numpy()
    assert (w[c[:, 1], c[:, 0]] > 0).all() and int(f1.sum()) == 0
    assert len({(int(x), int(y)) for x, y in c}) > 200          # the draws spread over the mask
    assert p1.min() >= 0 and p1.max() < H * W


# ---- 1b: rays at listed pixels -------------------------------------------------------------------------------------------------------
def test_gen_rays_at_equals_the_contiguous_entry():
    from diner_amd import objective, ops
    g = load("g11_helpers.npz")
    W, H = int(g["rays_W"]), int(g["rays_H"])
    E, K = torch.from_numpy(g["rays_E"]).float(), torch.from_numpy(g["rays_K"]).float()
    near, far = torch.from_numpy(g["rays_near"]).float(), torch.from_numpy(g["rays_far"]).float()
    B = E.shape[0]
    full = ops.gen_rays(E, K, W, H, near, far, "cuda")
    want = torch.from_numpy(g["rays"]).float().view(B, H * W, 8)
    s = 8
    fg = torch.ones(B, H, W, device="cuda")
    patch, _, _ = objective.sample_patch(fg, s, u=torch.tensor([0.1, 0.5, 0.9][:B] + [0.3] * max(0, B - 3), device="cuda"))
    rnd = torch.randint(0, H * W, (B, 500), generator=torch.Generator().manual_seed(2)).int().cuda()
    corners = torch.tensor([[0, W - 1, (H - 1) * W, H * W - 1]] * B, dtype=torch.int32, device="cuda")
    for pix in (patch, rnd, corners):
        got = ops.gen_rays_at(E, K, W, H, near, far, pix)
        idx = pix.long()[..., None].expand(-1, -1, 8)
        assert torch.equal(got, full.gather(1, idx))
        ref = want.gather(1, idx.cpu())
        assert (got.cpu() - ref).abs().max().item() <= 5e-7 and torch.equal(got.cpu()[..., 6:], ref[..., 6:])      # test_hip_parity's bar for gen_rays
    # indices outside the image are clamped, nothing is written out of bounds
    wild = torch.tensor([[-5, H * W, 2 ** 31 - 1, 3]] * B, dtype=torch.int32, device="cuda")
    got = ops.gen_rays_at(E, K, W, H, near, far, wild)
    assert torch.equal(got, full[:, [0, H * W - 1, H * W - 1, 3]])
    # more than 16 cameras go out in several calls
    E20, K20 = E[:1].expand(20, -1, -1).contiguous(), K[:1].expand(20, -1, -1).contiguous()
    got = ops.gen_rays_at(E20, K20, W, H, 0.5, 1.5, rnd[:1].expand(20, -1).contiguous())
    assert torch.equal(got[19], got[0]) and torch.equal(got[0, :, :6], full[0, rnd[0].long(), :6])


# ---- 1c: the objective ---------------------------------------------------------------------------------------------------------------
def test_objective_matches_reference_g25():
    from diner_amd import objective
    for case, pred, gt, ref in g25_cases():
        kind, SB, s, n, w, B, seed = case
        P, G = dev(pred), dev(gt)
        losses, d_pred = objective.objective(P, G, s, n, w)
        l, d = losses.cpu().numpy(), d_pred.cpu().numpy().astype(np.float64)
        _, g64 = host_objective(pred, gt, s, n, w)          # pinned to the reference's float64 gradient by tests/test_objective_cpu.py
        rel = [abs(l[k] - ref["loss64"][k]) / max(abs(ref["loss64"][k]), 1e-300) for k in range(3)]
        yard = [abs(ref["loss32"][k] - ref["loss64"][k]) / max(abs(ref["loss64"][k]), 1e-300) for k in range(3)]
        e_g = np.abs(d - g64).max()
        print(f"{case}: losses kernel-vs-fp64 {rel[0]:.1e} {rel[1]:.1e} {rel[2]:.1e}, reference fp32-vs-fp64 {yard[0]:.1e} {yard[1]:.1e} "
              f"{yard[2]:.1e}; gradient kernel-vs-fp64 {e_g:.2e}, reference fp32-vs-fp64 {ref['grad_spread']:.2e}")
        for k in range(3):
            assert abs(l[k] - ref["loss64"][k]) <= max(1e-12, 4 * yard[k]) * abs(ref["loss64"][k]), (case, k, l[k], ref["loss64"][k])
        assert e_g <= 4 * ref["grad_spread"], (case, e_g)
        assert np.abs(d.reshape(-1)[::ref["step"]] - ref["grad64"]).max() <= 4 * ref["grad_spread"], case      # the stored elements themselves
        assert (d[g64 == 0] == 0).all()
        if kind == "zero_cells":
            assert (g64 == 0).sum() == pred.size // 2
        # the images + indices route gathers the same colours: bit for bit the explicit-gt route; and a second run repeats the first
        H, W = 70, 90
        rs = np.random.RandomState(seed)
        pix = np.stack([rs.permutation(H * W)[:B] for _ in range(SB)]).astype(np.int32)
        images = rs.random_sample((SB, 3, H * W)).astype(np.float32)
        np.put_along_axis(images, np.broadcast_to(pix[:, None, :], (SB, 3, B)).astype(np.int64), gt.transpose(0, 2, 1), axis=2)
        l2, d2 = objective.objective(P, (dev(images.reshape(SB, 3, H, W)), dev(pix)), s, n, w)
        assert torch.equal(l2, losses) and torch.equal(d2, d_pred)
        l3, d3 = objective.objective(P, G, s, n, w)
        assert torch.equal(l3, losses) and torch.equal(d3, d_pred)


def test_photometric_autograd_and_antibias_module():
    from diner_amd import objective
    from src.losses import AntibiasLoss
    case, pred, gt, ref = list(g25_cases())[2]
    kind, SB, s, n, w, B, seed = case
    G = dev(gt)
    _, d_pred = objective.objective(dev(pred), G, s, n, w)
    P = dev(pred).requires_grad_(True)
    ph = objective.photometric(P, G, s, n, w)
    assert ph.total.dim() == 0 and ph.total.dtype == torch.float32 and ph.losses_f64.dtype == torch.float64
    assert not ph.rgb_fine.requires_grad and not ph.antibias.requires_grad and ph.total.requires_grad
    assert torch.equal(ph.losses_f64.float(), torch.stack([ph.rgb_fine, ph.antibias, ph.total]).detach())
    ph.total.backward()
    assert torch.equal(P.grad, d_pred)
    P.grad = None
    (0.5 * objective.photometric(P, G, s, n, w).total).backward()
    assert torch.equal(P.grad, 0.5 * d_pred)
    # the drop-in module: AntibiasLoss alone on (N,3,s,s) tensors
    x = dev(pred).view(SB, s, s, 3).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = G.view(SB, s, s, 3).permute(0, 3, 1, 2).contiguous()
    loss = AntibiasLoss(n_downsampling=n)(x, y)
    want, g_want = host_objective(pred, gt, s, n, 1.0, w_mse=0.0)
    assert abs(float(loss) - want[1]) <= 1e-6 * want[1] and abs(want[1] - ref["loss64"][1]) <= 1e-12 * want[1]
    loss.backward()
    got = x.grad.permute(0, 2, 3, 1).reshape(SB, B, 3).cpu().numpy().astype(np.float64)
    assert np.abs(got - g_want).max() <= 4 * ref["grad_spread"]
    with pytest.raises(ValueError):
        objective.objective(dev(pred), G, 0, 0, 1.0)
    with pytest.raises(ValueError):
        objective.objective(dev(pred), G, s, 6, 1.0)


def test_objective_ops_do_not_synchronise():
    from diner_amd import objective, ops
    (H, W, s), fg, u, _, _, _ = next(iter(g25_patches()))
    SB = fg.shape[0]
    F, U = dev(fg), dev(u)
    E = torch.eye(4)[None].repeat(SB, 1, 1)
    K = torch.tensor([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]])[None].repeat(SB, 1, 1)
    pred = torch.rand(SB, s * s, 3, device="cuda")
    images = torch.rand(SB, 3, H, W, device="cuda")

    def run():
        pix, _, _ = objective.sample_patch(F, s, u=U)
        objective.sample_patch(F, s, seed=5, step=1)
        rays = ops.gen_rays_at(E, K, W, H, 0.5, 1.5, pix)
        gt = torch.rand(SB, s * s, 3, device="cuda")
        objective.objective(pred, gt, s, 2, 1.0)
        objective.objective(pred, (images, pix), s, 2, 1.0)
        p = pred.clone().requires_grad_(True)
        objective.photometric(p, (images, pix), s, 2, 5.0).total.backward()
        return rays, p.grad

    run()                                             # warm-up: module loading, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rays, grad = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(rays).all() and torch.isfinite(grad).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_calc_losses_against_the_step_assembled_from_existing_pieces():
    from diner_amd import noise, objective, ops
    from diner_amd.synthetic import build_modules, make_scene, make_mlp_state_dict
    W = H = 64
    SB, s, n, K, G, n_cand, w_ab, w_vgg = 2, 32, 3, 40, 15, 1000, 1.0, 0.1
    B = s * s
    scs = [make_scene(W, H, seed=21 + i) for i in range(SB)]
    nerf, R = build_modules(scs, make_mlp_state_dict(), torch.device("cuda", 0))
    nerf.train()
    latent0 = nerf.encoder.latent.detach().clone()
    encode_calls = []

    def encode(images, depths, depths_std, extrinsics, intrinsics):
        """Stands in for the ResNet trunk (the scenes' seeded feature maps are injected, as everywhere in this suite): a fresh leaf latent
        per call, so that each route gets its own gradient; records that it was called with the batch's source tensors."""
        encode_calls.append((images, depths, depths_std, extrinsics, intrinsics))
        nerf.encoder.latent = latent0.clone().requires_grad_(True)
        nerf._scenes = {}

    nerf.encode = encode
    gen = torch.Generator().manual_seed(9)
    st = lambda k: torch.stack([sc[k] for sc in scs]).cuda()
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    alpha = (((yy - 30) ** 2 + (xx - 34) ** 2) < 20 ** 2).float() * (0.25 + 0.75 * torch.rand(SB, 1, H, W, generator=gen))
    batch = dict(src_rgbs=torch.rand(SB, 4, 3, H, W, generator=gen).cuda(), src_depths=st("depths"), src_depth_stds=st("depths_std"),
                 src_extrinsics=st("src_extrinsics"), src_intrinsics=st("src_intrinsics"), target_rgb=torch.rand(SB, 3, H, W, generator=gen).cuda(),
                 target_alpha=alpha.cuda(), target_extrinsics=torch.stack([sc["target_extrinsics"] for sc in scs]),
                 target_intrinsics=torch.stack([sc["target_intrinsics"] for sc in scs]))
    znear, zfar = scs[0]["znear"], scs[0]["zfar"]
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=True)
    inj = (torch.rand(SB, B, n_cand, generator=gen).cuda(), torch.randn(SB, B, G, generator=gen).cuda(), torch.rand(SB, B, K, generator=gen).cuda())
    u = torch.tensor([0.3, 0.7], device="cuda")
    torch.manual_seed(3)
    vgg_net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(8, 8, 3, padding=1)).cuda()
    for p in vgg_net.parameters():
        p.requires_grad = False
    vgg_fn = lambda a, b: (vgg_net(a) - vgg_net(b.detach())).abs().mean()
    params = dict(nerf.mlp_fine.named_parameters())

    def grads():
        out = {k: p.grad.clone() for k, p in params.items()}
        for p in nerf.parameters():
            p.grad = None
        return out

    def new_route(fn, w):
        info = {}
        with noise.inject(*inj):
            ld = objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, w_vgg=w, vgg_spatch=s, w_antibias=w_ab,
                                       antibias_downsampling=n, vgg_fn=fn, u=u, info=info)
        lat = nerf.encoder.latent
        ld["total"].backward()
        return ld, info, lat.grad.clone(), grads()

    def old_route(pix, fn, w):
        nerf.encode(images=batch["src_rgbs"], depths=batch["src_depths"], depths_std=batch["src_depth_stds"],
                    extrinsics=batch["src_extrinsics"], intrinsics=batch["src_intrinsics"])
        rays_all = ops.gen_rays(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, "cuda")
        idx = pix.long()
        rays = rays_all.gather(1, idx[..., None].expand(-1, -1, 8)).contiguous()
        with noise.inject(*inj):
            pred = ren.forward(nerf, rays).fine.rgb
        lat = nerf.encoder.latent
        gt = batch["target_rgb"].view(SB, 3, -1).permute(0, 2, 1).gather(1, idx[..., None].expand(-1, -1, 3))
        mse = torch.nn.functional.mse_loss(pred, gt)
        pn, gn = (t.view(SB, s, s, 3).permute(0, 3, 1, 2) for t in (pred, gt))
        pool = torch.nn.AvgPool2d(2 ** n, 2 ** n)
        ab = torch.nn.L1Loss()(pool(pn), pool(gn))
        total = mse + w_ab * ab
        vg = None
        if fn is not None:
            vg = fn(pn, gn)
            total = total + w * vg
        total.backward()
        return dict(rgb_fine=mse, antibias=ab, total=total, vgg_fine=vg), rays, pred.detach(), lat.grad.clone(), grads()

    # w_vgg != 0 selects the patch; a zero-valued vgg_fn leaves MSE + anti-bias
    zero_fn = lambda a, b: (a * 0).sum()
    ld, info, lat_new, g_new = new_route(zero_fn, 1e-30)
    assert set(ld) == {"rgb_fine", "vgg_fine", "antibias", "total"}
    assert len(encode_calls) == 1 and all(a is batch[k] for a, k in zip(encode_calls[0], ("src_rgbs", "src_depths", "src_depth_stds",
                                                                                         "src_extrinsics", "src_intrinsics")))
    pix = info["pix"]
    assert tuple(pix.shape) == (SB, B) and int(info["empty_mask"].sum()) == 0
    ref, rays_old, pred_old, lat_old, g_old = old_route(pix, None, 0.0)
    assert torch.equal(ops.gen_rays_at(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, pix), rays_old)
    assert torch.equal(info["pred"].detach(), pred_old)          # the same rays with the same noise: the same colours, bit for bit
    l64 = info["losses_f64"].cpu().numpy()
    want64, _ = host_objective(pred_old.cpu().numpy(), ref_gt(batch, pix, SB), s, n, w_ab)
    for k, name in enumerate(("rgb_fine", "antibias", "total")):
        yard = abs(float(ref[name]) - want64[k]) / want64[k]                    # the torch expression's own float32 error on this step
        assert abs(l64[k] - want64[k]) <= max(1e-12, 4 * yard) * want64[k], (name, l64[k], want64[k], yard)
        assert abs(float(ld[name]) - float(ref[name])) <= 1e-6 * float(ref[name]), name
    worst = max(max_norm_rel(g_new[k].cpu(), g_old[k].cpu()) for k in g_new)
    e_lat = max_norm_rel(lat_new.cpu(), lat_old.cpu())
    print(f"calc_losses against the assembled step: losses f64 {l64}, worst parameter gradient {worst:.2e}, d latent {e_lat:.2e}")
    assert worst < TOL_ROUTES and e_lat < TOL_ROUTES
    assert all(float(v.abs().max()) > 0 for v in g_new.values()) and float(lat_new.abs().max()) > 0
    # with a perceptual term
    ld_v, info_v, lat_v, g_v = new_route(vgg_fn, w_vgg)
    assert torch.equal(info_v["pix"], pix)
    ref_v, _, _, lat_ov, g_ov = old_route(pix, vgg_fn, w_vgg)
    assert float(ld_v["vgg_fine"]) > 0 and abs(float(ld_v["vgg_fine"]) - float(ref_v["vgg_fine"])) <= 1e-6 * float(ref_v["vgg_fine"])
    assert abs(float(ld_v["total"]) - (float(ld["total"]) + w_vgg * float(ld_v["vgg_fine"]))) <= 1e-6 * float(ld_v["total"])
    assert abs(float(ld_v["total"]) - float(ref_v["total"])) <= 1e-6 * float(ref_v["total"])
    worst_v = max(max_norm_rel(g_v[k].cpu(), g_ov[k].cpu()) for k in g_v)
    assert worst_v < TOL_ROUTES and max_norm_rel(lat_v.cpu(), lat_ov.cpu()) < TOL_ROUTES
    assert max(max_norm_rel(g_v[k].cpu(), g_new[k].cpu()) for k in g_v) > 1e-4          # the perceptual term did reach the gradients
    # the random-pixel mode (w_vgg == 0): loose pixels, MSE alone
    torch.manual_seed(4)
    info_r = {}
    ld_r = objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, ray_batch_size=128, info=info_r)
    assert tuple(info_r["pix"].shape) == (SB, 128) and info_r["empty_mask"] is None and ld_r["antibias"] == 0. and ld_r["vgg_fine"] == 0.
    assert torch.equal(ld_r["total"], ld_r["rgb_fine"]) and float(ld_r["total"]) > 0
    ld_r["total"].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params.values())
    # refusals
    with pytest.raises(ValueError, match="vgg_fn"):
        objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, w_vgg=0.1, vgg_spatch=s)
    with pytest.raises(ValueError, match="patch"):
        objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, w_antibias=1.0)


def ref_gt(batch, pix, SB):
    return batch["target_rgb"].view(SB, 3, -1).permute(0, 2, 1).gather(1, pix.long()[..., None].expand(-1, -1, 3)).cpu().numpy()
