"""GPU: diner_amd.fit (the loop, checkpoints) and what the first in-place optimiser closes on the training path: the persistent
packed-weights handle and the inference cache both see the weights DeviceAdam wrote.  Scene: the smallest one the training tests use
(tests.test_boundary_gpu.setup_model(32, 32, 6), K = 40, n_gaussian 15), feature maps injected."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
W = H = 32
K, G = 40, 15
LR = 1e-5       # Adam moves every weight by about lr a step whatever the gradient's size: 1e-3 takes this MLP to zero density in one step


def scene_model(n_obj=1):
    """-> (nerf in train mode with the scene(s) injected and encode() a no-op, renderer class, batch, znear, zfar, scene dict)"""
    from tests.helpers import oracle_setup
    from tests.test_boundary_gpu import setup_model
    sc, nerf, R, _ = setup_model(W, H, 6)
    scs = [sc] + [oracle_setup(W, H, 6 + i)[0] for i in range(1, n_obj)]
    if n_obj > 1:
        enc = nerf.encoder
        st = lambda k: torch.stack([s[k] for s in scs]).cuda()
        enc.depths, enc.depths_std, enc.normals, enc.latent = st("depths"), st("depths_std"), st("normals"), st("latent")
        enc.nobjects = n_obj
        Kin = torch.stack([s["src_intrinsics"] for s in scs])
        nerf.poses = st("src_extrinsics")
        nerf.c = Kin[:, :, :2, -1].cuda()
        nerf.focal = Kin[:, :, [0, 1], [0, 1]].cuda()
    nerf.encode = lambda *a, **k: None             # the injected maps stand in for the ResNet trunk, as everywhere in this suite
    nerf.train()
    st = lambda k: torch.stack([s[k] for s in scs])
    batch = dict(src_rgbs=torch.zeros(n_obj, 4, 3, H, W).cuda(), src_depths=st("depths").cuda(), src_depth_stds=st("depths_std").cuda(),
                 src_extrinsics=st("src_extrinsics").cuda(), src_intrinsics=st("src_intrinsics").cuda(),
                 target_rgb=torch.full((n_obj, 3, H, W), 0.25).cuda(), target_alpha=torch.ones(n_obj, 1, H, W).cuda(),
                 target_extrinsics=st("target_extrinsics"), target_intrinsics=st("target_intrinsics"))
    return nerf, R, batch, sc["znear"], sc["zfar"], sc


def renderer(R):
    return R(n_samples=K, n_depth_candidates=1000, n_gaussian=G, white_bkgd=False)


def mlp_params(nerf):
    return torch.cat([p.detach().reshape(-1) for p in nerf.mlp_fine.parameters()])


def test_three_fit_steps_track_the_loop_on_torch_adam():
    from diner_amd.fit import fit
    from diner_amd.objective import calc_losses
    nerf, R, batch, znear, zfar, _ = scene_model()
    twin = copy.deepcopy(nerf)
    ren = renderer(R)
    kw = dict(znear=znear, zfar=zfar, ray_batch_size=64)

    def fixed_loss(model):
        torch.manual_seed(99)
        return float(calc_losses(model, ren, batch, seed=5, step=0, **kw)["total"].detach())

    before = fixed_loss(nerf)
    logged = []
    torch.manual_seed(11)
    history, opt = fit(nerf, ren, [batch], steps=3, lr=LR, seed=5, on_log=logged.extend, **kw)
    assert [h["step"] for h in history] == [0, 1, 2] and logged == history and opt.stats()["step"] == 3
    assert all(set(h) == {"step", "rgb_fine", "vgg_fine", "antibias", "total"} for h in history)
    torch.manual_seed(11)
    ref = torch.optim.Adam([p for p in twin.parameters() if p.requires_grad], lr=LR)
    want = []
    for k in range(3):
        ref.zero_grad()
        total = calc_losses(twin, ren, batch, seed=5, step=k, **kw)["total"]
        total.backward()
        ref.step()
        want.append(float(total.detach()))
    got = [h["total"] for h in history]
    print("losses fit       ", " ".join(f"{x:.7f}" for x in got))
    print("losses torch Adam", " ".join(f"{x:.7f}" for x in want))
    assert max(abs(a - b) / b for a, b in zip(got, want)) < 1e-4
    after = fixed_loss(nerf)
    print(f"loss on a fixed draw of rays: {before:.6f} -> {after:.6f}")
    assert after < before


def test_inplace_weights_reach_the_persistent_handle():
    from diner_amd import train
    from diner_amd.objective import calc_losses
    from diner_amd.optim import DeviceAdam
    nerf, R, batch, znear, zfar, _ = scene_model(2)
    ren = renderer(R)
    kw = dict(znear=znear, zfar=zfar, ray_batch_size=512, seed=3)          # 2 objects x 512 rays x 40 samples: 20 480 points per object

    def forward(seed):
        torch.manual_seed(seed)
        info = {}
        losses = calc_losses(nerf, ren, batch, step=0, info=info, **kw)
        return losses["total"], info["pred"].detach().clone()

    opt = DeviceAdam([p for p in nerf.parameters() if p.requires_grad], lr=LR)
    _, pred_before = forward(2)
    total, _ = forward(1)
    total.backward()
    opt.step(zero_grads=True)                       # in place, no release_buffers(): the handle of the two forwards above lives on
    _, pred_kept = forward(2)
    train.release_buffers()                         # forces a fresh handle, packed from the same weights
    _, pred_fresh = forward(2)
    _, pred_again = forward(2)
    spread = float((pred_fresh - pred_again).abs().max())
    diff = float((pred_kept - pred_fresh).abs().max())
    print(f"two identical forwards differ by {spread:.3e}; kept handle against fresh handle {diff:.3e}; the step moved pred by "
          f"{float((pred_kept - pred_before).abs().max()):.3e}")
    if spread == 0.0:
        assert torch.equal(pred_kept, pred_fresh)
    else:
        assert diff <= 4 * spread
    assert not torch.equal(pred_kept, pred_before) and float((pred_kept - pred_before).abs().max()) > 4 * spread


def test_inference_cache_sees_the_step():
    from diner_amd.fit import fit
    from diner_amd.render import predict_image
    from tests.test_boundary_gpu import setup_model
    nerf, R, batch, znear, zfar, sc = scene_model()
    ren = renderer(R)
    E, Kt = sc["target_extrinsics"][None].cuda(), sc["target_intrinsics"][None].cuda()
    frame = lambda model: predict_image(model.eval(), ren, E, Kt, W, H, znear, zfar, seed=1234)
    rgb0, depth0 = frame(nerf)                      # packs the inference weights
    nerf.train()
    torch.manual_seed(4)
    fit(nerf, ren, [batch], znear=znear, zfar=zfar, steps=1, lr=LR, seed=5, ray_batch_size=64)
    rgb1, depth1 = frame(nerf)
    fresh = setup_model(W, H, 6)[1]
    fresh.load_state_dict(nerf.state_dict())
    rgb2, depth2 = frame(fresh)
    assert torch.equal(rgb1, rgb2) and torch.equal(depth1, depth2)
    assert not torch.equal(rgb1, rgb0)


def test_checkpoint_resumes_the_run(tmp_path):
    from diner_amd.fit import fit, load_checkpoint, save_checkpoint
    from diner_amd.optim import DeviceAdam

    def start():
        torch.manual_seed(7)
        nerf, R, batch, znear, zfar, _ = scene_model()
        return nerf, renderer(R), batch, dict(znear=znear, zfar=zfar, lr=LR, seed=5, ray_batch_size=64)

    def whole():
        nerf, ren, batch, kw = start()
        history, _ = fit(nerf, ren, [batch], steps=3, **kw)
        return mlp_params(nerf), history[-1]["total"]

    p_a, l_a = whole()
    p_b, l_b = whole()
    spread_p, spread_l = float((p_a - p_b).abs().max()), abs(l_a - l_b)
    nerf, ren, batch, kw = start()
    _, opt = fit(nerf, ren, [batch], steps=2, **kw)
    rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    path = str(tmp_path / "two.ckpt")
    save_checkpoint(path, nerf, opt, 2, znear=kw["znear"], zfar=kw["zfar"])
    ckpt = torch.load(path, weights_only=False)
    assert set(ckpt) == {"state_dict", "optimizer_states", "global_step"} and all(k.startswith("nerf.") or k in ("znear", "zfar") for k in ckpt["state_dict"])
    assert all(float(s["step"]) == 2.0 for s in ckpt["optimizer_states"][0]["state"].values())
    fresh, ren2, _, _ = start()
    with torch.no_grad():
        for p in fresh.mlp_fine.parameters():
            p.zero_()                               # nothing of the result may come from the fresh model's own weights
    fresh_opt = DeviceAdam([p for p in fresh.parameters() if p.requires_grad], lr=9.0)
    assert load_checkpoint(path, fresh, fresh_opt) == 2 and fresh_opt.stats()["step"] == 2 and fresh_opt.group["lr"] == LR
    torch.set_rng_state(rng[0])
    torch.cuda.set_rng_state(rng[1])
    history, _ = fit(fresh, ren2, [batch], steps=1, start_step=2, optimizer=fresh_opt, **kw)
    assert history[0]["step"] == 2 and fresh_opt.stats()["step"] == 3
    diff_p, diff_l = float((mlp_params(fresh) - p_a).abs().max()), abs(history[0]["total"] - l_a)
    print(f"uninterrupted runs differ by {spread_p:.3e} (weights) / {spread_l:.3e} (third loss); resumed against uninterrupted {diff_p:.3e} / {diff_l:.3e}")
    if spread_p == 0.0 and spread_l == 0.0:
        assert diff_p == 0.0 and diff_l == 0.0
    else:                                           # the logged loss is a float32: one unit in its last place where its own spread rounds to 0
        assert diff_p <= 4 * spread_p and diff_l <= max(4 * spread_l, 2.0 ** -23 * l_a)
