"""GPU: the perceptual network (csrc/perceptual.hip, diner_amd.perceptual) against torch on the CPU in float64, computed at run time.

The convolution's bound is a priori: every output is one sequential fp32 fmaf chain over K products that starts at the bias, so
|dev - f64| <= (K + 2) 2^-24 (|x| (*) |w| + |b|) element by element (K = 9 Cin forward, 9 Cout for the data gradient).  The pools are
compared bit for bit, the input kernels to 2 ulp, the two reductions (double on the device) to 1e-12, and LPIPS / the VGG loss end to
end to the project's parity bar of 1e-4 relative.  The end-to-end tests print the deviation they measure beside that of torch's own
float32 CPU evaluation (fixture G26); DESIGN.md section 8j quotes a run."""
import functools
import importlib.util
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import load, max_norm_rel
from tests.test_perceptual_cpu import generator

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CONV_SHAPES = ((2, 5, 7, 3, 8),          # smaller than a tile, all halo
               (1, 37, 45, 8, 20),       # tails in every dimension
               (2, 16, 24, 64, 64),      # a real layer shape, two images side by side
               (1, 9, 11, 512, 512),     # full K depth
               (3, 1, 1, 16, 16))        # only the centre tap is live


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def G():
    return generator()


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """Seeded operands of one shape and the float64 references of both directions, computed once."""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(1000 + Cin + H)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    r = torch.randn(N, Cin, H, W, generator=g)
    x = torch.where(r >= 0, r + 1e-3, r - 1e-3)          # forward: the input; backward: the pre-activation below, >= 1e-3 from zero
    gy = torch.randn(N, Cout, H, W, generator=g)
    addend = torch.randn(N, Cin, H, W, generator=g) * 0.5
    x64, w64, b64 = x.double(), w.double(), b.double()
    pre = F.conv2d(x64, w64, b64, padding=1)
    pre_bound = (9 * Cin + 2) * U * (F.conv2d(x64.abs(), w64.abs(), padding=1) + b64.abs().view(1, -1, 1, 1))
    # the data gradient: a = relu(x) feeds the convolution and is a tap (addend); autograd through conv + ReLU in float64
    leaf = x64.clone().requires_grad_(True)
    a = F.relu(leaf)
    loss = (F.conv2d(a, w64, b64, padding=1) * gy.double()).sum() + (a * addend.double()).sum()
    grad, = torch.autograd.grad(loss, leaf)
    grad_bound = (9 * Cout + 2) * U * (F.conv_transpose2d(gy.double().abs(), w64.abs(), padding=1) + addend.double().abs())
    return dict(x=x, w=w, b=b, gy=gy, addend=addend, pre=pre, pre_bound=pre_bound, grad=grad, grad_bound=grad_bound)


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_forward_within_the_fmaf_chain_bound(shape, relu):
    from diner_amd import ops
    N, H, W, Cin, Cout = shape
    c = conv_case(shape)
    wp = ops.pack_conv3x3(c["w"]).cuda()
    bias = torch.zeros(wp.shape[3])
    bias[:Cout] = c["b"]
    y = ops.conv3x3(nhwc(c["x"]).cuda(), wp, bias.cuda(), Cout, relu=relu)
    assert tuple(y.shape) == (N, H, W, Cout)
    want = F.relu(c["pre"]) if relu else c["pre"]
    err = (nchw(y.cpu()).double() - want).abs()
    print(f"conv3x3 {shape} relu={relu}: max |dev - f64| / bound = {float((err / c['pre_bound']).max()):.3f}, max abs {float(err.max()):.2e}")
    assert bool((err <= c["pre_bound"]).all())
    if relu:
        assert float(y.min()) >= 0.0 and float((y == 0).float().mean()) > 0.2


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3x3_data_gradient_with_addend_and_saved_mask(shape):
    from diner_amd import ops
    N, H, W, Cin, Cout = shape
    c = conv_case(shape)
    assert float(c["x"].abs().min()) >= 1e-3                     # no pre-activation near the ReLU's switch: the mask is unambiguous
    act = nhwc(F.relu(c["x"])).cuda()                           # the saved post-ReLU activation
    wt = ops.pack_conv3x3(c["w"], transpose=True).cuda()
    g = ops.conv3x3(nhwc(c["gy"]).cuda(), wt, None, Cin, addend=nhwc(c["addend"]).cuda(), mask=act)
    assert tuple(g.shape) == (N, H, W, Cin)
    got = nchw(g.cpu()).double()
    err = (got - c["grad"]).abs()
    print(f"conv3x3 data gradient {shape}: max |dev - f64| / bound = {float((err / c['grad_bound']).max()):.3f}")
    assert bool((err <= c["grad_bound"]).all())
    assert bool((got[c["x"] < 0] == 0).all()) and float((got != 0).double().mean()) > 0.3
    # without the epilogue: the plain transposed convolution
    plain = nchw(ops.conv3x3(nhwc(c["gy"]).cuda(), wt, None, Cin).cpu()).double()
    want = F.conv_transpose2d(c["gy"].double(), c["w"].double(), padding=1)
    assert bool(((plain - want).abs() <= c["grad_bound"]).all())


@pytest.mark.parametrize("size", ((5, 7), (37, 45), (2, 2)))
def test_maxpool2_is_torch_bit_for_bit(size):
    from diner_amd import ops
    H, W = size
    N, C = 2, 5
    g = torch.Generator().manual_seed(H * 100 + W)
    smooth = torch.randn(N, C, H, W, generator=g)
    ties = torch.randint(0, 3, (N, C, H, W), generator=g).float()          # equal positive values inside most windows
    for x in (smooth, ties):
        leaf = x.clone().requires_grad_(True)
        y = F.max_pool2d(leaf, 2, 2)
        gy = torch.randn(y.shape, generator=g)
        y.backward(gy)
        xd = nhwc(x).cuda()
        yd = ops.maxpool2(xd)
        assert tuple(yd.shape) == (N, H // 2, W // 2, C) and torch.equal(nchw(yd.cpu()), y.detach())
        gd = ops.maxpool2_bwd(xd, nhwc(gy).cuda())
        assert torch.equal(nchw(gd.cpu()), leaf.grad)
        addend = torch.randn(N, C, H, W, generator=g)
        full = ops.maxpool2_bwd(xd, nhwc(gy).cuda(), addend=nhwc(addend).cuda(), relu_mask=True)
        assert torch.equal(nchw(full.cpu()), (leaf.grad + addend) * (x > 0))
    assert int((ties[:, :, 0, 0] == ties[:, :, 0, 1]).sum()) > 0


def _ulps(got, want):
    return float(((got.double() - want.double()).abs() / torch.from_numpy(np.spacing(want.abs().numpy())).double()).max())


def test_image_in_and_its_adjoint_within_two_ulp():
    from diner_amd import ops, perceptual as P
    g = torch.Generator().manual_seed(4)
    N, H, W = 2, 9, 13
    for shift, scale, lo in ((P.VGG_MEAN, P.VGG_STD, 0.0), (P.LPIPS_SHIFT, P.LPIPS_SCALE, -1.0)):
        x = torch.rand(N, 3, H, W, generator=g) * (1.0 - lo) + lo
        sh, sc = torch.tensor(shift).view(1, 3, 1, 1), torch.tensor(scale).view(1, 3, 1, 1)
        leaf = x.clone().requires_grad_(True)
        want = (leaf - sh) / sc
        gz = torch.randn(N, 3, H, W, generator=g)
        want.backward(gz)
        for pad in (True, False):
            z = ops.image_in(x.cuda(), shift, scale, pad=pad).cpu()
            assert tuple(z.shape) == (N, H, W, 4 if pad else 3)
            assert _ulps(nchw(z[..., :3]), want.detach()) <= 2
            if pad:
                assert float(z[..., 3].abs().max()) == 0.0
            gpad = torch.cat([nhwc(gz), torch.full((N, H, W, 1), 7.0)], dim=3) if pad else nhwc(gz)      # the fourth channel is ignored
            gx = ops.image_in_bwd(gpad.cuda(), scale).cpu()
            assert tuple(gx.shape) == (N, 3, H, W) and _ulps(gx, leaf.grad) <= 2


@pytest.mark.parametrize("n", (1000, 300001))          # one pass per thread; more elements than 1024 workgroups hold at once
def test_feature_l1_mean_and_gradient_plane(n):
    from diner_amd import ops
    g = torch.Generator().manual_seed(n)
    fx = F.relu(torch.randn(n, generator=g))
    fy = F.relu(torch.randn(n, generator=g))
    fy[::7] = fx[::7]                                 # equal entries: sign 0
    w = 0.25
    mean, grad = ops.feature_l1(fx.cuda(), fy.cuda(), weight=w)
    want = float((fx.double() - fy.double()).abs().mean())
    assert mean.dtype == torch.float64 and abs(float(mean) - want) <= 1e-12 * want
    plane = torch.sign(fx - fy) * np.float32(w / n)
    assert torch.equal(grad.cpu(), plane)
    mean2, masked = ops.feature_l1(fx.cuda(), fy.cuda(), weight=w, mask_by_fx=True)
    assert torch.equal(mean2, mean) and torch.equal(masked.cpu(), plane * (fx > 0))
    assert ops.feature_l1(fx.cuda(), fy.cuda(), want_grad=False)[1] is None


@pytest.mark.parametrize("shape", ((1, 1, 1, 5), (2, 37, 45, 130), (3, 4, 4, 64)))      # C below, above and at one wave; strided pixels
def test_lpips_layer_against_float64(shape):
    from diner_amd import ops
    N, H, W, C = shape
    g = torch.Generator().manual_seed(C)
    fx, fy = F.relu(torch.randn(N, H, W, C, generator=g)), F.relu(torch.randn(N, H, W, C, generator=g))
    fx[0, 0, 0] = 0                                   # an all-zero pixel: 0 / (0 + 1e-10)
    lin = torch.rand(C, generator=g)
    a, b = fx.double(), fy.double()
    a = a / (a.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    b = b / (b.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    want = ((a - b) ** 2 * lin.double()).sum(-1).mean(dim=(1, 2))
    out = ops.lpips_layer(fx.cuda(), fy.cuda(), lin.cuda())
    assert out.dtype == torch.float64 and float(((out.cpu() - want).abs() / want).max()) <= 1e-12
    twice = ops.lpips_layer(fx.cuda(), fy.cuda(), lin.cuda(), out=out.clone())
    assert float(((twice.cpu() - 2 * want).abs() / want).max()) <= 1e-12


@pytest.mark.parametrize("case", (0, 1))
def test_lpips_end_to_end(case):
    from diner_amd import perceptual as P
    arch, div, N, H, W, seed = G().LPIPS_CASES[case]
    fx = load("g26_perceptual.npz")
    sd = G().state_dict(arch, div)
    pred, gt = G().lpips_inputs(N, H, W, seed)
    want = G().lpips_restated(sd, pred, gt)
    assert np.abs(want.numpy() - fx[f"lpips{case}_score64"]).max() <= 1e-12 * np.abs(want.numpy()).max()
    lp = P.Lpips(sd)
    got = lp(pred.cuda(), gt.cuda())
    assert tuple(got.shape) == (N, 1, 1, 1) and got.dtype == torch.float32 and got.is_cuda
    rel = ((got.cpu().view(-1).double() - want).abs() / want.abs()).numpy()
    print(f"lpips {arch} / {div} {N}x3x{H}x{W}: device-vs-f64 {rel.tolist()}, torch float32-vs-f64 {fx[f'lpips{case}_f32_rel'].tolist()}")
    assert rel.max() <= 1e-4
    assert float(lp(pred.cuda(), pred.cuda()).abs().max()) == 0.0
    with pytest.raises(ValueError, match=">= 16"):
        lp(pred[..., :15].cuda(), gt[..., :15].cuda())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lp(pred, gt)


@functools.lru_cache(maxsize=None)
def loss_reference(case):
    """float64 src.losses.VGGLoss on the CPU: (state dict, x, y, loss, gradient)."""
    from src.losses import VGGLoss
    arch, div, N, H, W, seed = G().LOSS_CASES[case]
    sd = G().state_dict(arch, div)
    x, y = G().loss_inputs(N, H, W, seed)
    leaf = x.double().requires_grad_(True)
    loss = VGGLoss(features=G().sequential_from(sd, arch).double())(leaf, y.double())
    loss.backward()
    return sd, x, y, float(loss.detach()), leaf.grad


@pytest.mark.parametrize("case", (0, 1, 2, 3))
def test_vgg_loss_end_to_end(case):
    from diner_amd import perceptual as P
    fx = load("g26_perceptual.npz")
    sd, x, y, want, gwant = loss_reference(case)
    # the reference side first: these inputs are well away from a switch of a sign, a mask or a pool's choice (torch's own float32
    # evaluation stays at rounding level), so the gradient can tell two float32 evaluations apart
    assert float(fx[f"loss{case}_grad_f32_rel"]) <= 1e-5 and abs(float(fx[f"loss{case}_loss64"]) - want) <= 1e-12 * want
    vgg = P.VggLoss(sd)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    loss = vgg(xd, yd)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    loss.backward()
    e_l = abs(float(loss.detach()) - want) / want
    e_g = float((xd.grad.cpu().double() - gwant).norm() / gwant.norm())
    print(f"vgg loss case {case} {G().LOSS_CASES[case]}: loss device-vs-f64 {e_l:.2e} (torch float32 {float(fx[f'loss{case}_f32_rel']):.2e}), "
          f"gradient {e_g:.2e} (torch float32 {float(fx[f'loss{case}_grad_f32_rel']):.2e})")
    assert e_l <= 1e-4 and e_g <= 1e-4
    assert yd.grad is None
    # a scaled loss scales the gradient; no gradient wanted: the same value, nothing saved
    g1 = xd.grad.clone()
    xd.grad = None
    (3.0 * vgg(xd, yd)).backward()
    assert torch.equal(xd.grad, 3.0 * g1)
    with torch.no_grad():
        assert torch.equal(vgg(xd, yd), loss.detach())
    if case == 0:
        with pytest.raises(ValueError, match=">= 8"):
            vgg(xd[..., :7], yd[..., :7])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            vgg(x, y)


def test_scores_do_not_depend_on_the_batch_and_runs_repeat():
    from diner_amd import perceptual as P
    arch, div, N, H, W, seed = G().LPIPS_CASES[0]
    lp = P.Lpips(G().state_dict(arch, div))
    pred, gt = (t.cuda() for t in G().lpips_inputs(4, H, W, seed + 1))
    alone = lp(pred[:1], gt[:1])
    four = lp(pred, gt)
    back = lp(pred.flip(0), gt.flip(0))          # image 0 at position 3
    assert torch.equal(four[0], alone[0]) and torch.equal(back[3], alone[0]) and torch.equal(lp(pred, gt), four)
    assert len({float(v) for v in four.view(-1)}) == 4
    # several passes through the stack (large batches) give the bits of one
    keep = P.PIXELS_PER_PASS
    P.PIXELS_PER_PASS = H * W * 3 - 1
    try:
        assert torch.equal(lp(pred, gt), four)
    finally:
        P.PIXELS_PER_PASS = keep
    sd, x, y, _, _ = loss_reference(0)
    vgg = P.VggLoss(sd)
    runs = []
    for _ in range(2):
        xd = x.cuda().requires_grad_(True)
        loss = vgg(xd, y.cuda())
        loss.backward()
        runs.append((loss.detach(), xd.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_perceptual_calls_do_not_synchronise():
    from diner_amd import perceptual as P
    arch, div, N, H, W, seed = G().LPIPS_CASES[0]
    lp = P.Lpips(G().state_dict(arch, div))
    pred, gt = (t.cuda() for t in G().lpips_inputs(N, H, W, seed))
    sd, x, y, _, _ = loss_reference(1)
    vgg = P.VggLoss(sd)
    xc, yc = x.cuda(), y.cuda()

    def run():
        s = lp(pred, gt)
        xd = xc.clone().requires_grad_(True)
        vgg(xd, yc).backward()
        return s, xd.grad

    run()                                             # warm-up: module loading, allocator
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s, grad = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(s).all() and torch.isfinite(grad).all()


def test_calc_losses_with_the_device_vgg_loss():
    """The small scene of tests/test_objective_gpu.py's end-to-end test (two 64 x 64 objects, a 32 x 32 patch), with the perceptual term
    computed by VggLoss on the device against src.losses.VGGLoss through torch on the same stack."""
    from diner_amd import noise, objective, perceptual as P
    from diner_amd.synthetic import build_modules, make_mlp_state_dict, make_scene
    from src.losses import VGGLoss
    W = H = 64
    SB, s, n, K, Gn, n_cand, w_ab, w_vgg = 2, 32, 3, 40, 15, 1000, 1.0, 0.1
    B = s * s
    scs = [make_scene(W, H, seed=21 + i) for i in range(SB)]
    nerf, R = build_modules(scs, make_mlp_state_dict(), torch.device("cuda", 0))
    nerf.train()
    latent0 = nerf.encoder.latent.detach().clone()

    def encode(images, depths, depths_std, extrinsics, intrinsics):
        nerf.encoder.latent = latent0.clone().requires_grad_(True)
        nerf._scenes = {}

    nerf.encode = encode
    gen = torch.Generator().manual_seed(9)
    st = lambda k: torch.stack([sc[k] for sc in scs]).cuda()          # noqa: E731
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    alpha = (((yy - 30) ** 2 + (xx - 34) ** 2) < 20 ** 2).float() * (0.25 + 0.75 * torch.rand(SB, 1, H, W, generator=gen))
    batch = dict(src_rgbs=torch.rand(SB, 4, 3, H, W, generator=gen).cuda(), src_depths=st("depths"), src_depth_stds=st("depths_std"),
                 src_extrinsics=st("src_extrinsics"), src_intrinsics=st("src_intrinsics"), target_rgb=torch.rand(SB, 3, H, W, generator=gen).cuda(),
                 target_alpha=alpha.cuda(), target_extrinsics=torch.stack([sc["target_extrinsics"] for sc in scs]),
                 target_intrinsics=torch.stack([sc["target_intrinsics"] for sc in scs]))
    znear, zfar = scs[0]["znear"], scs[0]["zfar"]
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=Gn, white_bkgd=True)
    inj = (torch.rand(SB, B, n_cand, generator=gen).cuda(), torch.randn(SB, B, Gn, generator=gen).cuda(), torch.rand(SB, B, K, generator=gen).cuda())
    u = torch.tensor([0.3, 0.7], device="cuda")
    stack = G().sequential_from(G().state_dict("vgg19", G().NARROW), "vgg19")

    def route(fn):
        with noise.inject(*inj):
            ld = objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, w_vgg=w_vgg, vgg_spatch=s, w_antibias=w_ab,
                                       antibias_downsampling=n, vgg_fn=fn, u=u)
        lat = nerf.encoder.latent
        ld["total"].backward()
        for p in nerf.parameters():
            p.grad = None
        return ld, lat.grad.clone()

    ld_d, lat_d = route(P.VggLoss(stack))
    ld_t, lat_t = route(VGGLoss(features=stack).cuda())
    e_v = abs(float(ld_d["vgg_fine"]) - float(ld_t["vgg_fine"])) / float(ld_t["vgg_fine"])
    e_t = abs(float(ld_d["total"]) - float(ld_t["total"])) / float(ld_t["total"])
    e_lat = float((lat_d - lat_t).norm() / lat_t.norm())
    print(f"calc_losses, device VggLoss against torch VGGLoss: vgg_fine {e_v:.2e}, total {e_t:.2e}, latent gradient (L2) {e_lat:.2e}")
    assert float(ld_t["vgg_fine"]) > 0 and e_v <= 1e-4 and e_t <= 1e-4 and e_lat <= 1e-4
    assert max_norm_rel(lat_d.cpu(), lat_t.cpu()) < 1e-3 and float(lat_d.abs().max()) > 0


def test_evaluate_folder_with_lpips_weights(tmp_path):
    from diner_amd import perceptual as P
    from diner_amd.evaluate import GT_SUFFIX, PRED_SUFFIX, evaluate_folder
    from diner_amd.png import write_png
    from src.evaluation import eval_suite as E
    sd = G().state_dict("vgg16", G().NARROW)
    weights = tmp_path / "lpips_vgg.pth"
    torch.save(sd, weights)
    src = tmp_path / "visualizations"
    src.mkdir()
    rs = np.random.RandomState(5)
    pairs = []
    for i, (h, w) in enumerate(((20, 24), (20, 24))):
        gt = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        pred = np.clip(gt.astype(np.int32) + rs.randint(-40, 41, gt.shape), 0, 255).astype(np.uint8)
        write_png(src / f"s{i}{GT_SUFFIX}", gt)
        write_png(src / f"s{i}{PRED_SUFFIX}", pred)
        pairs.append((pred, gt))
    avg = evaluate_folder(src, tmp_path / "with", lpips_weights=weights)
    assert set(avg) == {"ssim", "psnr", "l2", "l1", "lpips"}
    lp = P.Lpips(sd)
    to = lambda a: (torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1)[None] * 2.0 - 1.0).cuda()          # noqa: E731
    direct = [float(lp(to(p), to(g))) for p, g in pairs]
    report = json.load(open(tmp_path / "with" / "detailed_report.json"))
    assert [r["lpips"] for r in report] == direct and avg["lpips"] == float(np.mean(direct)) and min(direct) > 0
    # the drop-in passes its module attribute on
    E.LPIPS_WEIGHTS = weights
    try:
        assert E.evaluate_folder(src, tmp_path / "dropin") == avg
    finally:
        E.LPIPS_WEIGHTS = None
    with pytest.raises(ValueError, match="not both"):
        evaluate_folder(src, tmp_path / "both", lpips_fn=lp, lpips_weights=weights)
    # without the argument: as before -- the lpips package decides, and its absence warns
    if importlib.util.find_spec("lpips") is None:
        with pytest.warns(UserWarning, match="lpips is left out"):
            plain = evaluate_folder(src, tmp_path / "without")
        assert set(plain) == {"ssim", "psnr", "l2", "l1"} and all(plain[k] == avg[k] for k in plain)
