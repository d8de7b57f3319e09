"""GPU: the image encoder's trunk on the device (csrc/conv2d.hip, csrc/encoder.hip, diner_amd.encoder) against torch on the CPU in float64, computed at run
time.

The strided convolution's bound is a priori, the one tests/test_perceptual_gpu.py uses: every output is one sequential fp32 fmaf chain over
K = R R Cin products that starts at the bias, so |dev - f64| <= (K + 2) 2^-24 (|x| (*) |w| + |b|) element by element, whatever the order.
The pool and the input assembly are compared bit for bit, the resampling within 4 * 2^-24 max |x|, and the whole trunk -- fixture G27's
cases A, B, C (tools/make_golden_encoder.py) -- per pyramid level to the project's parity bar of 1e-4 of the level's maximum, printed
beside torch's own float32 CPU distance from float64 (the fixture's `yard`); DESIGN.md section 8l quotes a run."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import load
from tests.test_encoder_cpu import generator

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BAR = 1e-4
# (N, H, W, Cin, Cout, R)
CONV_SHAPES = ((2, 45, 58, 21, 64, 7),        # the stem of case A: 21 channels (element-wise loads), tails in both directions, two images
               (1, 12, 15, 64, 128, 3),       # layer2's first convolution ...
               (1, 12, 15, 64, 128, 1),       # ... and its downsample
               (1, 6, 8, 128, 256, 3),
               (3, 1, 1, 16, 16, 3),          # only the centre tap is live
               (1, 2, 3, 3, 65, 7),           # smaller than the kernel; Cout one past a tile
               (1, 7, 7, 8, 20, 1))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def G():
    return generator()


@functools.lru_cache(maxsize=None)
def conv_case(shape):
    """Seeded operands of one shape, the float64 reference and the bound, computed once."""
    N, H, W, Cin, Cout, R = shape
    g = torch.Generator().manual_seed(2000 + Cin + 10 * H + R)
    w = torch.randn(Cout, Cin, R, R, generator=g) * (2.0 / (R * R * Cin)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(N, Cin, H, W, generator=g)
    x64, w64, b64 = x.double(), w.double(), b.double()
    pre = F.conv2d(x64, w64, b64, stride=2, padding=R // 2)
    bound = (R * R * Cin + 2) * U * (F.conv2d(x64.abs(), w64.abs(), stride=2, padding=R // 2) + b64.abs().view(1, -1, 1, 1))
    return dict(x=x, w=w, b=b, pre=pre, bound=bound)


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_s2_within_the_fmaf_chain_bound(shape, relu):
    from diner_amd import ops
    N, H, W, Cin, Cout, R = shape
    c = conv_case(shape)
    y = ops.conv_s2(nhwc(c["x"]).cuda(), ops.pack_conv_s2(c["w"]).cuda(), c["b"].cuda(), Cout, R, relu=relu)
    assert tuple(y.shape) == (N, ops.conv_s2_out_size(H, R), ops.conv_s2_out_size(W, R), Cout) == tuple(nhwc(c["pre"]).shape)
    want = F.relu(c["pre"]) if relu else c["pre"]
    err = (nchw(y.cpu()).double() - want).abs()
    print(f"conv_s2 {shape} relu={relu}: max |dev - f64| / bound = {float((err / c['bound']).max()):.3f}, max abs {float(err.max()):.2e}")
    assert bool((err <= c["bound"]).all())
    if relu:
        assert float(y.min()) >= 0.0 and float((y == 0).float().mean()) > 0.2


def test_conv_s2_writes_its_channel_slice_only():
    """The stem as the trunk runs it: 24 input channels (three of them zero, the weights packed for 24), output into channels 64 .. 127
    of a 512-wide buffer; every other element keeps its canary, and the values are the bits of the dense 21-channel call."""
    from diner_amd import ops
    shape = CONV_SHAPES[0]
    N, H, W, Cin, Cout, R = shape
    c = conv_case(shape)
    x24 = torch.cat((nhwc(c["x"]), torch.zeros(N, H, W, 3)), dim=-1).cuda()
    Ho, Wo = ops.conv_s2_out_size(H, R), ops.conv_s2_out_size(W, R)
    out = torch.full((N, Ho, Wo, 512), -7.25, device="cuda")
    got = ops.conv_s2(x24, ops.pack_conv_s2(c["w"], Cin=24).cuda(), c["b"].cuda(), Cout, R, relu=True, out=out, coff=64)
    assert got is out
    o = out.cpu()
    assert bool((o[..., :64] == -7.25).all()) and bool((o[..., 128:] == -7.25).all())
    err = (nchw(o[..., 64:128]).double() - F.relu(c["pre"])).abs()
    print(f"conv_s2 into a slice: max |dev - f64| / bound = {float((err / c['bound']).max()):.3f}")
    assert bool((err <= c["bound"]).all())
    dense = ops.conv_s2(nhwc(c["x"]).cuda(), ops.pack_conv_s2(c["w"]).cuda(), c["b"].cuda(), Cout, R, relu=True)
    assert torch.equal(dense.cpu(), o[..., 64:128])


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("Cin", (12, 3))              # float4 patch loads with a ragged last chunk; element-wise loads
@pytest.mark.parametrize("size", ((11, 19), (17, 35)))
def test_conv_s2_3x3_is_conv3x3_subsampled_bit_for_bit(size, Cin, relu):
    """Both start at the bias and add the same products in the same K order (chunk, kernel row, kernel column, channel), and the zero
    padding adds exact zeros: the stride-2 output is every second pixel of the stride-1 output.  One kernel template behind both; this
    pins the parity-plane patch addressing of stride 2 against the plain one.  Odd sizes, tails in both tilings (8 x 16), two images,
    two Cout tiles with the last one ragged."""
    from diner_amd import ops
    (H, W), N, Cout = size, 2, 70
    g = torch.Generator().manual_seed(3000 + Cin + H)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = torch.zeros(128)
    b[:Cout] = torch.randn(Cout, generator=g) * 0.1
    x = torch.randn(N, H, W, Cin, generator=g).cuda()
    wp, b = ops.pack_conv3x3(w).cuda(), b.cuda()
    full = ops.conv3x3(x, wp, b, Cout, relu=relu)
    half = ops.conv_s2(x, wp, b, Cout, 3, relu=relu)
    assert tuple(half.shape) == (N, (H + 1) // 2, (W + 1) // 2, Cout)
    assert torch.equal(half, full[:, ::2, ::2])
    assert float(half.abs().max()) > 0.1 and (not relu or float((half == 0).float().mean()) > 0.2)


@pytest.mark.parametrize("size", ((1, 1), (2, 3), (7, 8), (23, 29)))
def test_maxpool3s2_is_torch_bit_for_bit(size):
    from diner_amd import ops
    H, W = size
    N, C = 2, 5
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(N, C, H, W, generator=g)
    x[:, :, : (H + 1) // 2] -= 6.0                    # whole windows negative: zero padding would win there, -inf must not
    x[1, 2] = -torch.rand(H, W, generator=g) - 0.5
    want = F.max_pool2d(x, 3, 2, 1)
    y = ops.maxpool3s2(nhwc(x).cuda())
    assert tuple(y.shape) == (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C) and torch.equal(nchw(y.cpu()), want)
    assert float(want[1, 2].max()) < 0
    # channels 0 .. 2 of a wider input (the stem's output inside the latent)
    y3 = ops.maxpool3s2(nhwc(x).cuda(), C=3)
    assert torch.equal(nchw(y3.cpu()), want[:, :3])
    # a NaN is its window's result, as in torch's CPU kernel
    xn = x.clone()
    xn[0, 1, H // 2, W // 2] = float("nan")
    wn = F.max_pool2d(xn, 3, 2, 1)
    yn = nchw(ops.maxpool3s2(nhwc(xn).cuda()).cpu())
    assert int(torch.isnan(wn).sum()) >= 1 and torch.equal(torch.isnan(yn), torch.isnan(wn)) and torch.equal(yn.nan_to_num(), wn.nan_to_num())


@pytest.mark.parametrize("channels", ((5, 11, 3), (8, 20, 4)))          # (c, Ctot, c0): element-wise, and the 16-byte path
@pytest.mark.parametrize("sizes", (((3, 4), (23, 29)), ((1, 1), (5, 7)), ((6, 8), (6, 8))))
def test_pyramid_level_against_float64_interpolate(sizes, channels):
    from diner_amd import ops
    (h, w), (Hf, Wf) = sizes
    c, Ctot, c0 = channels
    N = 2
    g = torch.Generator().manual_seed(h * 10 + w + c)
    x = torch.randn(N, c, h, w, generator=g)
    want = F.interpolate(x.double(), (Hf, Wf), mode="bilinear", align_corners=True)
    out = torch.full((N, Hf, Wf, Ctot), 3.5, device="cuda")
    assert ops.pyramid_level(nhwc(x).cuda(), out, c0) is out
    o = out.cpu()
    assert bool((o[..., :c0] == 3.5).all()) and bool((o[..., c0 + c:] == 3.5).all())
    got = nchw(o[..., c0:c0 + c])
    err = float((got.double() - want).abs().max())
    print(f"pyramid_level {sizes} {channels}: max |dev - f64| = {err:.2e}, bound {4 * U * float(x.abs().max()):.2e}")
    assert err <= 4 * U * float(x.abs().max())
    if (h, w) == (Hf, Wf):
        assert torch.equal(got, x)


@pytest.mark.parametrize("pad", (4, 8, 0))
def test_encoder_input_is_replication_pad_and_ring_bit_for_bit(pad):
    from diner_amd import ops
    N, H, W = 2, 9, 13
    g = torch.Generator().manual_seed(pad)
    x = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).cuda()
    ring = None
    want = F.pad(x, [pad] * 4, mode="replicate") if pad else x
    if pad:
        ys, xs = torch.meshgrid(torch.linspace(-1, 1, H + 2 * pad, device="cuda"), torch.linspace(-1, 1, W + 2 * pad, device="cuda"), indexing="ij")
        ring = ops.posenc(torch.stack((xs, ys), dim=-1), 4, float(np.pi), True).clone()
        ring[pad:-pad, pad:-pad] = 0
        assert tuple(ring.shape) == (H + 2 * pad, W + 2 * pad, 18) and float(ring.abs().max()) > 0.5
        want = torch.cat((want, ring.permute(2, 0, 1).unsqueeze(0).expand(N, -1, -1, -1)), dim=1)
    y = ops.encoder_input(x, ring, pad)
    assert tuple(y.shape) == (N, H + 2 * pad, W + 2 * pad, 21 if pad else 3) and torch.equal(nchw(y), want)
    wide = ops.encoder_input(x, ring, pad, C=24 if pad else 4)
    assert torch.equal(wide[..., :y.shape[3]], y) and bool((wide[..., y.shape[3]:] == 0).all())


# ---- the whole trunk ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trunk_case(case):
    """The seeded state dict and images of a G27 case and the float64 restatement of the latent, computed once."""
    sd, images, cfg = G().state_dict(case), G().images_of(case), G().config(case)
    with torch.no_grad():
        lat64 = G().trunk_restated(sd, images, torch.float64, **cfg)
    return sd, images, cfg, lat64


def make_encoder(case, sd=None):
    """The drop-in SpatialEncoder of a case with the seeded weights, on the device, in eval mode."""
    from src.models.image_encoder import SpatialEncoder
    cfg = G().config(case)
    enc = SpatialEncoder(pretrained=False, **cfg)
    enc.load_state_dict(sd if sd is not None else trunk_case(case)[0], strict=False)
    return enc.cuda().eval()


def live_strides(t):
    """Strides of the dimensions with more than one element (the others' are arbitrary)."""
    return [st for n, st in zip(t.shape, t.stride()) if n > 1]


def level_errors(lat, lat64, num_layers):
    """max |lat - lat64| / max |lat64| per pyramid level."""
    lat = lat.cpu().double()
    return [float((lat[:, :, s] - lat64[:, :, s]).abs().max() / lat64[:, :, s].abs().max()) for s in G().level_slices(num_layers)]


@pytest.mark.parametrize("case", ("A", "B", "C"))
def test_trunk_matches_the_float64_restatement(case):
    from diner_amd import encoder as E
    sd, images, cfg, lat64 = trunk_case(case)
    yard = load("g27_encoder.npz")[f"{case}_yard"]
    trunk = E.DeviceTrunk(sd, **cfg)
    lat = trunk(images.cuda())
    errs = level_errors(lat, lat64, cfg["num_layers"])
    print(f"trunk case {case}: per level max |dev - f64| / max |level| = {[f'{e:.2e}' for e in errs]}; / yard (torch CPU float32) = "
          f"{[f'{e / y:.2f}' for e, y in zip(errs, yard)]}")
    assert max(errs) <= BAR
    # shape, strides and dtype of the torch route
    enc = make_encoder(case)
    with torch.no_grad():
        enc(images.cuda(), None, None, None)
    ref = enc.latent
    assert lat.shape == ref.shape == lat64.shape and lat.dtype == ref.dtype == torch.float32 and live_strides(lat) == live_strides(ref)
    assert lat.movedim(-3, -1).is_contiguous()                      # NCHW shape, channels-last strides: what HipScene aliases
    print(f"trunk case {case}: torch route per level = {[f'{e:.2e}' for e in level_errors(ref, lat64, cfg['num_layers'])]}")
    # a module as the source gives the same bits as its state dict; a second call packs nothing and reuses the workspace
    t2 = E.DeviceTrunk(enc)
    assert torch.equal(t2(images.cuda()), lat)
    ws = t2._workspace.data_ptr()
    assert torch.equal(t2(images.cuda()), lat) and t2.packs == 1 and t2._workspace.data_ptr() == ws


def test_latent_does_not_depend_on_the_batch_position():
    from diner_amd import encoder as E
    sd, _, cfg, _ = trunk_case("A")
    g = torch.Generator().manual_seed(5)
    imgs = (torch.rand(2, 2, 3, 37, 50, generator=g) * 2 - 1).cuda()
    trunk = E.DeviceTrunk(sd, **cfg)
    full = trunk(imgs).clone()                                       # the image in question: position 3 of SB 2 x NV 2
    alone = trunk(imgs[1:, 1:]).clone()
    rev = trunk(imgs.flatten(0, 1).flip(0).reshape(2, 2, 3, 37, 50).contiguous()).clone()
    assert torch.equal(alone[0, 0], full[1, 1]) and torch.equal(rev[0, 0], full[1, 1])
    assert torch.equal(rev.flatten(0, 1).flip(0), full.flatten(0, 1))
    assert not torch.equal(full[0, 0], full[1, 1])


def test_repacking_follows_the_weights():
    from diner_amd import encoder as E
    sd, images, cfg, lat64 = trunk_case("C")
    enc = make_encoder("C")
    trunk = E.DeviceTrunk(enc)
    x = images.cuda()
    first = trunk(x).clone()
    assert max(level_errors(first, lat64, cfg["num_layers"])) <= BAR and trunk.packs == 1
    # other weights through load_state_dict: seen (in-place copies bump the version counters)
    other = G().seeded_state_dict(cfg["backbone"], 999, cfg["image_padding"], cfg["padding_pe"])
    enc.load_state_dict(other, strict=False)
    with torch.no_grad():
        want = G().trunk_restated(other, images, torch.float64, **cfg)
    second = trunk(x).clone()
    assert trunk.packs == 2 and not torch.equal(second, first) and max(level_errors(second, want, cfg["num_layers"])) <= BAR
    # an in-place operation on one BatchNorm buffer: seen
    enc.model.layer1[0].bn1.running_var.mul_(4.0)
    other["model.layer1.0.bn1.running_var"] = other["model.layer1.0.bn1.running_var"] * 4.0
    with torch.no_grad():
        want = G().trunk_restated(other, images, torch.float64, **cfg)
    third = trunk(x).clone()
    assert trunk.packs == 3 and not torch.equal(third, second) and max(level_errors(third, want, cfg["num_layers"])) <= BAR
    # a write through .data bumps no version: stale until invalidate()
    enc.model.bn1.weight.data.mul_(0.5)
    other["model.bn1.weight"] = other["model.bn1.weight"] * 0.5
    with torch.no_grad():
        want = G().trunk_restated(other, images, torch.float64, **cfg)
    stale = trunk(x).clone()
    assert trunk.packs == 3 and torch.equal(stale, third) and max(level_errors(stale, want, cfg["num_layers"])) > BAR
    trunk.invalidate()
    fresh = trunk(x).clone()
    assert trunk.packs == 4 and not torch.equal(fresh, third) and max(level_errors(fresh, want, cfg["num_layers"])) <= BAR


# ---- the switch on the drop-in module ------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def _raise(*a, **k):
    raise _Reached()


def test_switch_is_off_by_default_and_needs_eval_and_no_grad(monkeypatch):
    from diner_amd import encoder as E
    sd, images, cfg, lat64 = trunk_case("A")
    enc = make_encoder("A")
    x = images.cuda()
    real = E.DeviceTrunk
    monkeypatch.setattr(E, "DeviceTrunk", _raise)
    assert enc.device_trunk is False
    with torch.no_grad():
        enc(x, None, None, None)                                     # default off: never constructed
    torch_route = enc.latent.clone()
    enc.device_trunk = True
    with pytest.raises(_Reached):
        with torch.no_grad():
            enc(x, None, None, None)                                 # on, eval, no grad: taken
    enc(x, None, None, None)                                         # grad mode: the torch route
    assert enc.latent.grad_fn is not None
    enc.train()
    with torch.no_grad():
        enc(x, None, None, None)                                     # train mode: the torch route (batch statistics)
    enc.eval()
    enc.load_state_dict(sd, strict=False)                            # (the train-mode call moved the running statistics)
    monkeypatch.setattr(E, "DeviceTrunk", real)
    enc._scene_cache = {"stale": 1}
    with torch.no_grad():
        enc(x, "d", "s", "n")
    assert isinstance(enc._device_trunk, real) and enc._scene_cache == {} and (enc.depths, enc.depths_std, enc.normals) == ("d", "s", "n")
    assert (enc.nviews, enc.nobjects) == (images.shape[1], images.shape[0])
    lat = enc.latent
    assert lat.shape == torch_route.shape and live_strides(lat) == live_strides(torch_route) and lat.grad_fn is None
    assert max(level_errors(lat, lat64, cfg["num_layers"])) <= BAR and not torch.equal(lat, torch_route)


def test_predict_image_through_both_routes():
    """One predict_image of the 48 x 40 test scene, its source views encoded from images by nerf.encode, on the torch route and on the
    device route: the renders agree to 1e-4 (depth sampling does not read the latent, so no discrete choice can flip), and the scene the
    renderer reads aliases the device route's latent."""
    from diner_amd.render import predict_image
    from diner_amd.synthetic import make_mlp_state_dict, make_scene
    from src.util.import_helper import import_obj
    from tests.test_boundary_cpu import build_nerf
    W, H = 48, 40
    sc = make_scene(W, H, seed=3, latent=False)
    nerf = build_nerf()
    msd = make_mlp_state_dict()
    msd["lin_out.weight"][3].abs_()          # the density row reads a ReLU output: with weights >= 0 it is positive and follows the latent
    nerf.mlp_fine.load_state_dict(msd)       # (on this all-positive latent the plain seeded MLP gives an empty volume, a constant render)
    nerf.encoder.load_state_dict(G().seeded_state_dict("resnet34", 2720, 64, 4), strict=False)
    nerf = nerf.cuda().eval()
    g = torch.Generator().manual_seed(0)
    imgs = torch.rand(1, 4, 3, H, W, generator=g).cuda()
    ren = import_obj("src.models.nerf_renderer.NeRFRendererDGS")(n_samples=64, n_gaussian=24, white_bkgd=False)
    E, K = sc["target_extrinsics"][None].cuda(), sc["target_intrinsics"][None].cuda()
    out = {}
    for route in (False, True):
        nerf.encoder.device_trunk = route
        with torch.no_grad():
            nerf.encode(imgs, sc["depths"][None].cuda(), sc["depths_std"][None].cuda(), sc["src_extrinsics"][None].cuda(),
                        sc["src_intrinsics"][None].cuda())
        lat = nerf.encoder.latent
        assert tuple(lat.shape) == (1, 4, 512, (H + 128) // 2, (W + 128) // 2)
        if route:
            assert nerf.encoder._device_trunk is not None and nerf.hip_scene(0).latent_cl.data_ptr() == lat.data_ptr()
        out[route] = predict_image(nerf, ren, E, K, W, H, sc["znear"], sc["zfar"], ray_batch_size=700, seed=11) + (lat.clone(),)
    d_lat = float((out[True][2] - out[False][2]).abs().max() / out[False][2].abs().max())
    d_rgb = float((out[True][0] - out[False][0]).abs().max())
    d_depth = float((out[True][1] - out[False][1]).abs().max())
    print(f"both routes: latent {d_lat:.2e} of its maximum, rgb {d_rgb:.2e}, depth {d_depth:.2e}")
    assert d_lat > 0 and d_rgb <= 1e-4 and d_depth <= 1e-4
    assert float(out[True][0].std()) > 0.01                          # a render, not a constant
