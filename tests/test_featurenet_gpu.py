"""The kernels behind DeviceFeatureNet on the device against float64 on the host and fixture G31's yardsticks
(tests/golden/g31_featurenet.npz).

Whole cases are held against the float64 torch route (which tests/test_featurenet_cpu.py holds against the fixture) with
featurenet_util.BAR_FACTOR (4) times the case's recorded distance between the reference's float32 and float64, for all stages and all
views, no pixel excluded: the operation is continuous in its offsets.  Each kernel alone is held against a float64 restatement of its own
formula; its bar is 4 x the distance the same restatement in float32 on the CPU keeps from float64 on the same inputs.  The determinism
properties are bit-equalities.

Measured on an MI355X (max |kernel - float64| / bar): see DESIGN.md section 8p."""
import pytest
import torch

from diner_amd import mvs, ops
from tests import featurenet_util as U
from tests import mvs_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _device_module(name_or_seed):
    return U.make_module(name_or_seed).to(DEV)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cases_against_float64(name):
    fx, c = U.fixture(), U.CASES[name]
    net, imgs = _device_module(name), U.case_images(name).to(DEV)
    with torch.no_grad():
        assert net.uses_kernels(imgs[:, 0])
    got, want = U.run_case(net, imgs), U.expected64(name)
    for stage in U.STAGES:
        assert got[stage].shape == want[stage].shape and got[stage].dtype == torch.float32
        e, bar = _err(got[stage], want[stage]), U.BAR_FACTOR * float(fx[f"{name}_err_{stage}"])
        print(f"{name} {stage}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
        assert e <= bar, (name, stage, e, bar)


def _deform_problem(Cout, seed=3120, N=2, hw=(9, 19), Cin=32):
    """x, offmask (channels-last float32), weight, bias; the offsets N(0, 1.5 px) with planted exact cases: tap 0 of every pixel of image 0
    on integers, tap 1 exactly on the line py = -1, tap 2 exactly on px = -1, tap 3 exactly on the last row H - 1, tap 4 exactly on the last
    column W - 1, tap 5 exactly on py = H."""
    g = torch.Generator().manual_seed(seed + Cout)
    H, W = hw
    x = torch.randn(N, H, W, Cin, generator=g)
    om = torch.cat([1.5 * torch.randn(N, H, W, 18, generator=g), 1.2 * torch.randn(N, H, W, 9, generator=g)], -1)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, W)
    om[0, :, :, 0:2] = om[0, :, :, 0:2].round()
    om[0, :, :, 2] = -1.0 - (ys - 1 + 0)                  # tap 1 = (0, 1): py = -1
    om[0, :, :, 5] = -1.0 - (xs - 1 + 2)                  # tap 2 = (0, 2): px = -1
    om[0, :, :, 6] = (H - 1) - (ys - 1 + 1)               # tap 3 = (1, 0): py = H - 1
    om[0, :, :, 9] = (W - 1) - (xs - 1 + 1)               # tap 4 = (1, 1): px = W - 1
    om[0, :, :, 10] = H - (ys - 1 + 1)                    # tap 5 = (1, 2): py = H
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) / (Cin * 9) ** 0.5 * 3
    b = 0.2 * torch.randn(Cout, generator=g)
    return x, om.contiguous(), w, b


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("Cout", [32, 16, 8])
def test_deform_conv3x3_against_float64(Cout, relu):
    x, om, w, b = _deform_problem(Cout)
    want = U.deform_restated(x.double(), om.double(), w.double(), b.double(), relu)
    e32 = _err(U.deform_restated(x, om, w, b, relu), want)
    xd, omd = x.to(DEV), om.to(DEV)
    got = ops.deform_conv3x3(xd, omd, ops.pack_deform_conv3x3(w).to(DEV), b.to(DEV), Cout, relu=relu)
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"deform_conv3x3 32 -> {Cout} relu {relu}: |values| <= {float(want.abs().max()):.2f}, kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == want.shape and e <= bar
    assert torch.equal(xd.cpu(), x) and torch.equal(omd.cpu(), om)            # the inputs stay
    if relu:
        assert float(got.min()) == 0.0


@pytest.mark.parametrize("Cin,Cout", [(32, 32), (8, 40), (64, 3)])
def test_deform_conv3x3_huge_offsets_are_plain_outside(Cin, Cout):
    """Taps whose offsets are +-1e30 add nothing: the exact bits of the same call with those taps' modulation at zero instead."""
    x, om, w, b = _deform_problem(Cout, seed=3130, Cin=Cin)
    far, shut = om.clone(), om.clone()
    for k, (vy, vx) in ((0, (1e30, 0.3)), (4, (-1e30, -1e30)), (7, (0.2, 1e30)), (8, (-1e30, 0.0))):
        far[..., 2 * k], far[..., 2 * k + 1] = vy, vx
        shut[..., 18 + k] = -1e30                                              # sigmoid -> exactly 0
    pack, bd = ops.pack_deform_conv3x3(w).to(DEV), b.to(DEV)
    a = ops.deform_conv3x3(x.to(DEV), far.to(DEV), pack, bd, Cout)
    c = ops.deform_conv3x3(x.to(DEV), shut.to(DEV), pack, bd, Cout)
    assert torch.equal(a, c) and bool(torch.isfinite(a).all())
    want = U.deform_restated(x.double(), far.double(), w.double(), b.double(), False)
    e32 = _err(U.deform_restated(x, far, w, b, False), want)
    assert _err(a, want) <= U.BAR_FACTOR * e32                                 # other channel counts and column tiles on the way


def _conv_case(kernel, stride, padding, Cin, Cout, hw, seed, relu=True, N=2):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, *hw, Cin, generator=g)
    w = (torch.rand(Cout, Cin, kernel, kernel, generator=g) * 2 - 1) / (Cin * kernel * kernel) ** 0.5 * 3
    b = 0.2 * torch.randn(Cout, generator=g)
    want = U.conv_restated(x.double(), w.double(), b.double(), stride, padding, relu)
    return x, w, b, want, _err(U.conv_restated(x, w, b, stride, padding, relu), want)


@pytest.mark.parametrize("Cin,Cout", [(8, 16), (16, 32)])
def test_conv5x5_s2_against_float64(Cin, Cout):
    x, w, b, want, e32 = _conv_case(5, 2, 2, Cin, Cout, (13, 21), 3140 + Cin)
    got = ops.conv5x5_s2(x.to(DEV), ops.pack_conv5x5(w).to(DEV), b.to(DEV), Cout, relu=True)
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"conv5x5_s2 {Cin} -> {Cout}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == want.shape == (2, 7, 11, Cout) and e <= bar
    plain = ops.conv5x5_s2(x.to(DEV), ops.pack_conv5x5(w).to(DEV), None, Cout)
    assert _err(plain, U.conv_restated(x.double(), w.double(), None, 2, 2, False)) <= bar


def test_conv1x1_against_float64():
    x, w, b, want, e32 = _conv_case(1, 1, 0, 32, 32, (9, 19), 3150)
    got = ops.conv1x1(x.to(DEV), ops.pack_conv1x1(w).to(DEV), b.to(DEV), 32, relu=True)
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"conv1x1 32 -> 32: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == want.shape and e <= bar


@pytest.mark.parametrize("Clat", [16, 8])
def test_lateral_against_float64(Clat):
    g = torch.Generator().manual_seed(3160 + Clat)
    top, lat = torch.randn(2, 9, 13, 32, generator=g), torch.randn(2, 18, 26, Clat, generator=g)
    w, b = (torch.rand(32, Clat, 1, 1, generator=g) * 2 - 1) / Clat ** 0.5 * 3, 0.2 * torch.randn(32, generator=g)
    want = U.lateral_restated(top.double(), lat.double(), w.double(), b.double())
    e32 = _err(U.lateral_restated(top, lat, w, b), want)
    topd, latd = top.to(DEV), lat.to(DEV)
    got = ops.fpn_lateral(topd, latd, w.to(DEV), b.to(DEV))
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"fpn_lateral {Clat} -> 32: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == want.shape and e <= bar
    assert torch.equal(topd.cpu(), top) and torch.equal(latd.cpu(), lat)      # the inputs stay


def _views(NV, B=1, hw=(36, 52), seed=3170):
    g = torch.Generator().manual_seed(seed)
    return U.texture(g, B * NV, hw).view(B, NV, 3, *hw).to(DEV)


def test_an_image_does_not_depend_on_its_batch_position():
    net = _device_module("ragged")
    imgs = U.case_images("ragged").to(DEV)                                     # B = 2
    a, b = U.run_case(net, imgs), U.run_case(net, imgs.flip(0))
    for stage in U.STAGES:
        assert torch.equal(a[stage][:, 0], b[stage][:, 1]) and torch.equal(a[stage][:, 1], b[stage][:, 0]), stage


def test_a_view_does_not_depend_on_how_many_are_batched_with_it():
    net = _device_module("ragged")
    imgs = _views(4)
    full = U.run_case(net, imgs)
    for v in (0, 2, 3):
        alone = U.run_case(net, imgs[:, v:v + 1])
        assert all(torch.equal(alone[stage][0], full[stage][v]) for stage in U.STAGES), v


def test_two_runs_give_the_same_bits():
    net = _device_module("tiles")
    imgs = U.case_images("tiles").to(DEV)
    a, b = U.run_case(net, imgs), U.run_case(net, imgs)
    assert all(torch.equal(a[stage], b[stage]) for stage in U.STAGES)


def test_forward_views_is_forward_per_view():
    net = _device_module("ragged")
    imgs = _views(3, B=2)
    keep = imgs.clone()
    with torch.no_grad():
        views = net.forward_views(imgs)
        for v, f in enumerate(views):
            one = net(imgs[:, v].contiguous())
            for stage in U.STAGES:
                assert f[stage].shape == one[stage].shape and torch.equal(f[stage], one[stage]), (v, stage)
                assert f[stage].permute(0, 2, 3, 1).is_contiguous()            # a permuted view of channels-last memory
    assert torch.equal(imgs, keep)


def test_closed_gate_takes_the_torch_route_on_the_device(monkeypatch):
    fx = U.fixture()
    net, imgs = _device_module("tiny"), U.case_images("tiny").to(DEV)

    def no_kernels():
        raise AssertionError("the kernel route was taken")
    monkeypatch.setattr(mvs, "_ops", no_kernels)
    assert not net.uses_kernels(imgs[:, 0])                                    # gradients are enabled here
    got = net(imgs[:, 0])
    with torch.no_grad():
        assert not net.uses_kernels(imgs[:, 0, :, :, :22]) and not net.uses_kernels(imgs[:, 0].double())
        with pytest.raises(AssertionError):
            net(imgs[:, 0])                                                    # the open gate would have reached the kernels
    want = U.expected64("tiny")
    for stage in U.STAGES:
        e, bar = _err(got[stage], want[stage][0]), U.BAR_FACTOR * float(fx[f"tiny_err_{stage}"])
        assert got[stage].requires_grad and e <= bar, (stage, e, bar)


def _clean_footprint(agree, size):
    up = torch.nn.functional.interpolate(agree.float().unsqueeze(1), size, mode="bilinear", align_corners=False).squeeze(1)
    return up == 1.0


def test_depth_from_images_on_the_device():
    """Images in, depth maps out, on the kernels alone, against the float64 run, by tests/test_fmt_gpu.py's rule: the prob volumes within
    the stored bars, and the same winners wherever the top-2 gap rule keeps the pixel; a later stage is compared where the stages before
    it picked float64's plane throughout the pixel's footprint."""
    fx, s = U.fixture(), MU.STAGES
    want = U.stage_run_expected(torch.float64)
    got = U.stage_run(torch.float32, DEV)
    clean = torch.ones(want["stage1"]["depth"].shape, dtype=torch.bool)
    for i, stage in enumerate(U.STAGES):
        err = float(fx[f"run_err_{stage}"])
        diff = (got[stage]["prob_volume"].cpu().double() - want[stage]["prob_volume"]).abs()
        e, bar = float(diff[clean.unsqueeze(1).expand_as(diff)].max()), U.BAR_FACTOR * err
        keep, excluded = MU.excluded_share(want[stage]["prob_volume"], err)
        agree = got[stage]["prob_volume"].cpu().argmax(1) == want[stage]["prob_volume"].argmax(1)
        print(f"{stage}: prob {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}) on {100 * float(clean.double().mean()):.1f} % of the pixels, "
              f"excluded {100 * excluded:.2f} %, winners that differ {int((~agree & clean).sum())}")
        assert e <= bar and bool(agree[keep & clean].all()), stage
        if i + 1 < len(U.STAGES):
            nxt = s["scales"][i + 1]
            full = _clean_footprint(agree & clean, s["image"])
            clean = torch.nn.functional.avg_pool2d(full.float().unsqueeze(1), nxt).squeeze(1) == 1.0 if nxt > 1 else full
    assert got["depth"].is_cuda and got["stage3"]["depth"].shape == (2, 24, 40)
