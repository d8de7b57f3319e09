"""The depth estimator's FeatureNet without a GPU: the torch statement of the deformable convolution (mvs.deform_conv2d_torch) against
torch's own convolution, a shifted image, an independent grid_sample statement and gradcheck; the torch route of DeviceFeatureNet against
fixture G31 (tests/golden/g31_featurenet.npz, tools/make_golden_featurenet.py); the host logic around the kernels -- the state dict, the
gate, to_device, the pack layouts, the argument checks and the C symbols; and the host program that drives the kernel's addressing
function under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from diner_amd import _lib, build, mvs, ops
from diner_amd.mvs import DeviceFeatureNet
from tests import featurenet_util as U
from tests import mvs_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("diner_deform_conv3x3_pack_floats", "diner_deform_conv3x3_f32", "diner_conv5x5_s2_pack_floats", "diner_conv5x5_s2_f32",
           "diner_conv1x1_pack_floats", "diner_conv1x1_f32", "diner_fpn_lateral_f32")


def _dcn_problem(seed, B=2, Cin=5, Cout=4, hw=(7, 9), sigma=1.5):
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    off = sigma * torch.randn(B, 18, H, W, generator=g, dtype=torch.float64)
    mask = torch.rand(B, 9, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) / 3
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    return x, off, mask, w, b


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_zero_offsets_and_unit_mask_are_a_convolution():
    x, off, mask, w, b = _dcn_problem(1)
    got = mvs.deform_conv2d_torch(x, torch.zeros_like(off), w, b, 1, 1, 1, mask=torch.ones_like(mask))
    assert float((got - F.conv2d(x, w, b, padding=1)).abs().max()) <= 1e-12
    assert float((mvs.deform_conv2d_torch(x, torch.zeros_like(off), w, b, 1, 1, 1) - F.conv2d(x, w, b, padding=1)).abs().max()) <= 1e-12
    # the general form: stride 2, padding 2, dilation 2 on a 5 x 5 ... of a 3 x 3 kernel
    Ho, Wo = (7 + 4 - 4 - 1) // 2 + 1, (9 + 4 - 4 - 1) // 2 + 1
    zero = torch.zeros(2, 18, Ho, Wo, dtype=torch.float64)
    got = mvs.deform_conv2d_torch(x, zero, w, b, 2, 2, 2)
    assert float((got - F.conv2d(x, w, b, stride=2, padding=2, dilation=2)).abs().max()) <= 1e-12


def test_integer_offsets_are_the_convolution_of_the_shifted_image():
    """With every offset (dy, dx), tap (ky, kx) of pixel (h, w) reads x[h - 1 + ky + dy, w - 1 + kx + dx]: the unpadded convolution of the
    image shifted by (dy, dx) on the domain [-1, H] x [-1, W], zero where the shifted image leaves x."""
    x, off, mask, w, b = _dcn_problem(2)
    B, Cin, H, W = x.shape
    for dy, dx in ((1, 0), (0, -2), (-3, 2), (8, 0), (0, -10)):                # the last two move the whole image out
        o = torch.zeros_like(off)
        o[:, 0::2], o[:, 1::2] = dy, dx
        shifted = torch.zeros(B, Cin, H + 2, W + 2, dtype=x.dtype)            # shifted[i, j] = x[i - 1 + dy, j - 1 + dx]
        for i in range(H + 2):
            for j in range(W + 2):
                if 0 <= i - 1 + dy < H and 0 <= j - 1 + dx < W:
                    shifted[:, :, i, j] = x[:, :, i - 1 + dy, j - 1 + dx]
        got = mvs.deform_conv2d_torch(x, o, w, b, 1, 1, 1)
        assert float((got - F.conv2d(shifted, w, b)).abs().max()) <= 1e-12, (dy, dx)
    assert torch.equal(got, b.view(1, -1, 1, 1).expand_as(got))               # nothing but the bias is left


def test_agrees_with_the_grid_sample_statement():
    for seed, sigma in ((3, 0.4), (4, 1.5), (5, 4.0)):
        x, off, mask, w, b = _dcn_problem(seed, sigma=sigma)
        got = mvs.deform_conv2d_torch(x, off, w, b, 1, 1, 1, mask=mask)
        want = U.deform_conv2d_grid(x, off, w, b, mask)
        assert float((got - want).abs().max()) <= 1e-12, (seed, sigma)


def test_samples_on_the_outer_lines_contribute_exact_zeros():
    """py = -1 and py = H (px likewise) are outside: a tap sent there adds nothing, whatever the image holds -- the result is the bits
    of the same call with that tap's mask at zero."""
    x, off, mask, w, b = _dcn_problem(6)
    H, W = x.shape[2:]
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    for k, (line, axis) in enumerate(((-1.0, 0), (float(H), 0), (-1.0, 1), (float(W), 1), (1e30, 0), (float("inf"), 1), (float("nan"), 0))):
        ky, kx = divmod(k, 3)
        o, m = off.clone(), mask.clone()
        if axis == 0:
            o[:, 2 * k] = line - (ys + ky - 1)
        else:
            o[:, 2 * k + 1] = line - (xs + kx - 1)
        m[:, k] = 0.0
        assert torch.equal(mvs.deform_conv2d_torch(x * 1e6, o, w, b, 1, 1, 1, mask=mask), mvs.deform_conv2d_torch(x * 1e6, off, w, b, 1, 1, 1, mask=m)), k
    # exactly H - 1 is inside: the last row itself, the row below it missing
    o = torch.zeros_like(off)
    o[:, 0::2] = (H - 1) - (ys + (torch.arange(9) // 3 - 1).view(9, 1, 1)).unsqueeze(0)
    last = x[:, :, H - 1:H].expand_as(x)
    want = torch.einsum("ock,bckhw->bohw", w.reshape(4, 5, 9), torch.stack([F.pad(last, (1, 1))[..., kx:kx + W] for kx in (0, 1, 2)] * 3, 2))
    assert float((mvs.deform_conv2d_torch(x, o, w, None, 1, 1, 1) - want).abs().max()) <= 1e-12


def test_gradcheck():
    x, off, mask, w, b = _dcn_problem(7, B=1, Cin=2, Cout=2, hw=(4, 5), sigma=1.2)
    frac = off - off.floor()
    off = off.floor() + 0.2 + 0.6 * frac                                       # away from the integer lines, where the rule has kinks
    args = [t.clone().requires_grad_(True) for t in (x, off, w, b, mask)]
    assert torch.autograd.gradcheck(lambda x, o, w, b, m: mvs.deform_conv2d_torch(x, o, w, b, 1, 1, 1, mask=m), args, eps=1e-6, atol=1e-6)


def test_restatement_refuses_what_it_does_not_state():
    x, off, mask, w, b = _dcn_problem(8)
    with pytest.raises(ValueError, match="one offset group"):
        mvs.deform_conv2d_torch(x, torch.cat([off, off], 1), w, b, 1, 1, 1)
    with pytest.raises(ValueError, match="one weight group"):
        mvs.deform_conv2d_torch(x, off, w[:, :2], b, 1, 1, 1)
    with pytest.raises(ValueError, match="mask"):
        mvs.deform_conv2d_torch(x, off, w, b, 1, 1, 1, mask=mask[:, :8])


# ---- the torch route against G31 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.CASES))
def test_torch_route_against_fixture(name):
    """float32: the reference's own results, bit for bit.  float64: the stored values."""
    fx, c = U.fixture(), U.CASES[name]
    r32, r64 = U.expected32(name), U.expected64(name)
    H, W = c["hw"]
    for i, stage in enumerate(U.STAGES):
        s32, s64 = r32[stage], r64[stage]
        assert s32.shape == s64.shape == (c["NV"], c["B"], U.STAGE_CHANNELS[stage], H >> (2 - i), W >> (2 - i)) and s32.dtype == torch.float32
        assert torch.equal(torch.from_numpy(U.subsample(s32)), torch.from_numpy(fx[f"{name}_{stage}_32"])), (name, stage)
        assert np.abs(U.subsample(s64) - fx[f"{name}_{stage}_64"]).max() <= 1e-12, (name, stage)
        err = float((s32.double() - s64).abs().max())
        assert err <= 2.0 * float(fx[f"{name}_err_{stage}"]), (name, stage, err)     # the stored yardstick describes this host's float32 too


def test_stage_run_against_fixture():
    fx = U.fixture()
    r32, r64 = U.stage_run_expected(torch.float32), U.stage_run_expected(torch.float64)
    for stage in U.STAGES:
        assert torch.equal(torch.from_numpy(U.subsample(r32[stage]["prob_volume"])), torch.from_numpy(fx[f"run_{stage}_prob32"])), stage
        assert np.abs(U.subsample(r64[stage]["prob_volume"]) - fx[f"run_{stage}_prob64"]).max() <= 1e-12, stage
        assert float(fx[f"run_excluded_{stage}"]) < MU.EXCLUDED_CAP
    assert r64["depth"].shape == (2, 24, 40) and r64["stage1"]["depth"].shape == (2, 6, 10)


def test_fixture_inputs_are_the_generators():
    import tools.make_golden_mvs as G
    from tests import fmt_util as FU
    fx = U.fixture()
    for name, c in U.CASES.items():
        assert str(fx[f"{name}_sha256"]) == G.sha256_of({"images": U.case_images(name), "state_dict": U.featurenet_state_dict(c["seed"] + 50)}), name
    inp = MU.stage_inputs()
    assert str(fx["run_sha256"]) == G.sha256_of({"images": U.stage_run_images(), "inputs": {k: inp[k] for k in ("proj", "depth_values", "state_dict")},
                                                 "feature": U.featurenet_state_dict(U.STAGE_RUN_SEED),
                                                 "fmt": FU.fmt_state_dict(U.STAGE_RUN_SEED + 1)})
    assert os.path.getsize(U.FIXTURE) < 120 * 1024


def test_seeded_weights_hide_nothing():
    sd = U.featurenet_state_dict(7)
    for k, v in sd.items():
        if v.dim() >= 1:
            assert float(v.abs().max()) > 0 and float(v.std()) > 0.02, k      # no default BatchNorm, no zero bias, no zero offset convolution
    assert all(float(v.min()) >= 0.1 for k, v in sd.items() if k.endswith("running_var"))
    net = U.make_module("tiny")
    for layer, (x, om) in U.dcn_inputs(net, U.case_images("tiny").flatten(0, 1)).items():
        cov = U.sample_coverage(om, *x.shape[2:])
        assert all(v > 0 for v in cov.values()), (layer, cov)                  # every branch of the sampling rule, even on the smallest case


# ---- host checks ------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_round_trip():
    fx = U.fixture()
    net = DeviceFeatureNet(8)
    keys = list(net.state_dict().keys())
    assert keys == [str(k) for k in fx["keys"]]
    assert "out1.1.conv_offset_mask.weight" in keys and "out3.7.bias" in keys and "out2.5.running_var" in keys and "inner2.bias" in keys
    assert tuple(net.out3[7].weight.shape) == (8, 32, 3, 3) and tuple(net.out1[1].conv_offset_mask.weight.shape) == (27, 32, 3, 3)
    assert tuple(net.conv1[0].conv.weight.shape) == (16, 8, 5, 5) and tuple(net.out1[0].conv.weight.shape) == (32, 32, 1, 1)
    assert float(net.out2[4].conv_offset_mask.weight.detach().abs().max()) == 0.0      # the reference's own initialisation
    sd = U.featurenet_state_dict(5)
    net.load_state_dict(sd)
    new = DeviceFeatureNet.from_module(net.double().train())
    assert new.training and new.inner1.weight.dtype == torch.float64
    assert all(torch.equal(v, new.state_dict()[k]) for k, v in net.state_dict().items())


class _Stub(nn.Module):
    def __init__(self, with_feature):
        super().__init__()
        self.DepthNet = mvs.DeviceDepthNet()
        self.cost_regularization = mvs.DeviceCostRegNet(1, 8)
        if with_feature:
            self.feature = DeviceFeatureNet(8)


def test_to_device_swaps_the_feature_net_when_there_is_one():
    m = _Stub(True).eval()
    m.feature.load_state_dict(U.featurenet_state_dict(9))
    before = m.feature
    out = mvs.to_device(m)
    assert out is m and isinstance(m.feature, DeviceFeatureNet) and m.feature is not before and not m.feature.training
    assert all(torch.equal(v, m.feature.state_dict()[k]) for k, v in before.state_dict().items())
    assert not hasattr(mvs.to_device(_Stub(False)), "feature")


class _DeviceTensor:
    """What the gate asks of its argument, for a tensor that claims to live on the device (there is none here)."""

    def __init__(self, shape, dtype=torch.float32):
        self.is_cuda, self.dtype, self.shape = True, dtype, tuple(shape)

    def dim(self):
        return len(self.shape)


def test_gate():
    net = U.make_module("tiny")
    x = U.case_images("tiny")[:, 0]
    with torch.no_grad():
        assert not net.uses_kernels(x)                                         # a CPU tensor
        out = net(x)
        assert set(out) == set(U.STAGES) and out["stage3"].shape == (1, 8, 16, 24) and out["stage1"].is_contiguous()
        assert net.uses_kernels(_DeviceTensor((1, 3, 16, 24)))
        for shape in ((1, 3, 18, 24), (1, 3, 16, 26), (1, 3, 2, 24), (1, 4, 16, 24), (3, 16, 24)):
            assert not net.uses_kernels(_DeviceTensor(shape)), shape          # H or W no multiple of 4, not an image batch
        assert not net.uses_kernels(_DeviceTensor((1, 3, 16, 24), torch.float64))
        assert not net.train().uses_kernels(_DeviceTensor((1, 3, 16, 24)))
        assert net.eval().uses_kernels(_DeviceTensor((1, 3, 16, 24)))
        assert not U.make_module("tiny", torch.float64).uses_kernels(_DeviceTensor((1, 3, 16, 24)))          # float64 parameters
        wide = DeviceFeatureNet(16).eval()
        assert not wide.uses_kernels(_DeviceTensor((1, 3, 16, 24))) and wide(x)["stage1"].shape == (1, 64, 4, 6)      # base 16: torch
    assert not net.uses_kernels(_DeviceTensor((1, 3, 16, 24)))                 # gradients enabled


def test_closed_gate_runs_torch_in_training_and_with_gradients():
    net = U.make_module("tiny")
    x = U.case_images("tiny")[:, 0]
    out = net(x)
    assert out["stage2"].requires_grad
    out["stage2"].sum().backward()
    assert net.out2[1].conv_offset_mask.weight.grad is not None and float(net.out2[1].conv_offset_mask.weight.grad.abs().max()) > 0
    odd = torch.rand(1, 3, 16, 22)                                             # W = 22: the reference's own upsample-and-add fails
    with torch.no_grad(), pytest.raises(RuntimeError):
        net(odd)
    views = net.forward_views(U.case_images("ragged"))
    assert len(views) == 2 and views[1]["stage1"].shape == (2, 32, 9, 13)
    with pytest.raises(ValueError, match="forward_views"):
        net.forward_views(x)


def test_pack_layouts_against_numpy():
    g = torch.Generator().manual_seed(11)
    for Cout, Cin in ((32, 32), (16, 32), (8, 32), (40, 8), (1, 64)):
        w = torch.randn(Cout, Cin, 3, 3, generator=g)
        p = ops.pack_deform_conv3x3(w).numpy()
        bn = 16 if Cout <= 16 else 32
        tiles = -(-Cout // bn)
        assert p.shape == (tiles, 9, Cin, bn) and p.size == _lib.load().diner_deform_conv3x3_pack_floats(Cin, Cout)
        want = np.zeros((tiles, 9, Cin, bn), np.float32)
        for o in range(Cout):
            for k in range(9):
                want[o // bn, k, :, o % bn] = w[o, :, k // 3, k % 3].numpy()
        assert np.array_equal(p, want), (Cout, Cin)
    for R, pack, floats in ((5, ops.pack_conv5x5, "diner_conv5x5_s2_pack_floats"), (1, ops.pack_conv1x1, "diner_conv1x1_pack_floats")):
        for Cout, Cin in ((16, 8), (32, 16), (70, 11)):
            w = torch.randn(Cout, Cin, R, R, generator=g)
            p = pack(w).numpy()
            cp, op = -(-Cin // 8), -(-Cout // 64) * 64
            assert p.shape == (cp, R * R, 8, op) and p.size == getattr(_lib.load(), floats)(Cin, Cout)
            want = np.zeros((cp, R * R, 8, op), np.float32)
            for c in range(Cin):
                want[c // 8, :, c % 8, :Cout] = w[:, c].reshape(Cout, R * R).numpy().T
            assert np.array_equal(p, want), (R, Cout, Cin)
    lib = _lib.load()
    for bad in ((0, 8), (12, 8), (72, 8), (32, 0), (-8, 8)):
        assert lib.diner_deform_conv3x3_pack_floats(*bad) == 0, bad
    assert lib.diner_conv5x5_s2_pack_floats(0, 8) == 0 and lib.diner_conv1x1_pack_floats(8, 0) == 0
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.pack_deform_conv3x3(torch.zeros(8, 12, 3, 3))
    with pytest.raises(ValueError, match="3,3"):
        ops.pack_deform_conv3x3(torch.zeros(8, 16, 5, 5))


def test_packed_folds_batchnorm():
    """The kernel route's folded weights evaluate, in float64 torch, to the module's own torch route."""
    net = U.make_module("tiny")
    P = net.packed()
    assert P is net.packed()                                                   # cached
    with torch.no_grad():
        net.out2[2].running_mean += 0.5                                        # an in-place write bumps the version: packed again
    assert net.packed() is not P
    P = net.packed()
    sd = net.state_dict()
    s = sd["out2.2.weight"].double() / torch.sqrt(sd["out2.2.running_var"].double() + 1e-5)
    w = (sd["out2.1.weight"].double() * s.view(-1, 1, 1, 1)).float()
    b = ((sd["out2.1.bias"].double() - sd["out2.2.running_mean"].double()) * s + sd["out2.2.bias"].double()).float()
    assert torch.equal(P["out2.1"][0], ops.pack_deform_conv3x3(w)) and torch.equal(P["out2.1"][1], b)
    assert torch.equal(P["out3.7"][1], sd["out3.7.bias"]) and P["out3.7"][0].shape == (1, 9, 32, 16)
    assert P["conv0.0"][0].shape == (1, 9, 8, 64) and float(P["conv0.0"][0][0, :, 3:].abs().max()) == 0.0       # Cin 3 packed for 4: zeros beyond
    assert P["out1.4.offset"][0].shape == (4, 9, 8, 64) and P["out1.4.offset"][1].shape == (64,)
    assert P["conv1.0"][0].shape == (1, 25, 8, 64) and P["out1.0"][0].shape == (4, 1, 8, 64) and P["inner2"][0].shape == (32, 8, 1, 1)
    net.invalidate()
    assert net.packed() is not P


def test_symbols_declared_and_loaded():
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.diner_abi_version() == 6 and "#define DINER_ABI_VERSION 6 " in header
    assert f"#define DINER_DEFORM_MAX_CIN {ops.DEFORM_MAX_CIN}\n" in header
    assert "deform.hip" in build.SOURCES and "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["deform.hip"]
    assert ops.CONV_S2_KERNELS == (1, 3, 7) and lib.diner_conv2d_s2_pack_floats(8, 16, 5) == 0       # conv_s2 keeps refusing R = 5


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    q = C.c_void_p(p.value + 64)
    off = C.c_void_p(p.value + 4)

    def refused(rc, word):
        assert rc == _lib.E_INVALID and word in lib.diner_last_error(), lib.diner_last_error()
    dc = lib.diner_deform_conv3x3_f32
    refused(dc(p, p, p, p, q, 1, 4, 4, 12, 8, 0, None), b"multiple of 8")
    refused(dc(p, p, p, p, q, 1, 4, 4, 72, 8, 0, None), b"multiple of 8")
    refused(dc(p, p, p, p, q, 1, 4, 4, 0, 8, 0, None), b"N, H, W, C")
    refused(dc(p, p, p, p, q, 1, 4, 4, 32, 0, 0, None), b"Cout")
    refused(dc(p, p, p, p, q, 0, 4, 4, 32, 8, 0, None), b"N, H, W, C")
    refused(dc(p, p, p, p, q, 70000, 4, 4, 32, 8, 0, None), b"65535")
    refused(dc(p, p, p, p, q, 1, (1 << 14) + 1, 1, 32, 8, 0, None), b"2^14")
    refused(dc(None, p, p, p, q, 1, 4, 4, 32, 8, 0, None), b"null")
    refused(dc(p, None, p, p, q, 1, 4, 4, 32, 8, 0, None), b"null")
    refused(dc(p, p, p, p, None, 1, 4, 4, 32, 8, 0, None), b"null")
    refused(dc(off, p, p, p, q, 1, 4, 4, 32, 8, 0, None), b"aligned")
    refused(dc(p, p, off, p, q, 1, 4, 4, 32, 8, 0, None), b"aligned")
    refused(dc(p, C.c_void_p(p.value + 2), p, p, q, 1, 4, 4, 32, 8, 0, None), b"aligned")
    refused(dc(p, q, p, p, p, 1, 4, 4, 32, 8, 0, None), b"must not be")
    for fn, who in ((lib.diner_conv5x5_s2_f32, b"conv5x5_s2"), (lib.diner_conv1x1_f32, b"conv1x1")):
        refused(fn(p, p, p, q, 1, 4, 4, 0, 8, 0, None), who)
        refused(fn(p, p, p, q, 1, 4, 4, 8, 0, 0, None), who)
        refused(fn(p, p, p, q, 70000, 4, 4, 8, 8, 0, None), b"65535")
        refused(fn(None, p, p, q, 1, 4, 4, 8, 8, 0, None), b"null")
        refused(fn(p, off, p, q, 1, 4, 4, 8, 8, 0, None), b"aligned")
    assert lib.diner_conv2d_s2_f32(p, p, p, q, 1, 4, 4, 8, 8, 5, 0, 8, 0, None) == _lib.E_UNSUPPORTED          # R = 5 stays refused there
    fl = lib.diner_fpn_lateral_f32
    refused(fl(p, p, p, p, q, 1, 5, 4, 32, 8, None), b"even")
    refused(fl(p, p, p, p, q, 1, 4, 6 + (1 << 15), 32, 8, None), b"even")
    refused(fl(p, p, p, p, q, 1, 4, 4, 30, 8, None), b"Ctop")
    refused(fl(p, p, p, p, q, 1, 4, 4, 68, 8, None), b"Ctop")
    refused(fl(p, p, p, p, q, 1, 4, 4, 32, 65, None), b"Clat")
    refused(fl(p, p, p, p, q, 1, 4, 4, 32, 0, None), b"N, H, W, C")
    refused(fl(p, None, p, p, q, 1, 4, 4, 32, 8, None), b"null")
    refused(fl(off, p, p, p, q, 1, 4, 4, 32, 8, None), b"aligned")
    refused(fl(p, p, p, p, p, 1, 4, 4, 32, 8, None), b"must not be")


def test_wrappers_refuse_bad_arguments():
    x, om = torch.zeros(1, 4, 4, 32), torch.zeros(1, 4, 4, 27)
    wp = ops.pack_deform_conv3x3(torch.zeros(8, 32, 3, 3))
    for args, word in (((x[..., :12].contiguous(), om, wp, None, 8), "multiple of 8"), ((x, om[..., :26].contiguous(), wp, None, 8), "offmask"),
                       ((x, om, wp, None, 17), "wpack"), ((x, om, wp, torch.zeros(4), 8), "bias"), ((x.double(), om, wp, None, 8), "float32"),
                       ((x.permute(0, 2, 1, 3), om, wp, None, 8), "contiguous"), ((x, om, wp, None, 0), "Cout")):
        with pytest.raises(ValueError, match=word):
            ops._check_deform_conv3x3_args(*args)
    with pytest.raises(ValueError, match="must not be"):
        ops._check_deform_conv3x3_args(x, om, ops.pack_deform_conv3x3(torch.zeros(27, 32, 3, 3)), None, 27, out=om)
    with pytest.raises(RuntimeError):
        ops.deform_conv3x3(x, om, wp, None, 8)                                 # CPU tensors: no fall-back
    x8 = torch.zeros(1, 5, 7, 8)
    assert ops._check_conv_fixed_args("conv5x5", x8, ops.pack_conv5x5(torch.zeros(16, 8, 5, 5)), None, 16, 5, 2) == (1, 5, 7, 8, 3, 4)
    with pytest.raises(ValueError, match="wpack"):
        ops._check_conv_fixed_args("conv5x5", x8, ops.pack_conv1x1(torch.zeros(16, 8, 1, 1)), None, 16, 5, 2)
    with pytest.raises(ValueError, match="out"):
        ops._check_conv_fixed_args("conv1x1", x8, ops.pack_conv1x1(torch.zeros(16, 8, 1, 1)), None, 16, 1, 1, out=torch.zeros(1, 5, 7, 8))
    with pytest.raises(NotImplementedError):
        ops._check_conv_s2_args(x8, ops.pack_conv5x5(torch.zeros(16, 8, 5, 5)), None, 16, 5, None, 0)     # conv_s2 keeps refusing R = 5
    top, lat, w = torch.zeros(1, 2, 3, 32), torch.zeros(1, 4, 6, 8), torch.zeros(32, 8, 1, 1)
    assert ops._check_fpn_lateral_args(top, lat, w, torch.zeros(32)) == (1, 4, 6, 32, 8)
    for args, word in (((top, torch.zeros(1, 5, 6, 8), w, None), "even"), ((top, lat, torch.zeros(32, 16, 1, 1), None), "weight"),
                       ((torch.zeros(1, 2, 3, 16), lat, w, None), "top"), ((top, lat, w, torch.zeros(8)), "bias"),
                       ((top, lat, torch.zeros(30, 8), None), "multiple of 4")):
        with pytest.raises(ValueError, match=word):
            ops._check_fpn_lateral_args(*args)


# ---- the host program around the addressing function ------------------------------------------------------------------------------------------
def test_addressing_function_under_the_sanitizers(tmp_path):
    """tools/deform_geom_check.cpp, built for the host with AddressSanitizer, UBSan and the float-cast-overflow check, run as a program of
    its own (nothing is loaded into this process): adversarial offsets never yield a valid index outside the image."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) to build tools/deform_geom_check.cpp with")
    exe = str(tmp_path / "deform_geom_check")
    # the sanitizer runtimes linked statically, so that the program needs nothing preloaded: gcc's spelling, then clang's
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                                *static, os.path.join(ROOT, "tools", "deform_geom_check.cpp"), "-o", exe], capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "every valid index in range" in run.stdout, run.stdout + run.stderr
