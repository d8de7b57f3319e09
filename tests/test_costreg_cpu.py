"""The depth estimator's cost regulariser without a GPU: DeviceCostRegNet's torch route against fixture G29 (the reference's own float32
results and the float64 values, tests/golden/g29_costreg.npz, tools/make_golden_costreg.py), and the host logic around the kernels --
the BatchNorm fold, the pack layouts, the state dict, to_device, the gate, the argument checks and the C symbols."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from diner_amd import _lib, build, mvs, ops
from diner_amd.mvs import DeviceCostRegNet
from tests import costreg_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("diner_conv3d_pack_floats", "diner_conv3d_f32", "diner_deconv3d_s2_f32")


def test_symbols_declared_and_loaded():
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.diner_abi_version() == 6 and "#define DINER_ABI_VERSION 6 " in header
    assert f"#define DINER_CONV3D_CIN_CHUNK {ops.CONV3D_CIN_CHUNK}" in header and f"#define DINER_CONV3D_COUT_TILE {ops.CONV3D_COUT_TILE}" in header
    assert "costreg.hip" in build.SOURCES and "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["costreg.hip"]
    for (cin, cout), pad in (((1, 8), 16), ((8, 16), 16), ((16, 17), 32), ((64, 64), 64), ((12, 65), 128)):
        assert lib.diner_conv3d_pack_floats(cin, cout) == -(-cin // 8) * 27 * 8 * pad == ops.pack_conv3d(torch.zeros(cout, cin, 3, 3, 3)).numel()
    assert lib.diner_conv3d_pack_floats(0, 8) == 0 and lib.diner_conv3d_pack_floats(8, 0) == 0 and lib.diner_conv3d_pack_floats(-1, 8) == 0


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)

    def refused(rc, word):
        assert rc == _lib.E_INVALID and word in lib.diner_last_error(), lib.diner_last_error()
    refused(lib.diner_conv3d_f32(p, p, None, None, p, 1, 4, 4, 4, 1, 8, 3, 0, None), b"stride")
    refused(lib.diner_conv3d_f32(p, p, None, None, p, 0, 4, 4, 4, 1, 8, 1, 0, None), b"N, D, H, W, C")
    refused(lib.diner_conv3d_f32(p, p, None, None, p, 1, 4, 0, 4, 1, 8, 2, 0, None), b"N, D, H, W, C")
    refused(lib.diner_conv3d_f32(p, p, None, None, p, 1, 4, 4, 4, 1, 0, 1, 0, None), b"Cout")
    refused(lib.diner_conv3d_f32(p, p, None, None, p, 70000, 4, 4, 4, 1, 8, 1, 0, None), b"65535")
    refused(lib.diner_conv3d_f32(None, p, None, None, p, 1, 4, 4, 4, 1, 8, 1, 0, None), b"null")
    refused(lib.diner_conv3d_f32(p, C.c_void_p(p.value + 4), None, None, p, 1, 4, 4, 4, 1, 8, 1, 0, None), b"aligned")
    refused(lib.diner_deconv3d_s2_f32(p, p, None, None, p, 1, 4, 4, 4, 0, 8, 0, None), b"N, D, H, W, C")
    refused(lib.diner_deconv3d_s2_f32(p, p, None, None, None, 1, 4, 4, 4, 8, 8, 0, None), b"null")
    refused(lib.diner_deconv3d_s2_f32(p, p, None, None, p, 1, 1 << 30, 1, 1, 1, 1, 0, None), b"2^29")


@pytest.mark.parametrize("name", list(U.CASES))
def test_torch_route_against_fixture(name):
    """float32: the reference's own results, bit for bit.  float64: the stored values."""
    fx = U.fixture()
    r32, r64 = U.expected32(name), U.expected64(name)
    base, B, D, H, W = U.CASES[name]["shape"]
    assert r64.shape == r32.shape == (B, 1, D, H, W) and r32.dtype == torch.float32
    assert torch.equal(torch.from_numpy(U.subsample(r32)), torch.from_numpy(fx[f"{name}_cost32"])), name
    assert np.abs(U.subsample(r64) - fx[f"{name}_cost64"]).max() <= 1e-12, name
    err = float((r32.double() - r64).abs().max())
    assert err <= 2.0 * float(fx[f"{name}_err_cost"])                    # the stored yardstick describes this host's float32 too
    assert float(fx[f"{name}_excluded"]) <= U.EXCLUDED_CAP


def test_depthnet_with_the_regulariser_against_fixture():
    fx = U.fixture()
    (r32, _), (r64, _) = U.depthnet_expected(torch.float32), U.depthnet_expected(torch.float64)
    assert torch.equal(torch.from_numpy(U.subsample(r32["prob_volume"])), torch.from_numpy(fx["depthnet_prob32"]))
    assert np.abs(U.subsample(r64["prob_volume"]) - fx["depthnet_prob64"]).max() <= 1e-12
    assert float(fx["depthnet_excluded"]) <= U.EXCLUDED_CAP


def test_fixture_inputs_are_the_generators():
    """The regenerated weights and inputs are the ones the fixture was computed from."""
    import tools.make_golden_mvs as G
    fx = U.fixture()
    for name, c in U.CASES.items():
        sd = U.costreg_state_dict(c["shape"][0], c["seed"] + 50)
        assert str(fx[f"{name}_sha256"]) == G.sha256_of({"x": U.case_input(name), "state_dict": sd}), name
    assert str(fx["depthnet_sha256"]) == G.sha256_of(U.depthnet_inputs())
    assert os.path.getsize(U.FIXTURE) < 120 * 1024


def test_other_parameter_dtypes_stay_off_the_kernels():
    """A module in float64 keeps the gate closed and keeps its dtype through from_module; a float32 input then fails as in the reference."""
    net = U.make_net("one_voxel", torch.float64)
    twin = DeviceCostRegNet.from_module(net)
    assert twin.prob.weight.dtype == torch.float64 and twin.conv0.bn.running_var.dtype == torch.float64

    class OnDevice:
        is_cuda, dtype, shape = True, torch.float32, (1, 1, 8, 8, 8)

        def dim(self):
            return 5
    with torch.no_grad():
        assert not twin.uses_kernels(OnDevice()) and U.make_net("one_voxel").uses_kernels(OnDevice())
        with pytest.raises(RuntimeError):
            twin(U.case_input("one_voxel"))
    ws = U.make_net("one_voxel")
    ws._workspaces[("key",)] = {}
    ws.release_workspace()
    assert ws._workspaces == {}


@pytest.mark.parametrize("transposed", [False, True])
def test_fold_against_numpy(transposed):
    g = torch.Generator().manual_seed(11)
    cin, cout = 5, 7
    w = torch.randn((cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3), generator=g)
    gamma, beta = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g)
    mean, var = torch.randn(cout, generator=g), 0.5 + torch.rand(cout, generator=g)
    wf, bf = mvs.fold_conv_bn(w, gamma, beta, mean, var, transposed)
    s = gamma.numpy().astype(np.float64) / np.sqrt(var.numpy().astype(np.float64) + 1e-5)
    want_w = w.numpy().astype(np.float64) * (s.reshape(1, -1, 1, 1, 1) if transposed else s.reshape(-1, 1, 1, 1, 1))
    want_b = beta.numpy().astype(np.float64) - mean.numpy().astype(np.float64) * s
    assert wf.dtype == bf.dtype == torch.float32
    assert np.array_equal(wf.numpy(), want_w.astype(np.float32)) and np.array_equal(bf.numpy(), want_b.astype(np.float32))


def test_folded_layers_are_the_torch_route():
    """conv + folded bias + ReLU in float64 equals conv, BatchNorm on the running statistics, ReLU: the fold that packed() packs."""
    net = U.make_net("batch", torch.float64)
    x = U.case_input("batch").double()
    with torch.no_grad():
        want = net.conv0(x)
        sd = net.state_dict()
        s = sd["conv0.bn.weight"] / torch.sqrt(sd["conv0.bn.running_var"] + mvs.BN_EPS)
        got = torch.relu(torch.nn.functional.conv3d(x, sd["conv0.conv.weight"] * s.view(-1, 1, 1, 1, 1),
                                                    sd["conv0.bn.bias"] - sd["conv0.bn.running_mean"] * s, padding=1))
    assert float((got - want).abs().max()) <= 1e-13


@pytest.mark.parametrize("cin,cout", [(1, 8), (12, 20), (64, 64), (3, 70)])
def test_pack_layouts(cin, cout):
    g = torch.Generator().manual_seed(cin * 100 + cout)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g)
    wt = torch.randn(cin, cout, 3, 3, 3, generator=g)
    chunks, pad = -(-cin // 8), ops.conv3d_cout_pad(cout)
    assert pad == (16 if cout <= 16 else 32 if cout <= 32 else -(-cout // 64) * 64)
    want, want_t = np.zeros((chunks, 27, 8, pad), np.float32), np.zeros((chunks, 27, 8, pad), np.float32)
    for c in range(cin):
        for kd in range(3):
            for kh in range(3):
                for kw in range(3):
                    want[c // 8, (kd * 3 + kh) * 3 + kw, c % 8, :cout] = w[:, c, kd, kh, kw].numpy()
                    want_t[c // 8, (kd * 3 + kh) * 3 + kw, c % 8, :cout] = wt[c, :, kd, kh, kw].numpy()
    p, pt = ops.pack_conv3d(w), ops.pack_deconv3d(wt)
    assert p.is_contiguous() and pt.is_contiguous() and p.dtype == torch.float32
    assert np.array_equal(p.numpy(), want) and np.array_equal(pt.numpy(), want_t)          # zeros beyond Cin and Cout included


def test_state_dict_round_trip_and_keys():
    sd = U.costreg_state_dict(8, 5)
    net = DeviceCostRegNet(1, 8)
    assert set(net.state_dict()) == set(sd)
    names = ["conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11"]
    want = {f"{n}.{k}" for n in names for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked")}
    assert set(sd) == want | {"prob.weight"}
    net.load_state_dict(sd)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    twin = DeviceCostRegNet.from_module(net.train())
    assert twin.training and twin.base_channels == 8 and twin.in_channels == 1
    assert all(torch.equal(v, sd[k]) for k, v in twin.state_dict().items())
    assert not DeviceCostRegNet.from_module(net.eval()).training
    assert DeviceCostRegNet.from_module(DeviceCostRegNet(3, 4)).in_channels == 3


class _StubDepthNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.pixel_wise_net = mvs._PixelwiseNet()


class _StubModel(nn.Module):
    def __init__(self, shared):
        super().__init__()
        self.DepthNet = _StubDepthNet()
        self.cost_regularization = DeviceCostRegNet(1, 8) if shared else nn.ModuleList([DeviceCostRegNet(1, 8) for _ in range(3)])


@pytest.mark.parametrize("shared", [True, False])
def test_to_device_swaps_both_modules(shared):
    model = _StubModel(shared).eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    old = model.cost_regularization
    out = mvs.to_device(model)
    assert out is model and isinstance(model.DepthNet, mvs.DeviceDepthNet)
    if shared:
        assert isinstance(model.cost_regularization, DeviceCostRegNet) and model.cost_regularization is not old
    else:
        assert isinstance(model.cost_regularization, nn.ModuleList) and len(model.cost_regularization) == 3
        assert all(isinstance(m, DeviceCostRegNet) and m is not o for m, o in zip(model.cost_regularization, old))
    after = model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not model.cost_regularization.training if shared else not model.cost_regularization[0].training


def test_gate_sends_everything_else_to_the_torch_route(monkeypatch):
    """CPU tensors, training mode, enabled gradients and a size that is no multiple of 8 never reach the kernels."""
    net = U.make_net("one_voxel")
    x = U.case_input("one_voxel")

    def no_kernels():
        raise AssertionError("the kernel route was taken")
    monkeypatch.setattr(mvs, "_ops", no_kernels)
    with torch.no_grad():
        assert not net.uses_kernels(x)                                   # a CPU tensor
        assert torch.equal(net(x), U.expected32("one_voxel"))

    class OnDevice:                                                      # what the gate reads of a tensor
        is_cuda, dtype = True, torch.float32

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)
    with torch.no_grad():
        assert net.uses_kernels(OnDevice(1, 1, 8, 16, 24))
        for shape in ((1, 1, 8, 16, 20), (1, 1, 4, 16, 24), (1, 1, 8, 12, 24), (1, 2, 8, 16, 24), (1, 8, 16, 24)):
            assert not net.uses_kernels(OnDevice(*shape)), shape
        net.train()
        assert not net.uses_kernels(OnDevice(1, 1, 8, 16, 24))
        net.eval()
    assert not net.uses_kernels(OnDevice(1, 1, 8, 16, 24))               # gradients are enabled here
    y = net(x.requires_grad_(True))
    y.sum().backward()
    assert x.grad is not None and net.prob.weight.grad is not None       # the torch route is differentiable
    with torch.no_grad(), pytest.raises(RuntimeError):
        net(torch.zeros(1, 1, 8, 8, 12))                                 # fails where the reference fails: the skip additions do not match


def test_training_mode_uses_batch_statistics():
    net = U.make_net("batch")
    x = U.case_input("batch")
    before = net.conv0.bn.running_mean.clone()
    net.train()
    with torch.no_grad():
        y = net(x)
    assert not torch.equal(net.conv0.bn.running_mean, before) and int(net.conv0.bn.num_batches_tracked) == 101
    assert not torch.equal(y, U.expected32("batch"))


def test_wrappers_raise_value_errors():
    x = torch.zeros(1, 4, 4, 4, 8)
    wp, wt = ops.pack_conv3d(torch.zeros(16, 8, 3, 3, 3)), ops.pack_deconv3d(torch.zeros(8, 16, 3, 3, 3))
    b = torch.zeros(16)
    assert ops._check_conv3d_args("conv3d", x, wp, b, 16, 2, None, None) == (1, 4, 4, 4, 8, (1, 2, 2, 2, 16))
    assert ops._check_conv3d_args("conv3d", torch.zeros(1, 3, 5, 4, 8), wp, None, 16, 2, None, None)[5] == (1, 2, 3, 2, 16)
    assert ops._check_conv3d_args("deconv3d_s2", x, wt, b, 16, None, torch.zeros(1, 8, 8, 8, 16), None)[5] == (1, 8, 8, 8, 16)
    bad = (dict(x=torch.zeros(4, 4, 4, 8)), dict(x=x.double()), dict(x=x.permute(0, 1, 2, 4, 3)), dict(x=torch.zeros(1, 4, 4, 4, 9)),
           dict(wp=wp[:, :, :4]), dict(wp=wp.double()), dict(Cout=17), dict(Cout=0), dict(b=torch.zeros(15)), dict(b=b.double()),
           dict(stride=3), dict(addend=torch.zeros(1, 4, 4, 4, 16)), dict(out=torch.zeros(1, 2, 2, 2, 8)), dict(addend=torch.zeros(1, 2, 2, 2, 16).double()))
    for change in bad:
        a = dict(dict(x=x, wp=wp, b=b, Cout=16, stride=2, addend=None, out=None), **change)
        with pytest.raises(ValueError):
            ops._check_conv3d_args("conv3d", a["x"], a["wp"], a["b"], a["Cout"], a["stride"], a["addend"], a["out"])
    with pytest.raises(ValueError):
        ops._check_conv3d_args("deconv3d_s2", x, wt, b, 16, None, torch.zeros(1, 4, 4, 4, 16), None)      # the output is twice the input
    for w in (torch.zeros(8, 8, 3, 3), torch.zeros(8, 8, 3, 3, 1), torch.zeros(8, 8, 3, 3, 3).double(), torch.zeros(0, 8, 3, 3, 3), "w"):
        with pytest.raises(ValueError):
            ops.pack_conv3d(w)
        with pytest.raises(ValueError):
            ops.pack_deconv3d(w)
    for call in (lambda: ops.conv3d(x, wp, b, 16), lambda: ops.deconv3d_s2(x, wt, b, 16)):
        with pytest.raises(RuntimeError):
            call()                                                       # CPU tensors: there is no fallback
