"""The depth estimator's feature transformer without a GPU: the torch route of DeviceFMT / DeviceFMTWithPathway against fixture G30 (the
reference's own float32 results and the float64 values, tests/golden/g30_fmt.npz, tools/make_golden_fmt.py), and the host logic around
the kernels -- the state dict, the gate, to_device, the pack layout, the argument checks and the C symbols."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from diner_amd import _lib, build, mvs, ops
from diner_amd.mvs import DeviceFMT, DeviceFMTWithPathway
from tests import fmt_util as U
from tests import mvs_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("diner_fmt_pack_floats", "diner_fmt_kv_blocks", "diner_fmt_tokenise_f32", "diner_fmt_kv_f32", "diner_fmt_layer_f32",
           "diner_fpn_merge_f32")


def test_symbols_declared_and_loaded():
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.diner_abi_version() == 6 and "#define DINER_ABI_VERSION 6 " in header
    for macro, value in (("D_MODEL", ops.FMT_D_MODEL), ("NHEAD", ops.FMT_NHEAD), ("D_FF", ops.FMT_D_FF), ("MAX_HW", ops.FMT_MAX_HW),
                         ("STATE_FLOATS", ops.FMT_STATE_FLOATS), ("KV_TOKENS", ops.FMT_KV_TOKENS), ("PACK_FLOATS", ops.FMT_PACK_FLOATS)):
        assert f"#define DINER_FMT_{macro} {value}\n" in header, macro
    assert f"#define DINER_FPN_MAX_CHANNELS {ops.FPN_MAX_CHANNELS}\n" in header
    assert "fmt.hip" in build.SOURCES and "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["fmt.hip"]
    assert lib.diner_fmt_pack_floats() == ops.FMT_PACK_FLOATS == 4 * 32 * 32 + 2 * 32 * 64 + 9 * 32 + 64
    assert U.KV_TOKENS == ops.FMT_KV_TOKENS
    for L in (1, 35, 512, 513, 851, 2080, 20480):
        assert lib.diner_fmt_kv_blocks(L) == ops.fmt_kv_blocks(L) == -(-L // 512)
    assert lib.diner_fmt_kv_blocks(0) == 0 and lib.diner_fmt_kv_blocks(-3) == 0


def test_entries_refuse_bad_arguments_before_any_device_work():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    off = C.c_void_p(p.value + 4)

    def refused(rc, word):
        assert rc == _lib.E_INVALID and word in lib.diner_last_error(), lib.diner_last_error()
    refused(lib.diner_fmt_tokenise_f32(p, p, p, 1, 16, 4, 4, 600, 600, None), b"d_model")
    refused(lib.diner_fmt_tokenise_f32(p, p, p, 1, 32, 601, 4, 600, 600, None), b"H, W")
    refused(lib.diner_fmt_tokenise_f32(p, p, p, 1, 32, 4, 0, 600, 600, None), b"H, W")
    refused(lib.diner_fmt_tokenise_f32(p, p, p, 1, 32, 8, 8, 4, 600, None), b"positional")
    refused(lib.diner_fmt_tokenise_f32(p, p, p, 0, 32, 4, 4, 600, 600, None), b"N = 0")
    refused(lib.diner_fmt_tokenise_f32(p, None, p, 1, 32, 4, 4, 600, 600, None), b"null")
    refused(lib.diner_fmt_kv_f32(p, p, p, p, 70000, 8, None), b"65535")
    refused(lib.diner_fmt_kv_f32(p, p, p, p, 1, 0, None), b"L = 0")
    refused(lib.diner_fmt_kv_f32(p, p, p, p, 1, 360001, None), b"L = 360001")
    refused(lib.diner_fmt_kv_f32(p, p, None, p, 1, 8, None), b"null")
    refused(lib.diner_fmt_kv_f32(p, off, p, p, 1, 8, None), b"aligned")
    refused(lib.diner_fmt_layer_f32(p, p, p, p, 4, 8, 3, None), b"state_rows")
    refused(lib.diner_fmt_layer_f32(p, p, p, p, 4, 8, 0, None), b"state_rows")
    refused(lib.diner_fmt_layer_f32(p, p, None, p, 4, 8, 2, None), b"null")
    refused(lib.diner_fmt_layer_f32(off, p, p, p, 4, 8, 2, None), b"aligned")
    refused(lib.diner_fpn_merge_f32(p, p, p, p, p, 1, 4, 4, 32, 6, None), b"Clat")
    refused(lib.diner_fpn_merge_f32(p, p, p, p, p, 1, 4, 4, 65, 8, None), b"Ctop")
    refused(lib.diner_fpn_merge_f32(p, p, p, p, p, 1, 0, 4, 32, 8, None), b"N, H, W, C")
    refused(lib.diner_fpn_merge_f32(p, p, p, p, p, 1, 1 << 15, 1, 4, 4, None), b"2^14")
    refused(lib.diner_fpn_merge_f32(p, p, p, None, p, 1, 4, 4, 32, 8, None), b"null")
    refused(lib.diner_fpn_merge_f32(p, p, off, p, p, 1, 4, 4, 32, 8, None), b"aligned")


@pytest.mark.parametrize("name", list(U.CASES))
def test_torch_route_against_fixture(name):
    """float32: the reference's own results, bit for bit.  float64: the stored values."""
    fx = U.fixture()
    c = U.CASES[name]
    r32, r64 = U.expected32(name), U.expected64(name)
    B, (H, W) = c["B"], c["hw"]
    for i, stage in enumerate(U.case_stages(name)):
        s32, s64 = U.stacked(r32[stage]), U.stacked(r64[stage])
        assert s32.shape == s64.shape == (c["NV"], B, U.STAGE_CHANNELS[stage], H << i, W << i) and s32.dtype == torch.float32
        assert torch.equal(torch.from_numpy(U.subsample(s32)), torch.from_numpy(fx[f"{name}_{stage}_32"])), (name, stage)
        assert np.abs(U.subsample(s64) - fx[f"{name}_{stage}_64"]).max() <= 1e-12, (name, stage)
        err = float((s32.double() - s64).abs().max())
        assert err <= 2.0 * float(fx[f"{name}_err_{stage}"])                 # the stored yardstick describes this host's float32 too
    assert (f"{name}_stage2_64" in fx) == c["pathway"]


def test_stage_run_against_fixture():
    fx = U.fixture()
    r32, r64 = U.stage_run_expected(torch.float32), U.stage_run_expected(torch.float64)
    for stage in U.STAGES:
        assert torch.equal(torch.from_numpy(U.subsample(r32[stage]["prob_volume"])), torch.from_numpy(fx[f"run_{stage}_prob32"])), stage
        assert np.abs(U.subsample(r64[stage]["prob_volume"]) - fx[f"run_{stage}_prob64"]).max() <= 1e-12, stage
        assert float(fx[f"run_excluded_{stage}"]) <= MU.EXCLUDED_CAP


def test_fixture_inputs_are_the_generators():
    """The regenerated weights and inputs are the ones the fixture was computed from."""
    import tools.make_golden_mvs as G
    fx = U.fixture()
    for name, c in U.CASES.items():
        assert str(fx[f"{name}_sha256"]) == G.sha256_of({"features": U.case_features(name), "state_dict": U.fmt_state_dict(c["seed"] + 50)}), name
    inp = MU.stage_inputs()
    assert str(fx["run_sha256"]) == G.sha256_of({"inputs": {k: inp[k] for k in ("features", "proj", "depth_values", "state_dict")},
                                                 "state_dict": U.fmt_state_dict(U.STAGE_RUN_SEED)})
    assert os.path.getsize(U.FIXTURE) < 120 * 1024
    L = U.CASES["blocks"]["hw"][0] * U.CASES["blocks"]["hw"][1]
    assert ops.fmt_kv_blocks(L) >= 3 and L % ops.FMT_KV_TOKENS != 0        # three partial blocks or more, the last partly filled


def test_seeded_weights_hide_nothing():
    sd = U.fmt_state_dict(7)
    for k, v in sd.items():
        if v.dim() == 1:
            assert float(v.abs().min()) > 0 and float(v.std()) > 0.05, k      # no default LayerNorm, no zero bias
    assert all(0.5 <= float(v.min()) and float(v.max()) <= 1.5 for k, v in sd.items() if ".norm" in k and k.endswith(".weight"))


def test_state_dict_keys_and_round_trip():
    sd = U.fmt_state_dict(5)
    net = DeviceFMTWithPathway(8)
    keys = set(net.state_dict())
    layer = [f"attention.{p}_projection.{t}" for p in ("query", "key", "value", "out") for t in ("weight", "bias")] + \
            [f"{m}.{t}" for m in ("linear1", "linear2", "norm1", "norm2") for t in ("weight", "bias")]
    want = {f"FMT.layers.{i}.{k}" for i in range(8) for k in layer} | {"dim_reduction_1.weight", "dim_reduction_2.weight", "smooth_1.weight",
                                                                       "smooth_2.weight"}
    assert len(want) == 132 and keys == want == set(sd) and not any("pe" in k.split(".") for k in keys)
    assert "pe" in dict(net.FMT.named_buffers()) and tuple(net.FMT.pe.shape) == (1, 32, 600, 600)
    net.load_state_dict(dict(sd))                                        # from a plain dict
    plain = dict(net.state_dict())                                       # and into one
    assert all(torch.equal(plain[k], sd[k]) for k in sd)
    twin = DeviceFMTWithPathway.from_module(net.train())
    assert twin.training and twin.FMT.training and all(torch.equal(v, sd[k]) for k, v in twin.state_dict().items())
    assert not DeviceFMTWithPathway.from_module(net.eval()).training
    assert DeviceFMTWithPathway.from_module(net.double()).smooth_1.weight.dtype == torch.float64
    fmt = DeviceFMT.from_module(U.make_module(5).FMT)
    assert set(fmt.state_dict()) == {k[4:] for k in want if k.startswith("FMT.")} and fmt.layer_names == ["self", "cross"] * 4


def test_position_encoding_formula():
    """The buffer against a float64 numpy statement of the formula, and the crop the torch route adds."""
    pe = mvs.sine_position_encoding(32, (9, 13)).numpy()
    ys, xs = np.meshgrid(np.arange(1, 10, dtype=np.float64), np.arange(1, 14, dtype=np.float64), indexing="ij")
    for i in range(8):
        f = np.exp(-2.0 * i * np.log(10000.0) / 16.0)
        for j, want in enumerate((np.sin(xs * f), np.cos(xs * f), np.sin(ys * f), np.cos(ys * f))):
            assert np.abs(pe[4 * i + j] - want).max() < 1e-5, (i, j)
    net = U.make_module(5)
    assert torch.equal(net.FMT.pe[0, :, :9, :13], torch.from_numpy(pe))
    x = torch.zeros(1, 32, 3, 4)
    assert torch.equal(net.FMT.pos_encoding(x)[0], net.FMT.pe[0, :, :3, :4])


class _OnDevice:                                                         # what the gate reads of a tensor
    is_cuda = True

    def __init__(self, *shape, dtype=torch.float32, is_cuda=True):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, is_cuda

    def dim(self):
        return len(self.shape)


def _features(B=1, H=6, W=10, NV=3, s2=2, s3=4, **kw):
    return [{"stage1": _OnDevice(B, 32, H, W, **kw), "stage2": _OnDevice(B, 16, s2 * H, s2 * W, **kw), "stage3": _OnDevice(B, 8, s3 * H, s3 * W, **kw)}
            for _ in range(NV)]


def test_gate_truth_table():
    net = U.make_module(5)
    with torch.no_grad():
        assert net.uses_kernels(_features()) and net.FMT.uses_kernels(_OnDevice(1, 32, 600, 600))
        assert not net.uses_kernels(_features(is_cuda=False))                                    # CPU tensors
        assert not net.uses_kernels(_features(dtype=torch.float64))
        assert not net.uses_kernels(_features(s2=3))                                             # a 3 x stage 2
        assert not net.uses_kernels(_features(s3=2))
        assert not net.uses_kernels(_features(H=601)) and not net.uses_kernels(_features(W=601))
        assert not net.FMT.uses_kernels(_OnDevice(1, 32, 601, 4)) and not net.FMT.uses_kernels(_OnDevice(1, 16, 4, 4))
        odd = _features()
        odd[2]["stage1"] = _OnDevice(1, 32, 6, 11)                                               # a view of another shape
        assert not net.uses_kernels(odd) and not net.uses_kernels([])
        net.train()
        assert not net.uses_kernels(_features())                                                 # training mode
        net.eval()
        assert not U.make_module(5, torch.float64).uses_kernels(_features())                     # double parameters
        other = DeviceFMTWithPathway(8, {"d_model": 32, "nhead": 8, "layer_names": ["self", "cross"] * 3}).eval()
        assert not other.uses_kernels(_features())                                               # another layer schedule
        assert not DeviceFMTWithPathway(8, {"d_model": 32, "nhead": 4, "layer_names": ["self", "cross"] * 4}).eval().uses_kernels(_features())
    assert not net.uses_kernels(_features())                                                     # gradients are enabled here


def test_closed_gate_runs_the_torch_route(monkeypatch):
    """CPU tensors never reach the kernels, the route is differentiable, and it fails where the reference fails."""
    net = U.make_module("tiny")

    def no_kernels():
        raise AssertionError("the kernel route was taken")
    monkeypatch.setattr(mvs, "_ops", no_kernels)
    feats = U.case_features("tiny")
    with torch.no_grad():
        out = net([dict(f) for f in feats])
    want = U.expected32("tiny")
    assert all(torch.equal(out[v][k], want[k][v]) for v in range(2) for k in U.STAGES)
    assert out[0]["stage1"].shape == (1, 32, 5, 7) and out[1]["stage3"].shape == (1, 8, 20, 28)
    x = [dict(f) for f in feats]
    leaf = x[1]["stage1"] = x[1]["stage1"].clone().requires_grad_(True)
    y = net(x)                                                           # rewrites the dicts in place, as the reference does
    assert y is x and y[1]["stage1"] is not leaf
    sum(f[k].sum() for f in y for k in U.STAGES).backward()
    assert leaf.grad is not None and net.FMT.layers[7].linear2.weight.grad is not None and net.smooth_2.weight.grad is not None
    odd = [dict(f) for f in feats]
    odd[1]["stage2"] = torch.zeros(1, 16, 15, 21)                        # a 3 x stage 2 is resized by the torch route, as in the reference
    odd[1]["stage3"] = torch.zeros(1, 8, 30, 42)
    with torch.no_grad():
        assert net(odd)[1]["stage2"].shape == (1, 16, 15, 21)
        bad = [dict(f) for f in feats]
        bad[0]["stage1"] = torch.zeros(1, 16, 5, 7)
        with pytest.raises((AssertionError, RuntimeError)):
            net(bad)                                                     # d_model mismatch: the reference asserts
        with pytest.raises(ValueError):
            net.FMT(feats[0]["stage1"], feat="other")
    partial = DeviceFMT({"d_model": 32, "nhead": 8, "layer_names": ["self", "cross", "self"]}).eval()
    with torch.no_grad():
        assert len(partial(torch.zeros(1, 32, 3, 4), feat="ref")) == 2


class _StubDepthNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.pixel_wise_net = mvs._PixelwiseNet()


class _StubModel(nn.Module):
    def __init__(self, with_fmt):
        super().__init__()
        self.DepthNet = _StubDepthNet()
        self.cost_regularization = mvs.DeviceCostRegNet(1, 8)
        if with_fmt:
            self.FMT_with_pathway = nn.Module()                          # a foreign module with the reference's attributes and keys
            src = U.make_module(5)
            self.FMT_with_pathway.FMT = src.FMT
            for name in ("dim_reduction_1", "dim_reduction_2", "smooth_1", "smooth_2"):
                setattr(self.FMT_with_pathway, name, getattr(src, name))


def test_to_device_swaps_three_modules():
    model = _StubModel(True).eval()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    old = model.FMT_with_pathway
    assert mvs.to_device(model) is model
    assert isinstance(model.DepthNet, mvs.DeviceDepthNet) and isinstance(model.cost_regularization, mvs.DeviceCostRegNet)
    assert isinstance(model.FMT_with_pathway, DeviceFMTWithPathway) and model.FMT_with_pathway is not old
    assert not model.FMT_with_pathway.training
    after = model.state_dict()
    assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert mvs.to_device(_StubModel(True).train()).FMT_with_pathway.training
    plain = mvs.to_device(_StubModel(False).eval())                      # a model without the FMT is left as it is
    assert not hasattr(plain, "FMT_with_pathway") and isinstance(plain.DepthNet, mvs.DeviceDepthNet)


def test_pack_layout_against_numpy():
    net = U.make_module(9)
    sd = net.FMT.state_dict()
    p = ops.pack_fmt_layer(sd, "layers.3.")
    assert p.dtype == torch.float32 and p.is_contiguous() and tuple(p.shape) == (ops.FMT_PACK_FLOATS,)
    g = lambda k: sd["layers.3." + k].numpy()
    want = np.zeros(ops.FMT_PACK_FLOATS, np.float32)
    at = 0
    for key, (n_out, n_in) in (("attention.query_projection", (32, 32)), ("attention.key_projection", (32, 32)),
                               ("attention.value_projection", (32, 32)), ("attention.out_projection", (32, 32)), ("linear1", (64, 32)),
                               ("linear2", (32, 64))):
        w = g(key + ".weight")
        for k in range(n_in):
            for j in range(n_out):
                want[at + k * n_out + j] = w[j, k]                       # transposed: [in][out]
        at += n_in * n_out
    assert at == 8192
    for key in ("attention.query_projection.bias", "attention.key_projection.bias", "attention.value_projection.bias",
                "attention.out_projection.bias", "norm1.weight", "norm1.bias", "linear1.bias", "linear2.bias", "norm2.weight", "norm2.bias"):
        v = g(key)
        want[at:at + v.size] = v
        at += v.size
    assert at == ops.FMT_PACK_FLOATS and np.array_equal(p.numpy(), want)
    assert len(ops.FMT_LAYER_KEYS) == 16
    with pytest.raises(KeyError):
        ops.pack_fmt_layer(sd, "layers.8.")
    with pytest.raises(ValueError):
        ops.pack_fmt_layer({k: v.double() for k, v in sd.items()}, "layers.0.")
    with pytest.raises(ValueError):
        ops.pack_fmt_layer(dict(sd, **{"layers.0.linear1.weight": torch.zeros(32, 32)}), "layers.0.")


def test_packs_are_cached_on_version_counters(monkeypatch):
    net = U.make_module(9)
    calls = []
    real = ops.pack_fmt_layer
    monkeypatch.setattr(ops, "pack_fmt_layer", lambda sd, prefix: calls.append(prefix) or real(sd, prefix))
    first = net.FMT.packed()
    assert len(first) == 8 and len(calls) == 8 and net.FMT.packed() is first and len(calls) == 8
    with torch.no_grad():
        net.FMT.layers[2].norm1.bias.add_(1.0)                           # an in-place write bumps the version counter
    second = net.FMT.packed()
    assert second is not first and len(calls) == 16 and not torch.equal(second[2], first[2]) and torch.equal(second[1], first[1])
    net.FMT.layers[2].norm1.bias.data.zero_()                            # .data bumps nothing: invalidate() is the caller's part
    assert net.FMT.packed() is second
    net.invalidate()
    assert net.FMT.packed() is not second and len(calls) == 24
    a = net.packed()
    assert net.packed() is a and tuple(a[0].shape) == (2, 9, 8, 64) and tuple(a[1].shape) == (1, 9, 8, 64)
    net.invalidate()
    assert net.packed() is not a


def test_wrappers_raise_value_errors():
    tok, pack, state = torch.zeros(4, 35, 32), torch.zeros(ops.FMT_PACK_FLOATS), torch.zeros(2, 160)
    assert ops._check_fmt_layer_args(tok, pack, state) == (4, 35, 2)
    assert ops._check_fmt_kv_args(tok, pack) == (4, 35, 1) and ops._check_fmt_kv_args(torch.zeros(1, 2080, 32), pack)[2] == 5
    for change in (dict(tok=torch.zeros(4, 35, 16)), dict(tok=tok.double()), dict(tok=tok.transpose(0, 1)), dict(tok=torch.zeros(4, 0, 32)),
                   dict(tok=torch.zeros(35, 32)), dict(pack=pack[:-1]), dict(pack=pack.double()), dict(pack="p"), dict(state=torch.zeros(3, 160)),
                   dict(state=torch.zeros(2, 128)), dict(state=state.double()), dict(state=torch.zeros(160)), dict(out=torch.zeros(4, 34, 32))):
        a = dict(dict(tok=tok, pack=pack, state=state, out=None), **change)
        with pytest.raises(ValueError):
            ops._check_fmt_layer_args(a["tok"], a["pack"], a["state"], a["out"])
    for bad in (dict(partials=torch.zeros(4 * 160 - 1, dtype=torch.float64)), dict(partials=torch.zeros(4 * 160)), dict(out=torch.zeros(4, 128)),
                dict(out=torch.zeros(3, 160))):
        with pytest.raises(ValueError):
            ops._check_fmt_kv_args(tok, pack, **bad)
    x, pe = torch.zeros(2, 32, 5, 7), torch.zeros(32, 600, 600)
    assert ops._check_fmt_tokenise_args(x, pe) == (2, 5, 7)
    for bx, bpe in ((torch.zeros(2, 16, 5, 7), pe), (x.double(), pe), (x, pe.double()), (x, torch.zeros(32, 4, 600)), (x, torch.zeros(32, 601, 600)),
                    (x.permute(0, 1, 3, 2), pe), (torch.zeros(32, 5, 7), pe), (x, torch.zeros(1, 32, 600, 600))):
        with pytest.raises(ValueError):
            ops._check_fmt_tokenise_args(bx, bpe)
    with pytest.raises(ValueError):
        ops._check_fmt_tokenise_args(x, pe, torch.zeros(2, 36, 32))
    top, w, lat = torch.zeros(2, 5, 7, 32), torch.zeros(16, 32, 1, 1), torch.zeros(2, 10, 14, 16)
    assert ops._check_fpn_merge_args(top, w, lat) == (2, 5, 7, 32, 16) and ops._check_fpn_merge_args(top, w.view(16, 32), lat, lat)[4] == 16
    for bt, bw, bl in ((top, torch.zeros(16, 31, 1, 1), lat), (top, torch.zeros(6, 32), torch.zeros(2, 10, 14, 6)), (top, w, torch.zeros(2, 10, 15, 16)),
                       (top, w, torch.zeros(2, 15, 21, 16)), (top, w.double(), lat), (torch.zeros(2, 5, 7, 65), torch.zeros(16, 65), lat),
                       (top.permute(0, 2, 1, 3), w, lat), (top, torch.zeros(16, 32, 3, 3), lat)):
        with pytest.raises(ValueError):
            ops._check_fpn_merge_args(bt, bw, bl)
    for call in (lambda: ops.fmt_tokenise(x, pe), lambda: ops.fmt_kv(tok, pack), lambda: ops.fmt_layer(tok, pack, state),
                 lambda: ops.fpn_merge(top, w, lat)):
        with pytest.raises(RuntimeError):
            call()                                                       # CPU tensors: there is no fallback
