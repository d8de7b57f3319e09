"""The feature transformer's gradients without a device: the closed form mvs.fmt_layer_grad_torch against float64 autograd, fixture G35
against a regeneration of its inputs, the condition on the inputs (the ReLU's kink), the argument checks of ops.fmt_layer_grad, the
fmt_kernels switch on the torch route, and the new symbols of the header."""
import os
import re

import numpy as np
import pytest
import torch

from diner_amd import estimator, mvs, ops
from tests import fmt_grad_util as U
from tests import mvs_util as MU


def _err(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("name", list(U.LAYER_CASES))
def test_closed_form_against_float64_autograd(name):
    want, got = U.layer_expected64(name), U.closed_form(name, torch.float64)
    assert set(got) == set(U.layer_outputs(name))
    for key in got:
        assert got[key].shape == want[key].shape
        assert _err(got[key], want[key]) <= 1e-12 * max(1.0, float(want[key].abs().max())), (name, key)


def test_closed_form_in_float32_is_within_the_bar():
    """The arithmetic the kernels restate, in float32 on the host: inside the bar the kernels are held to."""
    name, fx = "cross_views", U.fixture()
    want, got = U.layer_expected64(name), U.closed_form(name, torch.float32)
    for key in got:
        assert got[key].dtype == torch.float32 and _err(got[key], want[key]) <= U.bar(fx, name, key), (name, key)


def test_fixture_matches_a_regeneration():
    fx = U.fixture()
    assert str(fx["sha256"]) == U.input_hash()
    assert list(fx["layer_cases"]) == list(U.LAYER_CASES) and list(fx["stack_cases"]) == list(U.STACK_CASES)
    assert list(fx["seeds"]) == [c["seed"] for c in list(U.LAYER_CASES.values()) + list(U.STACK_CASES.values())]
    assert int(fx["seed_offset"]) == U.SEED_OFFSET
    for name in U.LAYER_CASES:
        want = U.layer_expected64(name)
        for key in U.layer_outputs(name):
            assert float(fx[f"{name}_err_{key}"]) > 0.0
            np.testing.assert_allclose(U.sample(want[key]), fx[f"{name}_{key}64"], rtol=1e-9, atol=1e-12)
    for name in U.STACK_CASES:
        for kind, want in (("encode", U.encode_expected64(name)), ("pathway", U.pathway_expected64(name))):
            keys = [str(k) for k in fx[f"{name}_{kind}_keys"]]
            assert keys == sorted(want) and bool((fx[f"{name}_{kind}_errs"] > 0).all())
            for row, key in zip(fx[f"{name}_{kind}_64"], keys):
                got = U.sample(want[key])
                np.testing.assert_allclose(got, row[:got.size], rtol=1e-9, atol=1e-12)
                assert bool(np.isnan(row[got.size:]).all())
    assert sum(k.startswith("param_") for k in U.encode_expected64("stack_views")) == 128
    assert sum(k.startswith("param_") for k in U.pathway_expected64("stack_views")) == 132


@pytest.mark.parametrize("name", list(U.LAYER_CASES) + list(U.STACK_CASES))
def test_no_hidden_unit_sits_at_the_kink(name):
    """The condition on the inputs, nothing excluded: min |linear1 output| in float64 >= 4 max |float32 - float64| of those outputs."""
    ratio = U.layer_kink_ratio(name) if name in U.LAYER_CASES else U.stack_kink_ratio(name)
    print(f"{name}: min |linear1 output| / (4 max |float32 - float64|) = {ratio:.2f}")
    assert ratio >= 1.0
    assert abs(ratio - float(U.fixture()[f"{name}_kink"])) <= 1e-6 * ratio


def test_argument_checks_without_a_device():
    x, src, dy = torch.zeros(6, 129, 32), torch.zeros(2, 600, 32), torch.zeros(6, 129, 32)
    pack, state = torch.zeros(ops.FMT_PACK_FLOATS), torch.zeros(2, ops.FMT_STATE_FLOATS)
    assert ops._check_fmt_layer_grad_args(x, src, pack, state, dy) == (6, 129, 2, 600, False)
    assert ops._check_fmt_layer_grad_args(x, x, pack, torch.zeros(6, 160), dy) == (6, 129, 6, 129, True)
    bad = [dict(x=torch.zeros(6, 129, 31)), dict(x=x.double()), dict(x=x.transpose(0, 1)), dict(src=torch.zeros(4, 600, 32)),
           dict(dy=torch.zeros(6, 128, 32)), dict(pack=pack[:-1]), dict(state=torch.zeros(3, 160)), dict(state=state.double()),
           dict(want=(True, True)), dict(slabs=-1), dict(slabs=1025), dict(slabs=True), dict(slabs=2.0)]
    for change in bad:
        a = dict(x=x, src=src, pack=pack, state=state, dy=dy, want=(True, True, True), slabs=0)
        a.update(change)
        with pytest.raises(ValueError):
            ops._check_fmt_layer_grad_args(a["x"], a["src"], a["pack"], a["state"], a["dy"], a["want"], a["slabs"])
    with pytest.raises(RuntimeError):                                  # the checks pass; there is no CPU fallback
        ops.fmt_layer_grad(x, src, pack, state, dy)
    # the workspace and slab counts as the header states them
    assert ops.fmt_grad_slabs(1, 2080, 1, 2080) == (17, 17) and ops.fmt_grad_slabs(1, 2080, 1, 2080, 3) == (3, 3)
    assert ops.fmt_grad_slabs(4, 5120, 4, 5120) == (128, 128) and ops.fmt_grad_slabs(6, 129, 2, 600) == (12, 10)
    assert ops.fmt_grad_workspace_floats(6, 129, 2, 600) == 2 * 12 * 160 + 2 * 160 + 2 * (12 * 6432 + 10 * 2112)
    assert sum(int(np.prod(s)) for s in ops._FMT_LAYER_SHAPES) == ops.FMT_PACK_FLOATS
    views = ops.unpack_fmt_layer_grad(torch.arange(ops.FMT_PACK_FLOATS, dtype=torch.float32))
    assert [tuple(v.shape) for v in views] == list(ops._FMT_LAYER_SHAPES) and float(views[4][1, 0]) == 4096 + 32


def test_fmt_layer_on_the_cpu_is_the_torch_layer():
    """The closed gate: CPU tensors take _EncoderLayer.forward, a shared source repeated over the images that read it."""
    name = "cross_views"
    inp = U.layer_inputs(name)
    layer = U.make_layer(name)
    assert not mvs.fmt_layer_gate(inp["x"], inp["source"], layer)
    got = mvs.fmt_layer(inp["x"], inp["source"], layer)
    assert torch.equal(got, layer(inp["x"], inp["source"].repeat(3, 1, 1)))
    assert torch.equal(mvs.fmt_layer(inp["x"], inp["x"], layer), layer(inp["x"], inp["x"]))


def test_switch_plumbing_on_the_torch_route():
    """fmt_kernels on and off give equal results on the CPU (the training gate needs HIP tensors); the properties reach DeviceFMT."""
    name = "stack_tiny"
    off, on = U.run_pathway(name, torch.float32, fmt_kernels=False), U.run_pathway(name, torch.float32, fmt_kernels=True)
    assert set(on) == set(off) and all(torch.equal(on[k], off[k]) for k in on)
    off, on = U.run_encode(name, torch.float32, fmt_kernels=False), U.run_encode(name, torch.float32, fmt_kernels=True)
    assert all(torch.equal(on[k], off[k]) for k in on)
    net = mvs.DeviceFMTWithPathway(8)
    assert net.fmt_kernels is False and net.FMT.fmt_kernels is False
    net.fmt_kernels = 1
    assert net.fmt_kernels is True and net.FMT.fmt_kernels is True
    assert not net.FMT.trains_on_kernels(torch.zeros(1, 32, 5, 7))
    model = estimator.DeviceTransMVSNet()
    assert model.fmt_kernels is False
    model.fmt_kernels = True
    assert model.FMT_with_pathway.FMT.fmt_kernels is True and model.deform_kernels is False and model.match_kernels is False
    model.fmt_kernels = False
    assert model.FMT_with_pathway.fmt_kernels is False
    assert mvs.FMT_LAYER_SHORT == U.SHORT and len(mvs._layer_parameters(net.FMT.layers[0])) == 16
    sd = net.FMT.layers[0].state_dict()
    assert all(p.shape == sd[k].shape for p, k in zip(mvs._layer_parameters(net.FMT.layers[0]), ops.FMT_LAYER_KEYS))


def test_header_declares_the_new_symbols():
    with open(os.path.join(MU.ROOT, "include", "diner_hip.h")) as f:
        text = f.read()
    assert re.search(r"#define DINER_ABI_VERSION 6\b", text)
    assert re.search(r"size_t diner_fmt_layer_grad_workspace_floats\(int N, int L, int R, int S, int slabs\);", text)
    assert re.search(r"int diner_fmt_layer_grad_f32\(const float\* x, const float\* source, const float\* pack, const float\* state, const float\* dy,", text)
    for name, value in (("DINER_FMT_GRAD_TOKENS", ops.FMT_GRAD_TOKENS), ("DINER_FMT_GRAD_QUERY_SLAB_FLOATS", ops.FMT_GRAD_QUERY_SLAB_FLOATS),
                        ("DINER_FMT_GRAD_SOURCE_SLAB_FLOATS", ops.FMT_GRAD_SOURCE_SLAB_FLOATS), ("DINER_FMT_GRAD_MAX_SLABS", ops.FMT_GRAD_MAX_SLABS)):
        assert re.search(rf"#define {name} {value}\b", text), name
    from diner_amd import _lib
    with open(_lib.__file__) as f:
        assert "diner_fmt_layer_grad_f32" in f.read()
