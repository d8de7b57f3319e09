"""The feature transformer's backward pass on the device: diner_fmt_layer_grad_f32 (csrc/fmt_grad.hip) through ops.fmt_layer_grad,
mvs.fmt_layer, the fmt_kernels switches and fit_estimator(fmt_kernels=True).

The yardstick is float64 torch autograd on the host (which tests/test_fmt_grad_cpu.py holds against fixture G35); the bar is
mvs_util.BAR_FACTOR (4) times the distance the reference's own float32 autograd keeps from float64 on the same case and output, as the
fixture records it; no element is excluded, and every case meets the condition on its inputs (no linear1 output near the ReLU's kink:
fmt_grad_util.kink_ratio, asserted by the generator and by the CPU tests).  Shapes: fmt_grad_util.LAYER_CASES (35 tokens in one tile;
851 tokens in 7 tiles, two images; 6 images of 129 tokens reading 2 sources of 600; 2080 tokens in 17 tiles with the slab count forced)
and STACK_CASES (B 1, two views of 5 x 7; B 2, three views of 9 x 15).

Measured on an MI355X (max |kernel - float64| / bar per case and output): profiles/fmt_grad_ratios.txt, DESIGN.md section 8t."""
import pytest
import torch

from diner_amd import estimator, mvs, ops
from tests import estimator_util as EU
from tests import fmt_grad_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _device_case(name, flip=False):
    """-> (x, source (x itself for a self layer), pack, state, dy) on the device, as the C entry takes them."""
    inp = U.layer_inputs(name)
    x, dy = inp["x"].to(DEV), inp["dy"].to(DEV)
    if flip:
        x, dy = x.flip(0).contiguous(), dy.flip(0).contiguous()
    source = x if inp["source"] is None else inp["source"].to(DEV)
    pack = ops.pack_fmt_layer({k: v.to(DEV) for k, v in inp["state_dict"].items()})
    return x, source, pack, ops.fmt_kv(source, pack), dy


def _named(name, res):
    """(d_x, d_source, d_params) of ops.fmt_layer_grad -> {output: tensor}."""
    d_x, d_source, d_par = res
    out = {}
    if d_x is not None:
        out["d_x"] = d_x
    if d_source is not None:
        out["d_source"] = d_source
    if d_par is not None:
        out.update(zip(U.SHORT, ops.unpack_fmt_layer_grad(d_par)))
    return out


def _check(name, got, label):
    """Every output of `got` against float64 within the fixture's bar; prints error / bar."""
    fx, want = U.fixture(), U.layer_expected64(name)
    missed = []
    for key in U.layer_outputs(name):
        if got.get(key) is None:
            continue
        assert got[key].shape == want[key].shape and got[key].dtype == torch.float32 and got[key].is_cuda, (name, key)
        assert bool(torch.isfinite(got[key]).all()), (name, key)
        e, bar = _err(got[key], want[key]), U.bar(fx, name, key)
        print(f"{name} {label} {key}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}), max |value| {float(want[key].abs().max()):.3g}")
        if e > bar:
            missed.append((key, e, bar))
    assert not missed, (name, label, missed)


# ---- 1. every case and output against float64; the forward is the existing kernels ------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.LAYER_CASES))
def test_layer_against_float64(name):
    layer = U.make_layer(name, torch.float32, DEV)
    got = U.run_layer(name, torch.float32, DEV, fn=mvs.fmt_layer, layer=layer)
    x, source, pack, state, _ = _device_case(name)
    assert mvs.fmt_layer_gate(x, source, layer)
    assert torch.equal(got["y"], ops.fmt_layer(x, pack, state))
    assert ("d_source" in got) == (U.LAYER_CASES[name]["source"] is not None)
    _check(name, got, "function")


# ---- 2. the slab count ---------------------------------------------------------------------------------------------------------------------
def test_forced_slabs_against_the_default():
    """cross_blocks: 2080 tokens are 17 tiles on either side; three slabs walk them 6 + 6 + 5 (the last tile holds 32 tokens), one slab
    walks all of them, the default takes 17 slabs of one tile each."""
    name, fx = "cross_blocks", U.fixture()
    assert U.LAYER_CASES[name]["slabs"] == (0, 3, 1)
    assert ops.fmt_grad_slabs(1, 2080, 1, 2080, 3) == (3, 3) and ops.fmt_grad_slabs(1, 2080, 1, 2080) == (17, 17)
    args = _device_case(name)
    runs = {s: _named(name, ops.fmt_layer_grad(*args, slabs=s)) for s in U.LAYER_CASES[name]["slabs"]}
    for s, got in runs.items():
        _check(name, got, f"slabs={s or 'default'}")
    for key in ("d_x", "d_source"):
        assert torch.equal(runs[3][key], runs[0][key]) and torch.equal(runs[1][key], runs[0][key])       # the slab count touches the parameters only
    for s in (3, 1):
        for key in U.SHORT:
            d, bar = _err(runs[s][key], runs[0][key]), U.bar(fx, name, key)
            print(f"{name} slabs {s} against the default {key}: {d:.2e}, bar {bar:.2e} (x{d / bar:.2f})")
            assert d <= bar, (s, key, d, bar)


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["self_ragged", "cross_views"])
def test_two_runs_and_a_flipped_batch_give_the_same_bits(name):
    """All eighteen outputs: torch.equal between two runs.  A batch flipped along N gives the flipped d_x bits (the state rows are flipped
    with it: cross_views' three images a row stay with their row when both are reversed)."""
    a, b = (_named(name, ops.fmt_layer_grad(*_device_case(name))) for _ in range(2))
    assert set(a) == set(U.layer_outputs(name))
    for key in a:
        assert bool(a[key].any()) and torch.equal(a[key], b[key]), (name, key)
    x, source, pack, state, dy = _device_case(name, flip=True)
    if source is not x:
        source = source.flip(0).contiguous()
        state = ops.fmt_kv(source, pack)
    c = _named(name, ops.fmt_layer_grad(x, source, pack, state, dy))
    assert a["d_x"].shape[0] > 1 and torch.equal(a["d_x"], c["d_x"].flip(0))
    c["d_x"] = c["d_x"].flip(0)
    if "d_source" in c:
        c["d_source"] = c["d_source"].flip(0)
    _check(name, c, "flipped")


# ---- 4. outputs that are not wanted ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["self_tiny", "cross_views"])
def test_null_outputs_skip_their_work_and_leave_the_others(name):
    args = _device_case(name)
    self_layer = args[1] is args[0]
    full = ops.fmt_layer_grad(*args)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (False, False, False)):
        got = ops.fmt_layer_grad(*args, want=want)
        flags = (want[0] or want[1], False, want[2]) if self_layer else want           # a self layer has one token gradient, d_x
        for i, (flag, g, f) in enumerate(zip(flags, got, full)):
            assert (g is not None) == flag, (want, i)
            if flag:
                assert torch.equal(g, f), (want, i)


def test_function_computes_only_what_is_needed(monkeypatch):
    name = "cross_views"
    seen, inner = [], ops.fmt_layer_grad
    monkeypatch.setattr(ops, "fmt_layer_grad", lambda *a, **k: seen.append(tuple(k["want"])) or inner(*a, **k))
    inp = U.layer_inputs(name)
    layer = U.make_layer(name, torch.float32, DEV)
    x, source = inp["x"].to(DEV).requires_grad_(True), inp["source"].to(DEV)
    for p in layer.parameters():
        p.requires_grad_(False)
    (mvs.fmt_layer(x, source, layer) * inp["dy"].to(DEV)).sum().backward()
    assert seen == [(True, False, False)] and x.grad is not None
    layer.linear1.bias.requires_grad_(True)
    (mvs.fmt_layer(x.detach(), source.requires_grad_(True), layer) * inp["dy"].to(DEV)).sum().backward()
    assert seen[1] == (False, True, True) and layer.linear1.bias.grad is not None and layer.linear1.weight.grad is None


# ---- 5. the closed gate ------------------------------------------------------------------------------------------------------------------------
def test_closed_gate_takes_torch(monkeypatch):
    name = "self_tiny"
    calls = []
    inner_f, inner_b = ops.fmt_layer, ops.fmt_layer_grad
    monkeypatch.setattr(ops, "fmt_layer", lambda *a, **k: calls.append("f") or inner_f(*a, **k))
    monkeypatch.setattr(ops, "fmt_layer_grad", lambda *a, **k: calls.append("b") or inner_b(*a, **k))
    want = U.layer_expected64(name)
    # CPU tensors, and float64 on the device: the torch layer, silently
    cpu = U.run_layer(name, torch.float32, fn=mvs.fmt_layer)
    dev64 = U.run_layer(name, torch.float64, DEV, fn=mvs.fmt_layer)
    assert calls == []
    for key in U.layer_outputs(name):
        assert _err(dev64[key], want[key]) <= 1e-9 * max(1.0, float(want[key].abs().max())), key
        assert _err(cpu[key], want[key]) <= U.bar(U.fixture(), name, key), key
    # the open gate: one forward, one backward
    got = U.run_layer(name, torch.float32, DEV, fn=mvs.fmt_layer)
    assert calls == ["f", "b"]
    # create_graph=True: the forward on the kernels, the backward through the torch layer, which carries a second derivative
    inp = U.layer_inputs(name)
    layer = U.make_layer(name, torch.float32, DEV)
    x = inp["x"].to(DEV).requires_grad_(True)
    first = torch.autograd.grad((mvs.fmt_layer(x, x, layer) * inp["dy"].to(DEV)).sum(), [x, layer.linear2.weight], create_graph=True)
    assert calls == ["f", "b", "f"] and all(f.requires_grad for f in first)
    assert _err(first[0], got["d_x"]) <= U.bar(U.fixture(), name, "d_x")
    second = torch.autograd.grad(first[0].square().sum(), layer.linear1.weight)[0]
    ref_layer = U.make_layer(name, torch.float32, DEV)
    xr = inp["x"].to(DEV).requires_grad_(True)
    ref_first = torch.autograd.grad((ref_layer(xr, xr) * inp["dy"].to(DEV)).sum(), [xr], create_graph=True)
    ref_second = torch.autograd.grad(ref_first[0].square().sum(), ref_layer.linear1.weight)[0]
    assert bool(second.any()) and _err(second, ref_second) <= 1e-4 * float(ref_second.abs().max())


# ---- 6. the whole stack through DeviceFMT.encode -------------------------------------------------------------------------------------------
# The outputs on which the PARENT's torch route, run on the device, misses the fixture's bar by itself (measured on an MI355X, max |torch on
# the device - float64| over the bar): they are held to the bar plus that route's own distance, and to that route within the bar.
DEVICE_TORCH_MISSES = {
    ("encode", "stack_tiny"): {}, ("encode", "stack_views"): {},
    ("pathway", "stack_tiny"): {}, ("pathway", "stack_views"): {},
}

_RUNS = {}


def _runs(kind, name):
    """The step on the device with the switch on and off, run once per session."""
    if (kind, name) not in _RUNS:
        run = U.run_encode if kind == "encode" else U.run_pathway
        _RUNS[kind, name] = (run(name, torch.float32, DEV, fmt_kernels=True), run(name, torch.float32, DEV, fmt_kernels=False))
    return _RUNS[kind, name]


def _check_stack(kind, name, want, n_params):
    on, off = _runs(kind, name)
    bars = U.stack_bars(U.fixture(), name, kind)
    assert set(on) == set(want) == set(off) == set(bars) and sum(k.startswith("param_") for k in want) == n_params
    relaxed = DEVICE_TORCH_MISSES[kind, name]
    assert set(relaxed) <= set(want)
    worst, missed = 0.0, []
    for k in sorted(want):
        bar = bars[k]
        assert on[k].shape == want[k].shape and bool(torch.isfinite(on[k]).all()), k
        e, e_off, d = _err(on[k], want[k]), _err(off[k], want[k]), _err(on[k], off[k])
        tag = "  [held to torch on the device]" if k in relaxed else ""
        print(f"{kind} {name} {k}: max |value| {float(want[k].abs().max()):.2e}, kernels {e:.2e} (x{e / bar:.2f}), torch on the device {e_off:.2e} "
              f"(x{e_off / bar:.2f}), between them {d:.2e} (x{d / bar:.2f}), bar {bar:.2e}{tag}")
        if k in relaxed:
            worst = max(worst, d / bar)
            if e > bar + e_off or d > bar:
                missed.append((k, e, e_off, d, bar))
        else:
            worst = max(worst, e / bar)
            if e > bar:
                missed.append((k, e, e_off, d, bar))
    print(f"{kind} {name}: worst ratio x{worst:.2f}")
    assert not missed, missed


@pytest.mark.parametrize("name", list(U.STACK_CASES))
def test_encode_with_fmt_kernels_against_float64(name, monkeypatch):
    """DeviceFMT.encode with fmt_kernels: the outputs, the gradient of every input feature map and of all 128 FMT parameters against
    float64; 1 and 2 batch elements, 1 and 2 source views.  Every layer call runs the kernels: 4 for the reference view, 8 for the
    source views as one batch."""
    routes, inner = [], mvs.fmt_layer
    monkeypatch.setattr(mvs, "fmt_layer", lambda x, s, ly, **k: routes.append(mvs.fmt_layer_gate(x, s, ly)) or inner(x, s, ly, **k))
    _RUNS.pop(("encode", name), None)
    _check_stack("encode", name, U.encode_expected64(name), 128)
    assert routes == [True] * 12


@pytest.mark.parametrize("name", list(U.STACK_CASES))
def test_pathway_training_step_with_and_without_fmt_kernels(name):
    """DeviceFMTWithPathway.forward in training mode from identical state, fmt_kernels True against float64 and against fmt_kernels False
    on the same device: all three stages of every view, the gradients at every input and at the 132 parameters.  This shows that the
    switch wires the same step; the pathway's own backward is torch on both routes."""
    _check_stack("pathway", name, U.pathway_expected64(name), 132)


# ---- 7. the loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("others", [False, True])
def test_fit_estimator_with_fmt_kernels(others, monkeypatch):
    model, batch = EU.fit_model(DEV), EU.fit_batch(DEV)
    seen, routes = [], []
    inner, inner_layer = estimator.focal_loss_bld, mvs.fmt_layer

    def spy(inputs, depth_gt_ms, mask_ms, depth_interval, **kw):
        out = inner(inputs, depth_gt_ms, mask_ms, depth_interval, **kw)
        if not seen:
            def host(d, dt):
                return {k: (host(v, dt) if isinstance(v, dict) else v.detach().cpu().to(dt) if torch.is_tensor(v) else v) for k, v in d.items()}
            restated = [[float(t) for t in estimator.focal_loss_bld_torch(host(inputs, dt), host(depth_gt_ms, dt), host(mask_ms, dt),
                                                                          depth_interval.cpu().to(dt), **kw)]
                        for dt in (torch.float64, torch.float32)]
            seen.append(([float(t.detach()) for t in out], *restated))
        return out

    def layer_spy(x, source, layer, **kw):
        routes.append(mvs.fmt_layer_gate(x, source, layer))
        return inner_layer(x, source, layer, **kw)
    monkeypatch.setattr(estimator, "focal_loss_bld", spy)
    monkeypatch.setattr(mvs, "fmt_layer", layer_spy)
    steps = EU.FIT["steps"]
    assert model.fmt_kernels is False
    history, _ = estimator.fit_estimator(model, [batch], steps=steps, lr=EU.FIT["lr"], fmt_kernels=True, match_kernels=others, deform_kernels=others)
    assert model.fmt_kernels is False and model.deform_kernels is False and model.match_kernels is False and model.fused_readout is False
    assert len(routes) == 12 * steps and all(routes)          # 4 self layers of the reference view, 8 layers of the source views as one batch
    got, want, want32 = seen[0]
    assert history[0]["total"] == got[0]
    bar = max(EU.BAR_FACTOR * abs(want32[0] - want[0]), EU.FLOOR * abs(want[0]))            # tests/test_estimator_gpu.py's step-0 bar
    print(f"fit fmt_kernels with the other switches {others} step 0 total: {abs(got[0] - want[0]):.2e}, bar {bar:.2e}; "
          f"totals {[round(h['total'], 4) for h in history]}")
    assert abs(got[0] - want[0]) <= bar
    assert all(v == v and abs(v) != float("inf") for h in history for v in h.values())
    assert history[-1]["total"] < history[0]["total"]
