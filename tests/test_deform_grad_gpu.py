"""The deformable convolution's backward pass on the device: diner_deform_conv3x3_grad_f32 (csrc/deform_grad.hip) through
ops.deform_conv3x3_grad, mvs.deform_conv3x3, the deform_kernels switches and fit_estimator(deform_kernels=True).

The yardstick is the float64 torch restatement on the host (which tests/test_deform_grad_cpu.py holds against fixture G34); the bar is
mvs_util.BAR_FACTOR (4) times the distance the reference's own float32 autograd keeps from float64 on the same case and output, as the
fixture records it; no element is excluded.  Shapes: the last deformable layer of each head on featurenet_util's "tiny" (4 x 6, 8 x 12,
16 x 24: one partial tile) and "ragged" (four images of 9 x 13, 18 x 26, 36 x 52: ragged tails, several tiles and images) runs, Cout 32,
16 and 8; synthetic maps with Cin 8, 16, 64 and Cout 1, 27, 64, one of 5 tiles with the slab count forced to 3; the fresh layer (offmask
zero); planted NaN, +-inf and +-1e30 offsets.

Measured on an MI355X (max |kernel - float64| / bar per case and output): profiles/deform_grad_ratios.txt, DESIGN.md section 8s."""
import pytest
import torch

from diner_amd import estimator, mvs, ops
from tests import deform_grad_util as U
from tests import estimator_util as EU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _cl(name, flip=False):
    """A case's tensors on the device as the C entry takes them: channels-last activations, the plain weight."""
    inp = U.inputs(name)
    t = {k: inp[k].to(DEV) for k in ("x", "offmask", "dy")}
    if flip:
        t = {k: v.flip(0) for k, v in t.items()}
    t = {k: v.permute(0, 2, 3, 1).contiguous() for k, v in t.items()}
    return t["x"], t["offmask"], inp["weight"].to(DEV).contiguous(), t["dy"]


def _nchw(res):
    d_x, d_om, d_w, d_b = res
    return dict(d_x=None if d_x is None else d_x.permute(0, 3, 1, 2), d_offmask=None if d_om is None else d_om.permute(0, 3, 1, 2), d_weight=d_w,
                d_bias=d_b)


def _check(name, got, label):
    """Every output of `got` against float64 within the fixture's bar; prints error / bar."""
    fx, want = U.fixture(), U.expected64(name)
    missed = []
    for key in U.OUTPUTS:
        if got.get(key) is None:
            continue
        assert got[key].shape == want[key].shape and got[key].dtype == torch.float32 and got[key].is_cuda, (name, key)
        assert bool(torch.isfinite(got[key]).all()), (name, key)
        e, bar = _err(got[key], want[key]), U.bar(fx, name, key)
        print(f"{name} {label} {key}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}), max |value| {float(want[key].abs().max()):.3g}")
        if e > bar:
            missed.append((key, e, bar))
    assert not missed, (name, label, missed)


# ---- 1. every case and output against float64; the forward is the existing kernel ------------------------------------------------------------
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_kernels_against_float64(name):
    inp = U.inputs(name)
    dev = {k: inp[k].to(DEV) for k in ("x", "offmask", "weight", "bias")}
    assert mvs.deform_gate(dev["x"], dev["offmask"], dev["weight"], dev["bias"])
    got = U.run_layer(inp, torch.float32, DEV)
    x, om, w, dy = _cl(name)
    y = ops.deform_conv3x3(x, om, ops.pack_deform_conv3x3(w), dev["bias"], int(w.shape[0]))
    assert torch.equal(got["y"], y.permute(0, 3, 1, 2)) and got["y"].permute(0, 2, 3, 1).is_contiguous()
    _check(name, got, "function")


# ---- 2. the slab count ---------------------------------------------------------------------------------------------------------------------
def test_forced_slabs_against_the_default():
    """syn_16_27: 306 pixels are 5 tiles; three slabs walk them 2 + 2 + 1 (a ragged tail), the default takes 5 slabs of one tile each."""
    name, fx = "syn_16_27", U.fixture()
    assert U.inputs(name)["slabs"] == 3 and ops.deform_grad_slabs(1, 17, 18, 3) == 3 and ops.deform_grad_slabs(1, 17, 18) == 5
    x, om, w, dy = _cl(name)
    forced, default = _nchw(ops.deform_conv3x3_grad(x, om, w, dy, slabs=3)), _nchw(ops.deform_conv3x3_grad(x, om, w, dy))
    one = _nchw(ops.deform_conv3x3_grad(x, om, w, dy, slabs=1))
    _check(name, forced, "slabs=3")
    _check(name, default, "slabs=default")
    _check(name, one, "slabs=1")
    assert torch.equal(forced["d_offmask"], default["d_offmask"])            # the slab count touches d_weight and d_bias only
    for key in ("d_weight", "d_bias"):
        d, bar = _err(forced[key], default[key]), U.bar(fx, name, key)
        print(f"{name} slabs 3 against the default {key}: {d:.2e}, bar {bar:.2e} (x{d / bar:.2f})")
        assert d <= bar, (key, d, bar)


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged_16", "syn_8_1", "planted"])
def test_two_runs_and_a_flipped_batch_give_the_same_bits(name):
    """d_offmask, d_weight and d_bias: torch.equal between two runs; a flipped batch gives the flipped d_offmask bits.  (d_weight and d_bias
    of a flipped batch walk the tiles in another order; d_x is summed by float atomic adds.  Both are held to the bar only.)"""
    a, b = (_nchw(ops.deform_conv3x3_grad(*_cl(name))) for _ in range(2))
    c = _nchw(ops.deform_conv3x3_grad(*_cl(name, flip=True)))
    for key in ("d_offmask", "d_weight", "d_bias"):
        assert bool(a[key].any()) and torch.equal(a[key], b[key]), (name, key)
    assert a["d_offmask"].shape[0] > 1 and torch.equal(a["d_offmask"], c["d_offmask"].flip(0))
    c["d_x"] = c["d_x"].flip(0)
    c["d_offmask"] = c["d_offmask"].flip(0)
    _check(name, c, "flipped")


# ---- 4. outputs that are not wanted ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_8", "syn_64_64"])
def test_null_outputs_skip_their_work_and_leave_the_others(name):
    args = _cl(name)
    full = ops.deform_conv3x3_grad(*args)
    for want in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
                 (False, True, True, False), (True, False, False, True), (False, False, False, False)):
        got = ops.deform_conv3x3_grad(*args, want=want)
        for i, (flag, g, f) in enumerate(zip(want, got, full)):
            assert (g is not None) == flag, (want, i)
            if flag and i > 0:
                assert torch.equal(g, f), (want, i)
        _check(name, _nchw(got), "want=" + "".join("1" if f else "0" for f in want))


def test_function_computes_only_what_is_needed(monkeypatch):
    inp = U.inputs("tiny_16")
    seen, inner = [], ops.deform_conv3x3_grad
    monkeypatch.setattr(ops, "deform_conv3x3_grad", lambda *a, **k: seen.append(tuple(k["want"])) or inner(*a, **k))
    t = {k: inp[k].to(DEV) for k in ("x", "offmask", "weight", "bias", "dy")}
    for needs in ((True, True, True, True), (False, False, True, True), (True, False, False, False), (False, True, True, False)):
        leaves = [t[k].clone().requires_grad_(n) for k, n in zip(("x", "offmask", "weight", "bias"), needs)]
        (mvs.deform_conv3x3(*leaves) * t["dy"]).sum().backward()
        assert seen[-1] == needs and all((leaf.grad is not None) == n for leaf, n in zip(leaves, needs))
    leaves = [t[k].clone().requires_grad_(True) for k in ("x", "offmask", "weight")]
    (mvs.deform_conv3x3(*leaves) * t["dy"]).sum().backward()                 # no bias: no d_bias
    assert seen[-1] == (True, True, True, False)


# ---- 5. offsets that are not numbers -------------------------------------------------------------------------------------------------------------
def test_planted_offsets_give_exact_zeros():
    got = _nchw(ops.deform_conv3x3_grad(*_cl("planted")))
    for key in U.OUTPUTS:
        assert bool(torch.isfinite(got[key]).all()), key
    d_om = got["d_offmask"].cpu()
    for n, h, w, k in U.planted_taps():
        assert all(float(d_om[n, ch, h, w]) == 0.0 for ch in (2 * k, 2 * k + 1, 18 + k)), (n, h, w, k)
    want = U.expected64("planted")["d_offmask"]
    assert torch.equal(d_om == 0, want == 0)          # exact zeros exactly where float64 has them: the taps that lie outside, planted or not


def test_fresh_layer_sits_on_integer_coordinates():
    """offmask zero: every coordinate an exact integer (the right-sided difference), m = 0.5; the forward is then half a plain convolution."""
    inp = U.inputs("zero")
    got = U.run_layer(inp, torch.float32, DEV)
    plain = torch.nn.functional.conv2d(inp["x"].double(), 0.5 * inp["weight"].double(), inp["bias"].double(), padding=1)
    assert _err(got["y"], plain) <= 1e-5
    _check("zero", got, "function")


# ---- 6. the closed gate ----------------------------------------------------------------------------------------------------------------------
def test_closed_gate_takes_torch(monkeypatch):
    calls = []
    inner_f, inner_b = ops.deform_conv3x3, ops.deform_conv3x3_grad
    monkeypatch.setattr(ops, "deform_conv3x3", lambda *a, **k: calls.append("f") or inner_f(*a, **k))
    monkeypatch.setattr(ops, "deform_conv3x3_grad", lambda *a, **k: calls.append("b") or inner_b(*a, **k))
    g = torch.Generator().manual_seed(3499)

    def case(Cin, Cout, dtype, device):
        return dict(x=torch.randn(1, Cin, 5, 7, generator=g), offmask=torch.randn(1, 27, 5, 7, generator=g),
                    weight=0.1 * torch.randn(Cout, Cin, 3, 3, generator=g), bias=torch.randn(Cout, generator=g),
                    dy=torch.randn(1, Cout, 5, 7, generator=g)), dtype, device
    for inp, dtype, device in (case(32, 8, torch.float32, None), case(32, 8, torch.float64, DEV), case(12, 8, torch.float32, DEV),
                               case(32, 65, torch.float32, DEV)):
        a = U.run_layer(inp, dtype, device)
        b = U.run_layer(inp, dtype, device, fn=mvs._deform_torch)
        assert torch.equal(a["y"], b["y"]), (dtype, device)
        # the gradients: torch's own index scatter adds atomically on a device, so two runs of the same route differ in the last bits
        eps = 2.0 ** -52 if dtype == torch.float64 else 2.0 ** -23
        for k in U.OUTPUTS:
            assert a[k].dtype == dtype and _err(a[k], b[k]) <= 64 * eps * float(b[k].abs().max()), (dtype, device, k)
    assert calls == []
    inp, dtype, device = case(32, 8, torch.float32, DEV)
    U.run_layer(inp, dtype, device)
    assert calls == ["f", "b"]
    # a second derivative: the backward pass differentiates the restatement instead
    t = {k: inp[k].to(DEV) for k in inp}
    leaves = [t[k].clone().requires_grad_(True) for k in ("x", "offmask", "weight", "bias")]
    first = torch.autograd.grad((mvs.deform_conv3x3(*leaves) * t["dy"]).sum(), leaves, create_graph=True)
    assert calls == ["f", "b", "f"] and all(f.requires_grad for f in first[:3])
    second = torch.autograd.grad(first[0].square().sum(), leaves[2])[0]
    ref_leaves = [t[k].clone().requires_grad_(True) for k in ("x", "offmask", "weight", "bias")]
    ref_first = torch.autograd.grad((mvs._deform_torch(*ref_leaves) * t["dy"]).sum(), ref_leaves, create_graph=True)
    ref_second = torch.autograd.grad(ref_first[0].square().sum(), ref_leaves[2])[0]
    assert bool(second.any()) and _err(second, ref_second) <= 1e-4 * float(ref_second.abs().max())


# ---- 7. one whole FeatureNet training step, the switch on against off -----------------------------------------------------------------------
# The outputs on which the PARENT's torch route, run on the device, misses the fixture's bar by itself (measured on an MI355X, max |torch on
# the device - float64| over the bar): they are held to that route within the bar instead.
DEVICE_TORCH_MISSES = {
    "tiny": {"param_conv1.1.bn.weight": 1.05},          # 1.02 in another run, the kernel route 1.02 and 0.96
    # one ReLU between out2.5 and out2.7 falls the other way on the device than on the host the bars were recorded on
    "ragged": {"param_out2.4.weight": 12.99, "param_out2.4.conv_offset_mask.weight": 4.75, "param_out2.4.conv_offset_mask.bias": 4.92,
               "param_out2.5.weight": 6.88, "param_out2.5.bias": 15.38, "param_out2.7.conv_offset_mask.weight": 15.08,
               "param_out2.7.conv_offset_mask.bias": 21.87},
}


_STEPS = {}


def _steps(name):
    """The step on the device with the switch on (and the upstream magnitudes at the deformable layers) and off, run once per session."""
    if name not in _STEPS:
        sums = {}
        on = U.run_net(name, torch.float32, DEV, deform_kernels=True, dy_sums=sums)
        _STEPS[name] = (on, U.run_net(name, torch.float32, DEV, deform_kernels=False), sums)
    return _STEPS[name]


@pytest.mark.parametrize("name", U.NET_CASES)
def test_featurenet_training_step_with_and_without_deform_kernels(name):
    """One training-mode forward and backward of DeviceFeatureNet (batch statistics) from identical state: the three stage outputs and the
    gradient at every parameter (the six biases of test_biases_in_front_of_a_batchnorm apart), deform_kernels True against float64 and
    against deform_kernels False on the same device.  A WARNING: this shows that the switch wires the same step (which tensors get
    gradients, the channel order of the 27 offsets and logits, the layouts), not how accurate the kernel is -- the reference's own float32
    step is a median 4e-3 (relative) from float64 on "ragged", through ReLU flips and batch variances, and the bars are 4 x that recorded
    distance per output.  The tight check is test_kernels_against_float64.  The outputs of DEVICE_TORCH_MISSES, on which the torch route
    on the device misses the bar itself, are held to the bar plus that route's own distance, and to that route within the bar.
    Measured on an MI355X: worst ratio of the others x0.53 ("tiny") and x0.36 ("ragged"); the named ones within x0.17 of a bar from the
    torch route."""
    fx, want = U.fixture(), U.net_expected64(name)
    on, off, sums = _steps(name)
    assert set(on) == set(want) == set(off) and len(sums) == 9
    relaxed = DEVICE_TORCH_MISSES[name]
    assert set(relaxed) <= set(want) and not set(relaxed) & set(U.BN_FED_BIASES)
    worst, missed = 0.0, []
    for k in want:
        if k in U.BN_FED_BIASES:
            continue
        bar = U.BAR_FACTOR * float(fx[f"net_{name}_err_{k}"])
        e, e_off, d = _err(on[k], want[k]), _err(off[k], want[k]), _err(on[k], off[k])
        tag = "  [held to torch on the device]" if k in relaxed else ""
        print(f"step {name} {k}: max |value| {float(want[k].abs().max()):.2e}, kernels {e:.2e} (x{e / bar:.2f}), torch on the device {e_off:.2e} "
              f"(x{e_off / bar:.2f}), between them {d:.2e} (x{d / bar:.2f}), bar {bar:.2e}{tag}")
        if k in relaxed:
            worst = max(worst, d / bar)
            if e > bar + e_off or d > bar:
                missed.append((k, e, e_off, d, bar))
        else:
            worst = max(worst, e / bar)
            if e > bar:
                missed.append((k, e, e_off, d, bar))
    print(f"step {name}: worst ratio x{worst:.2f}")
    assert not missed, missed


# The biases on which the PARENT's torch route, run on the device, misses that limit itself (measured on an MI355X, max over the channels
# of |torch on the device - float64| / limit, the larger of two runs): held to the limit plus that route's own distance, and to that
# route within the limit, the rule of DEVICE_TORCH_MISSES.
DEVICE_TORCH_BIAS_MISSES = {
    "tiny": {"param_out1.1.bias": 1.57, "param_out1.4.bias": 1.27},
    "ragged": {},
}


@pytest.mark.parametrize("name", U.NET_CASES)
def test_biases_in_front_of_a_batchnorm(name):
    """The six DCN biases that sit in front of a BatchNorm have a gradient that is mathematically zero (1e-13 in float64, 1e-5 in
    float32): the sum over the pixels of an upstream gradient that BatchNorm's backward pass has centred.  They are held, per channel, to
    2^-23 sum_p |dy[p,o]| -- one float32 ulp of the sum of magnitudes -- or to their recorded float32 distance if that is larger.

    MEASURED on an MI355X in two runs, max over the channels of error / limit.  "ragged": x0.07 - x0.45 on the six biases in both runs
    (the torch route on the same device x0.08 - x0.40).  "tiny": x0.18 - x0.64 in one run (the torch route x0.22 - x0.36 on four biases,
    x1.57 on `out1.1.bias` and x1.27 on `out1.4.bias`); in the other run x0.19 - x0.50 on five biases and x1.07 on `out1.4.bias` (error
    7.63e-06 against a recorded distance of 7.15e-06, the torch route 4.77e-06 there).  What is measured here is NOISE that the kernel
    does not make: on "tiny" a layer is one tile, d_bias[o] is the double sum of the 24 float32 values dy[:,o] rounded once, i.e. the
    correctly rounded sum of the upstream it is handed; what is left is by how much torch's float32 BatchNorm backward misses a zero sum,
    a draw of the same noise the recorded distance is one draw of, and it changes from run to run on BOTH routes (torch's index scatter
    and d_x add atomically further down).  The limit is kept as the issue sets it; the two biases on which the torch route on the device
    exceeded it are named above and held to that route."""
    fx, want = U.fixture(), U.net_expected64(name)
    on, off, sums = _steps(name)
    relaxed = DEVICE_TORCH_BIAS_MISSES[name]
    assert set(relaxed) <= set(U.BN_FED_BIASES)
    missed = []
    for k in U.BN_FED_BIASES:
        recorded = float(fx[f"net_{name}_err_{k}"])
        ulp = 2.0 ** -23 * sums[k[len("param_"):-len(".bias")]]
        limit = torch.maximum(ulp, torch.full_like(ulp, recorded))
        e, e_off = ((r[k].detach().cpu().double() - want[k]).abs() for r in (on, off))
        d = (on[k].detach().cpu().double() - off[k].detach().cpu().double()).abs()
        ratio, ratio_off, ratio_d = float((e / limit).max()), float((e_off / limit).max()), float((d / limit).max())
        print(f"step {name} {k} [in front of a BatchNorm]: kernels {float(e.max()):.2e} (x{ratio:.2f}), torch on the device {float(e_off.max()):.2e} "
              f"(x{ratio_off:.2f}), between them {float(d.max()):.2e} (x{ratio_d:.2f}), one ulp of the sum of magnitudes {float(ulp.min()):.2e} .. "
              f"{float(ulp.max()):.2e}, recorded {recorded:.2e}{'  [held to torch on the device]' if k in relaxed else ''}")
        if k in relaxed:
            if bool((e > limit + e_off).any()) or ratio_d > 1.0:
                missed.append((k, ratio, ratio_off, ratio_d))
        elif ratio > 1.0:
            missed.append((k, ratio, ratio_off, ratio_d))
    assert not missed, missed


# ---- 8. the loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("match_kernels", [False, True])
def test_fit_estimator_with_deform_kernels(match_kernels, monkeypatch):
    model, batch = EU.fit_model(DEV), EU.fit_batch(DEV)
    seen, routes = [], []
    inner, inner_deform = estimator.focal_loss_bld, mvs.deform_conv3x3

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

    def deform_spy(x, offmask, weight, bias=None):
        routes.append(mvs.deform_gate(x, offmask, weight, bias))
        return inner_deform(x, offmask, weight, bias)
    monkeypatch.setattr(estimator, "focal_loss_bld", spy)
    monkeypatch.setattr(mvs, "deform_conv3x3", deform_spy)
    steps, views = EU.FIT["steps"], EU.FIT["NS"] + 1
    assert model.deform_kernels is False
    history, _ = estimator.fit_estimator(model, [batch], steps=steps, lr=EU.FIT["lr"], deform_kernels=True, match_kernels=match_kernels)
    assert model.deform_kernels is False and model.match_kernels is False and model.fused_readout is False        # all switches restored
    assert len(routes) == 9 * views * steps and all(routes)                      # every deformable layer of every view and step ran the kernels
    got, want, want32 = seen[0]
    assert history[0]["total"] == got[0]
    bar = max(EU.BAR_FACTOR * abs(want32[0] - want[0]), EU.FLOOR * abs(want[0]))            # tests/test_estimator_gpu.py's step-0 bar
    print(f"fit match_kernels={match_kernels} step 0 total: {abs(got[0] - want[0]):.2e}, bar {bar:.2e}; totals {[round(h['total'], 4) for h in history]}")
    assert abs(got[0] - want[0]) <= bar
    assert all(v == v and abs(v) != float("inf") for h in history for v in h.values())
    assert history[-1]["total"] < history[0]["total"]
