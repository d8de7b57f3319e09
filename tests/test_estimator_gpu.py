"""The depth estimator's fine-tuning objective, depth scores and fit loop on the device (csrc/mvsloss.hip, diner_amd/estimator.py) against
the float64 restatement on the host and fixture G32's yardsticks (tests/golden/g32_estimator_loss.npz).

Every case runs on three routes -- "cost" (the fused_readout stage dict), "init" (cost_init + init, both leaves) and "prob" (the
reference's call signature: prob_volume = exp(log_softmax(cost)) formed by torch on the device, FROM_PROB kernels) -- and is held against
the float64 restatement of the same route (which tests/test_estimator_cpu.py holds against the fixture).  The gradient bar is
estimator_util.BAR_FACTOR (4) times the case's recorded distance between the reference's float32 and float64; a scalar's bar is the
larger of 4 x its recorded distance and 2^-23 |value|, what rounding the double sum to the float32 result costs; less1 and less3 are
ratios of counts and must equal the float64 value after that rounding.  No pixel is excluded from anything: the inputs keep their margins
(estimator_util).  The determinism properties are bit-equalities.

Measured on an MI355X (max |kernel - float64| / bar over the six cases, the same on all three routes): total 0.25, depth_loss 0.24, epe
0.25, gradients 0.25 (at 0.25 the kernel's float32 is the reference's float32), depth scores 0.25; fused_readout against the default
route: total 0.01, depth_loss 0.02, epe 0.10; fit step 0's total 1.5e-7 against a bar of 1.7e-6.  DESIGN.md section 8q."""
import pytest
import torch

from diner_amd import estimator, mvs, ops
from tests import estimator_util as U
from tests import mvs_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROUTES = ("cost", "init", "prob")


def _check_scalars(fx, name, got, want, label):
    for k in U.SCALARS:
        g, w = float(got[k]), float(want[k])
        if k in ("less1", "less3"):
            print(f"{label} {k}: {g!r} (float64 {w!r})")
            assert g == float(torch.tensor(w, dtype=torch.float64).to(torch.float32)), (label, k, g, w)
            continue
        e, bar = abs(g - w), U.scalar_bar(fx, name, k, w)
        print(f"{label} {k}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
        assert e <= bar, (label, k, g, w, e, bar)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", list(U.CASES))
def test_cases_against_float64(name, route):
    fx = U.fixture()
    want, want_grad = U.expected(name, route, torch.float64)
    got, got_grad, inputs, leaves = U.run_loss(name, route, device=DEV)
    _check_scalars(fx, name, got, want, f"{name} {route}")
    for key, g in got_grad.items():
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        e = float((g.cpu().double() - want_grad[key]).abs().max())
        bar = U.BAR_FACTOR * float(fx[f"{name}_err_grad_{key}"])
        print(f"{name} {route} grad {key}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar if bar else float('inf') if e else 0.0:.2f})")
        assert e <= bar, (name, route, key, e, bar)
        if route == "init":
            assert torch.equal(leaves[key][0].grad, leaves[key][1].grad)
        if route != "prob" and U.CASES[name]["stages"][0][0] >= 2:
            d, h, w = g.shape[1:]
            assert float(g.reshape(g.shape[0], d, -1)[0, :, U.PIX_UNDERFLOW].abs().max()) == 0.0      # p_g underflows: exactly zero
    # the inputs stay
    for key, s in zip(U.stage_keys(name), U.case_inputs(name)):
        assert torch.equal(leaves[key][0].detach().cpu(), s["cost_init" if route == "init" else "cost"])
        hyp, nan = inputs[key]["depth_values"].cpu(), torch.isnan(s["gt"])
        assert torch.equal(hyp, s["hyp"]) and bool(nan.any())


def _stage_call(s, dev=DEV, gt=None, flip=False, from_prob=False, with_init=False, upstream=1.0):
    """estimator.stage_loss on one stage's inputs -> (result dict, gradient)."""
    t = lambda x: (x.flip(0) if flip else x).to(dev).contiguous()
    vol = t(s["cost_init"] if with_init else s["cost"])
    if from_prob:
        vol = torch.exp(torch.log_softmax(vol, 1))
    vol.requires_grad_(True)
    B = vol.shape[0]
    interval = torch.tensor([2.0 + 0.5 * b for b in range(B)], device=dev)
    r = estimator.stage_loss(vol, t(s["gt"] if gt is None else gt), t(s["mask"]), t(s["hyp"]), init=t(s["init"]) if with_init else None,
                             from_prob=from_prob, weight=1.5, depth_interval=interval.flip(0) if flip else interval)
    (r["term"] * upstream).backward()
    return r, vol.grad


@pytest.mark.parametrize("from_prob", [False, True])
def test_nan_gt_under_zero_mask_adds_nothing(from_prob):
    s = U.case_inputs("ragged")[0]
    assert bool(torch.isnan(s["gt"]).any()) and bool(torch.isinf(s["gt"]).any())
    clean = torch.where(torch.isfinite(s["gt"]), s["gt"], torch.zeros(()))
    a, ga = _stage_call(s, from_prob=from_prob)
    b, gb = _stage_call(s, gt=clean, from_prob=from_prob)
    for k in ("term", "entropy2", "depth_loss", "abs_err", "epe", "under", "depth", "confidence"):
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
    assert bool(torch.isfinite(ga).all()) and torch.equal(ga, gb)


@pytest.mark.parametrize("from_prob", [False, True])
def test_two_runs_same_bits(from_prob):
    s = U.case_inputs("ragged")[0]
    a, ga = _stage_call(s, from_prob=from_prob, with_init=not from_prob)
    b, gb = _stage_call(s, from_prob=from_prob, with_init=not from_prob)
    for k in ("term", "entropy2", "depth_loss", "abs_err", "epe", "under", "depth", "confidence"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(ga, gb)


def test_flipped_batch_gives_flipped_results():
    """An image's sums, depth and gradient do not depend on its place in the batch (the 1 / B of the gradient is the same everywhere)."""
    s = U.case_inputs("ragged")[0]
    t = lambda x, flip: (x.flip(0) if flip else x).to(DEV).contiguous()
    out = []
    for flip in (False, True):
        r = ops.mvs_stage_loss(t(s["cost"], flip), t(s["hyp"], flip), t(s["gt"], flip), t(s["mask"], flip))
        up = torch.ones((), device=DEV)
        g = ops.mvs_stage_loss_grad(t(s["cost"], flip), None, False, t(s["mask"], flip), r["record"], r["factors"], up)
        out.append((r, g))
    (a, ga), (b, gb) = out
    for k in ("depth", "confidence", "record", "factors", "sums"):
        assert torch.equal(a[k], b[k].flip(0)), k
    assert torch.equal(ga, gb.flip(0))
    assert bool((a["sums"][:, 0] > 0).any()) and float(a["sums"][1, 0]) == 0.0           # image 1 is the empty one


def test_upstream_scaling():
    s = U.case_inputs("init")[0]
    _, g1 = _stage_call(s)
    _, g3 = _stage_call(s, upstream=3.0)
    e = (g3.double() - 3.0 * g1.double()).abs()
    assert bool((e <= 2.0 ** -23 * (3.0 * g1.double()).abs()).all()) and float(g1.abs().max()) > 0.0


def test_depth_and_confidence_are_the_readout_kernels():
    s = U.case_inputs("init")[0]
    r, _ = _stage_call(s, with_init=True)
    depth, conf, _ = ops.mvs_select_depth(s["cost_init"].to(DEV), s["hyp"].to(DEV), s["init"].to(DEV), return_prob=False)
    assert torch.equal(r["depth"], depth) and torch.equal(r["confidence"], conf)


@pytest.mark.parametrize("name", list(U.CASES))
def test_depth_scores(name):
    fx = U.fixture()
    inputs, gts, masks, _ = U.loss_inputs(name, "prob", torch.float64, requires_grad=False)
    est64, gt64, m = inputs["stage3"]["depth"], gts["stage3"], masks["stage3"] > 0.5
    est, gt, md = est64.float().to(DEV), gt64.float().to(DEV), m.to(DEV)
    per_image, batch = ops.depth_scores(est, gt, md.float(), U.THRESHOLDS, U.BAND)
    rows = [("abs", 0, estimator.abs_depth_error_metrics_torch(est64[:1], gt64[:1], m[:1])),
            ("band", 1, estimator.abs_depth_error_metrics_torch(est64[:1], gt64[:1], m[:1], U.BAND))]
    rows += [(f"thres{i}", 2 + i, estimator.thres_metrics_torch(est64[:1], gt64[:1], m[:1], t)) for i, t in enumerate(U.THRESHOLDS)]
    for label, col, want in rows:
        g, w = float(per_image[0, col]), float(want)
        assert abs(w - float(fx[f"{name}_scores_f64_{label}"])) <= 1e-12 * abs(w)
        if label.startswith("thres"):
            assert g == float(want.to(torch.float32)), (name, label, g, w)
            continue
        e, bar = abs(g - w), max(U.BAR_FACTOR * float(fx[f"{name}_scores_err_{label}"]), U.FLOOR * abs(w))
        print(f"{name} scores {label}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar if bar else 0.0:.2f})")
        assert e <= bar, (name, label, g, w)
    # the drop-ins return the batch mean, NaN where an image has no valid pixel, as the reference's
    for got, want in ((estimator.abs_depth_error_metrics(est, gt, md), estimator.abs_depth_error_metrics_torch(est64, gt64, m)),
                      (estimator.abs_depth_error_metrics(est, gt, md, U.BAND), estimator.abs_depth_error_metrics_torch(est64, gt64, m, U.BAND)),
                      (estimator.thres_metrics(est, gt, md, U.THRESHOLDS[0]), estimator.thres_metrics_torch(est64, gt64, m, U.THRESHOLDS[0]))):
        if bool(torch.isnan(want)):
            assert bool(torch.isnan(got))
        else:
            assert abs(float(got) - float(want)) <= max(4 * U.FLOOR * abs(float(want)), 1e-30)
    assert torch.equal(batch, ops.depth_scores(est, gt, md.float(), U.THRESHOLDS, U.BAND)[1]) or bool(torch.isnan(batch).any())


def test_entropy_loss_and_trans_mvsnet_loss_drop_ins():
    fx, name = U.fixture(), "three_stage"
    inputs, gts, masks, _ = U.loss_inputs(name, "prob", device=DEV)
    want_in, wg, wm, _ = U.loss_inputs(name, "prob", torch.float64)
    got = estimator.trans_mvsnet_loss(inputs, gts, masks, dlossw=U.CASES[name]["dlossw"])
    want = estimator.trans_mvsnet_loss_torch(want_in, wg, wm, dlossw=U.CASES[name]["dlossw"])
    assert abs(float(got[0].detach()) - float(want[0].detach())) <= U.scalar_bar(fx, name, "total", want[0].detach())
    assert abs(float(got[1]) - float(want[1])) <= U.scalar_bar(fx, name, "depth_loss", want[1])
    assert abs(float(got[2]) - float(want[2])) <= U.scalar_bar(fx, name, "total", want[2])
    assert torch.equal(got[3].cpu().double(), want[3]) and got[0].requires_grad and not got[1].requires_grad
    s3 = inputs["stage3"]
    e, depth, conf = estimator.entropy_loss(s3["prob_volume"], gts["stage3"], masks["stage3"] > 0.5, s3["depth_values"], return_prob_map=True)
    e64, d64, c64 = estimator.entropy_loss_torch(want_in["stage3"]["prob_volume"], wg["stage3"], wm["stage3"] > 0.5,
                                                 want_in["stage3"]["depth_values"], return_prob_map=True)
    assert abs(float(e.detach()) - float(e64)) <= U.scalar_bar(fx, name, "total", e64) and torch.equal(depth.cpu().double(), d64)
    assert float((conf.cpu().double() - c64).abs().max()) <= 4 * U.FLOOR


def test_closed_gate_never_touches_the_kernels(monkeypatch):
    def boom():
        raise AssertionError("the kernels were reached")
    monkeypatch.setattr(estimator, "_ops", boom)
    monkeypatch.setattr(mvs, "_ops", boom)
    name = "sub_wave"
    want, _ = U.expected(name, "cost", torch.float64)
    got, _, _, _ = U.run_loss(name, "cost", torch.float64, device=DEV)              # float64 on the device: the restatement
    for k in U.SCALARS:
        assert abs(float(got[k]) - float(want[k])) <= 1e-12 * max(abs(float(want[k])), 1.0), k
    want32, _ = U.expected(name, "prob", torch.float32)
    got32, _, _, _ = U.run_loss(name, "prob", torch.float32)                       # float32 on the CPU: the restatement
    for k in U.SCALARS:
        assert float(got32[k]) == float(want32[k]), k
    inputs, gts, masks, _ = U.loss_inputs(name, "prob", torch.float64, device=DEV, requires_grad=False)
    m = masks["stage3"] > 0.5
    a = estimator.thres_metrics(inputs["stage3"]["depth"][:1], gts["stage3"][:1], m[:1], 1.5)
    b = estimator.thres_metrics_torch(inputs["stage3"]["depth"][:1].cpu(), gts["stage3"][:1].cpu(), m[:1].cpu(), 1.5)
    assert abs(float(a) - float(b)) <= U.FLOOR * float(b)          # torch's own float32 mean on either device


# ---- the model's fused read-out ---------------------------------------------------------------------------------------------------------
READOUT_CASE = "turned"            # D 8, 23 x 37, three source views, the view weights from the net, with a prob_volume_init


def _depthnet_run(fused, grad=True):
    inp = MU.case_inputs(READOUT_CASE)
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(inp["state_dict"])
    dn = dn.to(DEV).eval()
    dn.fused_readout = fused
    x = MU.cast(dict(features=inp["features"], proj=inp["proj"], depth_values=inp["depth_values"], prob_init=inp["prob_init"]), torch.float32, DEV)
    D = x["depth_values"].shape[1]
    gain = torch.full((), MU.GAIN, device=DEV, requires_grad=True)
    with torch.set_grad_enabled(grad):
        out, weights = dn(x["features"], x["proj"], x["depth_values"], D, lambda s: gain * s, prob_volume_init=x["prob_init"])
    return out, weights, x, gain


def test_fused_readout_off_is_the_parent_route():
    out, weights, x, gain = _depthnet_run(False)
    assert "cost" not in out and out["prob_volume"] is not None
    # the parent's statement of this route, operation by operation
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(MU.case_inputs(READOUT_CASE)["state_dict"])
    dn = dn.to(DEV).eval()
    sim, w = mvs.cost_volume_torch(x["features"], x["proj"], x["depth_values"], dn.pixel_wise_net, None)
    depth, conf, prob = mvs.select_depth_torch((gain * sim).squeeze(1), x["depth_values"], x["prob_init"])
    assert torch.equal(out["depth"], depth) and torch.equal(out["photometric_confidence"], conf.detach())
    assert torch.equal(out["prob_volume"], prob) and torch.equal(weights, w.detach())


def test_fused_readout_loss_equals_the_default_route():
    a, _, x, gain_a = _depthnet_run(True)
    b, _, _, gain_b = _depthnet_run(False)
    assert a["prob_volume"] is None and a["cost"].requires_grad and a["cost"].shape == b["prob_volume"].shape
    B, D, H, W = a["cost"].shape
    g = torch.Generator().manual_seed(3260)
    idx = torch.randint(0, D, (B, 1, H, W), generator=g).to(DEV)
    gt = torch.gather(x["depth_values"], 1, idx).squeeze(1)
    mask = (torch.rand(B, H, W, generator=g) < 0.8).float().to(DEV)
    interval = float((x["depth_values"][0, 1, 0, 0] - x["depth_values"][0, 0, 0, 0]).cpu()) if D > 1 else 1.0
    res = []
    for out, gain in ((a, gain_a), (b, gain_b)):
        r = estimator.focal_loss_bld({"stage3": out}, {"stage3": gt}, {"stage3": mask}, interval)
        r[0].backward()
        res.append(([float(t.detach()) for t in r], float(gain.grad)))
    # the yardstick: the float64 restatement from the cost, and what the float32 restatement on the host keeps from it
    host = lambda dt: ({"stage3": {k: (v.detach().cpu().to(dt) if torch.is_tensor(v) else v) for k, v in a.items()}},
                       {"stage3": gt.cpu().to(dt)}, {"stage3": mask.cpu().to(dt)}, interval)
    want, want32 = estimator.focal_loss_bld_torch(*host(torch.float64)), estimator.focal_loss_bld_torch(*host(torch.float32))
    for i, k in enumerate(U.SCALARS):
        w = float(want[i])
        bar = max(U.BAR_FACTOR * abs(float(want32[i]) - w), U.FLOOR * abs(w))
        for label, (r, _) in zip(("fused", "default"), res):
            if k.startswith("less"):
                assert r[i] == float(want[i].to(torch.float32)), (k, r[i], w)
                continue
            print(f"fused_readout {label} {k}: {abs(r[i] - w):.2e}, bar {bar:.2e} (x{abs(r[i] - w) / bar:.2f})")
            assert abs(r[i] - w) <= bar, (label, k, r[i], w)
    # the same gradient reaches the regulariser: two float32 sums of 1e4 signed terms each
    assert abs(res[0][1] - res[1][1]) <= 1e-4 * abs(res[1][1]) and res[1][1] != 0.0


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
def test_fit_estimator_on_the_device(monkeypatch):
    model, batch = U.fit_model(DEV), U.fit_batch(DEV)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    seen, flushes = [], []
    inner = estimator.focal_loss_bld

    def spy(inputs, depth_gt_ms, mask_ms, depth_interval, **kw):
        out = inner(inputs, depth_gt_ms, mask_ms, depth_interval, **kw)
        if not seen:
            assert all(inputs[k]["prob_volume"] is None and "cost" in inputs[k] for k in ("stage1", "stage2", "stage3"))
            def host(d, dt):
                return {k: (host(v, dt) if isinstance(v, dict) else v.detach().cpu().to(dt) if torch.is_tensor(v) else v) for k, v in d.items()}
            restated = [[float(t) for t in estimator.focal_loss_bld_torch(host(inputs, dt), host(depth_gt_ms, dt), host(mask_ms, dt),
                                                                          depth_interval.cpu().to(dt), **kw)]
                        for dt in (torch.float64, torch.float32)]
            seen.append(([float(t.detach()) for t in out], *restated))
        return out
    monkeypatch.setattr(estimator, "focal_loss_bld", spy)
    steps, log_every = U.FIT["steps"], 4
    history, opt = estimator.fit_estimator(model, [batch], steps=steps, lr=U.FIT["lr"], log_every=log_every, on_log=flushes.append)
    from diner_amd.optim import DeviceAdam
    assert isinstance(opt, DeviceAdam) and model.fused_readout is False
    assert len(history) == steps and [h["step"] for h in history] == list(range(steps))
    assert all(all(v == v and abs(v) != float("inf") for v in h.values()) for h in history)
    assert [len(f) for f in flushes] == [log_every, steps - log_every]              # one read-back of the ring per log_every steps
    got, want, want32 = seen[0]
    assert history[0]["total"] == got[0]
    bar = max(U.BAR_FACTOR * abs(want32[0] - want[0]), U.FLOOR * abs(want[0]))      # the scalar bar, the float32 restatement's own distance
    print(f"fit step 0 total: {abs(got[0] - want[0]):.2e}, bar {bar:.2e}; totals {[round(h['total'], 4) for h in history]}")
    assert abs(got[0] - want[0]) <= bar
    after = model.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before if before[k].is_floating_point())
    assert history[-1]["total"] < history[0]["total"]
    assert opt.stats()["skipped"] == 0
