"""The matching stage's backward pass on the device: diner_mvs_similarity_f32 / diner_mvs_similarity_grad_f32 (csrc/mvs.hip) through
mvs.match_similarity, mvs.cost_volume_train, DeviceDepthNet.match_kernels and fit_estimator(match_kernels=True).

The yardstick is the float64 torch restatement on the host (which tests/test_match_grad_cpu.py holds against fixture G33); the bar is
mvs_util.BAR_FACTOR (4) times the distance the reference's own float32 autograd keeps from float64 on the same case and output, as the
fixture records it.  Shapes: mvs_util's six cases (23 x 37: a ragged tail and less than a workgroup; D 200: 16 pixels a workgroup; D 1
with 15 views; C 32; a camera looking away; a band half outside) and the three stages of its 24 x 40 run.

Measured on an MI355X (max |kernel - float64| / bar over the cases): see DESIGN.md section 8r."""
import numpy as np
import pytest
import torch

from diner_amd import estimator, mvs, ops
from tests import estimator_util as EU
from tests import match_grad_util as U
from tests import mvs_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ---- 1. forward and both gradients against float64 ---------------------------------------------------------------------------------------
# The outputs on which the PARENT's torch route, run on the device, misses the fixture's bar by itself (measured on an MI355X, max |torch on
# the device - float64| over the bar).  All of them run back through the pixelwise module's second BatchNorm in training mode, torch's own
# device operations on both routes.  "turned": one view's similarity is constant 0, so conv1's output is constant per channel, its batch
# variance is 0 up to the rounding of the mean, and the division by sqrt(var + eps) carries that rounding 300-fold into everything from
# conv1 on and into d_ref.  "probe": one sum of 1e5 terms whose order on the device is not the host's.
DEVICE_TORCH_MISSES = {
    ("turned", "cv"): {"d_ref": 1.40, "param_conv1.conv.weight": 4.11, "param_conv1.bn.weight": 36.2, "param_conv1.bn.bias": 6.00,
                       "param_conv2.weight": 2.97, "param_conv2.bias": 4.48},
    ("probe", "cv"): {"param_conv1.conv.weight": 1.10},
}


@pytest.mark.parametrize("run", ["sim", "cv"])
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_kernels_against_float64(name, run):
    """"sim": the per-view upstream.  "cv": the aggregated upstream -- on the given-weights cases (deep, shifted, stage2, stage3) the
    aggregated form of the gradient kernel behind diner_mvs_cost_volume_f32; elsewhere match_similarity under the pixelwise module in
    training mode, the pixelwise parameters' gradients included.  Every output of every case is held to the fixture's bar against
    float64, no element excluded -- except the few of DEVICE_TORCH_MISSES, where the torch route on the device misses that bar itself:
    those are held to the bar plus the torch route's own distance, and to the torch route on the same device within the bar."""
    fx, inp = U.fixture(), U.inputs(name)
    assert mvs.match_gate(MU.cast(inp["features"], torch.float32, DEV), inp["proj"].to(DEV), inp["depth_values"].to(DEV))
    runner, torch_fn = (U.run_sim, mvs.match_similarity_torch) if run == "sim" else (U.run_cv, mvs.cost_volume_torch)
    got = U.outputs(runner(inp, torch.float32, DEV))
    on_device = U.outputs(runner(inp, torch.float32, DEV, fn=torch_fn))             # the torch route on the same device
    want = U.outputs(U.expected64(name, run))
    zero = set(fx[f"{name}_{run}_zero"].tolist())
    relaxed = DEVICE_TORCH_MISSES.get((name, run), {})
    assert set(got) == set(want) and set(relaxed) <= set(want)
    worst, missed = 0.0, []
    for key in want:
        assert got[key].shape == want[key].shape and got[key].dtype == torch.float32 and got[key].is_cuda
        if key in zero:
            assert not bool(got[key].any()), (name, run, key)
            continue
        bar = U.bar(fx, name, run, key)
        e, e_dev, d = _err(got[key], want[key]), _err(on_device[key], want[key]), _err(got[key], on_device[key])
        print(f"{name} {run} {key}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}); torch on the device {e_dev:.2e} (x{e_dev / bar:.2f}); "
              f"kernel against torch on the device {d:.2e} (x{d / bar:.2f}){'  [relaxed]' if key in relaxed else ''}")
        worst = max(worst, e / bar)
        if key in relaxed:
            if e > bar + e_dev or d > bar:
                missed.append((key, e, e_dev, d, bar))
        elif e > bar:
            missed.append((key, e, e_dev, d, bar))
    print(f"{name} {run}: worst ratio over all outputs x{worst:.2f}")
    assert not missed, (name, run, missed)


# ---- 2. a view that sees nothing ---------------------------------------------------------------------------------------------------------
def test_turned_view_takes_and_gives_nothing():
    inp = U.inputs("turned")
    res = U.run_sim(inp, torch.float32, DEV)
    assert not bool(res["d_src"][MU.SPECIAL_VIEW].any()) and not bool(res["similarity"][:, MU.SPECIAL_VIEW].any())
    only = torch.zeros_like(inp["G"])
    only[:, MU.SPECIAL_VIEW] = inp["G"][:, MU.SPECIAL_VIEW]
    alone = U.run_sim(inp, torch.float32, DEV, upstream=only)
    assert not bool(alone["d_ref"].any()) and all(not bool(g.any()) for g in alone["d_src"])
    rest = U.run_sim(inp, torch.float32, DEV, upstream=inp["G"] - only)
    assert torch.equal(rest["d_ref"], res["d_ref"])                  # d_ref's sum order is fixed, and the turned view adds no term to it


# ---- 3. nothing in, nothing out ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,run", [("probe", "sim"), ("shifted", "cv"), ("deep", "cv")])
def test_zero_upstream_gives_zero_gradients(name, run):
    inp = U.inputs(name)
    res = (U.run_sim if run == "sim" else U.run_cv)(inp, torch.float32, DEV, upstream=torch.zeros_like(inp["G" if run == "sim" else "g"]))
    assert not bool(res["d_ref"].any()) and all(not bool(g.any()) for g in res["d_src"])
    assert bool(res["similarity"].any())


# ---- 4. bits -----------------------------------------------------------------------------------------------------------------------------
def _channels_last(inp, flip=False):
    cl = torch.stack(inp["features"], 0).permute(0, 1, 3, 4, 2).contiguous().to(DEV)
    x = dict(ref=cl[0], src=cl[1:], proj=inp["proj"].to(DEV), depth=inp["depth_values"].to(DEV), G=inp["G"].to(DEV),
             g=inp["g"].squeeze(1).to(DEV), vw=None if inp["view_weights"] is None else inp["view_weights"].to(DEV))
    if flip:
        x = {k: (None if v is None else v.flip(1 if k == "src" else 0).contiguous()) for k, v in x.items()}
    return x


@pytest.mark.parametrize("name", ["deep", "shifted"])
def test_similarity_is_what_the_cost_volume_kernel_aggregates(name):
    """The existing kernel's result equals, bit for bit, the aggregation of diner_mvs_similarity_f32's output formed elementwise in that
    kernel's order -- acc = acc + s_v w_v view by view from 0, wsum = 1e-5 + w_0 + w_1 ..., acc / wsum -- in IEEE float32 on the host."""
    x = _channels_last(U.inputs(name))
    agg, _ = ops.mvs_cost_volume(x["ref"], x["src"], x["proj"], x["depth"], None, x["vw"])
    s, hom = ops.mvs_similarity(x["ref"], x["src"], x["proj"], x["depth"])
    s, w = s.cpu(), x["vw"].cpu()
    acc, wsum = torch.zeros_like(s[:, 0]), torch.full_like(w[:, 0], 1e-5)
    for v in range(s.shape[1]):
        acc = acc + s[:, v] * w[:, v].unsqueeze(1)
        wsum = wsum + w[:, v]
    assert torch.equal(agg.cpu(), acc / wsum.unsqueeze(1))


@pytest.mark.parametrize("name", ["probe", "deep", "wide"])
def test_two_runs_and_a_flipped_batch_give_the_same_bits(name):
    """The similarity and d_ref: torch.equal between two runs, and a flipped batch gives the flipped bits.  d_src is summed by float
    atomic adds, so its sum order is not fixed: it is held to the bar only (test_kernels_against_float64)."""
    outs = []
    for flip in (False, False, True):
        x = _channels_last(U.inputs(name), flip)
        s, hom = ops.mvs_similarity(x["ref"], x["src"], x["proj"], x["depth"])
        d_ref, d_src = ops.mvs_similarity_grad(x["ref"], x["src"], hom, x["depth"], grad_views=x["G"])
        res = [s, d_ref]
        if x["vw"] is not None:
            res.append(ops.mvs_similarity_grad(x["ref"], x["src"], hom, x["depth"], grad_aggregated=x["g"], view_weights=x["vw"])[0])
        outs.append(res)
    for a, b, c in zip(*outs):
        assert bool(a.any()) and torch.equal(a, b) and torch.equal(a, c.flip(0))


# ---- 5. DeviceDepthNet in training mode, match_kernels True against False ------------------------------------------------------------------
STEP = dict(image=(32, 64), nd=8, seed=3321)


def _step_inputs():
    """The three-stage construction of mvs_util.stage_inputs() at the smallest sizes a real CostRegNet takes: the 3-D U-Net's skip additions
    need D, H and W to be multiples of 8 at every stage (the reference fails otherwise), which the 24 x 40 run's 6 x 10 x 8, 12 x 20 x 4 and
    24 x 40 x 2 volumes are not.  So: image 32 x 64, stages of 8 x 16, 16 x 32 and 32 x 64 px with 32 / 16 / 8 channels, 8 planes each; stage 1
    computes the view weights, stages 2 and 3 take them nearest-upsampled, as TransMVSNet.forward does.  The hypotheses are fixed planes
    plus a per-pixel offset, not the previous stage's winner: an argmax that a rounding flips would otherwise send the two routes to
    different hypotheses, which is no property of the code under test."""
    s = MU.STAGES
    rng = np.random.default_rng(STEP["seed"])
    B, NS, (H, W), nd = s["B"], s["NS"], STEP["image"], STEP["nd"]
    E, K = MU.make_cameras(rng, B, NS, (H, W), None, focal=MU.FOCAL * 4, shift=s["shift"], turn=s["turn"])
    stages = []
    for C, sc in zip(s["channels"], s["scales"]):
        Ks = K.copy()
        Ks[:, :, :2, :] /= sc
        h, w = H // sc, W // sc
        f = MU.plane_features(E, Ks, (h, w), C, rng)
        depth = np.linspace(*s["depth_range"], nd).reshape(1, nd, 1, 1) + rng.uniform(0.0, 0.03, (B, 1, h, w))
        gt = 1.5 + 0.2 * rng.uniform(-1.0, 1.0, (B, h, w))
        stages.append(dict(features=[torch.from_numpy(v).float() for v in f], proj=torch.from_numpy(MU.proj_pairs(E, Ks)).float(),
                           depth=torch.from_numpy(depth).float(), gt=torch.from_numpy(gt).float(),
                           mask=torch.from_numpy((rng.uniform(size=(B, h, w)) < 0.8).astype(np.float32))))
    return stages, MU.pixelwise_state_dict(STEP["seed"] + 50)


def _depthnet_step(stages, state_dict, dtype, device, match_kernels, fused):
    torch.manual_seed(STEP["seed"])
    reg = mvs.DeviceCostRegNet(1, 8)
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(state_dict)
    reg, dn = reg.to(dtype=dtype, device=device).train(), dn.to(dtype=dtype, device=device).train()
    dn.match_kernels, dn.fused_readout = match_kernels, fused
    outputs, gts, masks, leaves, weights = {}, {}, {}, [], None
    for i, st in enumerate(stages):
        key = f"stage{i + 1}"
        x = MU.cast(st, dtype, device)
        feats = [f.clone().requires_grad_(True) for f in x["features"]]
        leaves.extend(feats)
        if weights is None:
            out, weights = dn(feats, x["proj"], x["depth"], STEP["nd"], reg)
        else:
            weights = torch.nn.functional.interpolate(weights, scale_factor=2, mode="nearest")
            out = dn(feats, x["proj"], x["depth"], STEP["nd"], reg, view_weights=weights)
        outputs[key], gts[key], masks[key] = out, x["gt"], x["mask"]
    total = estimator.focal_loss_bld(outputs, gts, masks, 0.7 / 8 / 2)[0]
    total.backward()
    res = {"total": total.detach().reshape(1)}
    for j, f in enumerate(leaves):
        res[f"feature{j}"] = f.grad
    for k, p in list(dn.pixel_wise_net.named_parameters()) + [("reg." + k, p) for k, p in reg.conv0.named_parameters()]:
        res["grad_" + k] = p.grad
    for k, v in list(dn.state_dict().items()) + [("reg." + k, v) for k, v in reg.state_dict().items()]:
        if "running" in k:
            res["stat_" + k] = v.detach().clone()
    return res


def _host_steps(monkeypatch, stages, sd):
    """The step's yardsticks on the host -> (float64 results, bars).  A training step is not continuous in the similarity: a ReLU of the
    regulariser or the arg max of the view weight that a last-bit change flips re-routes gradients, and a similarity perturbed by 1e-6 moves
    the regulariser's weight gradient by 1e-3 in float64 (measured on this step).  So test_kernels_against_float64's bars are scaled the
    way the step itself scales them: bar_s, BAR_FACTOR x the distance the float32 torch route's similarity keeps from float64's at each
    stage (that test's rule), is applied to the float64 step's similarities with seeded random signs, and a quantity's bar is how far
    that moves it, plus BAR_FACTOR x its own float32 distance (for the loss total at least one float32 ulp)."""
    inner = mvs.cost_volume_torch

    def run(dtype, perturb=None):
        sims, gen = [], torch.Generator().manual_seed(STEP["seed"] + 1)

        def wrapped(*a, **k):
            s, w = inner(*a, **k)
            sims.append(s.detach())
            if perturb is not None:
                s = s + perturb[len(sims) - 1] * (2 * torch.randint(0, 2, s.shape, generator=gen).to(s.dtype) - 1)
            return s, w
        with monkeypatch.context() as m:
            m.setattr(mvs, "cost_volume_torch", wrapped)
            return _depthnet_step(stages, sd, dtype, None, False, False), sims
    want, sims64 = run(torch.float64)
    host32, sims32 = run(torch.float32)
    bar_s = [U.BAR_FACTOR * _err(a, b) for a, b in zip(sims32, sims64)]
    moved, _ = run(torch.float64, bar_s)
    bars = {k: U.BAR_FACTOR * _err(host32[k], want[k]) + _err(moved[k], want[k]) for k in want}
    bars["total"] = max(bars["total"], EU.FLOOR * float(want["total"].abs()))
    return want, bars, bar_s


@pytest.mark.parametrize("fused", [False, True])
def test_depthnet_training_step_with_and_without_match_kernels(fused, monkeypatch):
    """One training step of DeviceDepthNet + a real DeviceCostRegNet(1, 8) over three stages from identical state: the loss total, the
    gradients at every feature map, at the pixel_wise_net parameters and at the regulariser's first layer, and every BatchNorm running
    statistic after the step.  match_kernels True is held to float64, and to match_kernels False on the same device, within the bars of
    _host_steps.  Those bars are generous -- every element of the similarity is moved by the full 4 x error at once -- so this test shows
    that the switch wires the same step (scales, view order, which tensors get gradients, the statistics' updates); the tight check of
    the gradient kernel itself is test_kernels_against_float64's "sim" run and its given-weights "cv" run."""
    stages, sd = _step_inputs()
    want, bars, bar_s = _host_steps(monkeypatch, stages, sd)
    on = _depthnet_step(stages, sd, torch.float32, DEV, True, fused)
    off = _depthnet_step(stages, sd, torch.float32, DEV, False, fused)
    assert set(on) == set(want) and len([k for k in want if k.startswith("feature")]) == 12
    print(f"step fused={fused}: similarity bars per stage {[f'{b:.2e}' for b in bar_s]}")
    worst, missed = 0.0, []
    for k in want:
        bar, size = bars[k], float(want[k].abs().max())
        e, e_off, d = _err(on[k], want[k]), _err(off[k], want[k]), _err(on[k], off[k])
        worst = max(worst, max(e, d) / bar if bar else float("inf"))
        print(f"step fused={fused} {k}: max |value| {size:.2e}, kernels {e:.2e} (x{e / bar:.2f}), torch on the device {e_off:.2e} "
              f"(x{e_off / bar:.2f}), between them {d:.2e} (x{d / bar:.2f}), bar {bar:.2e}")
        if not (bar > 0.0 and e <= bar and d <= bar):
            missed.append((k, e, e_off, d, bar))
    print(f"step fused={fused}: worst ratio x{worst:.2f}")
    assert not missed, missed


# ---- 6. the loop -------------------------------------------------------------------------------------------------------------------------
def test_fit_estimator_with_match_kernels(monkeypatch):
    model, batch = EU.fit_model(DEV), EU.fit_batch(DEV)
    seen, routes = [], []
    inner, inner_train = estimator.focal_loss_bld, mvs.cost_volume_train

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

    def train_spy(features, proj_matrices, depth_values, pixelwise_net=None, view_weights=None):
        routes.append(mvs.match_gate(features, proj_matrices, depth_values, view_weights))
        return inner_train(features, proj_matrices, depth_values, pixelwise_net, view_weights)
    monkeypatch.setattr(estimator, "focal_loss_bld", spy)
    monkeypatch.setattr(mvs, "cost_volume_train", train_spy)
    steps = EU.FIT["steps"]
    assert model.match_kernels is False
    history, _ = estimator.fit_estimator(model, [batch], steps=steps, lr=EU.FIT["lr"], match_kernels=True)
    assert model.match_kernels is False and model.fused_readout is False                  # both switches restored
    assert len(routes) == 3 * steps and all(routes)                                         # every stage of every step ran the kernels
    got, want, want32 = seen[0]
    assert history[0]["total"] == got[0]
    bar = max(EU.BAR_FACTOR * abs(want32[0] - want[0]), EU.FLOOR * abs(want[0]))            # tests/test_estimator_gpu.py's step-0 bar
    print(f"fit step 0 total: {abs(got[0] - want[0]):.2e}, bar {bar:.2e}; totals {[round(h['total'], 4) for h in history]}")
    assert abs(got[0] - want[0]) <= bar
    assert all(v == v and abs(v) != float("inf") for h in history for v in h.values())
    assert history[-1]["total"] < history[0]["total"]


# ---- 7. the closed gate and the default ---------------------------------------------------------------------------------------------------
def _forward(dn, inp, dtype=torch.float32, channels=None):
    x = MU.cast(dict(features=inp["features"], proj=inp["proj"], depth=inp["depth_values"]), dtype, DEV)
    feats = [f[:, :channels].contiguous() for f in x["features"]] if channels else x["features"]
    with torch.enable_grad():
        out, weights = dn(feats, x["proj"], x["depth"], x["depth"].shape[1], MU.regulariser)
    return [out["prob_volume"].detach(), out["depth"], out["photometric_confidence"], weights]


def test_closed_gate_and_default_off(monkeypatch):
    inp = U.inputs("probe")
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(inp["state_dict"])
    dn = dn.to(DEV).eval()
    before = _forward(dn, inp)                                       # the switch has never been touched
    calls = []
    inner = ops.mvs_similarity
    monkeypatch.setattr(ops, "mvs_similarity", lambda *a, **k: calls.append(1) or inner(*a, **k))
    dn.match_kernels = True
    on = _forward(dn, inp)
    assert calls == [1] and on[0].shape == before[0].shape           # the kernels ran
    closed = [_forward(dn, inp, torch.float32, channels=6), _forward(dn.double(), inp, torch.float64)]
    assert calls == [1]                                               # C = 6 and float64 never reach them
    dn.match_kernels = False
    open_ = [_forward(dn.float(), inp, torch.float32, channels=6), _forward(dn.double(), inp, torch.float64)]
    for a, b in zip(closed, open_):
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    after = _forward(dn.float(), inp)
    assert all(torch.equal(p, q) for p, q in zip(before, after))
