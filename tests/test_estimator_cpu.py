"""The host side of the depth estimator's fine-tuning (diner_amd/estimator.py) without a device: the torch restatement of the objective
and the scores against fixture G32 (tests/golden/g32_estimator_loss.npz: the reference's own float32 results and the float64 values the
generator found equal to the reference in float64), the inputs' margins, the planted cases' exact values, the schedule, the module's
state-dict keys, checkpoints, the fit loop with torch.optim.Adam, and the argument checks."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from diner_amd import _lib, estimator, mvs
from tests import estimator_util as U

ROOT = U.ROOT
NEW_SYMBOLS = ("diner_mvs_loss_partial_doubles", "diner_mvs_stage_loss_f32", "diner_mvs_loss_finish_f32", "diner_mvs_stage_loss_grad_f32",
               "diner_depth_scores_f32")


def test_new_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    assert re.search(r"#define DINER_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.diner_abi_version() == 6
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and hasattr(lib, name), name
    for macro, value in (("DINER_MVS_LOSS_SLOTS", _lib.MVS_LOSS_SLOTS), ("DINER_MVS_LOSS_MAX_THRESHOLDS", _lib.MVS_LOSS_MAX_THRESHOLDS),
                         ("DINER_MVS_LOSS_SCALARS", _lib.MVS_LOSS_SCALARS), ("DINER_DEPTH_SCORES", _lib.DEPTH_SCORES)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    lib.diner_mvs_loss_partial_doubles.restype = ctypes.c_size_t
    assert lib.diner_mvs_loss_partial_doubles(3, 17, 23) == 3 * 2 * 16 and lib.diner_mvs_loss_partial_doubles(0, 4, 4) == 0


@pytest.mark.parametrize("name", list(U.CASES))
def test_float64_restatement_matches_the_fixture(name):
    fx = U.fixture()
    c = U.CASES[name]
    assert int(fx[f"{name}_seed"]) == c["seed"] and fx[f"{name}_shapes"].tolist() == [[c["B"], *s] for s in c["stages"]]
    scalars, grads = U.expected(name, U.fixture_route(name), torch.float64)
    for k in U.SCALARS:
        want = float(fx[f"{name}_f64_{k}"])
        assert abs(float(scalars[k]) - want) <= 1e-12 * abs(want), (name, k)
    for key, g in grads.items():
        want = torch.from_numpy(fx[f"{name}_f64_grad_{key}"])
        assert float((g - want).abs().max()) <= 1e-12 * float(want.abs().max()) or float(want.abs().max()) == 0.0, (name, key)


@pytest.mark.parametrize("name", list(U.CASES))
def test_float32_restatement_is_within_the_reference_float32s_distance(name):
    fx = U.fixture()
    scalars, grads = U.expected(name, U.fixture_route(name), torch.float32)
    for k in U.SCALARS:
        e, bar = abs(float(scalars[k]) - float(fx[f"{name}_f64_{k}"])), U.BAR_FACTOR * float(fx[f"{name}_err_{k}"])
        assert e <= bar, (name, k, e, bar)
    for key, g in grads.items():
        e = float((g.double() - torch.from_numpy(fx[f"{name}_f64_grad_{key}"])).abs().max())
        assert e <= U.BAR_FACTOR * float(fx[f"{name}_err_grad_{key}"]), (name, key, e)


@pytest.mark.parametrize("name", list(U.CASES))
def test_inputs_keep_their_margins(name):
    """No pixel has to be excluded from any comparison: on the float64 values every valid pixel's ground-truth plane is nearest by 0.1
    spacing (or is the planted tie), the winner leads by 6, and no error lies within MARGIN of a threshold or band edge."""
    B = U.CASES[name]["B"]
    unit = (U.case_interval(name).double() * 1.5).view(B, 1, 1)
    for s in U.case_inputs(name):
        hyp, gt, valid, cost = s["hyp"].double(), s["gt"].double(), s["mask"] > 0.5, s["cost"].double()
        D = hyp.shape[1]
        assert bool(torch.isfinite(gt[valid]).all()) and not bool(torch.isfinite(gt).all())
        assert bool(valid[0].any()) and (B == 1 or not bool(valid[1].any()))
        dist = (hyp - gt.unsqueeze(1)).abs()
        assert torch.equal(dist.argmin(1)[valid], s["idx"][valid])
        if D >= 2:
            top2 = dist.topk(2, dim=1, largest=False)[0]
            gap = (top2[:, 1] - top2[:, 0]) / (hyp[:, 1] - hyp[:, 0])
            tie = torch.zeros_like(valid)
            tie.view(B, -1)[0, U.PIX_TIE] = True
            assert float(gap[valid & ~tie].min()) >= 0.1 and float(gap.view(B, -1)[0, U.PIX_TIE]) == 0.0
            ctop = cost.topk(2, dim=1)[0]
            assert float((ctop[:, 0] - ctop[:, 1]).min()) >= 6.0 - 1e-5
        assert torch.equal(cost.argmax(1), s["winner"])
        err = (torch.gather(hyp, 1, s["winner"].unsqueeze(1)).squeeze(1) - gt).abs()[valid]
        scaled = (err.new_zeros(valid.shape).masked_scatter(valid, err) / unit)[valid]
        for e in U.SCALED_EDGES:
            assert float((scaled - e).abs().min()) >= U.MARGIN
        for e in U.ABS_EDGES:
            assert float((err - e).abs().min()) >= U.MARGIN


def _single(dtype, D=8, **over):
    s = {k: v.clone() for k, v in U.stage_inputs(1, D, 6, 9, 3290).items()}
    s.update(over)
    cost = s["cost"].to(dtype).requires_grad_(True)
    inputs = {"stage3": {"cost": cost, "prob_volume": None, "depth_values": s["hyp"].to(dtype),
                         "depth": torch.gather(s["hyp"], 1, s["cost"].argmax(1, keepdim=True)).squeeze(1).to(dtype)}}
    return inputs, {"stage3": s["gt"].to(dtype)}, {"stage3": s["mask"].to(dtype)}, cost, s


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_planted_cases_give_their_exact_values(dtype):
    inputs, gts, masks, cost, s = _single(dtype)
    total, depth_loss, epe, less1, less3 = estimator.focal_loss_bld(inputs, gts, masks, 2.0)
    total.backward()
    prob = estimator.stage_prob_volume(inputs["stage3"]).detach()
    flat = lambda t: t.reshape(t.shape[0], -1) if t.dim() == 3 else t.reshape(t.shape[0], t.shape[1], -1)
    # the underflow pixel: p_g is exactly 0 in float32 (1e-87 in float64), ce = -log(1e-6), the gradient exactly 0 in float32
    g = int(flat(s["idx"])[0, U.PIX_UNDERFLOW])
    pg = float(flat(prob)[0, g, U.PIX_UNDERFLOW])
    assert (pg == 0.0) if dtype == torch.float32 else (0.0 < pg < 1e-80)
    ce = -torch.log(flat(prob)[0, g, U.PIX_UNDERFLOW] + 1e-6)
    assert float(ce) == float(-torch.log(torch.tensor(1e-6, dtype=dtype)))
    column = flat(cost.grad)[0, :, U.PIX_UNDERFLOW]
    assert (float(column.abs().max()) == 0.0) if dtype == torch.float32 else (float(column.abs().max()) < 1e-70)
    # the tie: the first index wins
    dist = (s["hyp"].to(dtype) - s["gt"].to(dtype).unsqueeze(1)).abs()
    d0, d1 = flat(dist)[0, :, U.PIX_TIE].topk(2, largest=False)[0]
    assert float(d0) == float(d1) and int(flat(dist.argmin(1))[0, U.PIX_TIE]) == int(flat(s["idx"])[0, U.PIX_TIE])
    # unmasked pixels: zero gradient, NaN / inf gt notwithstanding
    off = flat(s["mask"])[0] < 0.5
    assert bool(off[U.PIX_NAN]) and bool(off[U.PIX_INF]) and float(flat(cost.grad)[0][:, off].abs().max()) == 0.0
    assert all(math.isfinite(float(t.detach())) for t in (total, depth_loss, epe, less1, less3))
    assert total.requires_grad and not any(t.requires_grad for t in (depth_loss, epe, less1, less3))


def test_an_empty_image_adds_zero_and_an_empty_batch_has_nan_depth_loss():
    two = U.case_inputs("sub_wave")[0]
    hyp, gt, mask, cost = two["hyp"], two["gt"], two["mask"] > 0.5, two["cost"]
    prob = torch.exp(torch.log_softmax(cost, 1))
    both, _ = estimator.entropy_loss(prob, gt, mask, hyp)
    first, _ = estimator.entropy_loss(prob[:1], gt[:1], mask[:1], hyp[:1])
    assert not bool(mask[1].any()) and float(both) == float(first) / 2             # mean over two images, the second adds exactly 0
    inputs, gts, masks, _, _ = _single(torch.float32, mask=torch.zeros(1, 6, 9))
    total, depth_loss, epe, _, _ = estimator.focal_loss_bld(inputs, gts, masks, 2.0)
    assert float(total.detach()) == 0.0 and math.isnan(float(depth_loss)) and math.isnan(float(epe))
    assert float(estimator.abs_depth_error_metrics(gt[1:], gt[1:].nan_to_num(0.0, 0.0), mask[1:], (0.5, 6.0))) == 0.0
    assert math.isnan(float(estimator.thres_metrics(gt[1:], gt[1:], mask[1:], 1.0)))


def test_depth_interval_is_applied_per_image():
    inputs, gts, masks, _ = U.loss_inputs("ragged", "prob", requires_grad=False)
    interval = U.case_interval("ragged")
    whole = estimator.focal_loss_bld(inputs, gts, masks, interval)
    num, cnt = 0.0, 0.0
    for b in range(3):
        n = float((masks["stage3"][b] > 0.5).sum())
        if n:
            one = estimator.focal_loss_bld({"stage3": {k: v[b:b + 1] for k, v in inputs["stage3"].items() if v is not None}},
                                           {"stage3": gts["stage3"][b:b + 1]}, {"stage3": masks["stage3"][b:b + 1]}, float(interval[b]))
            num, cnt = num + n * float(one[2]), cnt + n
    assert abs(float(whole[2]) - num / cnt) <= 1e-6 * num / cnt
    with pytest.raises(ValueError):
        estimator.focal_loss_bld(inputs, gts, masks, torch.ones(2))


def test_scores_match_the_fixture():
    fx = U.fixture()
    for name in U.CASES:
        inputs, gts, masks, _ = U.loss_inputs(name, "prob", torch.float64, requires_grad=False)
        est, gt, m = inputs["stage3"]["depth"][:1], gts["stage3"][:1], masks["stage3"][:1] > 0.5
        got = {"abs": estimator.abs_depth_error_metrics(est, gt, m), "band": estimator.abs_depth_error_metrics(est, gt, m, U.BAND)}
        got.update({f"thres{i}": estimator.thres_metrics(est, gt, m, t) for i, t in enumerate(U.THRESHOLDS)})
        for label, v in got.items():
            want = float(fx[f"{name}_scores_f64_{label}"])
            assert abs(float(v) - want) <= 1e-12 * abs(want), (name, label)


class _Scheduled(torch.optim.lr_scheduler._LRScheduler):
    """The reference's WarmupMultiStepLR.get_lr formula ("linear") on torch's scheduler stepping."""

    def __init__(self, optimizer, milestones, gamma, warmup_factor=1.0 / 3, warmup_iters=500):
        self.milestones, self.gamma, self.warmup_factor, self.warmup_iters = milestones, gamma, warmup_factor, warmup_iters
        super().__init__(optimizer, -1)

    def get_lr(self):
        from bisect import bisect_right
        warmup_factor = 1
        if self.last_epoch < self.warmup_iters:
            alpha = float(self.last_epoch) / self.warmup_iters
            warmup_factor = self.warmup_factor * (1 - alpha) + alpha
        return [base_lr * warmup_factor * self.gamma ** bisect_right(self.milestones, self.last_epoch) for base_lr in self.base_lrs]


def test_warmup_multistep_lr():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=1e-3)
    sched = _Scheduled(opt, [600, 800], 0.5)
    rates = []
    for _ in range(810):
        rates.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    for step in (0, 1, 499, 500, 599, 600, 601, 799, 800, 809):
        assert estimator.warmup_multistep_lr(step, 1e-3, (600, 800), 0.5) == rates[step], step
    assert rates[0] == 1e-3 / 3 and rates[500] == 1e-3 and rates[600] == 5e-4 and rates[800] == 2.5e-4


def test_state_dict_keys_are_the_references():
    keys = [str(k) for k in U.fixture()["keys"]]
    model = estimator.DeviceTransMVSNet()
    assert list(model.state_dict().keys()) == keys and len(keys) > 400
    shared = estimator.DeviceTransMVSNet(share_cr=True)
    assert not any(k.startswith("cost_regularization.0.") for k in shared.state_dict()) and "cost_regularization.prob.weight" in shared.state_dict()
    torch.manual_seed(1)
    other = estimator.DeviceTransMVSNet()
    other.load_state_dict(model.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))
    copy = estimator.DeviceTransMVSNet.from_module(model.double().eval())
    assert not copy.training and next(copy.parameters()).dtype == torch.float64 and copy.fused_readout is False
    copy.fused_readout = True
    assert copy.DepthNet.fused_readout is True


def test_checkpoint_round_trip(tmp_path):
    model, batch = U.fit_model(), U.fit_batch()
    _, opt = estimator.fit_estimator(model, [batch], steps=2, log_every=2)
    path = str(tmp_path / "model_000007.ckpt")
    estimator.save_estimator_checkpoint(path, model, opt, epoch=7)
    assert sorted(torch.load(path, weights_only=False)) == ["epoch", "model", "optimizer"]
    fresh = U.fit_model()
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    fresh_opt = torch.optim.Adam(fresh.parameters(), lr=1.0)
    assert estimator.load_estimator_checkpoint(path, fresh, fresh_opt) == 7
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), fresh.state_dict().values()))
    a, b = opt.state_dict(), fresh_opt.state_dict()
    assert a["param_groups"][0]["weight_decay"] == b["param_groups"][0]["weight_decay"] == 1e-4 and len(a["state"]) == len(b["state"]) > 0
    for k in a["state"]:
        assert float(a["state"][k]["step"]) == float(b["state"][k]["step"]) == 2.0
        assert torch.equal(a["state"][k]["exp_avg"], b["state"][k]["exp_avg"]) and torch.equal(a["state"][k]["exp_avg_sq"], b["state"][k]["exp_avg_sq"])


def test_fit_estimator_on_the_cpu():
    model, batch = U.fit_model(), U.fit_batch()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flushes = []
    history, opt = estimator.fit_estimator(model, [batch], steps=U.FIT["steps"], lr=U.FIT["lr"], log_every=4, on_log=flushes.append)
    assert isinstance(opt, torch.optim.Adam) and [len(f) for f in flushes] == [4, U.FIT["steps"] - 4]
    assert [h["step"] for h in history] == list(range(U.FIT["steps"])) and all(math.isfinite(h["total"]) for h in history)
    assert any(not torch.equal(before[k], v) for k, v in model.state_dict().items())
    assert history[-1]["total"] < history[0]["total"]
    assert opt.param_groups[0]["lr"] == estimator.warmup_multistep_lr(U.FIT["steps"] - 1, U.FIT["lr"], (), 0.5)


def test_training_forward_carries_the_graph_and_eval_matches_depth_from_images():
    model, batch = U.fit_model(), U.fit_batch()
    model.train()
    model.fused_readout = True                         # CPU tensors: the switch changes nothing
    out = model(batch["imgs"], batch["proj_matrices"], batch["depth_values"], depth_interval=batch["base_interval"])
    assert all("cost" not in out[k] and out[k]["prob_volume"].requires_grad for k in ("stage1", "stage2", "stage3"))
    assert tuple(out["stage1"]["prob_volume"].shape) == (1, 16, 8, 16) and tuple(out["depth"].shape) == (1, 32, 64)
    model.eval()
    with torch.no_grad():
        a = model(batch["imgs"], batch["proj_matrices"], batch["depth_values"], depth_interval=batch["base_interval"])
        b = mvs.depth_from_images(batch["imgs"], batch["proj_matrices"], batch["depth_values"], model.feature, model.FMT_with_pathway,
                                  model.DepthNet, model.cost_regularization, ndepths=U.FIT["ndepths"], depth_interval=batch["base_interval"])
    assert torch.equal(a["depth"], b["depth"]) and torch.equal(a["photometric_confidence"], b["photometric_confidence"])


def test_argument_checks_need_no_device():
    from diner_amd import ops
    s = U.case_inputs("sub_wave")[0]
    with pytest.raises(ValueError, match="one shape"):
        ops._check_mvs_loss_args(s["cost"], s["hyp"][:, :4], s["gt"], s["mask"])
    with pytest.raises(ValueError, match="gt and mask"):
        ops._check_mvs_loss_args(s["cost"], s["hyp"], s["gt"][:, :2], s["mask"])
    with pytest.raises(ValueError, match="one shape"):
        ops._check_mvs_loss_args(s["cost"], s["hyp"], s["gt"], s["mask"], s["init"][:1])
    big = torch.zeros(1).expand(2, 1024, 1024, 1024)                         # B D H W = 2^31, no memory behind it
    with pytest.raises(ValueError, match="2\\^31"):
        ops._check_mvs_loss_args(big, big, big[:, 0], big[:, 0])
    with pytest.raises(ValueError, match="2\\^31"):
        ops._check_depth_scores_args(*[torch.zeros(1).expand(2, 32768, 32768)] * 3, ())
    with pytest.raises(ValueError, match="one shape"):
        ops._check_depth_scores_args(s["gt"], s["gt"][:1], s["mask"], ())
    with pytest.raises(ValueError, match="thresholds"):
        ops._check_depth_scores_args(s["gt"], s["gt"], s["mask"], tuple(range(9)))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mvs_stage_loss(s["cost"], s["hyp"], s["gt"], s["mask"])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.depth_scores(s["gt"], s["gt"], s["mask"])
    with pytest.raises(KeyError):
        estimator.focal_loss_bld({"stage1": {}}, {}, {}, 1.0)
