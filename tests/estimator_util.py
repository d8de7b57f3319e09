"""Shared by tools/make_golden_estimator_loss.py, tests/test_estimator_cpu.py and tests/test_estimator_gpu.py: the seeded inputs of
fixture G32 (regenerated, never stored), the case table, the runners of the loss on either route and the one fixed fine-tuning batch.

A stage's inputs (stage_inputs): integer-valued hypotheses hyp_d = start + d spacing per pixel (start an integer in [400, 600), spacing 2
or 4 per image), a ground-truth plane idx and gt = hyp[idx] + u 0.4 spacing with |u| <= 1, a winner plane idx + delta (delta in -6 .. 6,
clipped) whose cost is 6 above the largest of the N(0,1) noise planes, a random mask (80 % valid) and an addend init = 0.5 N(0,1) with
cost_init = float32(cost - init), so the same problem runs as cost, as cost_init + init and as prob = exp(log_softmax(cost)).  u is drawn
again wherever a scaled or absolute error would come within MARGIN of one of the EDGES, so no pixel has to be excluded anywhere.  Planted in
image 0 (pixels 0 .. 6; the ones that need two planes only when D >= 2): gt below the first and above the last hypothesis, gt exactly on a
hypothesis, an exact midpoint tie (first index wins), NaN and +inf gt under a zero mask, and a pixel whose cost at the ground-truth plane
is 200 below the maximum.  With B >= 2 image 1 has an all-zero mask (with one image that would leave nothing to compare)."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import mvs_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g32_estimator_loss.npz")
BAR_FACTOR = MU.BAR_FACTOR
FLOOR = 2.0 ** -23                   # rounding a double sum to the float32 result
MARGIN = 1e-3
SCALED_EDGES = (1.0, 3.0)            # less1, less3: errors in units of depth_interval 192 / 128
THRESHOLDS = (1.5, 5.0)              # thres_metrics, absolute
BAND = (0.5, 6.0)                    # abs_depth_error_metrics' band
ABS_EDGES = THRESHOLDS + BAND
PIX_BELOW, PIX_ABOVE, PIX_ON, PIX_TIE, PIX_NAN, PIX_INF, PIX_UNDERFLOW = range(7)
SCALARS = ("total", "depth_loss", "epe", "less1", "less3")

# name: the stages' (D, H, W), B, seed, dlossw, whether the fixture's run adds init
CASES = {
    "sub_wave": dict(B=2, stages=((48, 5, 7),), seed=3201, dlossw=None, init=False),        # less than one wavefront
    "ragged": dict(B=3, stages=((8, 17, 23),), seed=3202, dlossw=None, init=False),         # two workgroups, a ragged tail, an odd batch
    "one_plane": dict(B=1, stages=((1, 4, 4),), seed=3203, dlossw=None, init=False),        # D = 1
    "init": dict(B=2, stages=((32, 10, 14),), seed=3204, dlossw=None, init=True),
    "blocks": dict(B=1, stages=((8, 20, 28),), seed=3205, dlossw=None, init=False),         # three workgroups
    "three_stage": dict(B=2, stages=((48, 5, 7), (32, 10, 14), (8, 20, 28)), seed=3206, dlossw=(0.5, 1.0, 2.0), init=False),
}


def case_interval(name):
    """The (B,) depth_interval of a case: 2.0, 2.5, ..."""
    return torch.tensor([2.0 + 0.5 * b for b in range(CASES[name]["B"])], dtype=torch.float32)


def stage_keys(name):
    n = len(CASES[name]["stages"])
    return ["stage3"] if n == 1 else [f"stage{i + 1}" for i in range(n)]


def _too_close(err, unit):
    bad = np.zeros(err.shape, dtype=bool)
    for e in SCALED_EDGES:
        bad |= np.abs(err / unit - e) < 2 * MARGIN
    for e in ABS_EDGES:
        bad |= np.abs(err - e) < 2 * MARGIN
    return bad


def stage_inputs(B, D, H, W, seed):
    """-> dict of float32 tensors cost, init, cost_init, hyp (B,D,H,W), gt, mask (B,H,W), and idx, winner (B,H,W) int64."""
    rng = np.random.default_rng(seed)
    start = rng.integers(400, 600, (B, 1, H, W)).astype(np.float64)
    spacing = np.array([2.0 if b % 2 == 0 else 4.0 for b in range(B)]).reshape(B, 1, 1, 1)
    hyp = start + np.arange(D).reshape(1, D, 1, 1) * spacing
    idx = rng.integers(0, D, (B, H, W))
    winner = np.clip(idx + rng.integers(-6, 7, (B, H, W)), 0, D - 1)
    sp = spacing.reshape(B, 1, 1) * np.ones((B, H, W))
    unit = np.array([(2.0 + 0.5 * b) * 1.5 for b in range(B)]).reshape(B, 1, 1)
    u = rng.uniform(-1.0, 1.0, (B, H, W))
    hyp_idx = np.take_along_axis(hyp, idx[:, None], 1)[:, 0]
    hyp_win = np.take_along_axis(hyp, winner[:, None], 1)[:, 0]
    for _ in range(100):
        gt = (hyp_idx + u * 0.4 * sp).astype(np.float32).astype(np.float64)
        bad = _too_close(np.abs(hyp_win - gt), unit)
        if not bad.any():
            break
        u = np.where(bad, rng.uniform(-1.0, 1.0, (B, H, W)), u)
    else:
        raise AssertionError("stage_inputs: could not keep the errors away from the edges")
    mask = (rng.uniform(0.0, 1.0, (B, H, W)) < 0.8).astype(np.float64)
    noise = rng.normal(0.0, 1.0, (B, D, H, W))
    # planted pixels of image 0
    flat = lambda a: a.reshape(a.shape[0], -1)
    gt_f, mask_f, idx_f, win_f = flat(gt), flat(mask), flat(idx), flat(winner)
    hyp_f, sp0 = hyp.reshape(B, D, -1), float(spacing[0, 0, 0, 0])
    mask_f[0, :7] = 1.0
    gt_f[0, PIX_BELOW], idx_f[0, PIX_BELOW], win_f[0, PIX_BELOW] = hyp_f[0, 0, PIX_BELOW] - 0.3 * sp0, 0, 0
    gt_f[0, PIX_ABOVE], idx_f[0, PIX_ABOVE], win_f[0, PIX_ABOVE] = hyp_f[0, D - 1, PIX_ABOVE] + 0.3 * sp0, D - 1, D - 1
    k = D // 2
    gt_f[0, PIX_ON], idx_f[0, PIX_ON], win_f[0, PIX_ON] = hyp_f[0, k, PIX_ON], k, k
    if D >= 2:
        k = (D - 1) // 2
        gt_f[0, PIX_TIE], idx_f[0, PIX_TIE], win_f[0, PIX_TIE] = hyp_f[0, k, PIX_TIE] + 0.5 * sp0, k, k          # between planes k and k + 1
        k = D // 2
        gt_f[0, PIX_UNDERFLOW], idx_f[0, PIX_UNDERFLOW], win_f[0, PIX_UNDERFLOW] = hyp_f[0, k, PIX_UNDERFLOW], k, k - 1
    gt_f[0, PIX_NAN], mask_f[0, PIX_NAN] = np.nan, 0.0
    gt_f[0, PIX_INF], mask_f[0, PIX_INF] = np.inf, 0.0
    if B >= 2:
        mask_f[1, :] = 0.0
    cost = noise.copy()
    np.put_along_axis(cost, winner[:, None], noise.max(1, keepdims=True) + 6.0, 1)
    if D >= 2:
        cost.reshape(B, D, -1)[0, idx_f[0, PIX_UNDERFLOW], PIX_UNDERFLOW] = cost.reshape(B, D, -1)[0, :, PIX_UNDERFLOW].max() - 200.0
    init = 0.5 * rng.normal(0.0, 1.0, (B, D, H, W))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
    cost32, init32 = f32(cost), f32(init)
    return dict(cost=cost32, init=init32, cost_init=cost32 - init32, hyp=f32(hyp), gt=f32(gt), mask=f32(mask),
                idx=torch.from_numpy(idx.copy()), winner=torch.from_numpy(winner.copy()))


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> [stage_inputs per stage]; computed once per session and shared: treat as read-only."""
    c = CASES[name]
    return [stage_inputs(c["B"], D, H, W, c["seed"] + 10 * i) for i, (D, H, W) in enumerate(c["stages"])]


def loss_inputs(name, route, dtype=torch.float32, device=None, requires_grad=True):
    """-> (inputs, depth_gt_ms, mask_ms, leaves): the stage dicts of focal_loss_bld on a route -- "cost": {"cost"}; "init": {"cost":
    cost_init + init} with both as leaves; "prob": {"prob_volume": exp(log_softmax(cost))}, the leaf the cost -- and per stage the leaf
    tensors whose .grad the tests compare."""
    inputs, gts, masks, leaves = {}, {}, {}, {}
    for key, s in zip(stage_keys(name), case_inputs(name)):
        to = lambda t: t.to(dtype=dtype, device=device) if device is not None else t.to(dtype)
        hyp, gt, mask = to(s["hyp"]), to(s["gt"]), to(s["mask"])
        if route == "init":
            a, b = to(s["cost_init"]).clone().requires_grad_(requires_grad), to(s["init"]).clone().requires_grad_(requires_grad)
            pre = a + b
            pre = pre + ((s["cost_init"] + s["init"]).to(dtype=dtype, device=pre.device) - pre.detach())      # exactly the float32 sum the device forms
            leaf = (a, b)
        else:
            a = to(s["cost"]).clone().requires_grad_(requires_grad)
            pre, leaf = a, (a,)
        stage = {"depth_values": hyp}
        if route == "prob":
            stage["prob_volume"] = torch.exp(F.log_softmax(pre, dim=1))
        else:
            stage["cost"], stage["prob_volume"] = pre, None
        with torch.no_grad():
            index = torch.argmax(pre.detach(), dim=1, keepdim=True)
            stage["depth"] = torch.gather(hyp, 1, index).squeeze(1)
        inputs[key], gts[key], masks[key], leaves[key] = stage, gt, mask, leaf
    return inputs, gts, masks, leaves


def run_loss(name, route, dtype=torch.float32, device=None, force_torch=False, scale=1.0):
    """focal_loss_bld on a case -> ({scalar name: 0-dim tensor}, {stage: gradient of scale * total in the (first) leaf}, inputs, leaves)."""
    from diner_amd import estimator
    c = CASES[name]
    inputs, gts, masks, leaves = loss_inputs(name, route, dtype, device)
    interval = case_interval(name).to(dtype)
    if device is not None:
        interval = interval.to(device)
    out = estimator.focal_loss_bld(inputs, gts, masks, interval, dlossw=c["dlossw"], force_torch=force_torch)
    (out[0] * scale).backward()
    return dict(zip(SCALARS, (t.detach() for t in out))), {k: v[0].grad for k, v in leaves.items()}, inputs, leaves


@functools.lru_cache(maxsize=None)
def expected(name, route, dtype):
    """The restatement of a case on the CPU in `dtype`, computed once per session and shared; treat it as read-only."""
    scalars, grads, _, _ = run_loss(name, route, dtype, force_torch=True)
    return scalars, grads


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE, allow_pickle=False))


def fixture_route(name):
    return "init" if CASES[name]["init"] else "prob"


def scalar_bar(fx, name, quantity, value):
    """The larger of 4 x the recorded float32-float64 distance and 2^-23 |value|."""
    return max(BAR_FACTOR * float(fx[f"{name}_err_{quantity}"]), FLOOR * abs(float(value)))


# ---- the fine-tuning batch ------------------------------------------------------------------------------------------------------------------
FIT = dict(B=1, NS=2, image=(32, 64), ndepths=(16, 8, 8), depth_range=(1.2, 1.9), seed=3250, model_seed=3251, steps=6, lr=1e-3)


def fit_model(device=None):
    from diner_amd import estimator
    torch.manual_seed(FIT["model_seed"])
    model = estimator.DeviceTransMVSNet(ndepths=FIT["ndepths"])
    return model if device is None else model.to(device)


@functools.lru_cache(maxsize=None)
def _fit_batch_cpu():
    from diner_amd import mvs
    rng = np.random.default_rng(FIT["seed"])
    B, NS, (H, W) = FIT["B"], FIT["NS"], FIT["image"]
    E, K = MU.make_cameras(rng, B, NS, (H, W), None, focal=MU.FOCAL * 4, shift=0.08, turn=0.03)
    imgs = torch.from_numpy(0.5 + 0.5 * MU.plane_features(E, K, (H, W), 3, rng)).to(torch.float32).transpose(0, 1).contiguous()
    proj = mvs.proj_matrices_from_cameras(torch.from_numpy(E).float(), torch.from_numpy(K).float())
    lo, hi = FIT["depth_range"]
    D0 = FIT["ndepths"][0]
    depth_values = torch.from_numpy(np.linspace(lo, hi, D0)[None].repeat(B, 0)).to(torch.float32)
    depth, mask = {}, {}
    for i, s in enumerate((4, 2, 1)):
        Ks = K[:, 0].copy()
        Ks[:, :2, :] /= s
        h, w = H // s, W // s
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        pix = np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)
        z = np.zeros((B, h, w))
        for b in range(B):
            R, t = E[b, 0, :3, :3], E[b, 0, :3, 3]
            o, d = -R.T @ t, R.T @ (np.linalg.inv(Ks[b]) @ pix)
            z[b] = ((MU.PLANE_D - MU.PLANE_N @ o) / (MU.PLANE_N @ d)).reshape(h, w)      # the camera-frame ray has z = 1: the depth
        depth[f"stage{i + 1}"] = torch.from_numpy(z).to(torch.float32)
        m = np.ones((B, h, w))
        m[:, :, :max(1, w // 8)] = 0.0
        mask[f"stage{i + 1}"] = torch.from_numpy(m).to(torch.float32)
    base = (hi - lo) / D0
    return dict(imgs=imgs, proj_matrices=proj, depth_values=depth_values, depth=depth, mask=mask,
                depth_interval=torch.full((B,), base, dtype=torch.float32), base_interval=base)


def fit_batch(device=None):
    return MU.cast(_fit_batch_cpu(), torch.float32, device)
