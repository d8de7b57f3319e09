"""Shared by tools/make_golden_mvs.py, tests/test_mvs_cpu.py and tests/test_mvs_gpu.py: the seeded inputs of fixture G28 (regenerated, never
stored), the case table, the fixture's elementwise regulariser and the sub-sampling of its stored values.

The scene has structure, because random features give a flat probability volume whose top-2 gaps are rounding noise: every camera looks
at the textured plane -0.2 X + Z = 1.5 (world coordinates), feature channel c of a pixel is sin(k_c . (X, Y) + phi_c) of the world point
that pixel sees, |k_c| in [3, 17]; focal length 30 px, source cameras shifted by at most 0.2 and turned by at most 0.15 rad about y (less
in the three-stage run, whose first stage is 6 x 10 px); the hypotheses are linspace(1.2, 1.9, D) plus a per-pixel offset in [0, 0.03).  Everything is built in float64 and rounded once."""
import functools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g28_mvs.npz")
GAIN = 20.0                        # the fixture's regulariser: cost = GAIN * similarity, elementwise
SAMPLES = 192                      # values kept per stored array
FOCAL = 30.0
PLANE_N, PLANE_D = np.array([-0.2, 0.0, 1.0]), 1.5
BAR_FACTOR = 4.0                   # the kernels may be this many times the reference float32's own distance from float64
GAP_FACTOR = 3.0                   # argmax is compared where the float64 top-2 gap exceeds this many times that distance
EXCLUDED_CAP = 0.02

# name: B, NS, C, D, (H, W), seed, how the view weights come about, prob_volume_init, special camera
CASES = {
    "probe": dict(B=2, NS=3, C=8, D=8, hw=(23, 37), seed=2801, weights="net", prob_init=False, special=None),
    "wide": dict(B=2, NS=1, C=32, D=48, hw=(23, 37), seed=2802, weights="net", prob_init=True, special=None),
    "deep": dict(B=2, NS=3, C=8, D=200, hw=(9, 70), seed=2803, weights="given", prob_init=True, special=None),
    "views": dict(B=2, NS=15, C=8, D=1, hw=(23, 37), seed=2804, weights="net", prob_init=False, special=None),
    "turned": dict(B=2, NS=3, C=8, D=8, hw=(23, 37), seed=2805, weights="net", prob_init=True, special="turned"),
    "shifted": dict(B=2, NS=3, C=8, D=8, hw=(23, 37), seed=2806, weights="given", prob_init=False, special="shifted"),
}
# "deep": 200 planes over [1.2, 1.9] lie 0.009 px of disparity apart, so the matching cost alone leaves neighbouring planes within float32's
# noise of each other (the reference itself would disagree with float64 on a quarter of the pixels, whatever the baseline or the texture:
# a disparity of 0.3 px a plane needs views that no longer overlap on 70 px).  The case therefore carries a prob_volume_init, whose
# plane-to-plane differences set the top-2 gaps.
SPECIAL_VIEW = 1                   # the source view (0-based) the special camera replaces
# previous depth (h, w), image (H, W), stage scale, ndepth, interval, seed
HYPOTHESES = {
    "s1": dict(B=2, hw=(12, 20), image=(24, 40), scale=1, D=2, interval=0.0125, seed=2811),
    "s2": dict(B=2, hw=(6, 10), image=(24, 40), scale=2, D=4, interval=0.025, seed=2812),
    "s4": dict(B=2, hw=(5, 9), image=(23, 37), scale=4, D=8, interval=0.05, seed=2813),
    "s2_odd": dict(B=2, hw=(5, 9), image=(23, 37), scale=2, D=32, interval=0.01, seed=2814),
    "s1_odd": dict(B=2, hw=(11, 18), image=(23, 37), scale=1, D=8, interval=0.01, seed=2815),
}
STAGES = dict(B=2, NS=3, image=(24, 40), channels=(32, 16, 8), ndepths=(8, 4, 2), ratios=(4, 2, 1), scales=(4, 2, 1), seed=2821,
              depth_range=(1.2, 1.9), depth_interval=0.7 / 8 / 2,
              shift=0.08, turn=0.03)           # stage 1 is 6 x 10 px: with the cases' cameras a third of its samples would miss every view


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def make_cameras(rng, B, NS, hw, special=None, focal=FOCAL, shift=0.2, turn=0.15):
    """-> extrinsics (B,NS+1,4,4) world -> camera and intrinsics (B,NS+1,3,3), float64; view 0 is the reference."""
    H, W = hw
    E, K = np.zeros((B, NS + 1, 4, 4)), np.zeros((B, NS + 1, 3, 3))
    for b in range(B):
        for v in range(NS + 1):
            amp = 0.25 if v == 0 else 1.0                       # the reference camera stays near the origin, every sample its own
            centre = amp * rng.uniform(-shift, shift, 3) * np.array([1.0, 1.0, 0.25])
            angle = amp * rng.uniform(-turn, turn)
            if v == SPECIAL_VIEW + 1 and special == "turned":
                angle += np.pi                                   # looks away: every sample has z < 0
            if v == SPECIAL_VIEW + 1 and special == "shifted":
                centre[0] += 0.55                                # a band of samples falls outside, its edge half outside
            R = rot_y(angle).T                                   # world -> camera
            E[b, v, :3, :3], E[b, v, :3, 3], E[b, v, 3, 3] = R, -R @ centre, 1.0
            K[b, v] = np.array([[focal, 0.0, (W - 1) / 2.0], [0.0, focal, (H - 1) / 2.0], [0.0, 0.0, 1.0]])
    return E, K


def plane_features(E, K, hw, C, rng):
    """The texture of the plane as each camera sees it -> (NV, B, C, H, W) float64.  A turned camera sees the plane behind it: the
    intersection is still a point of the plane, and its features are never sampled."""
    H, W = hw
    B, NV = E.shape[:2]
    ang, mag, phi = rng.uniform(0, 2 * np.pi, C), rng.uniform(3.0, 17.0, C), rng.uniform(0, 2 * np.pi, C)
    kx, ky = mag * np.cos(ang), mag * np.sin(ang)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)
    out = np.zeros((NV, B, C, H, W))
    for b in range(B):
        for v in range(NV):
            R, t = E[b, v, :3, :3], E[b, v, :3, 3]
            o = -R.T @ t
            d = R.T @ (np.linalg.inv(K[b, v]) @ pix)
            s = (PLANE_D - PLANE_N @ o) / (PLANE_N @ d)
            P = o[:, None] + s[None] * d
            out[v, b] = np.sin(kx[:, None] * P[0][None] + ky[:, None] * P[1][None] + phi[:, None]).reshape(C, H, W)
    return out


def proj_pairs(E, K):
    """-> (B,NV,2,4,4) float64 in the estimator's layout: (extrinsics, intrinsics in the top-left 3x3 of a zero 4x4)."""
    B, NV = E.shape[:2]
    P = np.zeros((B, NV, 2, 4, 4))
    P[:, :, 0] = E
    P[:, :, 1, :3, :3] = K
    return P


def pixelwise_state_dict(seed):
    """A seeded state dict of DepthNet.pixel_wise_net: BatchNorm's running statistics and affine terms are random, nothing a folding
    mistake could cancel against."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cout, cin in (("conv0", 16, 1), ("conv1", 8, 16)):
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, 1, 1, 1, generator=g) * (2.0 / np.sqrt(cin))
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.3 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.2 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.25 + 1.5 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(100)
    sd["conv2.weight"] = torch.randn(1, 8, 1, 1, 1, generator=g) * 0.7
    sd["conv2.bias"] = 0.2 * torch.randn(1, generator=g)
    return sd


def case_inputs(name):
    """-> dict of float32 tensors: features [NV x (B,C,H,W)], proj (B,NV,2,4,4), depth_values (B,D,H,W), view_weights (B,NS,H,W) or None,
    prob_init (B,D,H,W) or None, and the pixelwise state dict."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    B, NS, C, D, (H, W) = c["B"], c["NS"], c["C"], c["D"], c["hw"]
    E, K = make_cameras(rng, B, NS, (H, W), c["special"])
    feats = plane_features(E, K, (H, W), C, rng)
    planes = np.linspace(1.2, 1.9, D) if D > 1 else np.array([1.5])
    depth = planes.reshape(1, D, 1, 1) + rng.uniform(0.0, 0.03, (B, 1, H, W))
    weights = rng.uniform(0.05, 1.0, (B, NS, H, W)) if c["weights"] == "given" else None
    init = rng.normal(0.0, 0.5, (B, D, H, W)) if c["prob_init"] else None
    f32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
    return dict(features=[f32(f) for f in feats], proj=f32(proj_pairs(E, K)), depth_values=f32(depth), view_weights=f32(weights),
                prob_init=f32(init), state_dict=pixelwise_state_dict(c["seed"] + 50))


def hypotheses_inputs(name):
    c = HYPOTHESES[name]
    rng = np.random.default_rng(c["seed"])
    h, w = c["hw"]
    ys, xs = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    depth = 1.5 + 0.2 * xs[None] - 0.1 * ys[None] + rng.uniform(-0.02, 0.02, (c["B"], h, w))
    return torch.from_numpy(depth).to(torch.float32)


def stage_inputs():
    """The three-stage run -> features: per view {"stage1": (B,32,H/4,W/4), ...}; proj: {"stage1": (B,NV,2,4,4), ...}; depth_values (B,D0);
    the pixelwise state dict.  The full-image cameras have focal 4 x 30 px, so stage 1 sees the 30 px the cost-volume cases use."""
    s = STAGES
    rng = np.random.default_rng(s["seed"])
    B, NS, (H, W) = s["B"], s["NS"], s["image"]
    E, K = make_cameras(rng, B, NS, (H, W), None, focal=FOCAL * 4, shift=s["shift"], turn=s["turn"])
    feats = [dict() for _ in range(NS + 1)]
    proj = {}
    for i, (C, sc) in enumerate(zip(s["channels"], s["scales"])):
        Ks = K.copy()
        Ks[:, :, :2, :] /= sc
        f = plane_features(E, Ks, (H // sc, W // sc), C, rng)
        for v in range(NS + 1):
            feats[v][f"stage{i + 1}"] = torch.from_numpy(f[v]).to(torch.float32)
        proj[f"stage{i + 1}"] = torch.from_numpy(proj_pairs(E, Ks)).to(torch.float32)
    lo, hi = s["depth_range"]
    depth_values = torch.from_numpy(np.linspace(lo, hi, 8)[None].repeat(B, 0)).to(torch.float32)
    return dict(features=feats, proj=proj, depth_values=depth_values, state_dict=pixelwise_state_dict(s["seed"] + 50), extrinsics=E, intrinsics=K)


def regulariser(similarity):
    return GAIN * similarity


def cast(x, dtype, device=None):
    """Tensors, lists and dicts of tensors -> dtype [and device]; None stays None."""
    if x is None:
        return None
    if torch.is_tensor(x):
        x = x.to(dtype) if x.is_floating_point() else x
        return x if device is None else x.to(device)
    if isinstance(x, dict):
        return {k: cast(v, dtype, device) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [cast(v, dtype, device) for v in x]
    return x


def run_case(inp, dtype=torch.float64, device=None):
    """diner_amd.mvs on one case's inputs -> dict(similarity (B,D,H,W), weights, depth, confidence, prob).  CPU tensors: the torch
    restatement in `dtype`; HIP tensors: the kernels."""
    from diner_amd import mvs
    x = cast({k: v for k, v in inp.items() if k != "state_dict"}, dtype, device)
    pw = None
    if x["view_weights"] is None:
        pw = mvs.fold_pixelwise(cast(inp["state_dict"], dtype, device))
    with torch.no_grad():
        sim, weights = mvs.cost_volume(x["features"], x["proj"], x["depth_values"], pw, x["view_weights"])
        depth, conf, prob = mvs.select_depth(regulariser(sim), x["depth_values"], x["prob_init"])
    return dict(similarity=sim.squeeze(1), weights=weights, depth=depth, confidence=conf, prob=prob)


def subsample(t):
    """A strided sub-sample (1-D numpy) of a tensor or array."""
    flat = (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).reshape(-1)
    return flat[::max(1, flat.size // SAMPLES) | 1].copy()


def top2_gap(prob):
    """(B,D,H,W) -> (B,H,W): the distance between the two largest probabilities of a pixel; +inf when there is one plane."""
    if prob.shape[1] == 1:
        return torch.full_like(prob[:, 0], float("inf"))
    top = torch.topk(prob, 2, dim=1).values
    return top[:, 0] - top[:, 1]


def excluded_share(prob64, err32):
    """-> (mask of the pixels whose float64 top-2 gap exceeds GAP_FACTOR x the float32 error, the share of the others)."""
    keep = top2_gap(prob64) > GAP_FACTOR * err32
    return keep, 1.0 - float(keep.double().mean())


@functools.lru_cache(maxsize=None)
def expected64(name):
    """The float64 restatement of a case on the CPU, computed once per session and shared; treat it as read-only."""
    return run_case(case_inputs(name), torch.float64)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))
