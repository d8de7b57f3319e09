"""Shared by tools/make_golden_match_grad.py, tests/test_match_grad_cpu.py and tests/test_match_grad_gpu.py: the seeded upstream gradients of
fixture G33 (the inputs are tests/mvs_util.py's, regenerated and never stored), the runs that turn a case into the similarity, the cost
volume and their gradients, and the names under which the fixture keeps them.

Two runs per case.  "sim": match_similarity under the per-view upstream G (B,NS,D,H,W), loss = sum(G similarity).  "cv": cost_volume_train
under the aggregated upstream g (B,1,D,H,W), loss = sum(g similarity); the view weights are the case's given ones, or come from the
pixelwise net as a module in TRAINING mode (batch statistics, which it then updates), whose parameters then receive gradients too.  The
three stages of mvs_util.stage_inputs() are three more cases ("stage1" computed weights, "stage2" / "stage3" given ones) on linspace
hypotheses."""
import functools
import os

import numpy as np
import torch

from tests import mvs_util as MU

FIXTURE = os.path.join(MU.ROOT, "tests", "golden", "g33_match_grad.npz")
SEED_OFFSET = 3300                 # the upstream gradients' generator: the case's seed + this
BAR_FACTOR = MU.BAR_FACTOR
CASE_NAMES = tuple(MU.CASES) + ("stage1", "stage2", "stage3")
GIVEN = ("deep", "shifted", "stage2", "stage3")          # the cases whose view weights are given
PARAMS = ("conv0.conv.weight", "conv0.bn.weight", "conv0.bn.bias", "conv1.conv.weight", "conv1.bn.weight", "conv1.bn.bias", "conv2.weight",
          "conv2.bias")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict of float32 CPU tensors: features, proj, depth_values, view_weights or None, state_dict, G, g.  Treat it as read-only."""
    if name in MU.CASES:
        inp = dict(MU.case_inputs(name))
        seed = MU.CASES[name]["seed"]
    else:
        s, st = MU.STAGES, MU.stage_inputs()
        i = int(name[-1]) - 1
        sc, nd = s["scales"][i], s["ndepths"][i]
        H, W = s["image"][0] // sc, s["image"][1] // sc
        B, NS = s["B"], s["NS"]
        rng = np.random.default_rng(s["seed"] + 10 * (i + 1))
        depth = np.linspace(*s["depth_range"], nd).reshape(1, nd, 1, 1) + rng.uniform(0.0, 0.03, (B, 1, H, W))
        weights = rng.uniform(0.05, 1.0, (B, NS, H, W)) if i > 0 else None
        f32 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
        inp = dict(features=[f[name] for f in st["features"]], proj=st["proj"][name], depth_values=f32(depth), view_weights=f32(weights),
                   state_dict=st["state_dict"])
        seed = s["seed"] + i
    B, C, H, W = inp["features"][0].shape
    NS, D = len(inp["features"]) - 1, inp["depth_values"].shape[1]
    gen = torch.Generator().manual_seed(seed + SEED_OFFSET)
    inp["G"] = torch.randn(B, NS, D, H, W, generator=gen)
    inp["g"] = torch.randn(B, 1, D, H, W, generator=gen)
    return inp


def pixelwise_module(state_dict, dtype, device=None):
    """DeviceDepthNet's pixel_wise_net with the seeded state, in training mode."""
    from diner_amd import mvs
    net = mvs._PixelwiseNet()
    net.load_state_dict(state_dict)
    return net.to(dtype=dtype, device=device).train()


def leaves(inp, dtype, device=None):
    return [f.detach().to(dtype=dtype, device=device).clone().requires_grad_(True) for f in inp["features"]]


def run_sim(inp, dtype=torch.float64, device=None, upstream=None, fn=None):
    """match_similarity (or fn) and its backward under G -> dict(similarity (B,NS,D,H,W), d_ref (B,C,H,W), d_src [NS x (B,C,H,W)])."""
    from diner_amd import mvs
    x = MU.cast(dict(proj=inp["proj"], depth=inp["depth_values"], G=inp["G"] if upstream is None else upstream), dtype, device)
    feats = leaves(inp, dtype, device)
    s = (fn or mvs.match_similarity)(feats, x["proj"], x["depth"])
    (s * x["G"]).sum().backward()
    return dict(similarity=s.detach(), d_ref=feats[0].grad, d_src=[f.grad for f in feats[1:]])


def run_cv(inp, dtype=torch.float64, device=None, upstream=None, fn=None):
    """cost_volume_train (or fn) and its backward under g -> dict(similarity (B,1,D,H,W), weights, d_ref, d_src[, params: {key: grad}, stats:
    {key: BatchNorm running statistic after the call}])."""
    from diner_amd import mvs
    x = MU.cast(dict(proj=inp["proj"], depth=inp["depth_values"], g=inp["g"] if upstream is None else upstream, vw=inp["view_weights"]),
                dtype, device)
    feats = leaves(inp, dtype, device)
    net = None if x["vw"] is not None else pixelwise_module(inp["state_dict"], dtype, device)
    sim, weights = (fn or mvs.cost_volume_train)(feats, x["proj"], x["depth"], net, x["vw"])
    (sim * x["g"]).sum().backward()
    out = dict(similarity=sim.detach(), weights=weights.detach(), d_ref=feats[0].grad, d_src=[f.grad for f in feats[1:]])
    if net is not None:
        named = dict(net.named_parameters())
        out["params"] = {k: named[k].grad for k in PARAMS}
        out["stats"] = {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k}
    return out


def outputs(res):
    """A run's results as a flat {key: tensor}: similarity, d_ref, d_src{v}, param_{key}."""
    flat = {"similarity": res["similarity"], "d_ref": res["d_ref"]}
    for v, g in enumerate(res["d_src"]):
        flat[f"d_src{v}"] = g
    for k, g in res.get("params", {}).items():
        flat["param_" + k] = g
    return flat


@functools.lru_cache(maxsize=None)
def expected64(name, run):
    """The float64 restatement of a case on the CPU ("sim" or "cv"), computed once per session and shared; treat it as read-only."""
    from diner_amd import mvs
    if run == "sim":
        return run_sim(inputs(name), torch.float64, fn=mvs.match_similarity_torch)
    return run_cv(inputs(name), torch.float64, fn=mvs.cost_volume_torch)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def bar(fx, name, run, key):
    return BAR_FACTOR * float(fx[f"{name}_{run}_err_{key}"])
