"""Fixture G33 (tests/golden/g33_match_grad.npz): the matching stage's similarity, cost volume and their gradients on seeded inputs.

    python tools/make_golden_match_grad.py     # rewrites the fixture; needs the reference tree (build container only)

The inputs are tests/mvs_util.py's six cases and the three stages of its stage_inputs(), regenerated from seeds; the upstream gradients
are seeded normals (tests/match_grad_util.py).  Per case and run ("sim": the per-view similarity under a per-view upstream; "cv": steps
1-2 of DepthNet.forward under an aggregated upstream, the pixelwise net in training mode where the weights are computed) this generator

  * runs the reference's own DepthNet.forward in training mode (deps/TransMVSNet/models, imported as tools/make_golden_mvs.py imports it)
    with autograd in float32, taking the similarities out through hooks -- its homo_warping builds the pixel grid in float32 whatever
    it is given, so it has no float64 run;
  * asserts that diner_amd.mvs's torch restatement (warp_torch route) in float32 equals it to 1e-12 on every output, gradients
    included, and only then trusts the restatement's float64 run;
  * stores per output (similarity, d_ref, d_src per view, the gradients at the pixelwise parameters) `err`: the reference float32's
    distance max |float32 - float64| -- the yardstick of the GPU tests, which allow the kernels match_grad_util.BAR_FACTOR times that --
    and a 192-value strided sub-sample of the float64 values.

Every stored distance is asserted non-zero.  An output whose float64 values are ALL exactly zero (the gradient at a view that sees
nothing: "turned") has no distance to store; it is listed under `<case>_<run>_zero`, and the tests demand exact zeros there."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs                                # noqa: E402
from tests import match_grad_util as U                   # noqa: E402
from tests import mvs_util as MU                         # noqa: E402

EQUAL_TOL = 1e-12


def reference_run(ref_net, inp, run):
    """The reference's own DepthNet, in training mode, float32, with autograd -> the dict of match_grad_util.run_sim / run_cv.  Its forward
    is called as it stands; two hooks take out what steps 1-2 compute.  "cv": the `cost_regularization` callable records the aggregated
    similarity it is handed, with its graph, and hands it back.  "sim": a forward pre-hook on `pixel_wise_net` records each view's
    similarity (the view weights are computed for that run whatever the case, so that the net is called for every view)."""
    feats = U.leaves(inp, torch.float32)
    net = ref_net.DepthNet()
    net.pixel_wise_net.load_state_dict(inp["state_dict"])
    net.train()
    given = inp["view_weights"] if run == "cv" else None
    aggregated, per_view = [], []

    def regulariser(similarity):
        aggregated.append(similarity)
        return similarity
    hook = net.pixel_wise_net.register_forward_pre_hook(lambda module, args: per_view.append(args[0]))
    got = net(feats, inp["proj"], inp["depth_values"], inp["depth_values"].shape[1], regulariser, view_weights=given)
    hook.remove()
    if run == "sim":
        out = torch.cat(per_view, 1)
        (out * inp["G"]).sum().backward()
        res = dict(similarity=out.detach())
    else:
        out, = aggregated
        (out * inp["g"]).sum().backward()
        res = dict(similarity=out.detach(), weights=(given if given is not None else got[1]).detach())
    res.update(d_ref=feats[0].grad, d_src=[f.grad for f in feats[1:]])
    if run == "cv" and given is None:
        named = dict(net.pixel_wise_net.named_parameters())
        res["params"] = {k: named[k].grad for k in U.PARAMS}
        res["stats"] = {k: v.detach().clone() for k, v in net.pixel_wise_net.state_dict().items() if "running" in k}
    return res


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def do_case(name, run, ref_net, out):
    inp = U.inputs(name)
    ref = reference_run(ref_net, inp, run)
    torch_fn = mvs.match_similarity_torch if run == "sim" else mvs.cost_volume_torch
    runner = U.run_sim if run == "sim" else U.run_cv
    r32, r64 = runner(inp, torch.float32, fn=torch_fn), U.expected64(name, run)
    o_ref, o32, o64 = U.outputs(ref), U.outputs(r32), U.outputs(r64)
    assert set(o_ref) == set(o32) == set(o64), (name, run)
    for extra in ("weights",) if run == "cv" else ():
        assert maxerr(ref[extra], r32[extra]) <= EQUAL_TOL, (name, run, extra)
    for k in ref.get("stats", {}):
        assert maxerr(ref["stats"][k], r32["stats"][k]) <= EQUAL_TOL, (name, run, k)
    zero, errs = [], {}
    for k in o_ref:
        assert maxerr(o_ref[k], o32[k]) <= EQUAL_TOL, (name, run, k, maxerr(o_ref[k], o32[k]))
        if not bool(o64[k].any()):
            assert not bool(o_ref[k].any()), (name, run, k)
            zero.append(k)
            continue
        err = maxerr(o_ref[k], o64[k])
        assert err > 0.0, (name, run, k, "a zero bar would be meaningless: pick another seed")
        errs[k] = err
        out[f"{name}_{run}_err_{k}"] = np.float64(err)
        out[f"{name}_{run}_{k}64"] = MU.subsample(o64[k])
    out[f"{name}_{run}_zero"] = np.array(zero, dtype=np.str_)
    print(f"{name} {run}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + (f" zero: {zero}" if zero else ""))


def main():
    from tools.make_golden_mvs import import_reference
    _, ref_net = import_reference()
    out = {}
    for name in U.CASE_NAMES:
        for run in ("sim", "cv"):
            do_case(name, run, ref_net, out)
    np.savez_compressed(U.FIXTURE, **out)
    print("wrote", U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
