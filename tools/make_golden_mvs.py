"""Fixture G28 (tests/golden/g28_mvs.npz): the matching stage of the depth estimator on seeded, structured inputs.

    python tools/make_golden_mvs.py            # rewrites the fixture; needs the reference tree (build container only)

The inputs are regenerated from seeds by tests/mvs_util.py and are not stored (a sha256 of their bytes is).  Per case the fixture holds
strided sub-samples of

  * the reference's own float32 results: DepthNet.forward / homo_warping / get_depth_range_samples of deps/TransMVSNet, imported straight
    from the reference tree under a private package name (torchvision.ops, which only the deformable convolutions need, is stubbed);
  * the float64 results of diner_amd.mvs's torch restatement.  homo_warping hard-codes float32, so float64 needs the restatement; it is
    trusted only after its float32 run has been found torch.equal to the reference on every output, which this generator asserts;
  * `err_*`: the reference float32's own distance (max |difference|) from float64 per output -- the yardstick of the GPU tests, which
    allow the kernels mvs_util.BAR_FACTOR times that;
  * `excluded`: the share of pixels whose float64 top-2 probability gap is within mvs_util.GAP_FACTOR x err_prob, where the argmax is
    not compared.  The generator asserts that the reference's own argmax agrees with float64's everywhere else and that the share
    stays below mvs_util.EXCLUDED_CAP.

The regulariser of the fixture is elementwise (cost = 20 similarity), so no convolution library's result enters the expected values."""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs                     # noqa: E402
from tests import mvs_util as U               # noqa: E402

from oracle.ref_import import REF_ROOT        # noqa: E402

REF_MODELS = os.path.join(REF_ROOT, "deps", "TransMVSNet", "models")
PKG = "_g28_transmvsnet_models"


def import_reference():
    """models/module.py and models/TransMVSNet.py of the reference as the private package PKG -> (module, TransMVSNet)."""
    if "torchvision" not in sys.modules:
        tv, tvo = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
        tvo.DeformConv2d = type("DeformConv2d", (torch.nn.Module,), {})
        tvo.deform_conv2d = None
        tv.ops = tvo
        sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, tvo
    pkg = types.ModuleType(PKG)
    pkg.__path__ = [REF_MODELS]
    sys.modules[PKG] = pkg
    out = []
    for name in ("module", "TransMVSNet"):
        spec = importlib.util.spec_from_file_location(f"{PKG}.{name}", os.path.join(REF_MODELS, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"{PKG}.{name}"] = mod
        spec.loader.exec_module(mod)
        out.append(mod)
    return out


def sha256_of(x):
    h = hashlib.sha256()

    def walk(v):
        if torch.is_tensor(v):
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
        elif isinstance(v, dict):
            for k in sorted(v):
                h.update(str(k).encode())
                walk(v[k])
        elif isinstance(v, (list, tuple)):
            for e in v:
                walk(e)
        elif isinstance(v, np.ndarray):
            h.update(np.ascontiguousarray(v).tobytes())
    walk(x)
    return h.hexdigest()


def reference_depthnet(ref_net, state_dict):
    net = ref_net.DepthNet()
    net.pixel_wise_net.load_state_dict(state_dict)
    return net.eval()


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def do_case(name, ref_net, out):
    c, inp = U.CASES[name], U.case_inputs(name)
    net = reference_depthnet(ref_net, inp["state_dict"])
    with torch.no_grad():
        init = None if inp["prob_init"] is None else inp["prob_init"].clone()
        res = net(inp["features"], inp["proj"], inp["depth_values"], c["D"], U.regulariser, prob_volume_init=init,
                  view_weights=inp["view_weights"])
    ref, ref_w = (res, inp["view_weights"]) if inp["view_weights"] is not None else res
    r32, r64 = U.run_case(inp, torch.float32), U.run_case(inp, torch.float64)
    # the restatement in float32 is the reference, bit for bit; only then are its float64 values trusted
    for key, val in (("prob", ref["prob_volume"]), ("weights", ref_w), ("depth", ref["depth"]), ("confidence", ref["photometric_confidence"])):
        assert torch.equal(r32[key], val), (name, key, maxerr(r32[key], val))
    err = {k: maxerr(r32[k], r64[k]) for k in ("similarity", "weights", "prob", "confidence")}
    keep, excluded = U.excluded_share(r64["prob"], err["prob"])
    arg32, arg64 = r32["prob"].argmax(1), r64["prob"].argmax(1)
    assert bool((arg32 == arg64)[keep].all()), (name, "the reference's argmax leaves float64's outside the excluded pixels")
    assert excluded <= U.EXCLUDED_CAP, (name, excluded)
    for k in ("similarity", "weights", "prob", "confidence", "depth"):
        out[f"{name}_{k}64"] = U.subsample(r64[k])
        out[f"{name}_{k}32"] = U.subsample(r32[k])
    for k, v in err.items():
        out[f"{name}_err_{k}"] = np.float64(v)
    out[f"{name}_excluded"] = np.float64(excluded)
    out[f"{name}_sha256"] = np.array(sha256_of({k: v for k, v in inp.items()}))
    out[f"{name}_seed"] = np.int64(c["seed"])
    print(f"case {name}: {c} errors {({k: f'{v:.2e}' for k, v in err.items()})} excluded {100 * excluded:.2f} % "
          f"gap<1e-4 {100 * float((U.top2_gap(r64['prob']) < 1e-4).double().mean()):.2f} %")


def do_hypotheses(name, ref_mod, out):
    c, cur = U.HYPOTHESES[name], U.hypotheses_inputs(name)
    H, W = c["image"]
    s, D = c["scale"], c["D"]
    up = F.interpolate(cur.unsqueeze(1), [H, W], mode="bilinear", align_corners=False).squeeze(1)
    samples = ref_mod.get_depth_range_samples(cur_depth=up, ndepth=D, depth_inteval_pixel=c["interval"], dtype=cur.dtype, device=cur.device,
                                              shape=[cur.shape[0], H, W])
    ref = F.interpolate(samples.unsqueeze(1), [D, H // s, W // s], mode="trilinear", align_corners=False).squeeze(1)
    h32 = mvs.depth_hypotheses(cur, D, c["interval"], (H, W), s)
    h64 = mvs.depth_hypotheses(cur.double(), D, c["interval"], (H, W), s)
    assert torch.equal(h32, ref), (name, maxerr(h32, ref))
    out[f"hyp_{name}_64"], out[f"hyp_{name}_32"] = U.subsample(h64), U.subsample(h32)
    out[f"hyp_{name}_err"] = np.float64(maxerr(h32, h64))
    out[f"hyp_{name}_sha256"] = np.array(sha256_of(cur))
    print(f"hypotheses {name}: {c} -> {tuple(h64.shape)} error {maxerr(h32, h64):.2e}")


def reference_stage_loop(ref_mod, net, inp):
    """The stage loop of TransMVSNet.forward after feature extraction, on the reference's own functions (float32)."""
    s = U.STAGES
    H, W = s["image"]
    B = inp["depth_values"].shape[0]
    outputs, depth, weights = {}, None, None
    for i, (nd, ratio, sc) in enumerate(zip(s["ndepths"], s["ratios"], s["scales"])):
        key = f"stage{i + 1}"
        cur = inp["depth_values"] if depth is None else F.interpolate(depth.unsqueeze(1), [H, W], mode="bilinear", align_corners=False).squeeze(1)
        samples = ref_mod.get_depth_range_samples(cur_depth=cur, ndepth=nd, depth_inteval_pixel=ratio * s["depth_interval"], dtype=torch.float32,
                                                  device=cur.device, shape=[B, H, W])
        hyp = F.interpolate(samples.unsqueeze(1), [nd, H // sc, W // sc], mode="trilinear", align_corners=False).squeeze(1)
        feats = [f[key] for f in inp["features"]]
        if weights is None:
            res, weights = net(feats, inp["proj"][key], depth_values=hyp, num_depth=nd, cost_regularization=U.regulariser, view_weights=None)
        else:
            weights = F.interpolate(weights, scale_factor=2, mode="nearest")
            res = net(feats, inp["proj"][key], depth_values=hyp, num_depth=nd, cost_regularization=U.regulariser, view_weights=weights)
        depth = torch.gather(res["depth_values"], 1, torch.argmax(res["prob_volume"], dim=1, keepdim=True)).squeeze(1)
        res["depth"] = depth
        outputs[key] = res
    return outputs


def do_stages(ref_mod, ref_net, out):
    s, inp = U.STAGES, U.stage_inputs()
    net = reference_depthnet(ref_net, inp["state_dict"])
    with torch.no_grad():
        ref = reference_stage_loop(ref_mod, net, inp)
    res = {}
    for dt in (torch.float32, torch.float64):
        dn = mvs.DeviceDepthNet()
        dn.pixel_wise_net.load_state_dict(inp["state_dict"])
        dn = dn.to(dt).eval()
        with torch.no_grad():
            res[dt] = mvs.coarse_to_fine(U.cast(inp["features"], dt), U.cast(inp["proj"], dt), inp["depth_values"].to(dt), dn, U.regulariser,
                                         ndepths=s["ndepths"], ratios=s["ratios"], image_hw=s["image"], depth_interval=s["depth_interval"])
    for i in range(3):
        key = f"stage{i + 1}"
        r32, r64 = res[torch.float32][key], res[torch.float64][key]
        for k in ("depth", "photometric_confidence", "prob_volume", "depth_values"):
            assert torch.equal(r32[k], ref[key][k]), (key, k, maxerr(r32[k], ref[key][k]))
        err = maxerr(r32["prob_volume"], r64["prob_volume"])
        # later stages inherit the earlier stages' winners: the float32 and the float64 chain only stay comparable where they agree
        assert torch.equal(r32["prob_volume"].argmax(1), r64["prob_volume"].argmax(1)), key
        keep, excluded = U.excluded_share(r64["prob_volume"], err)
        assert excluded <= U.EXCLUDED_CAP, (key, excluded)
        for k in ("depth", "photometric_confidence", "prob_volume", "depth_values"):
            out[f"stages_{key}_{k}64"], out[f"stages_{key}_{k}32"] = U.subsample(r64[k]), U.subsample(r32[k])
            out[f"stages_{key}_err_{k}"] = np.float64(maxerr(r32[k], r64[k]))
        out[f"stages_{key}_excluded"] = np.float64(excluded)
        print(f"stages {key}: prob error {err:.2e}, hypotheses error {maxerr(r32['depth_values'], r64['depth_values']):.2e}, excluded "
              f"{100 * excluded:.2f} %")
    out["stages_sha256"] = np.array(sha256_of({k: inp[k] for k in ("features", "proj", "depth_values", "state_dict")}))


def main():
    ref_mod, ref_net = import_reference()
    out = {}
    for name in U.CASES:
        do_case(name, ref_net, out)
    for name in U.HYPOTHESES:
        do_hypotheses(name, ref_mod, out)
    do_stages(ref_mod, ref_net, out)
    np.savez_compressed(U.FIXTURE, **out)
    print("wrote", U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
