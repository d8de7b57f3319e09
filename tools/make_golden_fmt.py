"""Fixture G30 (tests/golden/g30_fmt.npz): the depth estimator's feature transformer, FMT_with_pathway, on seeded weights and inputs.

    python tools/make_golden_fmt.py        # rewrites the fixture; needs the reference tree (build container only)

Weights and inputs are regenerated from seeds by tests/fmt_util.py and are not stored (a sha256 of their bytes is).  The generator first
asserts that DeviceFMTWithPathway's torch route in float32 is torch.equal to the reference's FMT_with_pathway (deps/TransMVSNet
models/FMT.py, imported the way tools/make_golden_mvs.py does) on every case, for all three stages of all views; only then are the
route's float64 values trusted.  Per case and stage the fixture holds strided sub-samples of the float64 and of the reference's float32
outputs and `err_<stage>`: the reference float32's own distance (max |difference|) from float64 -- the yardstick of the GPU tests, which
allow the kernels fmt_util.BAR_FACTOR times that.  No pixel is excluded from those comparisons.  The same is stored for the prob volumes
of coarse_to_fine on mvs_util's three-stage scene with its features sent through the module first, with the share of pixels whose float64
top-2 gap is within fmt_util.GAP_FACTOR x that distance (the argmax is compared elsewhere)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fmt_util as U                                                # noqa: E402
from tests import mvs_util as MU                                               # noqa: E402
from tools.make_golden_mvs import import_reference, maxerr, sha256_of          # noqa: E402


def reference_module(ref_net, state_dict):
    net = ref_net.FMT_with_pathway()
    net.load_state_dict(state_dict)
    return net.eval()


def reference_case(ref_net, name):
    """The reference's own float32 results of a case -> {stage: [view, ...]}."""
    c = U.CASES[name]
    net = reference_module(ref_net, U.fmt_state_dict(c["seed"] + 50))
    feats = [dict(f) for f in U.case_features(name)]
    with torch.no_grad():
        if c["pathway"]:
            out = net(feats)
            return {k: [f[k] for f in out] for k in U.STAGES}
        refs = net.FMT(feats[0]["stage1"].clone(), feat="ref")
        return {"stage1": [refs[-1]] + [net.FMT([r.clone() for r in refs], f["stage1"].clone(), feat="src") for f in feats[1:]]}


def do_case(name, ref_net, out):
    c = U.CASES[name]
    ref, r32, r64 = reference_case(ref_net, name), U.expected32(name), U.expected64(name)
    for stage in U.case_stages(name):
        assert len(ref[stage]) == len(r32[stage]) == c["NV"]
        for v, (a, b) in enumerate(zip(r32[stage], ref[stage])):
            # the module's torch route in float32 is the reference, bit for bit; only then are its float64 values trusted
            assert a.shape == b.shape and torch.equal(a, b), (name, stage, v, maxerr(a, b))
        s32, s64 = U.stacked(r32[stage]), U.stacked(r64[stage])
        err = maxerr(s32, s64)
        out[f"{name}_{stage}_64"], out[f"{name}_{stage}_32"] = U.subsample(s64), U.subsample(s32)
        out[f"{name}_err_{stage}"] = np.float64(err)
        print(f"case {name} {stage}: {tuple(s64.shape)} range {float(s64.min()):.2f} .. {float(s64.max()):.2f}, reference float32 from "
              f"float64 {err:.2e}")
    out[f"{name}_sha256"] = np.array(sha256_of({"features": U.case_features(name), "state_dict": U.fmt_state_dict(c["seed"] + 50)}))
    out[f"{name}_seed"] = np.int64(c["seed"])


def do_stage_run(ref_net, out):
    """coarse_to_fine behind the module: the module's float32 features are the reference's, so its float32 run is the reference's."""
    inp = MU.stage_inputs()
    net = reference_module(ref_net, U.fmt_state_dict(U.STAGE_RUN_SEED))
    with torch.no_grad():
        ref = net([dict(f) for f in inp["features"]])
    ours = U.make_module(U.STAGE_RUN_SEED)
    with torch.no_grad():
        got = ours([dict(f) for f in inp["features"]])
    for a, b in zip(got, ref):
        assert all(torch.equal(a[k], b[k]) for k in U.STAGES)
    r32, r64 = U.stage_run_expected(torch.float32), U.stage_run_expected(torch.float64)
    for stage in U.STAGES:
        p32, p64 = r32[stage]["prob_volume"], r64[stage]["prob_volume"]
        err = maxerr(p32, p64)
        keep, excluded = MU.excluded_share(p64, err)
        assert bool((p32.argmax(1) == p64.argmax(1))[keep].all()), (stage, "the reference's argmax leaves float64's outside the excluded pixels")
        out[f"run_{stage}_prob64"], out[f"run_{stage}_prob32"] = U.subsample(p64), U.subsample(p32)
        out[f"run_err_{stage}"], out[f"run_excluded_{stage}"] = np.float64(err), np.float64(excluded)
        print(f"stage run {stage}: prob {tuple(p64.shape)}, reference float32 from float64 {err:.2e}, excluded {100 * excluded:.2f} %")
    out["run_sha256"] = np.array(sha256_of({"inputs": {k: inp[k] for k in ("features", "proj", "depth_values", "state_dict")},
                                            "state_dict": U.fmt_state_dict(U.STAGE_RUN_SEED)}))


def main():
    _, ref_net = import_reference()
    out = {}
    for name in U.CASES:
        do_case(name, ref_net, out)
    do_stage_run(ref_net, out)
    np.savez_compressed(U.FIXTURE, **out)
    print("wrote", U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
