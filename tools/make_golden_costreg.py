"""Fixture G29 (tests/golden/g29_costreg.npz): the depth estimator's cost regulariser, CostRegNet, on seeded weights and inputs.

    python tools/make_golden_costreg.py        # rewrites the fixture; needs the reference tree (build container only)

Weights and inputs are regenerated from seeds by tests/costreg_util.py and are not stored (a sha256 of their bytes is).  The generator
first asserts that DeviceCostRegNet's torch route in float32 is torch.equal to the reference's CostRegNet (deps/TransMVSNet
models/module.py, imported the way tools/make_golden_mvs.py does) on every case; only then are the route's float64 values trusted.  Per
case the fixture holds strided sub-samples of the float64 cost and of the reference's float32 cost, `err_cost` / `err_prob`: the
reference float32's own distance (max |difference|) from float64 on the cost and on the prob volume select_depth forms of it -- the
yardstick of the GPU tests, which allow the kernels costreg_util.BAR_FACTOR times that -- and `excluded`: the share of pixels whose float64
top-2 probability gap is within costreg_util.GAP_FACTOR x err_prob.  The generator asserts that the reference's own argmax agrees with
float64's everywhere else and that the share stays under costreg_util.EXCLUDED_CAP; it fails, and never widens the cap, if not.  The same
is stored for DeviceDepthNet with the real regulariser on a G28-style scene."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import costreg_util as U                                            # noqa: E402
from tests import mvs_util as MU                                               # noqa: E402
from tools.make_golden_mvs import import_reference, maxerr, sha256_of          # noqa: E402


def reference_costregnet(ref_mod, base, state_dict):
    net = ref_mod.CostRegNet(in_channels=1, base_channels=base)
    net.load_state_dict(state_dict)
    return net.eval()


def check_winners(name, p32, p64, err_prob):
    keep, excluded = MU.excluded_share(p64, err_prob)
    assert bool((p32.argmax(1) == p64.argmax(1))[keep].all()), (name, "the reference's argmax leaves float64's outside the excluded pixels")
    assert excluded <= U.EXCLUDED_CAP, (name, excluded)
    return excluded


def do_case(name, ref_mod, out):
    c = U.CASES[name]
    base = c["shape"][0]
    x, sd = U.case_input(name), U.costreg_state_dict(base, c["seed"] + 50)
    with torch.no_grad():
        ref = reference_costregnet(ref_mod, base, sd)(x.clone())
    r32, r64 = U.expected32(name), U.expected64(name)
    # the module's torch route in float32 is the reference, bit for bit; only then are its float64 values trusted
    assert torch.equal(r32, ref), (name, maxerr(r32, ref))
    p32, p64 = U.softmax_d(r32), U.softmax_d(r64)
    err_cost, err_prob = maxerr(r32, r64), maxerr(p32, p64)
    excluded = check_winners(name, p32, p64, err_prob)
    out[f"{name}_cost64"], out[f"{name}_cost32"] = U.subsample(r64), U.subsample(r32)
    out[f"{name}_err_cost"], out[f"{name}_err_prob"] = np.float64(err_cost), np.float64(err_prob)
    out[f"{name}_excluded"] = np.float64(excluded)
    out[f"{name}_sha256"] = np.array(sha256_of({"x": x, "state_dict": sd}))
    out[f"{name}_seed"] = np.int64(c["seed"])
    print(f"case {name}: {c['shape']} cost range {float(r64.min()):.2f} .. {float(r64.max()):.2f}, reference float32 from float64: cost "
          f"{err_cost:.2e}, prob {err_prob:.2e}, excluded {100 * excluded:.2f} %")


def do_depthnet(ref_mod, ref_net, out):
    inp = U.depthnet_inputs()
    net = ref_net.DepthNet()
    net.pixel_wise_net.load_state_dict(inp["pixelwise"])
    reg = reference_costregnet(ref_mod, U.DEPTHNET["base"], inp["costreg"])
    with torch.no_grad():
        ref, ref_w = net.eval()(inp["features"], inp["proj"], inp["depth_values"], U.DEPTHNET["D"], reg)
    (r32, w32), (r64, _) = U.depthnet_expected(torch.float32), U.depthnet_expected(torch.float64)
    for key in ("prob_volume", "depth", "photometric_confidence"):
        assert torch.equal(r32[key], ref[key]), ("depthnet", key, maxerr(r32[key], ref[key]))
    assert torch.equal(w32, ref_w)
    err = maxerr(r32["prob_volume"], r64["prob_volume"])
    excluded = check_winners("depthnet", r32["prob_volume"], r64["prob_volume"], err)
    out["depthnet_prob64"], out["depthnet_prob32"] = U.subsample(r64["prob_volume"]), U.subsample(r32["prob_volume"])
    out["depthnet_err_prob"], out["depthnet_excluded"] = np.float64(err), np.float64(excluded)
    out["depthnet_sha256"] = np.array(sha256_of(inp))
    print(f"depthnet: {U.DEPTHNET} reference float32 prob from float64 {err:.2e}, excluded {100 * excluded:.2f} %")


def main():
    ref_mod, ref_net = import_reference()
    out = {}
    for name in U.CASES:
        do_case(name, ref_mod, out)
    do_depthnet(ref_mod, ref_net, out)
    np.savez_compressed(U.FIXTURE, **out)
    print("wrote", U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
