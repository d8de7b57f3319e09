"""Fixture G34 (tests/golden/g34_deform_grad.npz): the gradients of FeatureNet's modulated deformable convolutions on seeded inputs.

    python tools/make_golden_deform_grad.py     # rewrites the fixture; needs the reference tree (build container only)

The inputs are tests/deform_grad_util.py's cases, regenerated from seeds and never stored.  torchvision is not installed, so the
reference package's `dcn.deform_conv2d` is bound to diner_amd.mvs.deform_conv2d_torch, as tools/make_golden_featurenet.py does; the
reference's own modules then run around it.  Per layer case this generator

  * instantiates the reference's own DCN (models/dcn.py) with the case's weight and bias, hands it the case's raw offsets and logits in
    place of its conv_offset_mask, and runs it in float32 under autograd with the case's upstream gradient;
  * asserts that mvs.deform_conv3x3 (on the CPU: the restatement) in float32 equals it to 1e-12 on the output and on all four gradients,
    and that mvs.deform_conv3x3_grad_torch, the closed form, in float64 equals float64 autograd to 1e-12;
  * asserts the condition on the inputs: for every sample float32 and float64 agree on `inside` and on both floors, no sample excluded;
  * asserts sample_coverage on the layer inputs, and exact zeros (float32 and float64) at the planted non-finite offsets;
  * stores per output `err`, the reference float32's distance max |float32 - float64| -- the yardstick of the GPU tests, which allow the
    kernels deform_grad_util.BAR_FACTOR times that -- and a strided sub-sample of the float64 values.

Per net case (one FeatureNet training step) the same with the reference's FeatureNet in training mode against DeviceFeatureNet, per
stage output and per parameter gradient.  Every stored distance is asserted non-zero.  Seeds and a sha256 of all regenerated inputs are
stored beside them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs                                # noqa: E402
from tests import deform_grad_util as U                  # noqa: E402
from tests import featurenet_util as FU                  # noqa: E402
from tests import mvs_util as MU                         # noqa: E402
from tools.make_golden_mvs import PKG, import_reference  # noqa: E402

EQUAL_TOL = 1e-12
NET_SAMPLES = 24


class _Given(torch.nn.Module):
    """Stands where a DCN's conv_offset_mask stands and returns the case's raw offsets and logits, a leaf of the graph."""

    def __init__(self, offmask):
        super().__init__()
        self.offmask = offmask

    def forward(self, x):
        return self.offmask


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def reference_layer(dcn_module, inp):
    Cout, Cin = inp["weight"].shape[:2]
    mod = dcn_module.DCN(Cin, Cout, 3, 1, 1)
    with torch.no_grad():
        mod.weight.copy_(inp["weight"])
        mod.bias.copy_(inp["bias"])
    x = inp["x"].clone().requires_grad_(True)
    om = inp["offmask"].clone().requires_grad_(True)
    mod.conv_offset_mask = _Given(om)
    y = mod(x)
    (y * inp["dy"]).sum().backward()
    return dict(y=y.detach(), d_x=x.grad, d_offmask=om.grad, d_weight=mod.weight.grad, d_bias=mod.bias.grad)


def do_layer(name, dcn_module, out):
    inp = U.inputs(name)
    H, W = inp["x"].shape[2:]
    assert U.margin_holds(inp["offmask"]), (name, "float32 and float64 floor a sample differently: pick another seed")
    if name in U.LAYER_CASES:
        cov = FU.sample_coverage(inp["offmask"], H, W)
        assert all(v > 0 for v in cov.values()), (name, cov)
    ref = reference_layer(dcn_module, inp)
    r32, r64, c64 = U.run_layer(inp, torch.float32), U.expected64(name), U.closed_form(inp, torch.float64)
    errs = {}
    for k in ("y",) + U.OUTPUTS:
        assert maxerr(ref[k], r32[k]) <= EQUAL_TOL, (name, k, maxerr(ref[k], r32[k]))
        assert bool(torch.isfinite(r64[k]).all()), (name, k)
        if k == "y":
            continue
        assert maxerr(c64[k], r64[k]) <= EQUAL_TOL * max(1.0, float(r64[k].abs().max())), (name, k, maxerr(c64[k], r64[k]))
        errs[k] = maxerr(ref[k], r64[k])
        assert errs[k] > 0.0, (name, k, "a zero bar would be meaningless: pick another seed")
        out[f"{name}_err_{k}"] = np.float64(errs[k])
        out[f"{name}_{k}64"] = MU.subsample(r64[k])
    if name == "planted":
        for n, h, w, k in U.planted_taps():
            for res in (ref, r64, c64):
                for ch in (2 * k, 2 * k + 1, 18 + k):
                    assert float(res["d_offmask"][n, ch, h, w]) == 0.0, (name, n, h, w, k, ch)
    print(f"{name}: " + " ".join(f"{k} {v:.2e} (max {float(r64[k].abs().max()):.3g})" for k, v in errs.items()))


def do_net(name, ref_module, out):
    sys.modules[f"{PKG}.dcn"].deform_conv2d = mvs.deform_conv2d_torch
    ref = U.run_net(name, torch.float32, module=ref_module.FeatureNet(base_channels=8))
    r32, r64 = U.run_net(name, torch.float32), U.net_expected64(name)
    assert set(ref) == set(r32) == set(r64), name
    errs = {}
    for k in ref:
        assert maxerr(ref[k], r32[k]) <= EQUAL_TOL, (name, k, maxerr(ref[k], r32[k]))
        errs[k] = maxerr(ref[k], r64[k])
        assert errs[k] > 0.0, (name, k)
        out[f"net_{name}_err_{k}"] = np.float64(errs[k])
        flat = r64[k].detach().reshape(-1).numpy()
        out[f"net_{name}_{k}64"] = flat[::max(1, flat.size // NET_SAMPLES) | 1].copy()
    rel = sorted(errs[k] / max(float(r64[k].abs().max()), 1e-300) for k in errs if k not in U.BN_FED_BIASES)
    print(f"net {name}: {len(errs)} outputs, float32 distance relative to the largest value: median {rel[len(rel) // 2]:.2e}, max {rel[-1]:.2e}; "
          + "BatchNorm-fed biases: " + " ".join(f"{errs[k]:.1e}/{float(r64[k].abs().max()):.1e}" for k in U.BN_FED_BIASES))


def main():
    ref_module, _ = import_reference()
    dcn_module = sys.modules[f"{PKG}.dcn"]
    dcn_module.deform_conv2d = mvs.deform_conv2d_torch
    out = {"seed_offset": np.int64(U.SEED_OFFSET), "cases": np.array(U.CASE_NAMES), "net_cases": np.array(U.NET_CASES),
           "seeds": np.array([U.SYNTHETIC[n]["seed"] if n in U.SYNTHETIC else U.LAYER_NET_SEED[n.rsplit("_", 1)[0]] for n in U.CASE_NAMES])}
    for name in U.CASE_NAMES:
        do_layer(name, dcn_module, out)
    for name in U.NET_CASES:
        do_net(name, ref_module, out)
    out["sha256"] = np.array(U.input_hash())
    np.savez_compressed(U.FIXTURE, **out)
    size = os.path.getsize(U.FIXTURE)
    print("wrote", U.FIXTURE, size, "bytes")
    assert size < 300_000, size


if __name__ == "__main__":
    main()
