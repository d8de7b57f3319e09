"""Fixture G35 (tests/golden/g35_fmt_grad.npz): the gradients of the depth estimator's feature transformer on seeded inputs.

    python tools/make_golden_fmt_grad.py     # rewrites the fixture; needs the reference tree (build container only)

The inputs are tests/fmt_grad_util.py's cases, regenerated from seeds and never stored.  Per single-layer case this generator

  * instantiates the reference's own EncoderLayer (models/FMT.py) with fmt_util.fmt_state_dict's weights of the case (every bias and
    LayerNorm affine non-trivial) and runs it under autograd in float32 and in float64 against the case's seeded cotangent dy ~ N(0,1)
    (a source shared by several images is repeated over them, as FMT.forward hands the layer the reference view once per source view);
  * asserts that mvs._EncoderLayer in float32 gives the reference's bits, and that mvs.fmt_layer_grad_torch, the closed form, in float64
    equals float64 autograd to 1e-12 (relative to the output's largest value);
  * asserts the condition on the inputs (fmt_grad_util.kink_ratio >= 1): the smallest |linear1 output| in float64 is at least 4 x the
    largest |float32 - float64| of those outputs, nothing excluded;
  * stores per output `err`, the reference float32's distance max |float32 - float64| -- the yardstick of the GPU tests, which allow the
    kernels fmt_grad_util.BAR_FACTOR times that -- and a strided sub-sample of the float64 values.

Per whole-stack case the same with the reference's FMT called view by view (the gradients of every input map and of the 128 FMT
parameters) and with the reference's FMT_with_pathway in training mode (all three stages of every view, the 132 parameters).  Every
stored distance is asserted non-zero.  Seeds and a sha256 of all regenerated inputs are stored beside them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import fmt_grad_util as U                               # noqa: E402
from tools.make_golden_mvs import PKG, import_reference, maxerr    # noqa: E402

EQUAL_TOL = 1e-12
SAMPLES = U.SAMPLES


def sample(t):
    return U.sample(t)


def do_layer(name, ref_fmt, out):
    ratio = U.layer_kink_ratio(name)
    assert ratio >= 1.0, (name, ratio, "a linear1 output sits at the ReLU's kink: pick another seed")
    ref32 = U.run_layer(name, torch.float32, layer=U.make_layer(name, torch.float32, cls=ref_fmt.EncoderLayer))
    ref64 = U.run_layer(name, torch.float64, layer=U.make_layer(name, torch.float64, cls=ref_fmt.EncoderLayer))
    r32, r64, c64 = U.run_layer(name, torch.float32), U.layer_expected64(name), U.closed_form(name, torch.float64)
    errs = {}
    for k in ("y",) + U.layer_outputs(name):
        assert torch.equal(ref32[k], r32[k]), (name, k, maxerr(ref32[k], r32[k]))
        assert maxerr(ref64[k], r64[k]) <= EQUAL_TOL * max(1.0, float(r64[k].abs().max())), (name, k)
        if k == "y":
            continue
        assert maxerr(c64[k], r64[k]) <= EQUAL_TOL * max(1.0, float(r64[k].abs().max())), (name, k, maxerr(c64[k], r64[k]))
        errs[k] = maxerr(ref32[k], ref64[k])
        assert errs[k] > 0.0, (name, k, "a zero bar would be meaningless: pick another seed")
        out[f"{name}_err_{k}"] = np.float64(errs[k])
        out[f"{name}_{k}64"] = sample(r64[k])
    out[f"{name}_kink"] = np.float64(ratio)
    rel = sorted(errs[k] / float(r64[k].abs().max()) for k in errs)
    print(f"{name}: kink ratio {ratio:.2f}; float32 distance relative to the largest value: median {rel[len(rel) // 2]:.2e}, max {rel[-1]:.2e}")


def do_stack(name, ref_fmt, out):
    ratio = U.stack_kink_ratio(name)
    assert ratio >= 1.0, (name, ratio, "a linear1 output sits at the ReLU's kink: pick another seed")
    out[f"{name}_kink"] = np.float64(ratio)
    for kind, run, want in (("encode", U.run_encode, U.encode_expected64(name)), ("pathway", U.run_pathway, U.pathway_expected64(name))):
        ref32 = run(name, torch.float32, module=ref_fmt.FMT_with_pathway())
        ref64 = run(name, torch.float64, module=ref_fmt.FMT_with_pathway())
        r32 = run(name, torch.float32)
        assert set(ref32) == set(r32) == set(want), (name, kind)
        errs, values = {}, np.full((len(want), SAMPLES + 8), np.nan)
        for i, k in enumerate(sorted(want)):
            assert torch.equal(ref32[k], r32[k]), (name, kind, k, maxerr(ref32[k], r32[k]))
            assert maxerr(ref64[k], want[k]) <= EQUAL_TOL * max(1.0, float(want[k].abs().max())), (name, kind, k)
            errs[k] = maxerr(ref32[k], ref64[k])
            assert errs[k] > 0.0, (name, kind, k)
            got = sample(want[k])
            values[i, :got.size] = got
        # one array each per run: the sorted keys, their distances, and a row of float64 samples a key (NaN beyond the row's samples)
        out[f"{name}_{kind}_keys"] = np.array(sorted(want))
        out[f"{name}_{kind}_errs"] = np.array([errs[k] for k in sorted(want)])
        out[f"{name}_{kind}_64"] = values
        rel = sorted(errs[k] / float(want[k].abs().max()) for k in errs)
        print(f"{name} {kind}: kink ratio {ratio:.2f}; {len(errs)} outputs, float32 distance relative to the largest value: median "
              f"{rel[len(rel) // 2]:.2e}, max {rel[-1]:.2e}")


def main():
    import_reference()
    ref_fmt = sys.modules[f"{PKG}.FMT"]
    out = {"seed_offset": np.int64(U.SEED_OFFSET), "layer_cases": np.array(list(U.LAYER_CASES)), "stack_cases": np.array(list(U.STACK_CASES)),
           "seeds": np.array([c["seed"] for c in list(U.LAYER_CASES.values()) + list(U.STACK_CASES.values())])}
    for name in U.LAYER_CASES:
        do_layer(name, ref_fmt, out)
    for name in U.STACK_CASES:
        do_stack(name, ref_fmt, out)
    out["sha256"] = np.array(U.input_hash())
    np.savez_compressed(U.FIXTURE, **out)
    size = os.path.getsize(U.FIXTURE)
    print("wrote", U.FIXTURE, size, "bytes")
    assert size < 300_000, size


if __name__ == "__main__":
    main()
