"""Fixture G32 (tests/golden/g32_estimator_loss.npz): the depth estimator's fine-tuning objective and depth scores on seeded inputs.

    python tools/make_golden_estimator_loss.py      # rewrites the fixture; needs the reference tree (build container only)

The inputs are regenerated from seeds by tests/estimator_util.py and are not stored (their seeds, shapes and a sha256 of their bytes are).
Per case the fixture holds

  * `{case}_ref32_{total,depth_loss,epe,less1,less3}` and `{case}_ref32_grad_{stage}`: the reference's own float32 results --
    focal_loss_bld of deps/TransMVSNet/models/module.py, imported straight from the reference tree through make_golden_mvs.import_reference,
    on prob_volume = exp(log_softmax(cost [+ init])) as DepthNet forms it -- and d total / d cost by autograd;
  * `{case}_f64_*`: the float64 results of diner_amd.estimator's torch restatement on the same route;
  * `{case}_err_*`: per quantity the distance between the two (max |difference|) -- the yardstick of the tests, which allow
    estimator_util.BAR_FACTOR times that;
  * `{case}_scores_*`: Thres_metrics and AbsDepthError_metrics of the reference's utils.py (imported with stubs for the modules the two
    functions do not use) on image 0 of the stage-3 depth in float32, the restatement's float64 values and their distances;
  * `keys`: the state-dict keys of the reference's TransMVSNet().

The restatement is trusted only after its float64 run has been found equal to the reference run in float64: the stage terms and the
scores to 1e-12 relative, and the total after the same cast (the reference accumulates total_loss in a float32 tensor whatever the
volumes' dtype is).  At B > 1 the reference's epe / less1 / less3 broadcast a (B,) depth_interval along W, which is a bug
(estimator.focal_loss_bld's docstring); the reference is therefore handed the interval as (B,1,1), which broadcasts per image.  The
scores are taken on image 0 alone: image 1 of a case with B >= 2 has an empty mask, whose per-image mean is NaN in the reference too."""
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

from diner_amd import estimator                                  # noqa: E402
from tests import estimator_util as U                            # noqa: E402
from tools.make_golden_mvs import import_reference, sha256_of    # noqa: E402

from oracle.ref_import import REF_ROOT                            # noqa: E402


def import_reference_metrics():
    """Thres_metrics and AbsDepthError_metrics of the reference's utils.py; torchvision.utils, cv2 and matplotlib, which they do not use,
    are stubbed where they are not installed."""
    for name in ("torchvision", "torchvision.utils", "cv2", "matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["torchvision"], "utils"):
        sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    spec = importlib.util.spec_from_file_location("_g32_transmvsnet_utils", os.path.join(REF_ROOT, "deps", "TransMVSNet", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Thres_metrics, mod.AbsDepthError_metrics


def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300)


def reference_run(ref, name, dtype):
    """The reference's focal_loss_bld on the fixture's route -> (scalars, grads, stage terms)."""
    c = U.CASES[name]
    inputs, gts, masks, leaves = U.loss_inputs(name, U.fixture_route(name), dtype)
    for stage in inputs.values():
        if stage.get("prob_volume") is None:                      # the "init" route: DepthNet's own read-out
            stage["prob_volume"] = torch.exp(F.log_softmax(stage.pop("cost"), dim=1))
    interval = U.case_interval(name).to(dtype)
    B = c["B"]
    masks.setdefault("stage1", masks["stage3"])                   # the reference reads the device from mask_ms["stage1"]
    kw = {} if c["dlossw"] is None else {"dlossw": list(c["dlossw"])}
    total, depth_loss, epe, less1, less3 = ref.focal_loss_bld(inputs, gts, masks, interval[0] if B == 1 else interval.view(B, 1, 1), **kw)
    total.backward()
    scalars = dict(total=total.detach(), depth_loss=depth_loss.detach(), epe=epe.detach(), less1=less1.detach(), less3=less3.detach())
    terms = {}
    for key, stage in inputs.items():
        e, _ = ref.entropy_loss(stage["prob_volume"].detach(), gts[key], masks[key] > 0.5, stage["depth_values"])
        terms[key] = e.detach()
    return scalars, {k: v[0].grad for k, v in leaves.items()}, terms, inputs, gts, masks


def main():
    ref, ref_model = import_reference()
    thres_metrics, abs_metrics = import_reference_metrics()
    out = {"keys": np.array(list(ref_model.TransMVSNet().state_dict().keys()))}
    assert list(out["keys"]) == list(estimator.DeviceTransMVSNet().state_dict().keys()), "state-dict keys differ from the reference's"
    for name, c in U.CASES.items():
        route = U.fixture_route(name)
        out[f"{name}_seed"], out[f"{name}_shapes"] = np.array(c["seed"]), np.array([(c["B"],) + s for s in c["stages"]])
        out[f"{name}_sha256"] = np.array(sha256_of([{k: v for k, v in s.items()} for s in U.case_inputs(name)]))
        r32, g32, _, inputs32, gts32, masks32 = reference_run(ref, name, torch.float32)
        r64, g64, t64, inputs64, gts64, masks64 = reference_run(ref, name, torch.float64)
        s64, sg64 = U.expected(name, route, torch.float64)
        # the restatement against the reference in float64: the stage terms, then the total after the reference's float32 accumulator
        _, _, _, _, terms = estimator._accumulate_torch(*U.loss_inputs(name, route, torch.float64, requires_grad=False)[:3], c["dlossw"])
        acc = torch.zeros((), dtype=torch.float32)
        for key in t64:
            assert rel(terms[key][0], 2.0 * t64[key]) <= 1e-12, (name, key, float(terms[key][0]), float(t64[key]))
            w = 1.0 if c["dlossw"] is None else c["dlossw"][int(key[-1]) - 1]
            acc += w * terms[key][0].detach()
        assert float(acc) == float(r64["total"]), (name, float(acc), float(r64["total"]))
        for k in ("depth_loss", "epe", "less1", "less3"):
            assert rel(s64[k], r64[k]) <= 1e-12 or (np.isnan(float(s64[k])) and np.isnan(float(r64[k]))), (name, k, float(s64[k]), float(r64[k]))
        for key in g64:
            d = float((sg64[key] - g64[key]).abs().max())
            assert d <= 1e-12 * max(float(g64[key].abs().max()), 1e-30), (name, key, d)
        for k in U.SCALARS:
            out[f"{name}_ref32_{k}"], out[f"{name}_f64_{k}"] = np.array(float(r32[k]), dtype=np.float32), np.array(float(s64[k]))
            out[f"{name}_err_{k}"] = np.array(abs(float(r32[k]) - float(s64[k])))
        for key in g64:
            out[f"{name}_ref32_grad_{key}"], out[f"{name}_f64_grad_{key}"] = g32[key].numpy(), sg64[key].numpy()
            out[f"{name}_err_grad_{key}"] = np.array(float((g32[key].double() - sg64[key]).abs().max()))
        # the depth scores on the stage-3 depth
        est32, est64 = inputs32["stage3"]["depth"][:1], inputs64["stage3"]["depth"][:1]
        m = masks32["stage3"][:1] > 0.5
        rows = [("abs", lambda e, g: abs_metrics(e, g, m), lambda e, g: estimator.abs_depth_error_metrics_torch(e, g, m)),
                ("band", lambda e, g: abs_metrics(e, g, m, U.BAND), lambda e, g: estimator.abs_depth_error_metrics_torch(e, g, m, U.BAND))]
        for i, t in enumerate(U.THRESHOLDS):
            rows.append((f"thres{i}", lambda e, g, t=t: thres_metrics(e, g, m, t), lambda e, g, t=t: estimator.thres_metrics_torch(e, g, m, t)))
        for label, ref_fn, own_fn in rows:
            a32, a64, o64 = (float(ref_fn(est32, gts32["stage3"][:1])), float(ref_fn(est64, gts64["stage3"][:1])),
                             float(own_fn(est64, gts64["stage3"][:1])))
            assert rel(o64, a64) <= 1e-12 or (np.isnan(o64) and np.isnan(a64)), (name, label, o64, a64)
            out[f"{name}_scores_ref32_{label}"], out[f"{name}_scores_f64_{label}"] = np.array(a32, dtype=np.float32), np.array(o64)
            out[f"{name}_scores_err_{label}"] = np.array(abs(a32 - o64))
        print(name, {k: (float(out[f"{name}_f64_{k}"]), float(out[f"{name}_err_{k}"])) for k in U.SCALARS},
              {k: float(out[f"{name}_err_grad_{k}"]) for k in g64})
    os.makedirs(os.path.dirname(U.FIXTURE), exist_ok=True)
    np.savez_compressed(U.FIXTURE, **out)
    print(U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
