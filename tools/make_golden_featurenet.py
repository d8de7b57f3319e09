"""Fixture G31 (tests/golden/g31_featurenet.npz): the depth estimator's FeatureNet on seeded weights and images.

    python tools/make_golden_featurenet.py     # rewrites the fixture; needs the reference tree (build container only)

The weights and images are regenerated from seeds by tests/featurenet_util.py and are not stored (a sha256 of their bytes is).  The
reference's FeatureNet (models/module.py, models/dcn.py) is imported straight from the reference tree under make_golden_mvs's private
package; torchvision is not installed, so the package's `dcn.deform_conv2d` is bound to diner_amd.mvs.deform_conv2d_torch -- the
reference's own module code, wrappers and forward() then run around it.  (The restatement itself is held against torch's convolution, a
shifted image, an independent grid_sample statement and gradcheck by tests/test_featurenet_cpu.py.)  The generator asserts that
  * the reference's state-dict keys equal DeviceFeatureNet's;
  * DeviceFeatureNet's float32 torch route is torch.equal to that run on every stage of every case;
  * per deformable layer and case the learned offsets reach every branch of the sampling rule (featurenet_util.sample_coverage);
  * in the three-stage run the reference's argmax agrees with float64's outside the excluded pixels, whose share stays below
    mvs_util.EXCLUDED_CAP;
and then stores strided sub-samples of the float32 and float64 results, per case and stage `err`: the float32 run's distance (max
|difference|) from float64 -- the yardstick of the GPU tests, which allow the kernels featurenet_util.BAR_FACTOR times that --, the key
list and the sha256 of the regenerated inputs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs                                  # noqa: E402
from tests import featurenet_util as U                     # noqa: E402
from tests import fmt_util as FU                           # noqa: E402
from tests import mvs_util as MU                           # noqa: E402
from tools.make_golden_mvs import PKG, import_reference, sha256_of        # noqa: E402


def maxerr(a, b):
    return float((a.double() - b.double()).abs().max())


def reference_module(ref_module, sd):
    """The reference's FeatureNet with a seeded state dict, its deformable convolution on the restatement."""
    sys.modules[f"{PKG}.dcn"].deform_conv2d = mvs.deform_conv2d_torch
    net = ref_module.FeatureNet(base_channels=8)
    assert list(net.state_dict().keys()) == list(mvs.DeviceFeatureNet(8).state_dict().keys()), "state-dict keys differ from the reference's"
    net.load_state_dict(sd)
    return net.eval()


def do_case(name, ref_module, out):
    c = U.CASES[name]
    imgs = U.case_images(name)
    sd = U.featurenet_state_dict(c["seed"] + 50)
    ref = reference_module(ref_module, sd)
    with torch.no_grad():
        views = [ref(img) for img in torch.unbind(imgs, 1)]                  # TransMVSNet.forward's own loop
    ref32 = {k: torch.stack([v[k] for v in views], 0) for k in U.STAGES}
    got32, got64 = U.expected32(name), U.expected64(name)
    for stage in U.STAGES:
        assert torch.equal(got32[stage], ref32[stage]), (name, stage, "the float32 torch route differs from the reference's run")
        err = maxerr(ref32[stage], got64[stage])
        out[f"{name}_{stage}_32"], out[f"{name}_{stage}_64"] = U.subsample(ref32[stage]), U.subsample(got64[stage])
        out[f"{name}_err_{stage}"] = np.float64(err)
        print(f"{name} {stage}: {tuple(ref32[stage].shape)}, |values| <= {float(got64[stage].abs().max()):.2f}, reference float32 from float64 {err:.2e}")
    net = U.make_module(name)
    for layer, (x, om) in U.dcn_inputs(net, imgs.flatten(0, 1)).items():
        cov = U.sample_coverage(om, *x.shape[2:])
        print(f"  {name} {layer}: {tuple(x.shape)}, offsets sigma {float(om[:, :18].std()):.2f} px, logits sigma {float(om[:, 18:].std()):.2f}, {cov}")
        assert all(v > 0 for v in cov.values()), (name, layer, cov)
        assert 0.5 <= float(om[:, :18].std()) <= 4.0, (name, layer)
    out[f"{name}_sha256"] = np.array(sha256_of({"images": imgs, "state_dict": sd}))
    out[f"{name}_seed"] = np.int64(c["seed"])


def do_stage_run(ref_module, out):
    """depth_from_images on the three-stage scene: the float32 torch route of the feature net is the reference's (asserted per case above
    and here), the rest was pinned by fixtures G28 and G30."""
    imgs = U.stage_run_images()
    ref = reference_module(ref_module, U.featurenet_state_dict(U.STAGE_RUN_SEED))
    ours = U.make_module(U.STAGE_RUN_SEED)
    with torch.no_grad():
        for v, img in enumerate(torch.unbind(imgs, 1)):
            a, b = ref(img), ours(img)
            assert all(torch.equal(a[k], b[k]) for k in U.STAGES), v
    r32, r64 = U.stage_run_expected(torch.float32), U.stage_run_expected(torch.float64)
    for stage in U.STAGES:
        p32, p64 = r32[stage]["prob_volume"], r64[stage]["prob_volume"]
        err = maxerr(p32, p64)
        keep, excluded = MU.excluded_share(p64, err)
        assert bool((p32.argmax(1) == p64.argmax(1))[keep].all()), (stage, "the reference's argmax leaves float64's outside the excluded pixels")
        assert excluded < MU.EXCLUDED_CAP, (stage, excluded)
        out[f"run_{stage}_prob64"], out[f"run_{stage}_prob32"] = U.subsample(p64), U.subsample(p32)
        out[f"run_err_{stage}"], out[f"run_excluded_{stage}"] = np.float64(err), np.float64(excluded)
        print(f"stage run {stage}: prob {tuple(p64.shape)}, max prob {float(p64.max()):.3f}, reference float32 from float64 {err:.2e}, "
              f"excluded {100 * excluded:.2f} %")
    inp = MU.stage_inputs()
    out["run_sha256"] = np.array(sha256_of({"images": imgs, "inputs": {k: inp[k] for k in ("proj", "depth_values", "state_dict")},
                                            "feature": U.featurenet_state_dict(U.STAGE_RUN_SEED),
                                            "fmt": FU.fmt_state_dict(U.STAGE_RUN_SEED + 1)}))


def main():
    ref_module, _ = import_reference()
    out = {"keys": np.array(list(mvs.DeviceFeatureNet(8).state_dict().keys()))}
    for name in U.CASES:
        do_case(name, ref_module, out)
    do_stage_run(ref_module, out)
    np.savez_compressed(U.FIXTURE, **out)
    print("wrote", U.FIXTURE, os.path.getsize(U.FIXTURE), "bytes")
    assert os.path.getsize(U.FIXTURE) < 120 * 1024


if __name__ == "__main__":
    main()
