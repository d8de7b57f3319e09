"""The kernels of csrc/mvs.hip on the device against fixture G28's yardsticks (tests/golden/g28_mvs.npz).

The yardstick is the float64 torch restatement (diner_amd.mvs on CPU tensors, which tests/test_mvs_cpu.py holds against the fixture's
float64 values and the reference's own float32 results).  The bar for similarity, view weights, prob volume, confidence and hypotheses
is mvs_util.BAR_FACTOR (4) times the distance the reference's float32 keeps from float64 on the same case, as the fixture records it: the
kernels sum the channels and the four taps in another order, contract to fused multiply-adds and use a homography rounded once from
float64.  Depth and argmax must agree with float64's wherever the float64 top-2 probability gap exceeds mvs_util.GAP_FACTOR (3) times
that case's float32 prob error; the share of the other pixels is printed and must stay below mvs_util.EXCLUDED_CAP (2 %).

Measured on an MI355X (max |kernel - float64| / bar; the bar is 4 x the reference float32's own error):
  see DESIGN.md section 8m."""
import ctypes as C

import numpy as np
import pytest
import torch

from diner_amd import _lib, formats, mvs
from tests import mvs_util as U

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _bar(fx, name, key):
    return U.BAR_FACTOR * float(fx[f"{name}_err_{'prob' if key == 'confidence' else key}"])


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _check_argmax(name, prob_dev, depth_dev, r64, err_prob):
    keep, excluded = U.excluded_share(r64["prob"], err_prob)
    print(f"{name}: excluded share {100 * excluded:.2f} % (cap {100 * U.EXCLUDED_CAP:.0f} %)")
    assert excluded <= U.EXCLUDED_CAP
    agree = prob_dev.cpu().argmax(1) == r64["prob"].argmax(1)
    assert bool(agree[keep].all()), f"{name}: {int((~agree & keep).sum())} pixels with a clear float64 winner got another plane"
    want = r64["depth"].float()                                     # the hypotheses are float32 inputs: the winner's value is exact
    assert bool((depth_dev.cpu() == want)[keep].all())


@pytest.mark.parametrize("name", list(U.CASES))
def test_kernels_against_float64(name):
    fx, inp, r64 = U.fixture(), U.case_inputs(name), U.expected64(name)
    got = U.run_case(inp, torch.float32, DEV)
    torch.cuda.synchronize()
    on_device = _restatement_on_device(inp)
    for k in ("similarity", "weights", "prob", "confidence"):
        e, bar, e_dev = _err(got[k], r64[k]), _bar(fx, name, k), _err(on_device[k], r64[k])
        print(f"{name} {k}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar if bar else 0:.2f}); torch on the device {e_dev:.2e}")
        assert got[k].shape == r64[k].shape and got[k].dtype == torch.float32
        assert e <= bar, (name, k, e, bar)
        # against the restatement run on the device: both within their distance of float64
        assert _err(got[k], on_device[k]) <= bar + e_dev, (name, k)
    _check_argmax(name, got["prob"], got["depth"], r64, float(fx[f"{name}_err_prob"]))
    assert torch.equal(got["confidence"], got["prob"].max(1).values)


def _restatement_on_device(inp):
    """The torch restatement (the reference's operations) in float32 on the device."""
    x = U.cast({k: v for k, v in inp.items() if k != "state_dict"}, torch.float32, DEV)
    pw = mvs.fold_pixelwise(U.cast(inp["state_dict"], torch.float32, DEV)) if x["view_weights"] is None else None
    with torch.no_grad():
        sim, w = mvs.cost_volume_torch(x["features"], x["proj"], x["depth_values"], pw, x["view_weights"])
        depth, conf, prob = mvs.select_depth_torch(U.regulariser(sim).squeeze(1), x["depth_values"], x["prob_init"])
    return dict(similarity=sim.squeeze(1), weights=w, depth=depth, confidence=conf, prob=prob)


def test_turned_view_weight_is_the_net_at_zero():
    inp = U.case_inputs("turned")
    got = U.run_case(inp, torch.float32, DEV)
    w = got["weights"][:, U.SPECIAL_VIEW]
    assert float(w.max() - w.min()) == 0.0                          # every pixel, both samples: one value
    pw = mvs.fold_pixelwise(U.cast(inp["state_dict"], torch.float64))
    zero = mvs.pixelwise_torch(pw.raw, torch.zeros(1, 1, 1, 1, 1, dtype=torch.float64)).item()
    assert abs(float(w[0, 0, 0]) - zero) <= _bar(U.fixture(), "turned", "weights")


@pytest.mark.parametrize("name", ["probe", "deep"])
def test_batch_position_does_not_matter(name):
    """A sample's outputs are the same bits at batch position 0 and 1."""
    inp = U.case_inputs(name)
    flipped = {k: ([f.flip(0) for f in v] if isinstance(v, list) else v.flip(0) if torch.is_tensor(v) else v) for k, v in inp.items()}
    a, b = U.run_case(inp, torch.float32, DEV), U.run_case(flipped, torch.float32, DEV)
    for k in a:
        assert torch.equal(a[k], b[k].flip(0)), k


def test_select_depth_without_prob_volume():
    inp = U.case_inputs("wide")
    x = U.cast({k: inp[k] for k in ("depth_values", "prob_init")}, torch.float32, DEV)
    cost = torch.randn(x["depth_values"].shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    d0, c0, p0 = mvs.select_depth(cost, x["depth_values"], x["prob_init"], return_prob=True)
    d1, c1, p1 = mvs.select_depth(cost.unsqueeze(1), x["depth_values"], x["prob_init"], return_prob=False)
    assert p1 is None and torch.equal(d0, d1) and torch.equal(c0, c1)
    d2, _, p2 = mvs.select_depth(cost, x["depth_values"], None)
    assert not torch.equal(p0, p2) and float((p2.sum(1) - 1).abs().max()) < 1e-5
    first = torch.zeros(1, 5, 3, 4, device=DEV)                     # all planes tie: the first index wins
    hyp = torch.arange(5, dtype=torch.float32, device=DEV).view(1, 5, 1, 1).expand(1, 5, 3, 4).contiguous() + 1
    d3, c3, _ = mvs.select_depth(first, hyp)
    assert float(d3.max()) == 1.0 and float(d3.min()) == 1.0 and abs(float(c3[0, 0, 0]) - 0.2) < 1e-6


def test_refused_sizes_return_the_error():
    """C = 6, D = 257 and NS = 16 come back as DINER_E_INVALID from the C entry (checked before any device work), and as ValueError from
    the wrappers."""
    lib = _lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    p = C.c_void_p(buf.data_ptr())
    ok = dict(B=1, NS=2, C=8, D=4, H=5, W=6)
    for change in (dict(C=6), dict(D=257), dict(NS=16), dict(C=68), dict(D=0)):
        a = dict(ok, **change)
        rc = lib.diner_mvs_cost_volume_f32(p, p, p, p, None, p, p, None, p, a["B"], a["NS"], a["C"], a["D"], a["H"], a["W"], None)
        assert rc == _lib.E_INVALID, change
        assert lib.diner_last_error()
    assert lib.diner_mvs_cost_volume_f32(p, p, p, p, p, p, p, p, p, 1, 2, 8, 4, 5, 6, None) == _lib.E_INVALID      # both the net and the weights
    assert lib.diner_mvs_hypotheses_f32(p, p, 1, 5, 6, 20, 24, 3, 8, C.c_float(0.1), None) == _lib.E_INVALID
    assert lib.diner_mvs_hypotheses_f32(p, p, 1, 5, 6, 20, 24, 4, 1, C.c_float(0.1), None) == _lib.E_INVALID
    feats = [torch.zeros(1, 6, 5, 6, device=DEV) for _ in range(3)]
    with pytest.raises(ValueError):
        mvs.cost_volume(feats, torch.zeros(1, 3, 2, 4, 4, device=DEV), torch.ones(1, 4, 5, 6, device=DEV),
                        view_weights=torch.ones(1, 2, 5, 6, device=DEV))


@pytest.mark.parametrize("name", list(U.HYPOTHESES))
def test_hypotheses_kernel(name):
    fx, c, cur = U.fixture(), U.HYPOTHESES[name], U.hypotheses_inputs(name)
    h64 = mvs.depth_hypotheses(cur.double(), c["D"], c["interval"], c["image"], c["scale"])
    got = mvs.depth_hypotheses(cur.to(DEV), c["D"], c["interval"], c["image"], c["scale"])
    e, bar = _err(got, h64), U.BAR_FACTOR * float(fx[f"hyp_{name}_err"])
    print(f"hypotheses {name}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == h64.shape and e <= bar


def _clean_footprint(agree, size):
    """(B,h,w) bool -> (B,H,W) bool: the pixels of the next stage whose bilinear footprint in the previous stage agrees everywhere."""
    up = torch.nn.functional.interpolate(agree.float().unsqueeze(1), size, mode="bilinear", align_corners=False).squeeze(1)
    return up == 1.0


def test_depthnet_and_coarse_to_fine_on_the_device():
    """DeviceDepthNet and the stage loop on HIP tensors against the three-stage run's float64 values.  A later stage is compared where
    the stages before it picked float64's plane throughout the pixel's footprint; where they did not, the pixel must be one the top-2
    gap criterion excludes in the stage that went the other way."""
    fx, s, inp = U.fixture(), U.STAGES, U.stage_inputs()
    runs = {}
    for dt, dev in ((torch.float64, None), (torch.float32, DEV)):
        dn = mvs.DeviceDepthNet()
        dn.pixel_wise_net.load_state_dict(inp["state_dict"])
        dn = dn.to(dt).eval()
        if dev is not None:
            dn = mvs.DeviceDepthNet.from_module(dn.to(dev))
            assert dn.uses_kernels([torch.zeros(1, device=DEV)]) is False         # gradients are enabled here
        with torch.no_grad():
            if dev is not None:
                assert dn.uses_kernels([torch.zeros(1, device=DEV)])
            runs[dt] = mvs.coarse_to_fine(U.cast(inp["features"], dt, dev), U.cast(inp["proj"], dt, dev), U.cast(inp["depth_values"], dt, dev), dn,
                                          U.regulariser, ndepths=s["ndepths"], ratios=s["ratios"], image_hw=s["image"],
                                          depth_interval=s["depth_interval"])
    clean = None
    for i, sc in enumerate(s["scales"]):
        key = f"stage{i + 1}"
        got, want = runs[torch.float32][key], runs[torch.float64][key]
        err = {k: float(fx[f"stages_{key}_err_{k}"]) for k in ("prob_volume", "photometric_confidence", "depth_values")}
        if clean is None:
            clean = torch.ones(want["depth"].shape, dtype=torch.bool)
        for k in ("depth_values", "prob_volume", "photometric_confidence"):
            diff = (got[k].cpu().double() - want[k]).abs()
            diff = diff[clean.unsqueeze(1).expand_as(diff)] if diff.dim() == 4 else diff[clean]
            e, bar = float(diff.max()), U.BAR_FACTOR * max(err[k], err["prob_volume"] if k != "depth_values" else 0.0)
            print(f"{key} {k}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}) on {100 * float(clean.double().mean()):.1f} % of the pixels")
            assert e <= bar, (key, k)
        keep, excluded = U.excluded_share(want["prob_volume"], err["prob_volume"])
        agree = got["prob_volume"].cpu().argmax(1) == want["prob_volume"].argmax(1)
        print(f"{key}: excluded share {100 * excluded:.2f} %, winners that differ {int((~agree & clean).sum())}")
        assert excluded <= U.EXCLUDED_CAP and bool(agree[keep & clean].all())
        assert bool((got["depth"].cpu() == got["depth_values"].cpu().gather(1, got["prob_volume"].cpu().argmax(1, keepdim=True)).squeeze(1)).all())
        if i + 1 < len(s["scales"]):
            H, W = s["image"]
            nxt = s["scales"][i + 1]
            full = _clean_footprint(agree & clean, (H, W))                        # the previous depth goes to the image size first
            clean = torch.nn.functional.avg_pool2d(full.float().unsqueeze(1), nxt).squeeze(1) == 1.0 if nxt > 1 else full
    assert runs[torch.float32]["depth"].is_cuda and runs[torch.float32]["stage3"]["depth"].shape == (2, 24, 40)


def test_cameras_to_source_maps_on_the_device(tmp_path):
    """A batch's cameras and per-view stage features -> src_depths / src_depth_stds on the device, and the PNG round trip of the same
    maps: what the data sets would have read back, up to the container's 1e-4 quantisation."""
    s, inp = U.STAGES, U.stage_inputs()
    E, K = torch.from_numpy(inp["extrinsics"]).float().to(DEV), torch.from_numpy(inp["intrinsics"]).float().to(DEV)
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(inp["state_dict"])
    dn = dn.to(DEV).eval()
    with torch.no_grad():
        out = mvs.coarse_to_fine(U.cast(inp["features"], torch.float32, DEV), mvs.proj_matrices_from_cameras(E, K),
                                 inp["depth_values"].to(DEV), dn, U.regulariser, ndepths=s["ndepths"], ratios=s["ratios"], image_hw=s["image"],
                                 depth_interval=s["depth_interval"])
        depths, stds = mvs.to_source_maps(out["depth"], out["photometric_confidence"], law="facescape")
    assert depths.is_cuda and stds.is_cuda and depths.shape == stds.shape == (2, 24, 40)
    a, b = formats.CONF_TO_STD["facescape"]
    assert torch.equal(stds, a * out["photometric_confidence"] + b)
    reach = sum(nd / 2 * r * s["depth_interval"] for nd, r in zip(s["ndepths"][1:], s["ratios"][1:]))     # how far stages 2 and 3 can leave stage 1's range
    assert s["depth_range"][0] - reach - 1e-5 <= float(depths.min()) and float(depths.max()) <= s["depth_range"][1] + reach + 1e-5
    path = str(tmp_path / "depth.png")
    formats.write_transmvsnet_png(path, depths[0])
    back = formats.read_transmvsnet_png(path)
    assert np.abs(back - depths[0].cpu().numpy()).max() <= 0.5e-4 + 1e-6
