"""The depth estimator's matching stage without a GPU: diner_amd.mvs's torch restatement against fixture G28 (the reference's own float32
results and the float64 values, tests/golden/g28_mvs.npz, tools/make_golden_mvs.py), and the host logic around the kernels -- folding,
the DepthNet drop-in, the stage loop, the bridges to the renderer's batches, the PNG writer, the argument checks and the C symbols."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from diner_amd import _lib, formats, mvs
from tests import mvs_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("similarity", "weights", "prob", "confidence", "depth")
SYMBOLS = ("diner_mvs_cost_volume_f32", "diner_mvs_select_depth_f32", "diner_mvs_hypotheses_f32")


def test_symbols_declared_and_loaded():
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.diner_abi_version() == 6
    for macro, value in (("DINER_MVS_PIXELWISE_FLOATS", _lib.MVS_PIXELWISE_FLOATS), ("DINER_MVS_MAX_DEPTHS", _lib.MVS_MAX_DEPTHS),
                         ("DINER_MVS_MAX_CHANNELS", _lib.MVS_MAX_CHANNELS)):
        assert f"#define {macro} {value}" in header
    assert "mvs.hip" in open(os.path.join(ROOT, "diner_amd", "build.py")).read()


@pytest.mark.parametrize("name", list(U.CASES))
def test_restatement_against_fixture(name):
    """float64: the stored values to 1e-12.  float32: the reference's own results; bit-equal where this host's torch kernels are the
    generator's (printed), and in any case within the float32 noise the fixture records."""
    fx, inp = U.fixture(), U.case_inputs(name)
    r64, r32 = U.expected64(name), U.run_case(inp, torch.float32)
    for k in KEYS:
        assert np.abs(U.subsample(r64[k]) - fx[f"{name}_{k}64"]).max() <= 1e-12, (name, k)
        got, want = U.subsample(r32[k]), fx[f"{name}_{k}32"]
        assert got.dtype == np.float32 and want.dtype == np.float32
        print(f"{name} {k}: float32 restatement bit-equal to the reference: {np.array_equal(got, want)}")
        if k != "depth":
            bar = max(float(fx[f"{name}_err_{'prob' if k == 'confidence' else k}"]), 1e-7)
            assert np.abs(got.astype(np.float64) - want).max() <= bar, (name, k)
    assert r64["similarity"].shape == (U.CASES[name]["B"], U.CASES[name]["D"]) + U.CASES[name]["hw"]


def test_turned_view_gets_the_weight_of_zero():
    """Every sample of the turned camera is invalid (z < 0): its view weight is max_d sigmoid(net(0)) at every pixel."""
    inp, r = U.case_inputs("turned"), U.expected64("turned")
    pw = mvs.fold_pixelwise(U.cast(inp["state_dict"], torch.float64))
    zero = mvs.pixelwise_torch(pw.raw, torch.zeros(1, 1, 1, 1, 1, dtype=torch.float64)).item()
    w = r["weights"][:, U.SPECIAL_VIEW]
    assert float((w - zero).abs().max()) == 0.0 and 0.0 < zero < 1.0
    assert float((r["weights"][:, 0] - zero).abs().max()) > 1e-3          # the other views do see the plane


def test_shifted_view_has_partial_taps():
    """The shifted camera's samples leave the map through its edge: some land within one texel outside, where zero padding keeps part of
    the taps."""
    inp = U.cast(U.case_inputs("shifted"), torch.float64)
    v = U.SPECIAL_VIEW + 1
    proj = torch.unbind(inp["proj"], 1)
    P = torch.matmul(mvs._full_proj(proj[v]), torch.inverse(mvs._full_proj(proj[0])))
    H, W = U.CASES["shifted"]["hw"]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    xyz = torch.stack((xs, ys, torch.ones_like(xs)), 0).reshape(1, 3, 1, -1)
    p = (P[:, :3, :3] @ xyz.reshape(1, 3, -1)).unsqueeze(2) * inp["depth_values"].reshape(2, 1, -1, H * W) + P[:, :3, 3].reshape(2, 3, 1, 1)
    px = p[:, 0] / p[:, 2]
    partial = ((px > -1) & (px < 0)) | ((px > W - 1) & (px < W))
    outside = (px <= -1) | (px >= W)
    assert int(partial.sum()) > 20 and int(outside.sum()) > 200


@pytest.mark.parametrize("name", list(U.HYPOTHESES))
def test_hypotheses_against_fixture(name):
    fx, c, cur = U.fixture(), U.HYPOTHESES[name], U.hypotheses_inputs(name)
    h64 = mvs.depth_hypotheses(cur.double(), c["D"], c["interval"], c["image"], c["scale"])
    h32 = mvs.depth_hypotheses(cur, c["D"], c["interval"], c["image"], c["scale"])
    H, W = c["image"]
    assert tuple(h64.shape) == (c["B"], c["D"], H // c["scale"], W // c["scale"])
    assert np.abs(U.subsample(h64) - fx[f"hyp_{name}_64"]).max() <= 1e-12
    assert np.abs(U.subsample(h32).astype(np.float64) - fx[f"hyp_{name}_32"]).max() <= float(fx[f"hyp_{name}_err"])


def test_hypotheses_downsampling_is_two_taps_per_axis():
    """torch's trilinear resize does not low-pass: at scale 4 it averages the centre 2 x 2 of each 4 x 4 window."""
    cur = torch.arange(8 * 8, dtype=torch.float64).reshape(1, 8, 8)
    h = mvs.depth_hypotheses(cur, 2, 1.0, (8, 8), 4)
    lo = cur - 1.0
    assert torch.allclose(h[0, 0], torch.stack([lo[0, r:r + 2, c:c + 2].mean() for r in (1, 5) for c in (1, 5)]).reshape(2, 2), atol=1e-12)


def _device_depthnet(sd, dtype):
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(sd)
    return dn.to(dtype).eval()


def test_depthnet_and_coarse_to_fine_against_fixture():
    fx, s, inp = U.fixture(), U.STAGES, U.stage_inputs()
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        dn = _device_depthnet(inp["state_dict"], dt)
        with torch.no_grad():
            out = mvs.coarse_to_fine(U.cast(inp["features"], dt), U.cast(inp["proj"], dt), inp["depth_values"].to(dt), dn, U.regulariser,
                                     ndepths=s["ndepths"], ratios=s["ratios"], image_hw=s["image"], depth_interval=s["depth_interval"])
        assert set(out) == {"stage1", "stage2", "stage3", "depth", "photometric_confidence", "prob_volume", "depth_values"}
        assert out["depth"] is out["stage3"]["depth"]
        for i, (nd, sc) in enumerate(zip(s["ndepths"], s["scales"])):
            st = out[f"stage{i + 1}"]
            assert tuple(st["prob_volume"].shape) == (s["B"], nd, s["image"][0] // sc, s["image"][1] // sc)
            for k in ("depth", "photometric_confidence", "prob_volume", "depth_values"):
                tol = 1e-12 if tag == "64" else max(float(fx[f"stages_stage{i + 1}_err_prob_volume"]), float(fx[f"stages_stage{i + 1}_err_{k}"]))
                assert np.abs(U.subsample(st[k]).astype(np.float64) - fx[f"stages_stage{i + 1}_{k}{tag}"]).max() <= tol, (tag, i, k)


def test_depthnet_contract():
    """DepthNet.forward's contract: (dict, weights) when it computed the weights, else the dict; the reference's keys; its argument checks."""
    inp = U.case_inputs("probe")
    dn = _device_depthnet(inp["state_dict"], torch.float32)
    with torch.no_grad():
        out, w = dn(inp["features"], inp["proj"], inp["depth_values"], 8, U.regulariser)
        again = dn(inp["features"], inp["proj"], inp["depth_values"], 8, U.regulariser, view_weights=w)
    assert set(out) == {"depth", "photometric_confidence", "prob_volume", "depth_values"} and isinstance(again, dict)
    assert tuple(w.shape) == (2, 3, 23, 37) and not w.requires_grad
    assert torch.equal(out["prob_volume"], again["prob_volume"]) and out["depth_values"] is inp["depth_values"]
    assert not dn.uses_kernels(inp["features"])                  # CPU tensors: the restatement
    with pytest.raises(ValueError):
        dn(inp["features"], inp["proj"], inp["depth_values"], 9, U.regulariser)
    with pytest.raises(ValueError):
        dn(inp["features"][:-1], inp["proj"], inp["depth_values"], 8, U.regulariser)
    # with gradients enabled the restatement is differentiable down to the features and the net's parameters
    feats = [f.clone().requires_grad_(True) for f in inp["features"]]
    out, _ = dn(feats, inp["proj"], inp["depth_values"], 8, U.regulariser)
    out["prob_volume"][:, 3].sum().backward()
    assert feats[1].grad is not None and float(feats[1].grad.abs().max()) > 0
    assert float(dn.pixel_wise_net.conv0.conv.weight.grad.abs().max()) > 0


class _RefConvBn(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv, self.bn = nn.Conv3d(cin, cout, 1, bias=False), nn.BatchNorm3d(cout)


class _RefDepthNet(nn.Module):
    """A module with the state-dict keys of the reference's DepthNet."""

    def __init__(self):
        super().__init__()
        self.pixel_wise_net = nn.Module()
        self.pixel_wise_net.conv0, self.pixel_wise_net.conv1 = _RefConvBn(1, 16), _RefConvBn(16, 8)
        self.pixel_wise_net.conv2 = nn.Conv3d(8, 1, 1)


def test_state_dict_round_trip_through_from_module():
    ref = _RefDepthNet()
    ref.pixel_wise_net.load_state_dict(U.pixelwise_state_dict(7))
    ref.eval()
    dn = mvs.DeviceDepthNet.from_module(ref)
    assert not dn.training
    a, b = ref.state_dict(), dn.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    ref.load_state_dict(dn.state_dict())                            # and back, strictly
    assert {k[len("pixel_wise_net."):] for k in b if "num_batches" not in k} == set(mvs.PIXELWISE_KEYS)
    first = dn.pixelwise()
    assert dn.pixelwise() is first                                  # cached until a parameter changes
    with torch.no_grad():
        dn.pixel_wise_net.conv2.bias.add_(1.0)
    assert dn.pixelwise() is not first


def test_fold_pixelwise():
    """The folded net, evaluated in float64 from its 177 float32 values, is the unfolded net up to that one rounding."""
    sd = U.pixelwise_state_dict(11)
    pw = mvs.fold_pixelwise({"net." + k: v for k, v in sd.items()}, prefix="net.")
    f = pw.folded.double()
    assert pw.folded.dtype == torch.float32 and f.numel() == _lib.MVS_PIXELWISE_FLOATS
    s = torch.linspace(-1, 1, 41, dtype=torch.float64)
    h0 = torch.relu(f[0:16].view(16, 1) * s.view(1, -1) + f[16:32].view(16, 1))
    h1 = torch.relu(f[32:160].view(8, 16) @ h0 + f[160:168].view(8, 1))
    y = torch.sigmoid(f[168:176].view(1, 8) @ h1 + f[176])
    want = torch.sigmoid(_unfolded_logit(U.cast(sd, torch.float64), s))
    assert float((y.view(-1) - want).abs().max()) < 1e-6
    with pytest.raises(KeyError):
        mvs.fold_pixelwise(sd, prefix="missing.")


def _unfolded_logit(sd, s):
    x = s.view(1, 1, -1, 1, 1)
    for p in ("conv0.", "conv1."):
        x = torch.nn.functional.conv3d(x, sd[p + "conv.weight"])
        scale = (sd[p + "bn.weight"] / torch.sqrt(sd[p + "bn.running_var"] + 1e-5)).view(1, -1, 1, 1, 1)
        x = torch.relu((x - sd[p + "bn.running_mean"].view(1, -1, 1, 1, 1)) * scale + sd[p + "bn.bias"].view(1, -1, 1, 1, 1))
    return torch.nn.functional.conv3d(x, sd["conv2.weight"], sd["conv2.bias"]).reshape(-1)


@pytest.mark.parametrize("change, message", [(dict(C=6), "multiple of 4"), (dict(D=257), "depth hypotheses"), (dict(NS=16), "source views"),
                                             (dict(C=68), "multiple of 4")])
def test_refused_sizes(change, message):
    cfg = dict(B=1, NS=2, C=8, D=4, H=5, W=6)
    cfg.update(change)
    feats = [torch.zeros(cfg["B"], cfg["C"], cfg["H"], cfg["W"]) for _ in range(cfg["NS"] + 1)]
    proj = torch.zeros(cfg["B"], cfg["NS"] + 1, 2, 4, 4)
    depth = torch.ones(cfg["B"], cfg["D"], cfg["H"], cfg["W"])
    with pytest.raises(ValueError, match=message):
        mvs.cost_volume(feats, proj, depth, view_weights=torch.ones(cfg["B"], cfg["NS"], cfg["H"], cfg["W"]))


def test_argument_checks():
    feats = [torch.zeros(1, 8, 5, 6) for _ in range(3)]
    proj, depth, w = torch.zeros(1, 3, 2, 4, 4), torch.ones(1, 4, 5, 6), torch.ones(1, 2, 5, 6)
    pw = mvs.fold_pixelwise(U.pixelwise_state_dict(3))
    for bad in (lambda: mvs.cost_volume(feats, proj, depth),                                   # neither the net nor the weights
                lambda: mvs.cost_volume(feats, proj, depth, pw, w),                            # both
                lambda: mvs.cost_volume(feats, proj[:, :2], depth, view_weights=w),
                lambda: mvs.cost_volume(feats, proj, depth[:, :, :4], view_weights=w),
                lambda: mvs.cost_volume(feats[:1], proj[:, :1], depth, view_weights=w),
                lambda: mvs.depth_hypotheses(torch.ones(1, 5, 6), 1, 0.1, (20, 24), 4),        # one plane has no interval
                lambda: mvs.depth_hypotheses(torch.ones(1, 5, 6), 8, 0.1, (20, 24), 3),
                lambda: mvs.depth_hypotheses(torch.ones(5, 6), 8, 0.1, (20, 24), 4),
                lambda: mvs.coarse_to_fine([], {}, torch.ones(1, 8), None, None),
                lambda: mvs.to_source_maps(torch.ones(1, 5, 6), torch.ones(1, 5, 6), law="kitti")):
        with pytest.raises(ValueError):
            bad()


def test_proj_matrices_from_cameras():
    """The stage dict of datasets/dtu_yao.py: extrinsics untouched, the intrinsics' first two rows divided by the stage's scale, so that
    stage 2 is stage 1 times 2 and stage 3 stage 1 times 4 there."""
    inp = U.stage_inputs()
    E, K = torch.from_numpy(inp["extrinsics"]).float(), torch.from_numpy(inp["intrinsics"]).float()
    pm = mvs.proj_matrices_from_cameras(E, K)
    assert list(pm) == ["stage1", "stage2", "stage3"]
    for key in pm:
        assert tuple(pm[key].shape) == (2, 4, 2, 4, 4) and torch.equal(pm[key][:, :, 0], E)
        assert torch.equal(pm[key][:, :, 1, 3], torch.zeros(2, 4, 4)) and torch.equal(pm[key][:, :, 1, :3, 3], torch.zeros(2, 4, 3))
        assert torch.allclose(pm[key], inp["proj"][key], rtol=1e-6, atol=0)
    assert torch.equal(pm["stage3"][:, :, 1, :3, :3], K)
    assert torch.allclose(pm["stage2"][:, :, 1, :2], pm["stage1"][:, :, 1, :2] * 2) and torch.allclose(pm["stage3"][:, :, 1, :2], pm["stage1"][:, :, 1, :2] * 4)
    assert torch.equal(pm["stage1"][:, :, 1, 2, :3], K[:, :, 2])


def test_png_writer_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    depth = rng.uniform(0.0, 7.0, (13, 17)).astype(np.float32)          # some beyond the container's 6.5535
    depth[0, :4] = [0.0, 0.00014, 0.00026, 6.5535]                      # rounds to nearest, not down
    path = str(tmp_path / "d.png")
    q = formats.write_transmvsnet_png(path, torch.from_numpy(depth))
    assert q.dtype == np.uint16 and [int(v) for v in q[0, :4]] == [0, 1, 3, 65535] and int(q.max()) == 65535
    assert np.array_equal(q, (depth.clip(max=65535 * 1e-4) / 1e-4).round().astype(np.uint16))
    back = formats.read_transmvsnet_png(path)
    assert np.array_equal(back, q.astype(np.float32) * np.float32(1e-4))
    inside = depth <= 6.5535
    assert np.abs(back - depth)[inside].max() <= 0.5e-4 + 1e-6
    # the DTU factor: written times 0.7 / 872, read divided by it
    small = rng.uniform(400.0, 900.0, (5, 6)).astype(np.float32)
    formats.write_transmvsnet_png(path, small, dtu_rescale=True)
    assert np.abs(formats.read_transmvsnet_png(path, dtu_rescale=True) - small).max() <= 0.5e-4 / formats.DTU_DEPTH_RESCALE * 1.001
    with pytest.raises(ValueError):
        formats.write_transmvsnet_png(path, np.zeros((2, 3, 4), np.float32))


@pytest.mark.parametrize("law", ["dtu", "facescape", "multiface"])
def test_to_source_maps(law):
    r = U.expected64("probe")
    depth, conf = r["depth"].float(), r["confidence"].float()
    depth[0, 0, :5] = 0.0
    d, std = mvs.to_source_maps(depth, conf, law=law, dtu_rescale=(law == "dtu"))
    a, b = formats.CONF_TO_STD[law]
    want_d = depth / np.float32(formats.DTU_DEPTH_RESCALE) if law == "dtu" else depth
    want = a * conf + b
    if law == "multiface":
        want = want.clip(min=0)
        want[want_d == 0] = 0
        assert float(std[0, 0, :5].abs().max()) == 0.0
    assert torch.equal(d, want_d) and torch.equal(std, want) and d.dtype == torch.float32 and std.dtype == torch.float32


def test_fixture_inputs_are_the_generators():
    """The regenerated inputs are the ones the fixture was computed from."""
    import tools.make_golden_mvs as G
    fx = U.fixture()
    for name in U.CASES:
        assert str(fx[f"{name}_sha256"]) == G.sha256_of(U.case_inputs(name)), name
    inp = U.stage_inputs()
    assert str(fx["stages_sha256"]) == G.sha256_of({k: inp[k] for k in ("features", "proj", "depth_values", "state_dict")})
    assert os.path.getsize(U.FIXTURE) < 160 * 1024
