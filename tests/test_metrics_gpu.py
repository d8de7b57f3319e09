"""Image metrics on the device (diner_amd.metrics / csrc/metrics.hip) against skimage 0.18.3's scores of G24 and the host
restatement, the fp32 route against to_uint8 + the uint8 route, determinism, and the evaluation path end to end on the DTU fixture
(diner_amd.evaluate.write_prediction_folder -> src.evaluation.eval_suite.evaluate_folder)."""
import json
import os

import numpy as np
import pytest
import torch

from diner_amd.synthetic import metric_pair
from tests.metrics_host import host_metrics
from tests.test_metrics_cpu import g24_rows

pytestmark = pytest.mark.gpu
KEYS = ("l1", "l2", "psnr", "ssim")


def dev_scores(pred, gt):
    from diner_amd.metrics import image_metrics
    s = image_metrics(pred, gt)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in s.items()}


def test_metrics_match_skimage_g24():
    for case, p, gt, ref in g24_rows():
        s = dev_scores(torch.from_numpy(p).cuda(), torch.from_numpy(gt).cuda())
        assert abs(s["ssim"][0] - ref["ssim"]) <= 1e-9, (case, s["ssim"][0], ref["ssim"])
        if np.isinf(ref["psnr"]):
            assert s["psnr"][0] == ref["psnr"], case
        else:
            assert abs(s["psnr"][0] - ref["psnr"]) <= 1e-9, case
        assert abs(s["l2"][0] - ref["mse"]) <= 1e-12 * ref["mse"], case
        yard = max(1e-12 * ref["l1_f64"], abs(ref["l1"] - ref["l1_f64"]))
        assert abs(s["l1"][0] - ref["l1"]) <= yard, case
        assert abs(s["l1"][0] - ref["l1_f64"]) <= 1e-12 * ref["l1_f64"], case


def _check_host(s, pairs):
    for j, (p, g) in enumerate(pairs):
        h = host_metrics(p, g)
        assert abs(s["ssim"][j] - h["ssim"]) <= 1e-12, j
        assert abs(s["psnr"][j] - h["psnr"]) <= 1e-10, j
        assert abs(s["l2"][j] - h["l2"]) <= 1e-12 * h["l2"], j
        assert abs(s["l1"][j] - h["l1"]) <= 1e-12 * h["l1"], j


def test_metrics_large_batches_match_host():
    kinds = ("uniform", "smooth", "object", "near")
    pairs = [metric_pair(kinds[i % 4], 1024, 1024, 100 + i) for i in range(16)]
    s = dev_scores(torch.from_numpy(np.stack([p for p, _ in pairs])).cuda(), torch.from_numpy(np.stack([g for _, g in pairs])).cuda())
    _check_host(s, pairs)
    pairs = [metric_pair(k, 600, 800, 200 + i) for i, k in enumerate(("smooth", "object", "rgba"))]
    gts = [g[..., :3] for _, g in pairs]
    s = dev_scores(torch.from_numpy(np.stack([p for p, _ in pairs])).cuda(), torch.from_numpy(np.stack(gts)).cuda())
    _check_host(s, pairs)


def test_f32_route_equals_quantised_u8_route():
    from diner_amd.imageio import to_uint8
    g = torch.Generator().manual_seed(11)
    N, H, W = 3, 61, 83
    pred = torch.rand(N, 3, H, W, generator=g) * 1.4 - 0.2            # values outside [0, 1] too
    gt = torch.rand(N, 3, H, W, generator=g)
    pred[0, 1, 5, 7:20] = float("nan")
    gt[2, 0, 30, :] = float("nan")
    pred[1, 2, :4, :4] = float("inf")
    gt[1, 0, 9, 9] = float("-inf")
    pred, gt = pred.cuda(), gt.cuda()
    a = dev_scores(pred, gt)
    pu = torch.stack([to_uint8(pred[i]) for i in range(N)])
    gu = torch.stack([to_uint8(gt[i]) for i in range(N)])
    b = dev_scores(pu, gu)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    _check_host(b, [(pu[i].cpu().numpy(), gu[i].cpu().numpy()) for i in range(N)])


def test_metrics_deterministic_and_position_independent():
    pairs = [metric_pair(k, 257, 301, 300 + i) for i, k in enumerate(("uniform", "smooth", "object", "near", "rgba"))]
    P = torch.from_numpy(np.stack([p for p, _ in pairs])).cuda()
    G = torch.from_numpy(np.stack([g[..., :3] for _, g in pairs])).cuda()
    first = dev_scores(P, G)
    for _ in range(3):
        again = dev_scores(P, G)
        assert all(np.array_equal(first[k], again[k]) for k in KEYS)
    perm = [3, 0, 4, 2, 1]
    s = dev_scores(P[perm], G[perm])
    for j, i in enumerate(perm):
        single = dev_scores(P[i], G[i])
        for k in KEYS:
            assert s[k][j] == first[k][i] == single[k][0], (k, i)
    # the RGBA gt drops its alpha: same scores as the RGB gt
    ga = torch.from_numpy(pairs[4][1]).cuda()
    s4 = dev_scores(P[4], ga)
    assert all(s4[k][0] == first[k][4] for k in KEYS)


def test_metrics_edge_cases():
    from diner_amd.metrics import image_metrics
    x = torch.randint(0, 256, (2, 6, 40, 3), dtype=torch.uint8).cuda()
    with pytest.raises(ValueError):
        image_metrics(x, x)
    with pytest.raises(ValueError):
        image_metrics(torch.rand(3, 40, 6).cuda(), torch.rand(3, 40, 6).cuda())
    with pytest.raises(ValueError):
        image_metrics(torch.zeros(8, 8, 4, dtype=torch.uint8).cuda(), torch.zeros(8, 8, 3, dtype=torch.uint8).cuda())
    with pytest.raises(RuntimeError):
        image_metrics(torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8))
    for H, W in ((7, 7), (64, 9), (100, 300)):
        a = torch.randint(0, 256, (2, H, W, 3), dtype=torch.uint8).cuda()
        s = dev_scores(a, a.clone())
        assert (s["psnr"] == np.inf).all() and (s["ssim"] == 1.0).all() and (s["l1"] == 0).all() and (s["l2"] == 0).all()


@pytest.fixture(scope="module")
def dtu_eval(tmp_path_factory):
    from diner_amd.datasets import DTUSamples, collate
    from diner_amd.evaluate import write_prediction_folder
    from diner_amd.synthetic import make_mlp_state_dict
    from src.util.import_helper import import_obj
    from tests.helpers import GOLD
    from tests.test_boundary_cpu import build_nerf
    tree = os.path.join(GOLD, "dtu_tiny")
    ds = DTUSamples(tree, "val", scan_list=os.path.join(tree, "scan_list.txt"))
    torch.manual_seed(0)
    nerf = build_nerf().cuda().eval()
    nerf.mlp_fine.load_state_dict(make_mlp_state_dict())
    ren = import_obj("src.models.nerf_renderer.NeRFRendererDGS")(n_samples=64, n_gaussian=24, n_depth_candidates=1000,
                                                                 white_bkgd=False)
    vis = tmp_path_factory.mktemp("eval") / "visualizations"
    batches = [collate([ds[i]]) for i in (17, 45)]         # two samples whose views the fixture holds (17 is G13's)
    torch.manual_seed(1)
    scores = write_prediction_folder(nerf, ren, batches, str(vis), ds.znear, ds.zfar, ray_batch_size=8192)
    return vis, scores


def test_write_prediction_folder_and_evaluate_folder(dtu_eval):
    from diner_amd.png import read_png
    from src.evaluation import eval_suite as E
    vis, scores = dtu_eval
    names = scores["sample_name"]
    assert len(names) >= 1
    for stem in names:
        for suf in (E.PRED_SUFFIX, E.DEPTH_SUFFIX, E.REF_SUFFIX, E.GT_SUFFIX):
            assert (vis / (stem + suf)).exists(), stem + suf
    out = vis.parent
    with pytest.warns(UserWarning, match="lpips"):
        avg = E.evaluate_folder(str(vis), str(out))
    assert "lpips" not in avg
    for f in (E.AVERAGE_SCORE_FILENAME, E.REPORT_DETAIL_FILENAME, E.EXAMPLE_PLOT_FILENAME):
        assert (out / f).exists(), f
    assert json.load(open(out / E.AVERAGE_SCORE_FILENAME)) == avg
    report = json.load(open(out / E.REPORT_DETAIL_FILENAME))
    by_name = {os.path.basename(r["path"])[:-len(E.PRED_SUFFIX)]: r for r in report}
    dev = {k: scores[k].cpu().numpy() for k in KEYS}
    for j, stem in enumerate(names):
        r = by_name[stem]
        for k in KEYS:
            assert r[k] == dev[k][j], (stem, k)           # the PNG route scores exactly what the render route scored
        h = host_metrics(read_png(vis / (stem + E.PRED_SUFFIX)), read_png(vis / (stem + E.GT_SUFFIX)))
        assert abs(h["ssim"] - r["ssim"]) <= 1e-12 and abs(h["psnr"] - r["psnr"]) <= 1e-10
        assert abs(h["l2"] - r["l2"]) <= 1e-12 * h["l2"] and abs(h["l1"] - r["l1"]) <= 1e-12 * h["l1"]
    order = [names.index(os.path.basename(r["path"])[:-len(E.PRED_SUFFIX)]) for r in report]
    for k in KEYS:
        assert avg[k] == float(np.mean([dev[k][i] for i in order])), k
    ex = read_png(out / E.EXAMPLE_PLOT_FILENAME)
    pred = read_png(vis / (names[0] + E.PRED_SUFFIX))
    nref = read_png(vis / (names[0] + E.REF_SUFFIX)).shape[1] // pred.shape[1]
    assert ex.shape == (5 * pred.shape[0], (nref + 3) * pred.shape[1], 3)


def test_evaluate_folder_lpips_fn(dtu_eval, tmp_path):
    from diner_amd.evaluate import evaluate_folder
    vis, _ = dtu_eval
    seen = []

    def stub(pred, gt):
        assert pred.is_cuda and gt.is_cuda and pred.dim() == 4 and pred.shape[:2] == (1, 3) and pred.shape == gt.shape
        assert pred.dtype == torch.float32 and pred.min() >= -1 and pred.max() <= 1 and gt.min() >= -1 and gt.max() <= 1
        v = float((pred - gt).abs().mean())
        seen.append(v)
        return torch.tensor([[[[v]]]], device=pred.device)

    avg = evaluate_folder(vis, tmp_path, lpips_fn=stub)
    assert len(seen) >= 1 and avg["lpips"] == float(np.mean(seen))
    report = json.load(open(tmp_path / "detailed_report.json"))
    assert [r["lpips"] for r in report] == seen
