"""Generate tests/golden/g24_image_metrics.npz: the reference's per-image scores (eval_suite.py:62-68) on seeded uint8 pairs.

    python tools/make_golden_metrics.py SKIMAGE_DIR [REFERENCE_DIR]

The reference pins scikit-image 0.19.3.  SKIMAGE_DIR is a scikit-image 0.18.3 package tree (the directory holding
metrics/_structural_similarity.py); its metrics modules are loaded under numpy 2 with three shims -- the np.bool8 / np.float_ /
np.complex_ aliases, package stubs for skimage, skimage.util, skimage._shared and skimage.metrics (so that no package __init__ runs)
and skimage.util.img_as_float taken from skimage.util.dtype.  For every pair of diner_amd.synthetic.METRIC_CASES it stores:
  - ssim (multichannel=True, the 0.18 spelling of channel_axis=-1), psnr and mse with data_range=1 from that skimage;
  - l1 as eval_suite.py:68 writes it (np.mean of float32 |pred - gt|) and the same mean in float64 (l1_f64); their difference is
    the float32 accumulation error of the reference, the yardstick of the l1 comparison;
  - ssim_f32: the same SSIM steps on float32 arrays (scipy uniform_filter in float32), which is what 0.19 is believed to do with
    float32 inputs; reported as the size of the 0.18 / 0.19 gap, never asserted against;
  - sha256 of the regenerated pred / gt bytes (no images are stored).
With REFERENCE_DIR it also stores the reference's public names of src/evaluation/eval_suite.py, parsed with ast (no code is run):
the module constants and evaluate_folder's parameter names."""
import ast
import hashlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diner_amd.synthetic import METRIC_CASES, metric_pair   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g24_image_metrics.npz")
CONSTANTS = ("METRIC_OPT_DICT", "METRIC_LIMIT_DICT", "AVERAGE_SCORE_FILENAME", "REPORT_DETAIL_FILENAME", "EXAMPLE_PLOT_FILENAME",
             "N_EXAMPLE_PLOTS", "PRED_SUFFIX", "GT_SUFFIX", "REF_SUFFIX", "DEPTH_SUFFIX")


def load_skimage(tree):
    for alias, target in (("bool8", np.bool_), ("float_", np.float64), ("complex_", np.complex128)):
        if not hasattr(np, alias):
            setattr(np, alias, target)
    for name, sub in (("skimage", ""), ("skimage.util", "util"), ("skimage._shared", "_shared"), ("skimage.metrics", "metrics")):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(tree, sub) if sub else tree]
        sys.modules[name] = m
    import importlib
    dtype = importlib.import_module("skimage.util.dtype")
    sys.modules["skimage.util"].img_as_float = dtype.img_as_float
    ssim_mod = importlib.import_module("skimage.metrics._structural_similarity")
    simple = importlib.import_module("skimage.metrics.simple_metrics")
    version = None
    with open(os.path.join(tree, "__init__.py")) as f:
        for line in f:
            if line.startswith("__version__"):
                version = line.split("=")[1].strip().strip("'\"")
    return ssim_mod.structural_similarity, simple.peak_signal_noise_ratio, simple.mean_squared_error, version


def ssim_f32(p, g):
    """SSIM by the same steps as skimage 0.18, but on float32 arrays throughout (uniform_filter in float32)."""
    from scipy.ndimage import uniform_filter
    vals = []
    for c in range(3):
        x, y = p[..., c], g[..., c]
        f = lambda a: uniform_filter(a, size=7)                     # noqa: E731
        ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
        cn = np.float32(49 / 48)
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        C1, C2 = np.float32(0.01 ** 2), np.float32(0.03 ** 2)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        vals.append(S[3:-3, 3:-3].mean(dtype=np.float64))
    return float(np.mean(vals))


def reference_names(ref_dir):
    path = os.path.join(ref_dir, "src", "evaluation", "eval_suite.py")
    tree = ast.parse(open(path).read())
    consts, params = {}, None
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
            if name in CONSTANTS:
                v = node.value
                if isinstance(v, ast.Call) and isinstance(v.func, ast.Name) and v.func.id == "dict":
                    consts[name] = {kw.arg: ast.literal_eval(kw.value) for kw in v.keywords}
                else:
                    consts[name] = ast.literal_eval(v)
        if isinstance(node, ast.FunctionDef) and node.name == "evaluate_folder":
            params = [a.arg for a in node.args.args]
    assert set(consts) == set(CONSTANTS) and params, (sorted(consts), params)
    return consts, params


def main():
    ssim, psnr, mse, version = load_skimage(sys.argv[1])
    rows, shas = [], []
    for kind, H, W, seed in METRIC_CASES:
        pu, gu = metric_pair(kind, H, W, seed)
        shas.append(hashlib.sha256(pu.tobytes()).hexdigest() + hashlib.sha256(gu.tobytes()).hexdigest())
        pred = pu.astype(np.float32) / 255.0                     # eval_suite.py:63-64
        gt = gu.astype(np.float32)[..., :3] / 255.0
        with np.errstate(divide="ignore"):
            s = ssim(pred, gt, multichannel=True, data_range=1)
            ps = psnr(pred, gt, data_range=1)
        m = mse(pred, gt)
        l1 = np.mean(np.abs(pred - gt))                          # float32, as eval_suite.py:68
        l1_64 = np.abs(pred - gt).mean(dtype=np.float64)
        rows.append([s, ps, m, float(l1), float(l1_64), ssim_f32(pred, gt)])
        print(f"{kind:9s} {H:4d}x{W:<4d} ssim {s:.15f} psnr {ps:.12f} mse {m:.6e} l1 f32-f64 {float(l1) - l1_64:+.2e} "
              f"ssim f32-f64 {rows[-1][5] - s:+.2e}")
    out = dict(cases=np.array([f"{k}:{h}:{w}:{s}" for k, h, w, s in METRIC_CASES]), sha=np.array(shas),
               scores=np.array(rows, np.float64), columns=np.array(["ssim", "psnr", "mse", "l1", "l1_f64", "ssim_f32"]),
               skimage_version=np.array(version))
    if len(sys.argv) > 2:
        consts, params = reference_names(sys.argv[2])
        out["ref_constants_json"] = np.array(json.dumps(consts, sort_keys=True))
        out["ref_evaluate_folder_params"] = np.array(params)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, "skimage", version)


if __name__ == "__main__":
    main()
