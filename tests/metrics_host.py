"""Tests-only host restatement of the four image metrics of the reference's evaluate_folder (eval_suite.py:62-68) in numpy:
pixel values fl32(k) / 255, l1 / l2 summed in float64 over float32 differences, psnr with data_range 1, and skimage's SSIM
(7x7 uniform window, K1 0.01, K2 0.03, sample covariance, 3 px crop, channel mean) from separable 7-sums of float64 moments."""
import numpy as np


def _ssim_channel(x, y):
    H, W = x.shape
    mom = (x, y, x * x, y * y, x * y)
    m = []
    for a in mom:
        v = a[0:H - 6]
        for k in range(1, 7):
            v = v + a[k:k + H - 6]
        h = v[:, 0:W - 6]
        for k in range(1, 7):
            h = h + v[:, k:k + W - 6]
        m.append(h * (1.0 / 49.0))
    ux, uy, uxx, uyy, uxy = m
    cov_norm = 49.0 / 48.0
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.mean(dtype=np.float64)


def host_metrics(pred_u8, gt_u8):
    """(H,W,3) uint8 pred, (H,W,3|4) uint8 gt -> dict of python floats {l1, l2, psnr, ssim}."""
    p = pred_u8.astype(np.float32) / 255.0
    g = gt_u8[..., :3].astype(np.float32) / 255.0
    assert p.shape == g.shape and p.shape[-1] == 3 and min(p.shape[:2]) >= 7
    d = p - g
    l1 = float(np.abs(d).mean(dtype=np.float64))
    l2 = float((d * d).mean(dtype=np.float64))
    with np.errstate(divide="ignore"):
        psnr = float(10 * np.log10(1.0 / np.float64(l2)))
    x, y = p.astype(np.float64), g.astype(np.float64)
    ssim = float(np.mean([_ssim_channel(x[..., c], y[..., c]) for c in range(3)]))
    return dict(l1=l1, l2=l2, psnr=psnr, ssim=ssim)
