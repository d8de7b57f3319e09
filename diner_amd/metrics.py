"""Image-quality metrics on the device: the per-image scores of the reference's evaluate_folder (eval_suite.py:62-68) -- l1, l2
(skimage mean_squared_error), psnr (data_range 1) and ssim (skimage structural_similarity, channel_axis=-1, data_range=1) -- computed
by the HIP kernels of csrc/metrics.hip (C ABI: diner_image_metrics_u8 / _f32).  Like diner_amd.ops there is no CPU fallback."""
import torch

from . import _lib
from .ops import _ptr, _stream

lib = _lib.load()
KEYS = ("l1", "l2", "psnr", "ssim")


def _batch(t, name):
    """-> (tensor, route) with route "u8" for (N,H,W,C) uint8 and "f32" for (N,3,H,W) float32; a single image gains N = 1."""
    if t.dtype == torch.uint8:
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4:
            raise ValueError(f"image_metrics: {name} uint8 must be (N,H,W,C) or (H,W,C), got {tuple(t.shape)}")
        return t.contiguous(), "u8"
    if t.dtype == torch.float32:
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4 or t.shape[1] != 3:
            raise ValueError(f"image_metrics: {name} float32 must be (N,3,H,W) or (3,H,W), got {tuple(t.shape)}")
        return t.contiguous(), "f32"
    raise ValueError(f"image_metrics: {name} must be uint8 (N,H,W,C) or float32 (N,3,H,W), got {t.dtype}")


def image_metrics(pred, gt):
    """Scores of N image pairs on the device.

    pred / gt: uint8 (N,H,W,C) or (H,W,C) -- pred with 3 channels, gt with 3 or 4 (the alpha channel is dropped) -- or float32
    (N,3,H,W) or (3,H,W) renders / targets, quantised exactly as save_image (imageio.to_uint8) would write them.  Both tensors use the
    same route and live on the same HIP device.  Returns {"l1", "l2", "psnr", "ssim"} -> float64 tensors (N,) on that device.
    H and W must be at least 7 (the SSIM window), as skimage requires."""
    for t in (pred, gt):
        if not t.is_cuda:
            raise RuntimeError("image_metrics: tensors must live on a HIP device (MI355X); there is no CPU fallback")
    if pred.device != gt.device:
        raise ValueError(f"image_metrics: pred on {pred.device}, gt on {gt.device}")
    pred, route = _batch(pred, "pred")
    gt, route_gt = _batch(gt, "gt")
    if route != route_gt:
        raise ValueError("image_metrics: pred and gt must both be uint8 or both float32")
    if route == "u8":
        N, H, W, pc = pred.shape
        gc = gt.shape[3]
        if tuple(gt.shape[:3]) != (N, H, W):
            raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in size")
        if pc != 3:
            raise ValueError(f"image_metrics: pred has {pc} channels, need 3")
        if gc not in (3, 4):
            raise ValueError(f"image_metrics: gt has {gc} channels, need 3 or 4")
    else:
        N, _, H, W = pred.shape
        if gt.shape != pred.shape:
            raise ValueError(f"image_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in size")
    if N < 1:
        raise ValueError("image_metrics: empty batch")
    if H < 7 or W < 7:
        raise ValueError(f"image_metrics: {H}x{W} images; H and W must be at least 7 (the 7x7 SSIM window)")
    nbytes = lib.diner_image_metrics_workspace_bytes(N, H, W)
    if nbytes == 0:
        raise ValueError(f"image_metrics: {N} images of {H}x{W} exceed the kernel's grid")
    dev = pred.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(N, 4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if route == "u8":
            rc = lib.diner_image_metrics_u8(_ptr(pred), _ptr(gt), N, H, W, pc, gc, _ptr(ws), _ptr(out), _stream())
        else:
            rc = lib.diner_image_metrics_f32(_ptr(pred), _ptr(gt), N, H, W, _ptr(ws), _ptr(out), _stream())
        _lib.check(rc)
    return {k: out[:, i] for i, k in enumerate(KEYS)}
