"""The training objective on the device: what the reference's DINER.calc_losses does around renderer.forward (src/models/diner.py:217-290)
-- the ray patch of the step, the rays of its pixels, the ground-truth colours at those pixels and MSELoss + w_antibias * AntibiasLoss
with its gradient -- in the HIP kernels of csrc/objective.hip and prep.hip (C ABI: diner_sample_patch, diner_gen_rays_at_f32,
diner_objective_f32).  Enqueue-only on the current stream; like diner_amd.ops there is no CPU fallback.

    losses = calc_losses(nerf, renderer, batch, znear=.., zfar=.., w_vgg=0.1, w_antibias=1., vgg_fn=my_vgg_loss)
    losses["total"].backward()
"""
import collections
import ctypes as C

import torch

from . import _lib
from .ops import _f32c, _ptr, _stream, gen_rays_at

lib = _lib.load()

Photometric = collections.namedtuple("Photometric", "rgb_fine antibias total losses_f64")


def _need_hip(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("diner_amd.objective: tensors must live on a HIP device (MI355X); there is no CPU fallback")


def sample_patch(fg, s, u=None, seed=0, step=0):
    """The s x s ray patch of a training step (diner.py:233-247): fg (SB,H,W) foreground weights >= 0 on a HIP device, u (SB) uniform
    numbers in [0, 1) or None (in-kernel Philox keyed by (seed, step, object)).  With pad = (s + 1) // 2 the first and last pad rows and
    columns never hold a centre; the centre is the first pixel in row-major order whose inclusive prefix sum of weights exceeds
    u * total.  -> pix (SB, s*s) int32 (y * W + x, rows of the patch first), centres (SB,2) int32 (x, y), flags (SB) int32: 1 where the
    padded mask was all zero and the image centre was taken instead (read it whenever convenient; nothing here waits for it)."""
    _need_hip(fg, u)
    fg = _f32c(fg)
    if fg.dim() != 3:
        raise ValueError(f"sample_patch: fg must be (SB,H,W), got {tuple(fg.shape)}")
    SB, H, W = fg.shape
    s = int(s)
    if s < 1 or s + 1 > min(H, W):
        raise ValueError(f"sample_patch: a patch of side {s} does not fit a {H}x{W} image (need 1 <= s and s + 1 <= min(H, W))")
    if u is not None:
        u = _f32c(u).reshape(-1)
        if u.numel() != SB:
            raise ValueError(f"sample_patch: u has {u.numel()} entries for {SB} objects")
    pix = torch.empty(SB, s * s, dtype=torch.int32, device=fg.device)
    centres = torch.empty(SB, 2, dtype=torch.int32, device=fg.device)
    flags = torch.empty(SB, dtype=torch.int32, device=fg.device)
    with torch.cuda.device(fg.device):
        _lib.check(lib.diner_sample_patch(_ptr(fg), SB, H, W, s, _ptr(u), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(step), _ptr(pix),
                                          _ptr(centres), _ptr(flags), _stream()))
    return pix, centres, flags


def objective(pred, gt, s=0, n_downsampling=3, w_antibias=0.0, w_mse=1.0):
    """One launch (plus the finalising one) for value and gradient: pred (SB,B,3); gt (SB,B,3), or the pair (images (SB,3,H,W),
    pix (SB,B) int32) whose colours are gathered in the kernel.  s: patch side (B == s*s, s a multiple of 2^n_downsampling) or 0 for
    loose pixels (then w_antibias must be 0).  -> losses (3) float64 on the device = {rgb_fine, antibias, w_mse rgb_fine +
    w_antibias antibias}, d_pred (SB,B,3) float32 = d losses[2] / d pred."""
    images = pix = None
    if isinstance(gt, (tuple, list)):
        images, pix = gt
        gt = None
    _need_hip(pred, gt, images, pix)
    pred = _f32c(pred)
    if pred.dim() != 3 or pred.shape[2] != 3:
        raise ValueError(f"objective: pred must be (SB,B,3), got {tuple(pred.shape)}")
    SB, B, _ = pred.shape
    H = W = 0
    if gt is not None:
        gt = _f32c(gt)
        if gt.shape != pred.shape:
            raise ValueError(f"objective: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ")
    else:
        images = _f32c(images)
        if images.dim() != 4 or images.shape[0] != SB or images.shape[1] != 3:
            raise ValueError(f"objective: images must be ({SB},3,H,W), got {tuple(images.shape)}")
        if pix.dtype != torch.int32 or tuple(pix.shape) != (SB, B):
            raise ValueError(f"objective: pix must be int32 ({SB},{B}), got {pix.dtype} {tuple(pix.shape)}")
        pix = pix.contiguous()
        H, W = int(images.shape[2]), int(images.shape[3])
    s, n = int(s), int(n_downsampling)
    if w_antibias > 0 and s == 0:
        raise ValueError("objective: the anti-bias term needs a patch (s > 0)")
    if s > 0 and (s * s != B or s % (1 << n) != 0):
        raise ValueError(f"objective: {B} rays per object are not a {s} x {s} patch whose side is a multiple of 2^{n}")
    nbytes = lib.diner_objective_workspace_bytes(SB, B, s, n)
    if nbytes == 0:
        raise ValueError(f"objective: sizes SB {SB}, B {B}, s {s}, n_downsampling {n} are outside what the kernel takes")
    dev = pred.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    losses = torch.empty(3, dtype=torch.float64, device=dev)
    d_pred = torch.empty_like(pred)
    with torch.cuda.device(dev):
        _lib.check(lib.diner_objective_f32(_ptr(pred), _ptr(gt), _ptr(images), _ptr(pix), SB, B, H, W, s, n, float(w_mse),
                                           float(w_antibias), _ptr(ws), _ptr(losses), _ptr(d_pred), _stream()))
    return losses, d_pred


class _PhotometricFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, images, pix, s, n, w_antibias, w_mse):
        losses, d_pred = objective(pred, gt if gt is not None else (images, pix), s, n, w_antibias, w_mse)
        ctx.save_for_backward(d_pred)
        rgb_fine, antibias, total = losses.to(torch.float32).unbind(0)
        ctx.mark_non_differentiable(rgb_fine, antibias, losses)
        return rgb_fine, antibias, total, losses

    @staticmethod
    def backward(ctx, g_rgb, g_antibias, g_total, g_losses):
        (d_pred,) = ctx.saved_tensors
        return (g_total * d_pred,) + (None,) * 7


def photometric(pred, gt, s=0, n_downsampling=3, w_antibias=0.0, w_mse=1.0):
    """MSELoss + w_antibias * AntibiasLoss(n_downsampling) as one autograd node (arguments as `objective`).  -> (rgb_fine, antibias,
    total, losses_f64): three 0-dim float32 device tensors -- `total` differentiable with respect to pred, its backward one
    elementwise product with the gradient the forward kept -- and the (3,) float64 tensor they are copies of."""
    images = pix = None
    if isinstance(gt, (tuple, list)):
        images, pix = gt
        gt = None
    return Photometric(*_PhotometricFn.apply(pred, gt, images, pix, int(s), int(n_downsampling), float(w_antibias), float(w_mse)))


def calc_losses(nerf, renderer, batch, *, znear, zfar, ray_batch_size=128, w_vgg=0., vgg_spatch=64, w_antibias=0.,
                antibias_downsampling=3, vgg_fn=None, seed=None, u=None, step=0, info=None, w_alpha=0.):
    """DINER.calc_losses (diner.py:217-290) for the drop-in modules: encode the batch's source views, pick the rays of the step, ONE
    renderer.forward, the objective.  -> {rgb_fine, vgg_fine, antibias, total}; total.backward() reaches the MLP parameters and
    encoder.latent.

    As in the reference, w_vgg != 0 selects the patch mode (a vgg_spatch x vgg_spatch patch per object whose centre is drawn from
    batch["target_alpha"][:, 0]; ray_batch_size is then vgg_spatch^2, diner.py:57) and w_vgg == 0 draws ray_batch_size loose pixels with
    torch.randint; the anti-bias term needs the patch (ValueError otherwise).  The perceptual term is supplied by the caller:
    vgg_fn(pred (SB,3,s,s), gt (SB,3,s,s)) -> scalar, differentiated by torch and added as w_vgg * vgg_fn(...) (src.losses.VGGLoss
    wraps a feature stack into such a function).  The patch centre comes from u (SB uniform numbers) or the in-kernel Philox generator
    keyed by (seed, step, object); seed None draws one from torch's global CPU generator.  batch["target_extrinsics"] /
    ["target_intrinsics"] are read on the host (keep them there to avoid the copy's wait).  info: an optional dict that receives the pixel
    indices of the step (`pix`), the sampler's per-object flag (`empty_mask`: 1 where the padded mask was all zero and the image centre
    was taken) the float64 losses (`losses_f64`) and the rendered colours (`pred`).
    w_alpha > 0 (not in the reference) supervises the ray's opacity: adds w_alpha * mean((alpha - batch["target_alpha"] at the step's
    pixels)^2), returned as losses["alpha"]; the opacity is a differentiable output of the compositor node
    (renderer.forward(want_alpha=True)).  With w_alpha == 0 nothing changes."""
    target = batch["target_rgb"]
    SB, _, H, W = target.shape
    if w_vgg > 0 and vgg_fn is None:
        raise ValueError("calc_losses: w_vgg > 0 needs vgg_fn (the VGG-19 weights are not part of this package; see src.losses.VGGLoss)")
    patch = w_vgg != 0
    if w_antibias > 0 and not patch:
        raise ValueError("calc_losses: w_antibias > 0 needs the patch mode (w_vgg != 0), as the reference's reshape does (diner.py:279-282)")
    _need_hip(target)
    nerf.encode(images=batch["src_rgbs"], depths=batch["src_depths"], depths_std=batch["src_depth_stds"],
                extrinsics=batch["src_extrinsics"], intrinsics=batch["src_intrinsics"])
    target = _f32c(target)
    if patch:
        s = int(vgg_spatch)
        if seed is None and u is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        pix, _, flags = sample_patch(batch["target_alpha"][:, 0], s, u=u, seed=seed or 0, step=step)
    else:
        s, flags = 0, None
        pix = torch.randint(0, H * W, (SB, int(ray_batch_size)), device=target.device, dtype=torch.int32)
    rays = gen_rays_at(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, pix)
    fine = renderer.forward(nerf, rays, want_alpha=True).fine if w_alpha > 0 else renderer.forward(nerf, rays).fine
    pred = fine.rgb
    ph = photometric(pred, (target, pix), s, antibias_downsampling, w_antibias if patch else 0.0)
    total, loss_vgg = ph.total, 0.
    if w_vgg > 0:
        gt_nchw = target.view(SB, 3, H * W).gather(2, pix.long()[:, None, :].expand(-1, 3, -1)).view(SB, 3, s, s)
        loss_vgg = vgg_fn(pred.view(SB, s, s, 3).permute(0, 3, 1, 2), gt_nchw)
        total = total + w_vgg * loss_vgg
    if info is not None:        # pix (SB,B) int32; empty_mask (SB) int32 on the device (None without a patch): 1 where the image centre was taken
        info.update(pix=pix, empty_mask=flags, losses_f64=ph.losses_f64, pred=pred)
    losses = dict(rgb_fine=ph.rgb_fine, vgg_fine=loss_vgg, antibias=ph.antibias if w_antibias > 0 else 0., total=total)
    if w_alpha > 0:
        gt_alpha = _f32c(batch["target_alpha"][:, 0]).to(target.device).view(SB, H * W).gather(1, pix.long())
        losses["alpha"] = (fine.alpha - gt_alpha).square().mean()
        losses["total"] = total + w_alpha * losses["alpha"]
    return losses
