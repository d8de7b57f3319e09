"""Fine-tuning the multi-view depth estimator: what the reference's deps/TransMVSNet/finetune.py does around the model -- the objective
(models/module.py:490-587: entropy_loss, focal_loss_bld, trans_mvsnet_loss), the depth scores (utils.py:240-274: Thres_metrics,
AbsDepthError_metrics), the warm-up / multi-step learning rate (utils.py:323-367), the loop and the {epoch, model, optimizer} checkpoints
(finetune.py:96-100, 343-347) -- and the whole estimator as one module under the reference's state-dict keys (DeviceTransMVSNet).

On float32 HIP tensors the objective and the scores run on the kernels of csrc/mvsloss.hip: per stage one forward launch, one finish
launch and, in the backward pass, one launch that writes the gradient volume; no probability, one-hot or log volume is formed and nothing
is read back.  On CPU tensors, other dtypes or with force_torch=True they run a torch restatement with the reference's operations in the
reference's order (`*_torch`, any floating dtype), which is the host oracle of the tests and the baseline of
tools/time_estimator_loss.py.

    model = DeviceTransMVSNet().to("cuda"); model.load_state_dict(torch.load(path)["model"])
    history, opt = fit_estimator(model, batches, steps=1000, lr=1e-3, milestones=(600, 800), dlossw=(1, 1, 1))
    save_estimator_checkpoint("model_000001.ckpt", model, opt, epoch=1)
"""
import itertools
from bisect import bisect_right

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import mvs

ENTROPY_WEIGHT = 2.0               # module.py:540, 567
SCORE_UNIT = 192.0 / 128.0         # focal_loss_bld scales the stage-3 error by depth_interval * 192 / 128
SCORE_THRESHOLDS = (1.0, 3.0)      # less1, less3
LOSS_TERMS = ("total", "depth_loss", "epe", "less1", "less3")


def _ops():
    from . import ops              # loads libdiner_hip.so; only the device route needs it
    return ops


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------
def _hypothesis_volume(depth_value, shape):
    if depth_value.dim() < 3:      # (B,D) -> (B,D,H,W), as the reference repeats it
        return depth_value.repeat(shape[1], shape[2], 1, 1).permute(2, 3, 0, 1)
    return depth_value


def stage_prob_volume(stage):
    """A stage dict's probability volume: its "prob_volume", or for a fused_readout stage exp(log_softmax("cost"))."""
    if stage.get("prob_volume") is not None:
        return stage["prob_volume"]
    return torch.exp(F.log_softmax(stage["cost"], dim=1))


def entropy_loss_torch(prob_volume, depth_gt, mask, depth_value, return_prob_map=False):
    """entropy_loss (module.py:490-526) operation by operation, in prob_volume's dtype."""
    mask_true = mask
    valid_pixel_num = torch.sum(mask_true, dim=[1, 2]) + 1e-6
    shape = depth_gt.shape
    depth_num = depth_value.shape[1]
    depth_value_mat = _hypothesis_volume(depth_value, shape)
    gt_index_image = torch.argmin(torch.abs(depth_value_mat - depth_gt.unsqueeze(1)), dim=1)
    gt_index_image = torch.mul(mask_true, gt_index_image.type(torch.float))
    gt_index_image = torch.round(gt_index_image).type(torch.long).unsqueeze(1)
    gt_index_volume = torch.zeros(shape[0], depth_num, shape[1], shape[2], dtype=mask_true.dtype, device=mask_true.device).scatter_(1, gt_index_image, 1)
    cross_entropy_image = -torch.sum(gt_index_volume * torch.log(prob_volume + 1e-6), dim=1).squeeze(1)
    masked_cross_entropy_image = torch.mul(mask_true, cross_entropy_image)
    masked_cross_entropy = torch.sum(masked_cross_entropy_image, dim=[1, 2])
    masked_cross_entropy = torch.mean(masked_cross_entropy / valid_pixel_num)
    wta_index_map = torch.argmax(prob_volume, dim=1, keepdim=True).type(torch.long)
    wta_depth_map = torch.gather(depth_value_mat, 1, wta_index_map).squeeze(1)
    if return_prob_map:
        return masked_cross_entropy, wta_depth_map, torch.max(prob_volume, dim=1)[0]
    return masked_cross_entropy, wta_depth_map


def _stages(inputs):
    return [(inputs[k], k) for k in inputs.keys() if "stage" in k]


def _score_unit(depth_interval, B, device, dtype):
    """depth_interval (a number, a one-element tensor or a (B,) tensor) -> the (B,) error unit depth_interval * 192 / 128 in `dtype`."""
    if torch.is_tensor(depth_interval):
        t = depth_interval.detach().to(device=device, dtype=dtype).reshape(-1)
        if t.numel() not in (1, B):
            raise ValueError(f"diner_amd: depth_interval must be a number, one element or ({B},), got {tuple(depth_interval.shape)}")
        return (t * SCORE_UNIT).expand(B).contiguous()
    return torch.full((B,), float(depth_interval) * SCORE_UNIT, dtype=dtype, device=device)


def _accumulate_torch(inputs, depth_gt_ms, mask_ms, depth_loss_weights):
    """The stage loop both losses share.  The accumulators have the volumes' dtype (the reference's are float32 whatever the volumes are)."""
    first = stage_prob_volume(_stages(inputs)[0][0])
    total_loss = torch.zeros((), dtype=first.dtype, device=first.device)
    total_entropy = torch.zeros((), dtype=first.dtype, device=first.device)
    depth_loss = depth_entropy = None
    terms = {}
    for stage_inputs, stage_key in _stages(inputs):
        prob_volume = stage_prob_volume(stage_inputs)
        depth_values = stage_inputs["depth_values"]
        depth_gt = depth_gt_ms[stage_key]
        mask = mask_ms[stage_key] > 0.5
        entro_loss, depth_entropy = entropy_loss_torch(prob_volume, depth_gt, mask, depth_values)
        entro_loss = entro_loss * ENTROPY_WEIGHT
        depth_loss = F.smooth_l1_loss(depth_entropy[mask], depth_gt[mask], reduction="mean")
        total_entropy = total_entropy + entro_loss.detach()
        if depth_loss_weights is not None:
            stage_idx = int(stage_key.replace("stage", "")) - 1
            total_loss = total_loss + depth_loss_weights[stage_idx] * entro_loss
        else:
            total_loss = total_loss + entro_loss
        terms[stage_key] = (entro_loss, depth_loss)
    return total_loss, total_entropy, depth_loss, depth_entropy, terms


def trans_mvsnet_loss_torch(inputs, depth_gt_ms, mask_ms, **kwargs):
    total_loss, total_entropy, depth_loss, depth_entropy, _ = _accumulate_torch(inputs, depth_gt_ms, mask_ms, kwargs.get("dlossw", None))
    return total_loss, depth_loss, total_entropy, depth_entropy


def focal_loss_bld_torch(inputs, depth_gt_ms, mask_ms, depth_interval, **kwargs):
    total_loss, _, depth_loss, _, _ = _accumulate_torch(inputs, depth_gt_ms, mask_ms, kwargs.get("dlossw", None))
    gt = depth_gt_ms["stage3"]
    abs_err = (gt - inputs["stage3"]["depth"]).abs()
    abs_err_scaled = abs_err / _score_unit(depth_interval, gt.shape[0], gt.device, abs_err.dtype).view(-1, 1, 1)      # per image
    mask = mask_ms["stage3"] > 0.5
    epe = abs_err_scaled[mask].mean()
    less1 = (abs_err_scaled[mask] < 1.).to(gt.dtype).mean()
    less3 = (abs_err_scaled[mask] < 3.).to(gt.dtype).mean()
    return total_loss, depth_loss, epe, less1, less3


def _per_image_mean(fn, depth_est, depth_gt, mask, *args):
    return torch.stack([fn(depth_est[i], depth_gt[i], mask[i], *args) for i in range(depth_gt.shape[0])]).mean()


def thres_metrics_torch(depth_est, depth_gt, mask, thres):
    """Thres_metrics (utils.py:254-261): per image the share of valid pixels with |est - gt| > thres, then the batch mean."""
    assert isinstance(thres, (int, float))

    def one(est, gt, m, t):
        return torch.mean((torch.abs(est[m] - gt[m]) > t).float())
    with torch.no_grad():
        return _per_image_mean(one, depth_est, depth_gt, mask, thres)


def abs_depth_error_metrics_torch(depth_est, depth_gt, mask, thres=None):
    """AbsDepthError_metrics (utils.py:265-274): per image the mean |est - gt| over the valid pixels [with an error inside thres = (lo, hi);
    0 when there is none], then the batch mean."""
    def one(est, gt, m):
        error = (est[m] - gt[m]).abs()
        if thres is not None:
            error = error[(error >= float(thres[0])) & (error <= float(thres[1]))]
            if error.shape[0] == 0:
                return torch.tensor(0, device=error.device, dtype=error.dtype)
        return torch.mean(error)
    with torch.no_grad():
        return _per_image_mean(one, depth_est, depth_gt, mask)


# ---- the kernel route -----------------------------------------------------------------------------------------------------------------
def _on_device(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _mask_f32(mask):
    return mask if mask.dtype == torch.float32 else (mask > 0.5 if mask.dtype != torch.bool else mask).to(torch.float32)


class _StageLoss(torch.autograd.Function):
    """One stage on csrc/mvsloss.hip.  -> (scalars, depth, confidence); only scalars[0] = weight 2 entropy carries a gradient, and the
    backward is one launch of the gradient kernel with the upstream gradient as a device scalar."""

    @staticmethod
    def forward(ctx, vol, init, hyp, gt, mask, unit, weight, from_prob, thresholds):
        ops = _ops()
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        r = ops.mvs_stage_loss(vol.detach(), hyp.detach(), gt.detach(), mask, None if init is None else init.detach(), from_prob, unit, thresholds,
                               weight, record=need)
        if need:
            ctx.save_for_backward(vol.detach(), None if init is None else init.detach(), mask, r["record"], r["factors"])
        ctx.weight, ctx.from_prob = float(weight), bool(from_prob)
        ctx.mark_non_differentiable(r["depth"], r["confidence"])
        return r["scalars"], r["depth"], r["confidence"]

    @staticmethod
    def backward(ctx, g_scalars, _g_depth, _g_conf):
        vol, init, mask, record, factors = ctx.saved_tensors
        upstream = g_scalars[0].to(torch.float32).contiguous()           # the other scalars are handed out detached
        grad = _ops().mvs_stage_loss_grad(vol, init, ctx.from_prob, mask, record, factors, upstream, ctx.weight)
        return (grad if ctx.needs_input_grad[0] else None, grad if init is not None and ctx.needs_input_grad[1] else None,
                None, None, None, None, None, None, None)


def stage_loss(volume, depth_gt, mask, depth_values, init=None, from_prob=False, weight=1.0, depth_interval=None,
               thresholds=SCORE_THRESHOLDS):
    """One stage on the kernels.  volume (B,D,H,W): the regularised cost [+ init], or with from_prob a probability volume; mask: float
    (valid where > 0.5) or bool.  -> dict: term = weight 2 entropy (0-dim, differentiable in volume / init), and without a graph entropy2
    = 2 entropy, depth_loss, abs_err, epe and under (the shares of valid pixels with |err| / (depth_interval 192 / 128) under each
    threshold; zeros without depth_interval), depth, confidence (B,H,W)."""
    B = volume.shape[0]
    hyp = _hypothesis_volume(depth_values, depth_gt.shape)
    if hyp.dim() == 4 and tuple(hyp.shape) != tuple(volume.shape):
        hyp = hyp.expand(volume.shape)
    _ops()._check_mvs_loss_args(volume, hyp, depth_gt, mask, init)
    unit = None if depth_interval is None else _score_unit(depth_interval, B, volume.device, torch.float64)
    scalars, depth, conf = _StageLoss.apply(volume, init, hyp, depth_gt, _mask_f32(mask), unit, float(weight), bool(from_prob),
                                            tuple(thresholds) if unit is not None else ())
    s = scalars.detach()
    return dict(term=scalars[0], entropy2=s[1], depth_loss=s[2], abs_err=s[3], epe=s[4], under=s[5:], depth=depth, confidence=conf)


def _stage_volume(stage):
    """-> (volume, from_prob): a stage dict that carries "cost" (DeviceDepthNet.fused_readout) is taken from the cost."""
    if stage.get("cost") is not None:
        return stage["cost"], False
    return stage["prob_volume"], True


def _kernel_route(inputs, depth_gt_ms, mask_ms, force_torch):
    if force_torch:
        return False
    for stage, key in _stages(inputs):
        vol, _ = _stage_volume(stage)
        if vol is None or not _on_device(vol, stage["depth_values"], depth_gt_ms[key]) or not mask_ms[key].is_cuda:
            return False
    return True


def entropy_loss(prob_volume, depth_gt, mask, depth_value, return_prob_map=False, force_torch=False):
    """Drop-in for the reference's entropy_loss: prob_volume (B,D,H,W), depth_gt (B,H,W), mask (B,H,W) bool, depth_value (B,D) or
    (B,D,H,W) -> (masked cross entropy, winner-take-all depth (B,H,W)[, confidence (B,H,W)]).  The kernels need float32 HIP tensors and a
    bool mask (the reference multiplies by the mask, so a float mask weights the pixels: that stays with the restatement)."""
    if force_torch or not _on_device(prob_volume, depth_gt, depth_value) or mask.dtype != torch.bool or not mask.is_cuda:
        return entropy_loss_torch(prob_volume, depth_gt, mask, depth_value, return_prob_map)
    r = stage_loss(prob_volume, depth_gt, mask, depth_value, from_prob=True, weight=1.0 / ENTROPY_WEIGHT)      # weight 2 entropy = entropy
    return (r["term"], r["depth"], r["confidence"]) if return_prob_map else (r["term"], r["depth"])


def _accumulate(inputs, depth_gt_ms, mask_ms, depth_loss_weights, depth_interval=None):
    dev = mask_ms[_stages(inputs)[0][1]].device
    total_loss = torch.zeros((), dtype=torch.float32, device=dev)
    total_entropy = torch.zeros((), dtype=torch.float32, device=dev)
    last = scored = None
    for stage, key in _stages(inputs):
        vol, from_prob = _stage_volume(stage)
        weight = 1.0 if depth_loss_weights is None else float(depth_loss_weights[int(key.replace("stage", "")) - 1])
        last = stage_loss(vol, depth_gt_ms[key], mask_ms[key], stage["depth_values"], from_prob=from_prob, weight=weight,
                          depth_interval=depth_interval if key == "stage3" else None)
        total_entropy = total_entropy + last["entropy2"]
        total_loss = total_loss + last["term"]
        if key == "stage3":
            scored = last
    return total_loss, total_entropy, last, scored


def trans_mvsnet_loss(inputs, depth_gt_ms, mask_ms, **kwargs):
    """Drop-in for the reference's trans_mvsnet_loss -> (total, depth_loss, total_entropy, depth_entropy): total = sum over the stages of
    dlossw[stage] 2 entropy (differentiable in each stage's "cost" / "prob_volume"); depth_loss (smooth-L1 of the winner-take-all depth
    over the valid pixels) and depth_entropy (that depth map) are the LAST stage's, as in the reference."""
    if not _kernel_route(inputs, depth_gt_ms, mask_ms, kwargs.get("force_torch", False)):
        return trans_mvsnet_loss_torch(inputs, depth_gt_ms, mask_ms, **kwargs)
    total, total_entropy, last, _ = _accumulate(inputs, depth_gt_ms, mask_ms, kwargs.get("dlossw", None))
    return total, last["depth_loss"], total_entropy, last["depth"]


def focal_loss_bld(inputs, depth_gt_ms, mask_ms, depth_interval, **kwargs):
    """Drop-in for the reference's focal_loss_bld -> (total, depth_loss, epe, less1, less3).  inputs: the model's outputs ("stage1" ..
    "stage3", each with "depth_values" and "prob_volume", or "cost" from a fused_readout model); depth_gt_ms / mask_ms: {"stage k":
    (B,H,W)}, mask valid where > 0.5; dlossw: the stages' weights.  total is differentiable; the other four carry no graph.  epe, less1 and
    less3 score stage 3's winner-take-all depth, which is the model's "depth", in units of depth_interval 192 / 128.

    One deliberate difference from the reference: depth_interval may be a number, a one-element tensor or a (B,) tensor and is applied PER
    IMAGE.  The reference's `abs_err / (depth_interval * 192 / 128)` is right at batch size 1, where all fine-tuning runs; at B > 1 it
    broadcasts a (B,) tensor along W, which is a bug that is not reproduced here."""
    if "stage3" not in inputs:
        raise KeyError("stage3")
    if not _kernel_route(inputs, depth_gt_ms, mask_ms, kwargs.get("force_torch", False)):
        return focal_loss_bld_torch(inputs, depth_gt_ms, mask_ms, depth_interval, **kwargs)
    total, _, last, scored = _accumulate(inputs, depth_gt_ms, mask_ms, kwargs.get("dlossw", None), depth_interval)
    return total, last["depth_loss"], scored["epe"], scored["under"][0], scored["under"][1]


def _scores(depth_est, depth_gt, mask, thresholds=(), band=None):
    return _ops().depth_scores(depth_est.detach(), depth_gt.detach(), _mask_f32(mask), thresholds, band)[1]


def thres_metrics(depth_est, depth_gt, mask, thres, force_torch=False):
    """Drop-in for the reference's Thres_metrics on diner_depth_scores_f32 (float32 HIP tensors; otherwise the restatement)."""
    assert isinstance(thres, (int, float))
    if force_torch or not _on_device(depth_est, depth_gt) or not mask.is_cuda:
        return thres_metrics_torch(depth_est, depth_gt, mask, thres)
    return _scores(depth_est, depth_gt, mask, (thres,))[2]


def abs_depth_error_metrics(depth_est, depth_gt, mask, thres=None, force_torch=False):
    """Drop-in for the reference's AbsDepthError_metrics on diner_depth_scores_f32 (float32 HIP tensors; otherwise the restatement)."""
    if force_torch or not _on_device(depth_est, depth_gt) or not mask.is_cuda:
        return abs_depth_error_metrics_torch(depth_est, depth_gt, mask, thres)
    return _scores(depth_est, depth_gt, mask, (), thres)[0 if thres is None else 1]


# ---- the whole estimator ---------------------------------------------------------------------------------------------------------------
class DeviceTransMVSNet(nn.Module):
    """The reference's TransMVSNet (models/TransMVSNet.py:109-226, refine=False) as one module of this library's parts: `feature`
    (DeviceFeatureNet), `FMT_with_pathway`, `cost_regularization` (one shared DeviceCostRegNet, or a ModuleList of one per stage) and
    `DepthNet`, so the state-dict keys are the reference's and load_state_dict(checkpoint["model"]) works strictly.
    forward(imgs (B,NV,3,H,W), proj_matrices {"stage k": (B,NV,2,4,4)}, depth_values (B,D0), depth_interval=None) is
    mvs.depth_from_images: in eval mode under torch.no_grad() the kernels; in training the parts' torch routes -- differentiable, BatchNorm
    on batch statistics.  depth_interval: the base interval (max - min) / D0 as a host number; None reads it back from depth_values as the
    reference does (one synchronisation).  grad_method is kept for the reference's signature: the depth a stage hands on is a gather of
    hypotheses at an argmax, which carries no gradient to any parameter either way, and it is handed on detached.
    fused_readout, match_kernels: DeviceDepthNet's switches (see there); deform_kernels: DeviceFeatureNet's (see there); fmt_kernels:
    DeviceFMT's (see there)."""

    def __init__(self, ndepths=(48, 32, 8), depth_interals_ratio=(4, 2, 1), share_cr=False, cr_base_chs=(8, 8, 8), grad_method="detach"):
        super().__init__()
        if len(ndepths) != len(depth_interals_ratio):
            raise ValueError("diner_amd: DeviceTransMVSNet: ndepths and depth_interals_ratio differ in length")
        self.ndepths, self.depth_interals_ratio = tuple(int(n) for n in ndepths), tuple(depth_interals_ratio)
        self.share_cr, self.cr_base_chs, self.grad_method = bool(share_cr), tuple(int(c) for c in cr_base_chs), grad_method
        self.num_stage = len(self.ndepths)
        self.feature = mvs.DeviceFeatureNet(base_channels=8)
        self.FMT_with_pathway = mvs.DeviceFMTWithPathway()
        if self.share_cr:
            self.cost_regularization = mvs.DeviceCostRegNet(in_channels=1, base_channels=8)
        else:
            self.cost_regularization = nn.ModuleList([mvs.DeviceCostRegNet(in_channels=1, base_channels=self.cr_base_chs[i])
                                                      for i in range(self.num_stage)])
        self.DepthNet = mvs.DeviceDepthNet()

    @property
    def fused_readout(self):
        return self.DepthNet.fused_readout

    @fused_readout.setter
    def fused_readout(self, value):
        self.DepthNet.fused_readout = bool(value)

    @property
    def match_kernels(self):
        return self.DepthNet.match_kernels

    @match_kernels.setter
    def match_kernels(self, value):
        self.DepthNet.match_kernels = bool(value)

    @property
    def deform_kernels(self):
        return self.feature.deform_kernels

    @deform_kernels.setter
    def deform_kernels(self, value):
        self.feature.deform_kernels = bool(value)

    @property
    def fmt_kernels(self):
        return self.FMT_with_pathway.fmt_kernels

    @fmt_kernels.setter
    def fmt_kernels(self, value):
        self.FMT_with_pathway.fmt_kernels = bool(value)

    @classmethod
    def from_module(cls, model):
        """A reference TransMVSNet (or a DeviceTransMVSNet) -> a DeviceTransMVSNet with its state, device and mode."""
        if getattr(model, "refine", False):
            raise ValueError("diner_amd: DeviceTransMVSNet has no refine network")
        new = cls(model.ndepths, model.depth_interals_ratio, model.share_cr, model.cr_base_chs, model.grad_method)
        p = next(model.parameters())
        new.to(device=p.device, dtype=p.dtype)
        new.load_state_dict(model.state_dict(), strict=True)
        new.train(model.training)
        return new

    def forward(self, imgs, proj_matrices, depth_values, depth_interval=None):
        return mvs.depth_from_images(imgs, proj_matrices, depth_values, self.feature, self.FMT_with_pathway, self.DepthNet,
                                     self.cost_regularization, ndepths=self.ndepths, ratios=self.depth_interals_ratio,
                                     depth_interval=depth_interval)


# ---- schedule, loop, checkpoints -------------------------------------------------------------------------------------------------------
def warmup_multistep_lr(step, base_lr, milestones, gamma, warmup_factor=1.0 / 3, warmup_iters=500):
    """WarmupMultiStepLR.get_lr (utils.py:352-367, "linear" warm-up) as a function of the step (the scheduler's last_epoch)."""
    factor = 1
    if step < warmup_iters:
        alpha = float(step) / warmup_iters
        factor = warmup_factor * (1 - alpha) + alpha
    return base_lr * factor * gamma ** bisect_right(list(milestones), step)


def fit_estimator(model, batches, *, steps, optimizer=None, lr=1e-3, weight_decay=1e-4, milestones=(), gamma=0.5, dlossw=(1, 1, 1),
                  start_step=0, log_every=50, on_log=None, match_kernels=False, deform_kernels=False, fmt_kernels=False):
    """`steps` fine-tuning steps k = start_step, ...: model.train(); outputs = model(imgs, proj_matrices, depth_values) with fused_readout;
    focal_loss_bld(outputs, depth, mask, depth_interval, dlossw=dlossw); total.backward(); optimizer.step at warmup_multistep_lr(k, lr,
    milestones, gamma).  batches: any iterable of the reference's sample dicts {"imgs", "proj_matrices", "depth_values", "depth": {"stage
    k": ..}, "mask": {..}, "depth_interval"}, cycled; an optional "base_interval" (a host number, (max - min) / D0 of depth_values) keeps
    the model's forward free of its read-back, otherwise it is read once per distinct batch.  optimizer: a DeviceAdam (made here when
    None and the model is on a HIP device: coupled weight decay as the reference's Adam, skip_nonfinite, so a non-finite step changes
    nothing where the reference catches NanError on the host) or any torch optimiser (made here as torch.optim.Adam when the model is on
    the CPU).  The five scalars of a step go into a device ring of log_every rows that is read back once per log_every steps (and once at
    the end): the loop's only wait.  on_log(rows) receives the rows just read.  match_kernels=True sets the model's switch of that name for
    the loop (the cost volume and its gradients at the feature maps on the kernels of csrc/mvs.hip) and restores it afterwards;
    deform_kernels=True does the same with that switch (FeatureNet's deformable convolutions and their gradients on the kernels of
    csrc/deform.hip and csrc/deform_grad.hip); fmt_kernels=True with that one (the feature transformer's layers and their gradients on the
    kernels of csrc/fmt.hip and csrc/fmt_grad.hip).  The three compose with each other and with fused_readout.
    -> (history, optimizer); history: one dict {step, total, depth_loss, epe, less1, less3} per step."""
    params = [p for p in model.parameters() if p.requires_grad]
    dev = params[0].device
    device_adam = None
    if dev.type == "cuda":
        from .optim import DeviceAdam
        device_adam = DeviceAdam
    if optimizer is None:
        if device_adam is not None:
            optimizer = device_adam(params, lr=lr, weight_decay=weight_decay, skip_nonfinite=True)
        else:
            optimizer = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay)
    on_device = device_adam is not None and isinstance(optimizer, device_adam)
    steps, log_every = int(steps), max(1, int(log_every))
    ring = torch.zeros(log_every, len(LOSS_TERMS), dtype=torch.float32, device=dev)
    history, first = [], start_step
    model.train()
    had_fused = getattr(model, "fused_readout", None)
    if had_fused is not None:
        model.fused_readout = True
    had_match = getattr(model, "match_kernels", None) if match_kernels else None
    if had_match is not None:
        model.match_kernels = True
    had_deform = getattr(model, "deform_kernels", None) if deform_kernels else None
    if had_deform is not None:
        model.deform_kernels = True
    had_fmt = getattr(model, "fmt_kernels", None) if fmt_kernels else None
    if had_fmt is not None:
        model.fmt_kernels = True
    optimizer.zero_grad()
    intervals = {}

    def flush(upto):
        nonlocal first
        rows = ring[:upto - first].cpu()                               # the wait
        new = [dict(step=first + i, **{k: float(rows[i, j]) for j, k in enumerate(LOSS_TERMS)}) for i in range(rows.shape[0])]
        history.extend(new)
        first = upto
        if on_log is not None and new:
            on_log(new)

    def base_interval(batch):
        if batch.get("base_interval") is not None:
            return float(batch["base_interval"])
        if id(batch) not in intervals:
            dv = batch["depth_values"]
            intervals[id(batch)] = float((dv[0, -1] - dv[0, 0]).item()) / dv.shape[1]
        return intervals[id(batch)]

    try:
        source = itertools.cycle(batches)
        for k in range(start_step, start_step + steps):
            batch = next(source)
            outputs = model(batch["imgs"], batch["proj_matrices"], batch["depth_values"], depth_interval=base_interval(batch))
            terms = focal_loss_bld(outputs, batch["depth"], batch["mask"], batch["depth_interval"], dlossw=dlossw)
            terms[0].backward()
            rate = warmup_multistep_lr(k, lr, milestones, gamma)
            if on_device:
                optimizer.step(lr=rate, zero_grads=True)
            else:
                for group in optimizer.param_groups:
                    group["lr"] = rate
                optimizer.step()
                optimizer.zero_grad()
            ring[k - first].copy_(torch.stack([t.detach().to(torch.float32) for t in terms]))
            if k + 1 - first == log_every:
                flush(k + 1)
        if first < start_step + steps:
            flush(start_step + steps)
    finally:
        if had_fused is not None:
            model.fused_readout = had_fused
        if had_match is not None:
            model.match_kernels = had_match
        if had_deform is not None:
            model.deform_kernels = had_deform
        if had_fmt is not None:
            model.fmt_kernels = had_fmt
    return history, optimizer


def save_estimator_checkpoint(path, model, optimizer, epoch):
    """torch.save of the reference's checkpoint dict (finetune.py:343-347): {"epoch", "model": model.state_dict(), "optimizer":
    optimizer.state_dict()}."""
    torch.save({"epoch": int(epoch), "model": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                "optimizer": optimizer.state_dict()}, path)


def load_estimator_checkpoint(path, model, optimizer=None):
    """Loads what save_estimator_checkpoint or the reference's finetune.py wrote: the weights strictly, the optimiser's state when an
    optimiser is given -> epoch."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(ckpt["model"], strict=True)
    if optimizer is not None:
        optimizer.load_state_dict(ckpt["optimizer"])
    return int(ckpt.get("epoch", 0))
