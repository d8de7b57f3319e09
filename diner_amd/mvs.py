"""The matching stage of the multi-view depth estimator on the device: what TransMVSNet's DepthNet.forward (models/TransMVSNet.py:37-106)
and the stage loop of TransMVSNet.forward do between the learned networks -- homography warping fused with the feature similarity, the
pixelwise view weights, the weighted aggregation, the winner-take-all read-out of the regularised cost and the next stage's depth
hypotheses -- on the kernels of csrc/mvs.hip, and the cost regulariser between them, the 3-D U-Net CostRegNet (models/module.py:424-455),
on the kernels of csrc/costreg.hip (DeviceCostRegNet), and the feature transformer in front of the loop, FMT_with_pathway (models/FMT.py),
on the kernels of csrc/fmt.hip (DeviceFMT, DeviceFMTWithPathway), and the feature pyramid in front of that, FeatureNet
(models/module.py:343-421) with its nine modulated deformable convolutions, on the kernels of csrc/deform.hip and csrc/conv2d.hip
(DeviceFeatureNet); depth_from_images chains them from the images to the stage outputs.

Every thin function takes the reference's tensor layouts (NCHW).  On HIP tensors it runs the kernels; on CPU tensors it runs a torch
restatement of the same mathematics with the reference's own operations in the reference's order (`*_torch`, any floating dtype),
which is the host oracle of the tests and the baseline of tools/time_mvs.py.  The networks' kernels are inference only; the matching
stage alone has a backward pass in HIP (match_similarity, cost_volume_train: the similarity's gradients at the feature maps).
DeviceDepthNet uses torch operations whenever gradients are enabled or the module is in training mode (fine-tuning: diner_amd.estimator),
and with match_kernels those kernels for the cost volume."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import formats

BN_EPS = 1e-5                      # torch.nn.BatchNorm3d's default, which the reference's ConvBnReLU3D keeps
PIXELWISE_KEYS = ("conv0.conv.weight", "conv0.bn.weight", "conv0.bn.bias", "conv0.bn.running_mean", "conv0.bn.running_var",
                  "conv1.conv.weight", "conv1.bn.weight", "conv1.bn.bias", "conv1.bn.running_mean", "conv1.bn.running_var",
                  "conv2.weight", "conv2.bias")
STAGE_SCALES = (4, 2, 1)           # stage1 .. stage3 of TransMVSNet.stage_infos


def _ops():
    from . import ops              # loads libdiner_hip.so; only the device route needs it
    return ops


# ---- the pixelwise view-weight net --------------------------------------------------------------------------------------------------
class Pixelwise:
    """PixelwiseNet's parameters: `raw`, the tensors under the reference's keys (what the restatement evaluates, BatchNorm unfolded like
    the reference), and `folded`, the 177 float32 values w0[16] b0[16] w1[8][16] b1[8] w2[8] b2 of diner_mvs_cost_volume_f32 with
    BatchNorm's running statistics folded in float64 and rounded once."""

    def __init__(self, raw, folded):
        self.raw, self.folded = raw, folded


def fold_pixelwise(state_dict, prefix=""):
    """DepthNet.pixel_wise_net's state dict (keys conv0.conv.weight, conv0.bn.*, conv1.conv.weight, conv1.bn.*, conv2.weight, conv2.bias
    under `prefix`) -> Pixelwise.  Runs on the tensors' own device without a host read-back."""
    missing = [k for k in PIXELWISE_KEYS if prefix + k not in state_dict]
    if missing:
        raise KeyError(f"diner_amd: fold_pixelwise misses {[prefix + k for k in missing]}")
    raw = {k: state_dict[prefix + k].detach() for k in PIXELWISE_KEYS}
    want = {"conv0.conv.weight": (16, 1, 1, 1, 1), "conv1.conv.weight": (8, 16, 1, 1, 1), "conv2.weight": (1, 8, 1, 1, 1), "conv2.bias": (1,)}
    for k, shape in want.items():
        if tuple(raw[k].shape) != shape:
            raise ValueError(f"diner_amd: fold_pixelwise expects {prefix + k} of shape {shape}, got {tuple(raw[k].shape)}")
    parts = []
    for i, (cout, cin) in enumerate(((16, 1), (8, 16))):
        p = f"conv{i}."
        s = raw[p + "bn.weight"].double() / torch.sqrt(raw[p + "bn.running_var"].double() + BN_EPS)
        parts.append(((raw[p + "conv.weight"].double().view(cout, cin) * s.view(-1, 1)).reshape(-1),
                      raw[p + "bn.bias"].double() - raw[p + "bn.running_mean"].double() * s))
    (w0, b0), (w1, b1) = parts
    folded = torch.cat([w0, b0, w1, b1, raw["conv2.weight"].double().reshape(-1), raw["conv2.bias"].double().reshape(-1)]).to(torch.float32)
    return Pixelwise(raw, folded)


def pixelwise_torch(raw, similarity):
    """PixelwiseNet.forward: similarity (B,1,D,H,W) -> view weight (B,1,H,W) = max_d sigmoid(conv2(conv1(conv0(similarity)))), each of
    conv0 / conv1 a 1x1x1 convolution, BatchNorm on its running statistics and a ReLU, in the similarity's dtype."""
    x, dt = similarity, similarity.dtype
    for p in ("conv0.", "conv1."):
        x = F.conv3d(x, raw[p + "conv.weight"].to(dt))
        x = F.relu(F.batch_norm(x, raw[p + "bn.running_mean"].to(dt), raw[p + "bn.running_var"].to(dt), raw[p + "bn.weight"].to(dt),
                                raw[p + "bn.bias"].to(dt), False, 0.0, BN_EPS))
    x = F.conv3d(x, raw["conv2.weight"].to(dt), raw["conv2.bias"].to(dt)).squeeze(1)
    return torch.max(torch.sigmoid(x), dim=1, keepdim=True)[0]


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------
def _full_proj(pair):
    """(B,2,4,4) camera pair -> the extrinsics with their top three rows replaced by K[:3,:3] E[:3,:4]."""
    out = pair[:, 0].clone()
    out[:, :3, :4] = torch.matmul(pair[:, 1, :3, :3], pair[:, 0, :3, :4])
    return out


def warp_torch(src_fea, src_proj, ref_proj, depth_values):
    """homo_warping (models/module.py:284-322) in src_fea's dtype: the source features (B,C,H,W) sampled where the reference view's pixels
    land at each depth hypothesis (B,D,H,W) -> (B,C,D,H,W).  Materialises the grid and the warped volume, as the reference does."""
    B, C, H, W = src_fea.shape
    D = depth_values.shape[1]
    dt, dev = src_fea.dtype, src_fea.device
    with torch.no_grad():                        # the sampling positions carry no gradient, as in the reference
        proj = torch.matmul(src_proj, torch.inverse(ref_proj))
        rot, trans = proj[:, :3, :3], proj[:, :3, 3:4]
        y, x = torch.meshgrid(torch.arange(0, H, dtype=dt, device=dev), torch.arange(0, W, dtype=dt, device=dev), indexing="ij")
        y, x = y.contiguous().view(H * W), x.contiguous().view(H * W)
        xyz = torch.stack((x, y, torch.ones_like(x))).unsqueeze(0).repeat(B, 1, 1)
        rot_xyz = torch.matmul(rot, xyz)
        rot_depth_xyz = rot_xyz.unsqueeze(2).repeat(1, 1, D, 1) * depth_values.reshape(B, 1, D, -1)
        proj_xyz = rot_depth_xyz + trans.view(B, 3, 1, 1)
        invalid = (proj_xyz[:, 2:3] < 1e-6).squeeze(1)
        proj_xy = proj_xyz[:, :2] / proj_xyz[:, 2:3]
        gx = proj_xy[:, 0] / ((W - 1) / 2) - 1
        gx[invalid] = -99.
        gy = proj_xy[:, 1] / ((H - 1) / 2) - 1
        gy[invalid] = -99.
        grid = torch.stack((gx, gy), dim=3)
    warped = F.grid_sample(src_fea, grid.view(B, D * H, W, 2), mode="bilinear", padding_mode="zeros", align_corners=True)
    return warped.view(B, C, D, H, W)


def cost_volume_torch(features, proj_matrices, depth_values, pixelwise=None, view_weights=None):
    """Steps 1-2 of DepthNet.forward, in features[0]'s dtype -> (similarity (B,1,D,H,W), view weights (B,NS,H,W)).
    pixelwise: a Pixelwise, or any callable similarity (B,1,D,H,W) -> weight (B,1,H,W) such as the module itself."""
    dt = features[0].dtype
    weight_of = pixelwise if callable(pixelwise) else (lambda s: pixelwise_torch(pixelwise.raw, s))
    projs = torch.unbind(proj_matrices.to(dt), 1)
    ref_feature, ref_proj = features[0], _full_proj(projs[0])
    depth_values = depth_values.to(dt)
    weights, sim_sum, w_sum = [], 0, 1e-5
    for i, (src_fea, src_pair) in enumerate(zip(features[1:], projs[1:])):
        warped = warp_torch(src_fea, _full_proj(src_pair), ref_proj, depth_values)
        similarity = (warped * ref_feature.unsqueeze(2)).mean(1, keepdim=True)
        del warped
        if view_weights is None:
            w = weight_of(similarity)
            weights.append(w)
        else:
            w = view_weights[:, i:i + 1].to(dt)
        sim_sum = sim_sum + similarity * w.unsqueeze(1)
        w_sum = w_sum + w.unsqueeze(1)
    return sim_sum / w_sum, (torch.cat(weights, dim=1) if view_weights is None else view_weights)


def select_depth_torch(cost, depth_values, prob_init=None):
    """Step 3 of DepthNet.forward after the regulariser -> (depth (B,H,W), confidence (B,H,W), prob volume (B,D,H,W))."""
    pre = cost if prob_init is None else cost + prob_init
    prob = torch.exp(F.log_softmax(pre, dim=1))
    index = torch.argmax(prob, dim=1, keepdim=True)
    return torch.gather(depth_values, 1, index).squeeze(1), torch.max(prob, dim=1)[0], prob


def depth_hypotheses_torch(cur_depth, ndepth, interval, image_hw, stage_scale):
    """The hypotheses of stages 2 and 3 as TransMVSNet.forward forms them: the previous depth (B,h,w) bilinearly resized to the image,
    get_cur_depth_range_samples (models/module.py:590-599), then the trilinear resize to (ndepth, H // s, W // s)."""
    H, W = (int(v) for v in image_hw)
    s = int(stage_scale)
    up = F.interpolate(cur_depth.unsqueeze(1), [H, W], mode="bilinear", align_corners=False).squeeze(1)
    lo = up - ndepth / 2 * interval
    hi = up + ndepth / 2 * interval
    step = (hi - lo) / (ndepth - 1)
    samples = lo.unsqueeze(1) + torch.arange(0, ndepth, device=up.device, dtype=up.dtype).reshape(1, -1, 1, 1) * step.unsqueeze(1)
    return F.interpolate(samples.unsqueeze(1), [ndepth, H // s, W // s], mode="trilinear", align_corners=False).squeeze(1)


# ---- the thin functions ---------------------------------------------------------------------------------------------------------------
def _check_features(features, proj_matrices, depth_values):
    if len(features) < 2 or any(f.dim() != 4 or f.shape != features[0].shape for f in features):
        raise ValueError("diner_amd: cost_volume expects a list of at least two feature maps (B,C,H,W) of one shape, reference first")
    B, _, H, W = features[0].shape
    if proj_matrices.dim() != 5 or tuple(proj_matrices.shape) != (B, len(features), 2, 4, 4):
        raise ValueError(f"diner_amd: cost_volume expects proj_matrices ({B},{len(features)},2,4,4), got {tuple(proj_matrices.shape)}")
    if depth_values.dim() != 4 or depth_values.shape[0] != B or tuple(depth_values.shape[2:]) != (H, W):
        raise ValueError(f"diner_amd: cost_volume expects depth_values ({B},D,{H},{W}), got {tuple(depth_values.shape)}")


def cost_volume(features, proj_matrices, depth_values, pixelwise=None, view_weights=None):
    """features: [reference, source 1, ...] each (B,C,H,W); proj_matrices (B,NV,2,4,4); depth_values (B,D,H,W); pixelwise: a Pixelwise
    (fold_pixelwise) when the view weights are to be computed, else view_weights (B,NV-1,H,W)
    -> (aggregated similarity (B,1,D,H,W), view weights (B,NV-1,H,W))."""
    _check_features(features, proj_matrices, depth_values)
    if (pixelwise is None) == (view_weights is None):
        raise ValueError("diner_amd: cost_volume takes either pixelwise (a Pixelwise) or view_weights")
    if not features[0].is_cuda:
        B, Cf, H, W = features[0].shape
        _ops()._check_mvs_limits(B, len(features) - 1, Cf, depth_values.shape[1], H, W)       # the device route's limits hold here too
        return cost_volume_torch(features, proj_matrices, depth_values, pixelwise, view_weights)
    ops = _ops()
    cl = torch.stack([f.detach() for f in features], 0).to(torch.float32).permute(0, 1, 3, 4, 2).contiguous()      # the one repack
    sim, weights = ops.mvs_cost_volume(cl[0], cl[1:], proj_matrices.detach().to(torch.float32), depth_values.detach().to(torch.float32),
                                       None if pixelwise is None else pixelwise.folded,
                                       None if view_weights is None else view_weights.detach().to(torch.float32))
    return sim.unsqueeze(1), weights


# ---- the matching stage in training: the kernels with a backward pass ------------------------------------------------------------------
def match_gate(features, proj_matrices, depth_values, view_weights=None):
    """Whether match_similarity / cost_volume_train run the kernels: float32 HIP tensors inside diner_mvs_cost_volume_f32's limits."""
    tensors = list(features) + [proj_matrices, depth_values] + ([] if view_weights is None else [view_weights])
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return False
    B, Cf, H, W = (int(n) for n in features[0].shape)
    try:
        _ops()._check_mvs_limits(B, len(features) - 1, Cf, int(depth_values.shape[1]), H, W)
    except ValueError:
        return False
    return True


def _channels_last_stack(features):
    return torch.stack([f.detach() for f in features], 0).permute(0, 1, 3, 4, 2).contiguous()         # the one repack: (NV,B,H,W,C)


def _feature_grads(ctx, d_ref, d_src, first):
    """The gradients as NCHW views of the kernels' channels-last results, None where a feature map needs none."""
    maps = [d_ref] + list(torch.unbind(d_src, 0))
    return tuple(m.permute(0, 3, 1, 2) if ctx.needs_input_grad[first + i] else None for i, m in enumerate(maps))


class _MatchSimilarity(torch.autograd.Function):
    """diner_mvs_similarity_f32 / diner_mvs_similarity_grad_f32 (per-view upstream).  Saves the channels-last features, the homography and
    the depth; no gradient to proj or depth.  The backward pass is a kernel on detached tensors: once differentiable, a second derivative
    raises."""

    @staticmethod
    def forward(ctx, proj, depth, *features):
        cl = _channels_last_stack(features)
        depth = depth.detach().contiguous()
        sim, hom = _ops().mvs_similarity(cl[0], cl[1:], proj.detach(), depth)
        ctx.save_for_backward(cl, hom, depth)
        return sim

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        cl, hom, depth = ctx.saved_tensors
        d_ref, d_src = _ops().mvs_similarity_grad(cl[0], cl[1:], hom, depth, grad_views=grad.to(torch.float32).contiguous())
        return (None, None) + _feature_grads(ctx, d_ref, d_src, 2)


class _CostVolumeGiven(torch.autograd.Function):
    """diner_mvs_cost_volume_f32 with given view weights / diner_mvs_similarity_grad_f32 (aggregated upstream): no per-view volume in
    either direction.  No gradient to proj, depth or the weights (DeviceDepthNet hands the weights on detached, as the reference does)."""

    @staticmethod
    def forward(ctx, proj, depth, view_weights, *features):
        cl = _channels_last_stack(features)
        depth, view_weights = depth.detach().contiguous(), view_weights.detach().contiguous()
        sim, _, hom = _ops().mvs_cost_volume(cl[0], cl[1:], proj.detach(), depth, None, view_weights, return_homography=True)
        ctx.save_for_backward(cl, hom, depth, view_weights)
        return sim.unsqueeze(1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        cl, hom, depth, view_weights = ctx.saved_tensors
        d_ref, d_src = _ops().mvs_similarity_grad(cl[0], cl[1:], hom, depth, grad_aggregated=grad.to(torch.float32).squeeze(1).contiguous(),
                                                  view_weights=view_weights)
        return (None, None, None) + _feature_grads(ctx, d_ref, d_src, 3)


def match_similarity_torch(features, proj_matrices, depth_values):
    """The per-view similarity of cost_volume_torch, stacked: mean_c(homo_warping(src_v) ref) -> (B,NS,D,H,W), in features[0]'s dtype."""
    dt = features[0].dtype
    projs = torch.unbind(proj_matrices.to(dt), 1)
    ref_feature, ref_proj = features[0], _full_proj(projs[0])
    depth_values = depth_values.to(dt)
    sims = []
    for src_fea, src_pair in zip(features[1:], projs[1:]):
        warped = warp_torch(src_fea, _full_proj(src_pair), ref_proj, depth_values)
        sims.append((warped * ref_feature.unsqueeze(2)).mean(1))
        del warped
    return torch.stack(sims, 1)


def match_similarity(features, proj_matrices, depth_values):
    """features: [reference, source 1, ...] each (B,C,H,W); proj_matrices (B,NV,2,4,4); depth_values (B,D,H,W) -> the per-view similarity
    (B,NV-1,D,H,W), differentiable in every feature map (the sampling positions carry no gradient, as in the reference).  On float32 HIP
    tensors inside the kernels' limits: diner_mvs_similarity_f32 and, in the backward pass, diner_mvs_similarity_grad_f32, with neither a
    sampling grid nor a warped volume; anything else (CPU tensors, other dtypes, C % 4 != 0) runs match_similarity_torch, the host oracle."""
    _check_features(features, proj_matrices, depth_values)
    if not match_gate(features, proj_matrices, depth_values):
        return match_similarity_torch(features, proj_matrices, depth_values)
    return _MatchSimilarity.apply(proj_matrices, depth_values, *features)


def cost_volume_train(features, proj_matrices, depth_values, pixelwise_net=None, view_weights=None):
    """cost_volume_torch's results -- (similarity (B,1,D,H,W), view weights (B,NS,H,W)) -- differentiable in the feature maps and the
    pixelwise net's parameters, on the kernels where match_gate lets them run (otherwise cost_volume_torch itself).
    Given view_weights: diner_mvs_cost_volume_f32 forward, the aggregated form of diner_mvs_similarity_grad_f32 backward.
    Otherwise pixelwise_net, a callable similarity (B,1,D,H,W) -> weight (B,1,H,W) (the module itself: in training mode it runs on batch
    statistics and updates them, view by view, as the reference does): match_similarity, then the reference's torch expressions on the
    one-channel volumes."""
    _check_features(features, proj_matrices, depth_values)
    if (pixelwise_net is None) == (view_weights is None):
        raise ValueError("diner_amd: cost_volume_train takes either pixelwise_net (a callable) or view_weights")
    if not match_gate(features, proj_matrices, depth_values, view_weights):
        return cost_volume_torch(features, proj_matrices, depth_values, pixelwise_net, view_weights)
    if view_weights is not None:
        return _CostVolumeGiven.apply(proj_matrices, depth_values, view_weights, *features), view_weights
    s = _MatchSimilarity.apply(proj_matrices, depth_values, *features)
    weights, sim_sum, w_sum = [], 0, 1e-5
    for v in range(s.shape[1]):
        similarity = s[:, v:v + 1]
        w = pixelwise_net(similarity)
        weights.append(w)
        sim_sum = sim_sum + similarity * w.unsqueeze(1)
        w_sum = w_sum + w.unsqueeze(1)
    return sim_sum / w_sum, torch.cat(weights, dim=1)


def select_depth(cost, depth_values, prob_init=None, return_prob=True):
    """cost (B,D,H,W) or (B,1,D,H,W) from the regulariser [+ prob_init], depth_values (B,D,H,W)
    -> (depth (B,H,W), confidence (B,H,W), prob volume (B,D,H,W) or None)."""
    if cost.dim() == 5 and cost.shape[1] == 1:
        cost = cost.squeeze(1)
    if not cost.is_cuda:
        depth, conf, prob = select_depth_torch(cost, depth_values, prob_init)
        return depth, conf, (prob if return_prob else None)
    return _ops().mvs_select_depth(cost.detach().to(torch.float32), depth_values.detach().to(torch.float32),
                                   None if prob_init is None else prob_init.detach().to(torch.float32), return_prob)


def depth_hypotheses(cur_depth, ndepth, interval, image_hw, stage_scale):
    """The previous stage's depth (B,h,w) -> this stage's hypotheses (B, ndepth, H // s, W // s), spread over ndepth * interval around it.
    interval: this stage's depth interval (ratio x the estimator's base interval), a host number."""
    ops = _ops()
    ops._check_mvs_hypotheses_args(cur_depth, ndepth, image_hw, stage_scale)
    if not cur_depth.is_cuda:
        return depth_hypotheses_torch(cur_depth, int(ndepth), float(interval), image_hw, stage_scale)
    return ops.mvs_hypotheses(cur_depth.detach().to(torch.float32), int(ndepth), int(ndepth) / 2 * float(interval), image_hw, stage_scale)


# ---- the drop-in for the reference's DepthNet ----------------------------------------------------------------------------------------
class _ConvBnReLU3d(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 1, bias=False)
        self.bn = nn.BatchNorm3d(cout)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class _PixelwiseNet(nn.Module):
    """The parameters of the reference's PixelwiseNet under its state-dict keys; forward() serves the torch route (in training mode on batch
    statistics)."""

    def __init__(self):
        super().__init__()
        self.conv0, self.conv1 = _ConvBnReLU3d(1, 16), _ConvBnReLU3d(16, 8)
        self.conv2 = nn.Conv3d(8, 1, 1)

    def forward(self, x):
        return torch.max(torch.sigmoid(self.conv2(self.conv1(self.conv0(x))).squeeze(1)), dim=1, keepdim=True)[0]


class DeviceDepthNet(nn.Module):
    """A replacement for the reference's DepthNet: the same state-dict keys (pixel_wise_net.*), the same forward() signature and results.
    On HIP tensors, in eval mode and with gradients disabled it runs the kernels; otherwise torch operations (which are
    differentiable, so fine-tuning keeps working).  `model.DepthNet = DeviceDepthNet.from_module(model.DepthNet)` switches a loaded
    TransMVSNet over.

    fused_readout (default False: every route is as it was, bit for bit).  When True and the module is on its torch route with gradients
    enabled and float32 HIP tensors, it does not form the probability volume: depth and confidence come from the read-out kernel on the
    detached cost, and the stage dict carries "cost" (the regulariser's output plus prob_volume_init, with its graph) and "prob_volume":
    None -- what diner_amd.estimator's losses take.  The kernel's winner may differ from argmax(prob_volume) of the torch route on an exact
    tie that exp creates (two planes whose probabilities round to the same float32 in one chain and not in the other), and nowhere else.

    match_kernels (default False: every route is as it was, bit for bit).  When True and the module is on its torch route, the cost volume
    comes from cost_volume_train: on float32 HIP tensors inside the kernels' limits the similarity and its gradients at the feature maps
    run on the kernels of csrc/mvs.hip (no sampling grid and no warped volume is kept for the backward pass), the pixelwise net and the
    aggregation stay torch operations; any other input takes the torch route silently.  Composes with fused_readout."""

    def __init__(self):
        super().__init__()
        self.pixel_wise_net = _PixelwiseNet()
        self.fused_readout = False
        self.match_kernels = False
        self._folded, self._folded_key = None, None

    @classmethod
    def from_module(cls, depthnet):
        new = cls()
        new.load_state_dict(depthnet.state_dict())
        p = next(depthnet.parameters())
        new.to(p.device)
        new.train(depthnet.training)
        return new

    def pixelwise(self):
        """The Pixelwise of the current parameters; folded again only after a parameter or buffer changed (no host read-back either way)."""
        sd = self.pixel_wise_net.state_dict()
        key = tuple((k, v.data_ptr(), v._version, str(v.device)) for k, v in sd.items())
        if key != self._folded_key:
            self._folded, self._folded_key = fold_pixelwise(sd), key
        return self._folded

    def uses_kernels(self, features):
        return features[0].is_cuda and not self.training and not torch.is_grad_enabled()

    def forward(self, features, proj_matrices, depth_values, num_depth, cost_regularization, prob_volume_init=None, view_weights=None):
        if len(features) != proj_matrices.shape[1]:
            raise ValueError("diner_amd: DeviceDepthNet: different number of images and projection matrices")
        if depth_values.shape[1] != num_depth:
            raise ValueError(f"diner_amd: DeviceDepthNet: depth_values has {depth_values.shape[1]} planes, num_depth is {num_depth}")
        given = view_weights is not None
        if self.uses_kernels(features):
            similarity, weights = cost_volume(features, proj_matrices, depth_values, None if given else self.pixelwise(), view_weights)
            depth, conf, prob = select_depth(cost_regularization(similarity), depth_values, prob_volume_init)
        else:
            # the view weights from the module itself: differentiable down to its parameters, and in training mode on BatchNorm's batch
            # statistics (which it then also updates), like the reference
            matching = cost_volume_train if self.match_kernels else cost_volume_torch        # the former falls back to the latter by itself
            similarity, weights = matching(features, proj_matrices, depth_values, None if given else self.pixel_wise_net, view_weights)
            cost = cost_regularization(similarity).squeeze(1)
            if (self.fused_readout and torch.is_grad_enabled() and cost.is_cuda and cost.dtype == torch.float32
                    and depth_values.dtype == torch.float32 and (prob_volume_init is None or prob_volume_init.dtype == torch.float32)):
                # no probability volume: the read-out kernel on the detached cost, and the cost itself (with its graph) for the loss
                depth, conf, _ = select_depth(cost, depth_values, prob_volume_init, return_prob=False)
                out = {"depth": depth, "photometric_confidence": conf, "prob_volume": None, "depth_values": depth_values,
                       "cost": cost if prob_volume_init is None else cost + prob_volume_init}
                return out if given else (out, weights.detach())
            depth, conf, prob = select_depth_torch(cost, depth_values, prob_volume_init)
        out = {"depth": depth, "photometric_confidence": conf.detach(), "prob_volume": prob, "depth_values": depth_values}
        return out if given else (out, weights.detach())

    def hypotheses(self, cur_depth, ndepth, interval, image_hw, stage_scale):
        """depth_hypotheses behind the same gate as forward()."""
        if self.uses_kernels([cur_depth]):
            return depth_hypotheses(cur_depth, ndepth, interval, image_hw, stage_scale)
        return depth_hypotheses_torch(cur_depth, int(ndepth), float(interval), image_hw, stage_scale)


def coarse_to_fine(features, proj_matrices, depth_values, depthnet, cost_regularization, ndepths=(48, 32, 8), ratios=(4, 2, 1),
                   image_hw=None, depth_interval=None, scales=STAGE_SCALES):
    """The stage loop of TransMVSNet.forward after feature extraction.
    features: per view a dict {"stage1": (B,C1,H/4,W/4), "stage2": ..., "stage3": ...}; proj_matrices: {"stage1": (B,NV,2,4,4), ...};
    depth_values (B,D0): stage 1's hypothesis range; depthnet: a DeviceDepthNet (or the reference's DepthNet); cost_regularization: one
    callable or one per stage; image_hw: the full image size; depth_interval: the base interval, a host number -- the reference reads it
    back from depth_values ((max - min) / D0); pass it to keep the loop free of host synchronisation.
    -> the reference's `outputs` dict: "stage1" .. "stage3" and the last stage's entries at the top level."""
    if image_hw is None:
        raise ValueError("diner_amd: coarse_to_fine needs image_hw, the full image size")
    H, W = (int(v) for v in image_hw)
    if depth_interval is None:
        depth_interval = float((depth_values[0, -1] - depth_values[0, 0]).item()) / depth_values.shape[1]
    outputs, depth, view_weights = {}, None, None
    B = depth_values.shape[0]
    for i, (nd, ratio, s) in enumerate(zip(ndepths, ratios, scales)):
        key = f"stage{i + 1}"
        feats = [f[key] for f in features]
        if depth is None:
            lo, hi = depth_values[:, 0], depth_values[:, -1]
            step = (hi - lo) / (nd - 1)
            samples = lo.unsqueeze(1) + torch.arange(0, nd, device=depth_values.device, dtype=depth_values.dtype).reshape(1, -1) * step.unsqueeze(1)
            hyp = samples.view(B, nd, 1, 1).expand(B, nd, H // s, W // s).contiguous()
        else:
            hypotheses = getattr(depthnet, "hypotheses", depth_hypotheses)           # the reference's DepthNet has none
            hyp = hypotheses(depth.detach(), nd, ratio * depth_interval, (H, W), s)
        reg = cost_regularization[i] if isinstance(cost_regularization, (list, tuple, nn.ModuleList)) else cost_regularization
        if view_weights is None:
            out, view_weights = depthnet(feats, proj_matrices[key], depth_values=hyp, num_depth=nd, cost_regularization=reg, view_weights=None)
        else:
            view_weights = F.interpolate(view_weights, scale_factor=2, mode="nearest")
            out = depthnet(feats, proj_matrices[key], depth_values=hyp, num_depth=nd, cost_regularization=reg, view_weights=view_weights)
        depth = out["depth"]
        outputs[key] = out
        outputs.update(out)
    return outputs


# ---- the drop-in for the reference's CostRegNet ---------------------------------------------------------------------------------------
# name, kind, Cin and Cout in units of base_channels (conv0's Cin is in_channels), stride -- CostRegNet.__init__ (models/module.py:424-444)
COSTREG_LAYERS = (("conv0", "conv", 0, 1, 1), ("conv1", "conv", 1, 2, 2), ("conv2", "conv", 2, 2, 1), ("conv3", "conv", 2, 4, 2),
                  ("conv4", "conv", 4, 4, 1), ("conv5", "conv", 4, 8, 2), ("conv6", "conv", 8, 8, 1), ("conv7", "deconv", 8, 4, 2),
                  ("conv9", "deconv", 4, 2, 2), ("conv11", "deconv", 2, 1, 2))


class _Conv3dBnReLU(nn.Module):
    """The reference's Conv3d / Deconv3d block (models/module.py:108-191) with BatchNorm and ReLU, under its state-dict keys."""

    def __init__(self, cin, cout, stride=1, transposed=False):
        super().__init__()
        if transposed:
            self.conv = nn.ConvTranspose3d(cin, cout, 3, stride=stride, padding=1, output_padding=1, bias=False)
        else:
            self.conv = nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False)
        self.bn = nn.BatchNorm3d(cout, momentum=0.1)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


def fold_conv_bn(weight, gamma, beta, mean, var, transposed=False):
    """A bias-free convolution followed by BatchNorm on its running statistics as one convolution with a bias, folded in float64 on the
    tensors' own device and rounded once: s = gamma / sqrt(var + eps), w' = w s (along Cout: dim 0, or dim 1 of a transposed
    convolution's weight), b' = beta - mean s -> (w', b') float32."""
    s = gamma.detach().double() / torch.sqrt(var.detach().double() + BN_EPS)
    shape = (1, -1, 1, 1, 1) if transposed else (-1, 1, 1, 1, 1)
    return ((weight.detach().double() * s.view(shape)).to(torch.float32),
            (beta.detach().double() - mean.detach().double() * s).to(torch.float32))


class DeviceCostRegNet(nn.Module):
    """A replacement for the reference's CostRegNet (models/module.py:424-455): the same state-dict keys (conv0.conv.weight, conv0.bn.*,
    ... conv11.*, prob.weight), the same forward(): similarity (B,in_channels,D,H,W) -> cost (B,1,D,H,W).  On float32 HIP tensors, in
    eval mode, with gradients disabled and D, H, W all multiples of 8 (the only sizes at which the reference's skip additions match) it
    runs the kernels of csrc/costreg.hip: eleven launches, BatchNorm folded into the weights, the skip additions in the epilogues.
    Otherwise the same torch operations as the reference in its order: differentiable, on batch statistics in training mode, and failing
    where the reference fails.  The kernel route keeps its intermediate volumes in a per-shape workspace (release_workspace()) and
    serves one stream at a time.  `mvs.to_device(model)` switches a loaded TransMVSNet over."""

    def __init__(self, in_channels=1, base_channels=8):
        super().__init__()
        self.in_channels, self.base_channels = int(in_channels), int(base_channels)
        for name, kind, ci, co, stride in COSTREG_LAYERS:
            cin = self.in_channels if ci == 0 else ci * self.base_channels
            setattr(self, name, _Conv3dBnReLU(cin, co * self.base_channels, stride, kind == "deconv"))
        self.prob = nn.Conv3d(self.base_channels, 1, 3, stride=1, padding=1, bias=False)
        self._packed, self._packed_key, self._workspaces = None, None, {}

    @classmethod
    def from_module(cls, costregnet):
        sd = costregnet.state_dict()
        base, cin = sd["conv0.conv.weight"].shape[:2]
        new = cls(int(cin), int(base))
        new.to(device=sd["conv0.conv.weight"].device, dtype=sd["conv0.conv.weight"].dtype)     # the source's dtype: nothing is cast down
        new.load_state_dict(sd)
        new.train(costregnet.training)
        return new

    def invalidate(self):
        """Forget the packed weights: call after writing a parameter or buffer through `.data`, which bumps no version counter."""
        self._packed_key = None

    def packed(self):
        """Per layer (name, kind, stride, Cout, packed weight, bias or None, relu) of the current parameters; folded and packed again only
        after a parameter or buffer changed (no host read-back either way)."""
        sd = self.state_dict()
        key = tuple((k, v.data_ptr(), v._version, str(v.device)) for k, v in sd.items())
        if key != self._packed_key:
            ops = _ops()
            layers = []
            for name, kind, _, co, stride in COSTREG_LAYERS:
                w, b = fold_conv_bn(sd[name + ".conv.weight"], sd[name + ".bn.weight"], sd[name + ".bn.bias"], sd[name + ".bn.running_mean"],
                                    sd[name + ".bn.running_var"], kind == "deconv")
                pack = ops.pack_deconv3d(w) if kind == "deconv" else ops.pack_conv3d(w)
                layers.append((name, kind, stride, co * self.base_channels, pack, b.contiguous(), True))
            layers.append(("prob", "conv", 1, 1, ops.pack_conv3d(sd["prob.weight"].detach().to(torch.float32)), None, False))
            self._packed, self._packed_key = layers, key
        return self._packed

    def uses_kernels(self, x):
        """The gate.  Parameters of another dtype than float32 (after .double(), .half()) leave it closed, so that a float32 input then
        fails in torch's own convolution as it does in the reference."""
        return (x.is_cuda and x.dtype == torch.float32 and self.prob.weight.dtype == torch.float32 and not self.training
                and not torch.is_grad_enabled() and x.dim() == 5 and x.shape[1] == self.in_channels
                and all(int(n) >= 8 and int(n) % 8 == 0 for n in x.shape[2:]))

    def release_workspace(self):
        """Drop the cached intermediate volumes of every input shape seen so far (they are allocated again on the next forward)."""
        self._workspaces.clear()

    def _workspace(self, B, D, H, W, device):
        """The seven intermediate volumes of one input shape, kept between calls -- one set per distinct (B, D, H, W); release_workspace()
        drops them.  The up path overwrites the skip volumes in place, so a module serves ONE stream at a time: two streams running the
        same module on the same shape would race on them (give each stream its own module, e.g. copy.deepcopy)."""
        key = (B, D, H, W, self.base_channels, str(device))
        ws = self._workspaces.get(key)
        if ws is None:
            c = self.base_channels
            vol = lambda s, m: torch.empty(B, D // s, H // s, W // s, m * c, dtype=torch.float32, device=device)
            ws = dict(conv0=vol(1, 1), conv1=vol(2, 2), conv2=vol(2, 2), conv3=vol(4, 4), conv4=vol(4, 4), conv5=vol(8, 8), conv6=vol(8, 8))
            self._workspaces[key] = ws
        return ws

    def forward_torch(self, x):
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)

    def forward(self, x):
        if not self.uses_kernels(x):
            return self.forward_torch(x)
        ops = _ops()
        B, Cin, D, H, W = (int(n) for n in x.shape)
        x = x.detach()
        cur = x.contiguous().view(B, D, H, W, 1) if Cin == 1 else x.permute(0, 2, 3, 4, 1).contiguous()
        ws = self._workspace(B, D, H, W, x.device)
        # the up path writes over the skip tensor it adds: conv7 -> conv4's volume, conv9 -> conv2's, conv11 -> conv0's
        skip = {"conv7": "conv4", "conv9": "conv2", "conv11": "conv0"}
        for name, kind, stride, cout, pack, bias, relu in self.packed():
            if kind == "deconv":
                cur = ops.deconv3d_s2(cur, pack, bias, cout, relu=relu, addend=ws[skip[name]], out=ws[skip[name]])
            else:
                cur = ops.conv3d(cur, pack, bias, cout, stride=stride, relu=relu, out=ws.get(name))      # prob: a new tensor
        return cur.view(B, 1, D, H, W)


# ---- the drop-ins for the reference's FMT and FMT_with_pathway ------------------------------------------------------------------------
FMT_LAYER_NAMES = ("self", "cross") * 4
FMT_PE_SHAPE = (600, 600)


def sine_position_encoding(d_model=32, max_shape=FMT_PE_SHAPE):
    """The 2-D sinusoidal encoding PositionEncodingSine (models/position_encoding.py, temp_bug_fix=True) registers as its buffer, built
    with the same float32 torch operations so that it has the same bits -> (d_model, *max_shape).  Channel 4 i + (0, 1, 2, 3) is
    (sin x f_i, cos x f_i, sin y f_i, cos y f_i) with x, y counted from 1 and f_i = exp(-2 i ln(10000) / (d_model / 2))."""
    pe = torch.zeros((d_model, *max_shape))
    ys = torch.ones(max_shape).cumsum(0).float().unsqueeze(0)
    xs = torch.ones(max_shape).cumsum(1).float().unsqueeze(0)
    freq = torch.exp(torch.arange(0, d_model // 2, 2).float() * (-np.log(10000.0) / (d_model // 2)))[:, None, None]
    pe[0::4], pe[1::4] = torch.sin(xs * freq), torch.cos(xs * freq)
    pe[2::4], pe[3::4] = torch.sin(ys * freq), torch.cos(ys * freq)
    return pe


class _AttentionLayer(nn.Module):
    """The reference's AttentionLayer around LinearAttention (models/FMT.py:16-75) under its state-dict keys."""

    def __init__(self, d_model, n_heads):
        super().__init__()
        self.query_projection, self.key_projection = nn.Linear(d_model, d_model), nn.Linear(d_model, d_model)
        self.value_projection, self.out_projection = nn.Linear(d_model, d_model), nn.Linear(d_model, d_model)
        self.n_heads = n_heads

    def forward(self, queries, keys, values):
        N, L, _ = queries.shape
        S, H = keys.shape[1], self.n_heads
        Q = F.elu(self.query_projection(queries).view(N, L, H, -1)) + 1
        K = F.elu(self.key_projection(keys).view(N, S, H, -1)) + 1
        values = self.value_projection(values).view(N, S, H, -1)
        KV = torch.einsum("nshd,nshm->nhmd", K, values)
        Z = 1 / (torch.einsum("nlhd,nhd->nlh", Q, K.sum(dim=1)) + 1e-6)
        V = torch.einsum("nlhd,nhmd,nlh->nlhm", Q, KV, Z)
        return self.out_projection(V.contiguous().view(N, L, -1))


class _EncoderLayer(nn.Module):
    """The reference's EncoderLayer (models/FMT.py:78-111; its dropout has probability 0)."""

    def __init__(self, d_model, n_heads):
        super().__init__()
        self.attention = _AttentionLayer(d_model, n_heads)
        self.linear1, self.linear2 = nn.Linear(d_model, 2 * d_model), nn.Linear(2 * d_model, d_model)
        self.norm1, self.norm2 = nn.LayerNorm(d_model), nn.LayerNorm(d_model)

    def forward(self, x, source):
        x = self.norm1(x + self.attention(x, source, source))
        return self.norm2(x + self.linear2(F.relu(self.linear1(x))))


def _tokens(x):
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])


def _maps(tokens, H):
    N, L, C = tokens.shape
    return tokens.reshape(N, H, L // H, C).permute(0, 3, 1, 2)


# the short names of one encoder layer's sixteen tensors in ops.FMT_LAYER_KEYS' order
FMT_LAYER_SHORT = ("wq", "wk", "wv", "wo", "w1", "w2", "bq", "bk", "bv", "bo", "g1", "be1", "b1", "b2", "g2", "be2")


def _layer_parameters(layer):
    """An _EncoderLayer's sixteen parameters in ops.FMT_LAYER_KEYS' order."""
    a = layer.attention
    return (a.query_projection.weight, a.key_projection.weight, a.value_projection.weight, a.out_projection.weight, layer.linear1.weight,
            layer.linear2.weight, a.query_projection.bias, a.key_projection.bias, a.value_projection.bias, a.out_projection.bias,
            layer.norm1.weight, layer.norm1.bias, layer.linear1.bias, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias)


def fmt_layer_grad_torch(x, source, weights, dy):
    """The gradients of one encoder layer y = _EncoderLayer(x, source) under the upstream dy, in closed form and in torch operations, any
    floating dtype: the host restatement of diner_fmt_layer_grad_f32.  x (N,L,32), source (R,S,32) with image n reading source n mod R,
    weights a dict under FMT_LAYER_SHORT's names (torch's (out, in) matrices), dy (N,L,32) -> (d_x, d_source, {name: gradient}).  When
    `source is x` (a self layer) both paths are added into d_x and d_source is None.  relu'(0) = 0; elu'(v) = 1 for v > 0, else exp(v);
    LayerNorm with the biased variance and eps 1e-5."""
    if x.dim() != 3 or source.dim() != 3 or dy.shape != x.shape or x.shape[0] % source.shape[0] or x.shape[2] != source.shape[2]:
        raise ValueError(f"diner_amd: fmt_layer_grad_torch: shapes {tuple(x.shape)}, {tuple(source.shape)}, {tuple(dy.shape)} do not belong together")
    self_layer = source is x
    w = {k: v.detach() for k, v in weights.items()}
    x, source, dy = x.detach(), source.detach(), dy.detach()
    N, L, C = (int(n) for n in x.shape)
    R, S = int(source.shape[0]), int(source.shape[1])
    H = 8
    rows = torch.arange(N, device=x.device) % R
    slope = lambda v: torch.where(v > 0, torch.ones_like(v), torch.exp(v))
    kp = source @ w["wk"].T + w["bk"]
    K = (F.elu(kp) + 1).view(R, S, H, -1)
    V = (source @ w["wv"].T + w["bv"]).view(R, S, H, -1)
    kv, ksum = torch.einsum("rshd,rshm->rhmd", K, V)[rows], K.sum(1)[rows]
    qp = x @ w["wq"].T + w["bq"]
    Q = (F.elu(qp) + 1).view(N, L, H, -1)
    den = torch.einsum("nlhd,nhd->nlh", Q, ksum) + 1e-6
    A = torch.einsum("nlhd,nhmd->nlhm", Q, kv) / den.unsqueeze(-1)

    def norm(v):
        mean = v.mean(-1, keepdim=True)
        rstd = 1 / torch.sqrt(((v - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
        return (v - mean) * rstd, rstd

    def norm_back(g, hat, rstd, gamma):
        gh = g * gamma
        return rstd * (gh - gh.mean(-1, keepdim=True) - hat * (gh * hat).mean(-1, keepdim=True))

    hat1, rstd1 = norm(x + A.reshape(N, L, C) @ w["wo"].T + w["bo"])
    x1 = hat1 * w["g1"] + w["be1"]
    hp = x1 @ w["w1"].T + w["b1"]
    hr = torch.relu(hp)
    hat2, rstd2 = norm(x1 + hr @ w["w2"].T + w["b2"])
    g = {"g2": (dy * hat2).sum((0, 1)), "be2": dy.sum((0, 1))}
    dv2 = norm_back(dy, hat2, rstd2, w["g2"])
    g["w2"], g["b2"] = torch.einsum("nlj,nlk->jk", dv2, hr), dv2.sum((0, 1))
    dh = (dv2 @ w["w2"]) * (hp > 0).to(x.dtype)
    g["w1"], g["b1"] = torch.einsum("nlk,nli->ki", dh, x1), dh.sum((0, 1))
    dx1 = dv2 + dh @ w["w1"]
    g["g1"], g["be1"] = (dx1 * hat1).sum((0, 1)), dx1.sum((0, 1))
    dv1 = norm_back(dx1, hat1, rstd1, w["g1"])
    g["wo"], g["bo"] = torch.einsum("nlj,nlm->jm", dv1, A.reshape(N, L, C)), dv1.sum((0, 1))
    dA = (dv1 @ w["wo"]).view(N, L, H, -1)
    dnum = dA / den.unsqueeze(-1)
    dden = -(dA * A).sum(-1) / den
    dqp = ((torch.einsum("nlhm,nhmd->nlhd", dnum, kv) + dden.unsqueeze(-1) * ksum.unsqueeze(1)) * slope(qp).view(N, L, H, -1)).reshape(N, L, C)
    g["wq"], g["bq"] = torch.einsum("nld,nli->di", dqp, x), dqp.sum((0, 1))
    d_x = dv1 + dqp @ w["wq"]
    d_kv = torch.einsum("nlhm,nlhd->nhmd", dnum, Q).view(N // R, R, H, 4, 4).sum(0)          # d_state: the images that share a row
    d_ksum = torch.einsum("nlh,nlhd->nhd", dden, Q).view(N // R, R, H, 4).sum(0)
    dkp = ((torch.einsum("rhmd,rshm->rshd", d_kv, V) + d_ksum.unsqueeze(1)) * slope(kp).view(R, S, H, -1)).reshape(R, S, C)
    dV = torch.einsum("rhmd,rshd->rshm", d_kv, K).reshape(R, S, C)
    g["wk"], g["bk"] = torch.einsum("rsd,rsi->di", dkp, source), dkp.sum((0, 1))
    g["wv"], g["bv"] = torch.einsum("rsm,rsi->mi", dV, source), dV.sum((0, 1))
    d_source = dkp @ w["wk"] + dV @ w["wv"]
    if self_layer:
        return d_x + d_source, None, g
    return d_x, d_source, g


def _layer_torch(layer, x, source):
    """_EncoderLayer.forward with fmt_layer's row rule: image n of x reads source n mod R."""
    if source is not x and source.shape[0] != x.shape[0]:
        source = source.repeat(x.shape[0] // source.shape[0], 1, 1)
    return layer(x, source)


def fmt_layer_gate(x, source, layer):
    """Whether fmt_layer runs the kernels: float32 HIP tokens and parameters at d_model 32 with 8 heads, inside diner_fmt_layer_grad_f32's
    limits."""
    params = _layer_parameters(layer)
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in (x, source) + params):
        return False
    if layer.attention.n_heads != 8 or tuple(layer.linear1.weight.shape) != (64, 32) or x.dim() != 3 or source.dim() != 3:
        return False
    N, L, R, S = int(x.shape[0]), int(x.shape[1]), int(source.shape[0]), int(source.shape[1])
    top = FMT_PE_SHAPE[0] * FMT_PE_SHAPE[1]
    return x.shape[2] == 32 and source.shape[2] == 32 and 1 <= R <= N <= 65535 and N % R == 0 and 1 <= L <= top and 1 <= S <= top


class _FmtLayer(torch.autograd.Function):
    """diner_fmt_kv_f32 + diner_fmt_layer_f32 / diner_fmt_layer_grad_f32.  Saves x, the source, the layer pack and the 160-float state and
    nothing else.  source None is the self layer (the source is x).  The backward pass is one entry on detached tensors and computes only
    what is needed; asked for a graph of its own (a second derivative) it differentiates _EncoderLayer.forward on the saved inputs."""

    @staticmethod
    def forward(ctx, x, source, layer, pack, *params):
        ops = _ops()
        xs = x.detach().contiguous()
        src = xs if source is None else source.detach().contiguous()
        if pack is None:
            pack = ops.pack_fmt_layer(dict(zip(ops.FMT_LAYER_KEYS, (p.detach() for p in params))))
        state = ops.fmt_kv(src, pack)
        y = ops.fmt_layer(xs, pack, state)
        ctx.save_for_backward(x, source, pack, state)
        ctx.layer = layer
        return y

    @staticmethod
    def backward(ctx, grad):
        x, source, pack, state = ctx.saved_tensors
        need = ctx.needs_input_grad
        params = _layer_parameters(ctx.layer)
        if torch.is_grad_enabled():                 # create_graph=True: the torch layer carries the second derivative
            with torch.enable_grad():
                inputs = [t for t, n in zip((x, source, None, None) + params, need) if n]
                got = iter(torch.autograd.grad(_layer_torch(ctx.layer, x, x if source is None else source), inputs, grad, create_graph=True))
            return tuple(next(got) if n else None for n in need)
        ops = _ops()
        xs = x.detach().contiguous()
        src = xs if source is None else source.detach().contiguous()
        d_x, d_src, d_par = ops.fmt_layer_grad(xs, src, pack, state, grad.detach().to(torch.float32).contiguous(),
                                               want=(need[0], need[1], any(need[4:])))
        d_params = ops.unpack_fmt_layer_grad(d_par) if d_par is not None else [None] * 16
        return (d_x, d_src, None, None) + tuple(g if n else None for g, n in zip(d_params, need[4:]))


def fmt_layer(x, source, layer, pack=None):
    """One encoder layer of the feature transformer, differentiable: x (N,L,32), source (R,S,32) with N a multiple of R (image n reads
    source n mod R), layer an _EncoderLayer -> (N,L,32).  On float32 HIP tensors and parameters it is one once-differentiable autograd
    Function over x, source and the sixteen parameters: ops.fmt_kv + ops.fmt_layer forward (the bits of DeviceFMT.encode_tokens),
    diner_fmt_layer_grad_f32 in the backward pass, which has no atomics and gives the same bits on every run.  `source is x` is the self
    layer: one gradient for x.  pack: the layer's ops.pack_fmt_layer when the caller keeps it.  Anything else (CPU tensors, other dtypes,
    other sizes, a second derivative) runs _EncoderLayer.forward."""
    if not fmt_layer_gate(x, source, layer):
        return _layer_torch(layer, x, source)
    return _FmtLayer.apply(x, None if source is x else source, layer, pack, *_layer_parameters(layer))


class DeviceFMT(nn.Module):
    """A replacement for the reference's FMT (models/FMT.py:114-174): the same state-dict keys (layers.{i}.attention.*_projection.*,
    linear1/2, norm1/2; the positional encoding `pe` is a non-persistent buffer), the same forward(ref_feature, src_feature, feat).
    encode(ref, sources) is the device route: the reference view's tokens through the four self layers and all source views as ONE batch
    through the eight layers on the kernels of csrc/fmt.hip, a cross layer's attention state computed once per batch element from the
    reference view.  forward() itself always runs the reference's torch operations in the reference's order."""

    def __init__(self, config=None):
        super().__init__()
        config = config or {"d_model": 32, "nhead": 8, "layer_names": list(FMT_LAYER_NAMES)}
        self.d_model, self.nhead, self.layer_names = int(config["d_model"]), int(config["nhead"]), list(config["layer_names"])
        self.layers = nn.ModuleList([_EncoderLayer(self.d_model, self.nhead) for _ in self.layer_names])
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
        self.register_buffer("pe", sine_position_encoding(self.d_model).unsqueeze(0), persistent=False)
        self._packed, self._packed_key = None, None
        self.fmt_kernels = False

    @classmethod
    def from_module(cls, fmt):
        new = cls({"d_model": fmt.d_model, "nhead": fmt.nhead, "layer_names": list(fmt.layer_names)})
        p = next(fmt.parameters())
        new.to(device=p.device, dtype=p.dtype)
        new.load_state_dict(fmt.state_dict())
        new.train(fmt.training)
        return new

    def invalidate(self):
        """Forget the packed weights: call after writing a parameter through `.data`, which bumps no version counter."""
        self._packed_key = None

    def packed(self):
        """One ops.pack_fmt_layer per layer of the current parameters; packed again only after a parameter changed."""
        sd = self.state_dict()
        key = tuple((k, v.data_ptr(), v._version, str(v.device)) for k, v in sd.items())
        if key != self._packed_key:
            ops = _ops()
            self._packed, self._packed_key = [ops.pack_fmt_layer(sd, f"layers.{i}.") for i in range(len(self.layers))], key
        return self._packed

    def uses_kernels(self, x):
        """The gate: a float32 HIP map (B,32,H,W) with H, W <= 600, float32 parameters, eval mode, gradients disabled, and the
        reference's layer schedule at d_model 32 with 8 heads."""
        return (x.is_cuda and x.dtype == torch.float32 and self.layers[0].linear1.weight.dtype == torch.float32 and not self.training
                and not torch.is_grad_enabled() and tuple(self.layer_names) == FMT_LAYER_NAMES and self.d_model == 32 and self.nhead == 8
                and x.dim() == 4 and x.shape[1] == 32 and 1 <= x.shape[2] <= FMT_PE_SHAPE[0] and 1 <= x.shape[3] <= FMT_PE_SHAPE[1])

    def trains_on_kernels(self, x):
        """The training gate: fmt_kernels set, gradients enabled, a float32 HIP map (B,32,H,W) with H, W <= 600, float32 parameters and the
        reference's layer schedule at d_model 32 with 8 heads."""
        return (self.fmt_kernels and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32
                and self.layers[0].linear1.weight.dtype == torch.float32 and self.layers[0].linear1.weight.is_cuda
                and tuple(self.layer_names) == FMT_LAYER_NAMES and self.d_model == 32 and self.nhead == 8
                and x.dim() == 4 and x.shape[1] == 32 and 1 <= x.shape[2] <= FMT_PE_SHAPE[0] and 1 <= x.shape[3] <= FMT_PE_SHAPE[1])

    def pos_encoding(self, x):
        return x + self.pe[:, :, :x.size(2), :x.size(3)]

    def forward(self, ref_feature=None, src_feature=None, feat="ref"):
        assert ref_feature is not None
        if feat == "ref":
            assert self.d_model == ref_feature.size(1)
            H = ref_feature.shape[2]
            x = _tokens(self.pos_encoding(ref_feature))
            out = []
            for layer, name in zip(self.layers, self.layer_names):
                if name == "self":
                    x = layer(x, x)
                    out.append(_maps(x, H))
            return out
        if feat == "src":
            assert self.d_model == ref_feature[0].size(1)
            H = ref_feature[0].shape[2]
            refs = [_tokens(r) for r in ref_feature]
            x = _tokens(self.pos_encoding(src_feature))
            for i, (layer, name) in enumerate(zip(self.layers, self.layer_names)):
                if name == "self":
                    x = layer(x, x)
                elif name == "cross":
                    x = layer(x, refs[i // 2])
                else:
                    raise KeyError
            return _maps(x, H)
        raise ValueError("Wrong feature name")

    def encode_tokens(self, maps):
        """maps (NV,B,32,H,W) contiguous float32 on the device, view 0 the reference -> tokens (NV,B,H W,32): the reference view after its
        four self layers, every source view after all eight.  Everything on the current stream, no host synchronisation."""
        ops = _ops()
        NV, B, _, H, W = (int(n) for n in maps.shape)
        L = H * W
        packs = self.packed()
        maps = maps.contiguous()                 # stacked channels-last views (DeviceFeatureNet's kernel route) keep their strides
        tok = ops.fmt_tokenise(maps.view(NV * B, 32, H, W), self.pe[0]).view(NV, B, L, 32)
        ref, src = tok[0], tok[1:].reshape((NV - 1) * B, L, 32) if NV > 1 else None
        partials = torch.empty(max(NV - 1, 1) * B * ops.fmt_kv_blocks(L) * ops.FMT_STATE_FLOATS, dtype=torch.float64, device=maps.device)
        cross = []
        for j in range(4):
            ops.fmt_layer(ref, packs[2 * j], ops.fmt_kv(ref, packs[2 * j], partials), out=ref)
            if src is not None:
                cross.append(ops.fmt_kv(ref, packs[2 * j + 1], partials))         # reference output j feeds cross layer 2 j + 1
        if src is not None:
            for j in range(4):
                ops.fmt_layer(src, packs[2 * j], ops.fmt_kv(src, packs[2 * j], partials), out=src)
                ops.fmt_layer(src, packs[2 * j + 1], cross[j], out=src)          # image n = view B + b reads row n mod B
        return tok

    def encode_train(self, views):
        """encode_tokens' schedule out of place through fmt_layer, differentiable: views a list of (B,32,H,W), view 0 the reference ->
        (ref', [source', ...]).  The reference view runs its four self layers; all source views run as one batch of NS B images through
        the eight layers, cross layer 2 j + 1 reading the reference output j as a (B, S, 32) source, so the sum over the views reaches
        that output's gradient through d_state."""
        B, _, H, W = (int(n) for n in views[0].shape)
        packs = self.packed()
        ref = _tokens(self.pos_encoding(views[0]))
        outs = []
        for j in range(4):
            ref = fmt_layer(ref, ref, self.layers[2 * j], pack=packs[2 * j])
            outs.append(ref)
        if len(views) == 1:
            return _maps(ref, H), []
        NS = len(views) - 1
        src = _tokens(self.pos_encoding(torch.stack(views[1:], 0).view(NS * B, 32, H, W)))
        for j in range(4):
            src = fmt_layer(src, src, self.layers[2 * j], pack=packs[2 * j])
            src = fmt_layer(src, outs[j], self.layers[2 * j + 1], pack=packs[2 * j + 1])      # image n = view B + b reads row n mod B
        src = src.view(NS, B, H * W, 32)
        return _maps(ref, H), [_maps(src[v], H) for v in range(NS)]

    def encode(self, ref, sources):
        """The device route of one sample batch: ref (B,32,H,W), sources a list of (B,32,H,W) -> (ref', [source', ...]), each (B,32,H,W)
        as a permuted view of channels-last memory.  Outside the gate: forward() per view, as the reference's FMT_with_pathway calls it."""
        views = [ref] + list(sources)
        if self.uses_kernels(ref) and all(v.shape == ref.shape and v.is_cuda and v.dtype == torch.float32 for v in views):
            B, _, H, W = ref.shape
            tok = self.encode_tokens(torch.stack([v.detach() for v in views], 0))
            out = [tok[v].view(B, H, W, 32).permute(0, 3, 1, 2) for v in range(len(views))]
            return out[0], out[1:]
        if self.trains_on_kernels(ref) and all(v.shape == ref.shape and v.is_cuda and v.dtype == torch.float32 for v in views):
            return self.encode_train(views)
        refs = self.forward(ref.clone(), feat="ref")
        return refs[-1], [self.forward([r.clone() for r in refs], s.clone(), feat="src") for s in sources]


class DeviceFMTWithPathway(nn.Module):
    """A replacement for the reference's FMT_with_pathway (models/FMT.py:178-225): the same 132 state-dict keys (FMT.layers.*,
    dim_reduction_{1,2}.weight, smooth_{1,2}.weight), the same forward(features): it rewrites "stage1" / "stage2" / "stage3" of each
    view's dict in place and returns the list.  The kernel route (csrc/fmt.hip, and diner_conv3x3_f32 for the smooth convolutions) needs
    float32 HIP tensors and parameters, eval mode, gradients disabled, layer_names ['self','cross'] * 4, every view of one shape,
    stage 2 and stage 3 exactly 2 x and 4 x stage 1 with 16 and 8 channels, and H, W <= 600; all views then run as one batch.  Its results
    have the reference's shapes (B,C,H,W) but are PERMUTED VIEWS OF CHANNELS-LAST MEMORY (call .contiguous() where NCHW strides matter).
    Outside the gate it runs the reference's torch operations in the reference's order: differentiable, and failing where the reference
    fails.  `mvs.to_device(model)` switches a loaded TransMVSNet over."""

    def __init__(self, base_channels=8, FMT_config=None):
        super().__init__()
        c = int(base_channels)
        self.base_channels = c
        self.FMT = DeviceFMT(FMT_config)
        self.dim_reduction_1 = nn.Conv2d(c * 4, c * 2, 1, bias=False)
        self.dim_reduction_2 = nn.Conv2d(c * 2, c * 1, 1, bias=False)
        self.smooth_1 = nn.Conv2d(c * 2, c * 2, 3, padding=1, bias=False)
        self.smooth_2 = nn.Conv2d(c * 1, c * 1, 3, padding=1, bias=False)
        self._packed, self._packed_key = None, None

    @classmethod
    def from_module(cls, module):
        fmt = module.FMT
        new = cls(int(module.dim_reduction_2.weight.shape[0]), {"d_model": fmt.d_model, "nhead": fmt.nhead, "layer_names": list(fmt.layer_names)})
        p = module.dim_reduction_1.weight
        new.to(device=p.device, dtype=p.dtype)
        new.load_state_dict(module.state_dict())
        new.train(module.training)
        return new

    @property
    def fmt_kernels(self):
        return self.FMT.fmt_kernels

    @fmt_kernels.setter
    def fmt_kernels(self, value):
        self.FMT.fmt_kernels = bool(value)

    def invalidate(self):
        """Forget the packed weights of the pathway and of the FMT: call after writing a parameter through `.data`."""
        self._packed_key = None
        self.FMT.invalidate()

    def packed(self):
        """(smooth_1 packed, smooth_2 packed) in ops.pack_conv3x3's layout of the current parameters."""
        ws = (self.smooth_1.weight, self.smooth_2.weight)
        key = tuple((w.data_ptr(), w._version, str(w.device)) for w in ws)
        if key != self._packed_key:
            ops = _ops()
            self._packed, self._packed_key = tuple(ops.pack_conv3x3(w.detach()) for w in ws), key
        return self._packed

    def uses_kernels(self, features):
        if not features or not self.FMT.uses_kernels(features[0]["stage1"]) or self.training or self.base_channels != 8:
            return False
        s1, s2, s3 = (features[0][k] for k in ("stage1", "stage2", "stage3"))
        B, _, H, W = s1.shape
        if tuple(s2.shape) != (B, 16, 2 * H, 2 * W) or tuple(s3.shape) != (B, 8, 4 * H, 4 * W) or self.smooth_1.weight.dtype != torch.float32:
            return False
        return all(f[k].shape == features[0][k].shape and f[k].is_cuda and f[k].dtype == torch.float32
                   for f in features for k in ("stage1", "stage2", "stage3"))

    def _upsample_add(self, x, y):
        return F.interpolate(x, size=(y.shape[2], y.shape[3]), mode="bilinear") + y

    def forward_torch(self, features):
        refs = None
        for i, f in enumerate(features):
            if i == 0:
                refs = self.FMT(f["stage1"].clone(), feat="ref")
                f["stage1"] = refs[-1]
            else:
                f["stage1"] = self.FMT([r.clone() for r in refs], f["stage1"].clone(), feat="src")
            f["stage2"] = self.smooth_1(self._upsample_add(self.dim_reduction_1(f["stage1"]), f["stage2"]))
            f["stage3"] = self.smooth_2(self._upsample_add(self.dim_reduction_2(f["stage2"]), f["stage3"]))
        return features

    def pathway(self, tok, lateral2, lateral3):
        """tok (N,H,W,32), lateral2 (N,2H,2W,16), lateral3 (N,4H,4W,8), channels-last -> (stage 2, stage 3) channels-last.  The merges
        write over the laterals."""
        ops = _ops()
        p1, p2 = self.packed()
        m2 = ops.fpn_merge(tok, self.dim_reduction_1.weight.detach(), lateral2, out=lateral2)
        s2 = ops.conv3x3(m2, p1, None, 16)
        m3 = ops.fpn_merge(s2, self.dim_reduction_2.weight.detach(), lateral3, out=lateral3)
        return s2, ops.conv3x3(m3, p2, None, 8)

    def forward_train(self, features):
        """forward_torch with the transformer on DeviceFMT.encode's training route (fmt_kernels); the pathway stays torch, per view."""
        ref, sources = self.FMT.encode(features[0]["stage1"], [f["stage1"] for f in features[1:]])
        for f, stage1 in zip(features, [ref] + list(sources)):
            f["stage1"] = stage1
            f["stage2"] = self.smooth_1(self._upsample_add(self.dim_reduction_1(f["stage1"]), f["stage2"]))
            f["stage3"] = self.smooth_2(self._upsample_add(self.dim_reduction_2(f["stage2"]), f["stage3"]))
        return features

    def forward(self, features):
        if not self.uses_kernels(features):
            if features and self.FMT.trains_on_kernels(features[0]["stage1"]) and all(
                    f["stage1"].shape == features[0]["stage1"].shape and f["stage1"].is_cuda and f["stage1"].dtype == torch.float32 for f in features):
                return self.forward_train(features)
            return self.forward_torch(features)
        NV = len(features)
        B, _, H, W = (int(n) for n in features[0]["stage1"].shape)
        tok = self.FMT.encode_tokens(torch.stack([f["stage1"].detach() for f in features], 0))
        cl = lambda key: torch.stack([f[key].detach() for f in features], 0).permute(0, 1, 3, 4, 2).contiguous().view(NV * B, *(
            features[0][key].shape[i] for i in (2, 3, 1)))                    # the one repack of each lateral: a copy the merge may write over
        s2, s3 = self.pathway(tok.view(NV * B, H, W, 32), cl("stage2"), cl("stage3"))
        for v, f in enumerate(features):
            f["stage1"] = tok[v].view(B, H, W, 32).permute(0, 3, 1, 2)
            f["stage2"] = s2[v * B:(v + 1) * B].permute(0, 3, 1, 2)
            f["stage3"] = s3[v * B:(v + 1) * B].permute(0, 3, 1, 2)
        return features


# ---- the drop-in for the reference's FeatureNet -------------------------------------------------------------------------------------------
def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else tuple(int(a) for a in v)


def deform_conv2d_torch(input, offset, weight, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), mask=None):
    """torchvision.ops.deform_conv2d in torch operations (index gathers; differentiable in every argument; any floating dtype), with one
    offset group and one weight group: input (B,Cin,H,W), offset (B, 2 kh kw, Ho, Wo) with channel 2 k the row and 2 k + 1 the column
    offset of tap k = ky kw + kx, weight (Cout,Cin,kh,kw), mask (B, kh kw, Ho, Wo) or None -> (B,Cout,Ho,Wo).  Tap k of output pixel
    (h, w) samples the input at py = (h stride - padding + ky dilation) + dy, px likewise, with torchvision's bilinear_interpolate: 0 when
    py <= -1, py >= H, px <= -1 or px >= W; otherwise y0 = floor(py), ly = py - y0, hy = 1 - ly (columns likewise), corners outside the
    image contribute 0, value = hy hx v00 + hy lx v01 + ly hx v10 + ly lx v11; times the mask; then the convolution's sum and the bias."""
    if input.dim() != 4 or weight.dim() != 4 or offset.dim() != 4:
        raise ValueError("diner_amd: deform_conv2d_torch expects input (B,Cin,H,W), offset (B,2 kh kw,Ho,Wo) and weight (Cout,Cin,kh,kw)")
    B, Cin, H, W = (int(n) for n in input.shape)
    Cout, Cw, kh, kw = (int(n) for n in weight.shape)
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    K = kh * kw
    if Cw != Cin:
        raise ValueError(f"diner_amd: deform_conv2d_torch is stated for one weight group: weight has {Cw} input channels, input {Cin}")
    if tuple(offset.shape) != (B, 2 * K, Ho, Wo):
        raise ValueError(f"diner_amd: deform_conv2d_torch is stated for one offset group: offset must be {(B, 2 * K, Ho, Wo)}, got "
                         f"{tuple(offset.shape)}")
    if mask is not None and tuple(mask.shape) != (B, K, Ho, Wo):
        raise ValueError(f"diner_amd: deform_conv2d_torch expects mask {(B, K, Ho, Wo)}, got {tuple(mask.shape)}")
    dt, dev = input.dtype, input.device
    ky, kx = torch.arange(kh, device=dev).repeat_interleave(kw), torch.arange(kw, device=dev).repeat(kh)
    base_y = (torch.arange(Ho, device=dev) * sh - ph).view(1, Ho, 1) + (ky * dh).view(K, 1, 1)          # integers first, as torchvision sums them
    base_x = (torch.arange(Wo, device=dev) * sw - pw).view(1, 1, Wo) + (kx * dw).view(K, 1, 1)
    py = base_y.to(dt).unsqueeze(0) + offset[:, 0::2]
    px = base_x.to(dt).unsqueeze(0) + offset[:, 1::2]
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)                   # a NaN fails every comparison: outside
    py, px = torch.where(inside, py, torch.zeros_like(py)), torch.where(inside, px, torch.zeros_like(px))
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    hy, hx = 1 - ly, 1 - lx
    y0i, x0i = y0.detach().long(), x0.detach().long()
    flat = input.reshape(B, Cin, H * W)

    def corner(yi, xi):
        valid = inside & (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).reshape(B, 1, K * Ho * Wo).expand(B, Cin, K * Ho * Wo)
        v = flat.gather(2, idx).reshape(B, Cin, K, Ho, Wo)
        return torch.where(valid.unsqueeze(1), v, torch.zeros_like(v))

    val = ((hy * hx).unsqueeze(1) * corner(y0i, x0i) + (hy * lx).unsqueeze(1) * corner(y0i, x0i + 1)
           + (ly * hx).unsqueeze(1) * corner(y0i + 1, x0i) + (ly * lx).unsqueeze(1) * corner(y0i + 1, x0i + 1))
    if mask is not None:
        val = val * mask.unsqueeze(1)
    out = torch.matmul(weight.reshape(Cout, Cin * K), val.reshape(B, Cin * K, Ho * Wo)).reshape(B, Cout, Ho, Wo)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def _deform_samples(x, offmask):
    """The sampling geometry of the 3 x 3, stride 1, padding 1 layer, deform_conv2d_torch's expressions: x (B,Cin,H,W), offmask (B,27,H,W)
    -> inside (B,9,H,W), (ly, lx, hy, hx), and per corner (y0,x0), (y0,x1), (y1,x0), (y1,x1): the index (B,9 H W) into the flattened map,
    valid (B,9,H,W) and the values (B,Cin,9,H,W), zero where the corner is not valid."""
    B, Cin, H, W = (int(n) for n in x.shape)
    dt, dev = x.dtype, x.device
    k = torch.arange(9, device=dev)
    base_y = (torch.arange(H, device=dev) - 1).view(1, H, 1) + (k // 3).view(9, 1, 1)
    base_x = (torch.arange(W, device=dev) - 1).view(1, 1, W) + (k % 3).view(9, 1, 1)
    py = base_y.to(dt).unsqueeze(0) + offmask[:, 0:18:2]
    px = base_x.to(dt).unsqueeze(0) + offmask[:, 1:18:2]
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    py, px = torch.where(inside, py, torch.zeros_like(py)), torch.where(inside, px, torch.zeros_like(px))
    y0, x0 = torch.floor(py), torch.floor(px)
    ly, lx = py - y0, px - x0
    y0i, x0i = y0.long(), x0.long()
    flat = x.reshape(B, Cin, H * W)
    corners = []
    for yi, xi in ((y0i, x0i), (y0i, x0i + 1), (y0i + 1, x0i), (y0i + 1, x0i + 1)):
        valid = inside & (yi >= 0) & (yi <= H - 1) & (xi >= 0) & (xi <= W - 1)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).reshape(B, 9 * H * W)
        v = flat.gather(2, idx.unsqueeze(1).expand(B, Cin, 9 * H * W)).reshape(B, Cin, 9, H, W)
        corners.append((idx, valid, torch.where(valid.unsqueeze(1), v, torch.zeros_like(v))))
    return inside, (ly, lx, 1 - ly, 1 - lx), corners


def deform_conv3x3_grad_torch(x, offmask, weight, dy):
    """The gradients of y = deform_conv2d_torch(x, offmask[:, :18], weight, bias, 1, 1, 1, mask=sigmoid(offmask[:, 18:])) under the upstream
    dy (B,Cout,H,W), in closed form and in torch operations, any floating dtype: the host restatement of diner_deform_conv3x3_grad_f32.
    x (B,Cin,H,W), the raw offmask (B,27,H,W), weight (Cout,Cin,3,3) -> (d_x, d_offmask, d_weight, d_bias).  With m the sigmoid, S the
    sample, v_i its corner values (0 where not valid), G[b,c,k] = sum_o dy[b,o] w[o,c,k]: d_logit = m (1 - m) sum_c G S; d_dy = m sum_c G
    (-hx v00 - lx v01 + hx v10 + lx v11), d_dx = m sum_c G (-hy v00 + hy v01 - ly v10 + ly v11) -- at an integer coordinate the
    right-sided difference, as autograd through floor() gives it; d_x adds m wt_i G at every valid corner; d_weight = sum dy m S;
    d_bias = sum dy.  A tap that lies outside (a NaN offset included) has gradients that are exactly 0."""
    if x.dim() != 4 or offmask.dim() != 4 or weight.dim() != 4 or dy.dim() != 4:
        raise ValueError("diner_amd: deform_conv3x3_grad_torch expects x (B,Cin,H,W), offmask (B,27,H,W), weight (Cout,Cin,3,3), dy (B,Cout,H,W)")
    B, Cin, H, W = (int(n) for n in x.shape)
    Cout = int(weight.shape[0])
    if tuple(offmask.shape) != (B, 27, H, W) or tuple(weight.shape) != (Cout, Cin, 3, 3) or tuple(dy.shape) != (B, Cout, H, W):
        raise ValueError(f"diner_amd: deform_conv3x3_grad_torch: shapes {tuple(x.shape)}, {tuple(offmask.shape)}, {tuple(weight.shape)}, "
                         f"{tuple(dy.shape)} do not belong together")
    x, offmask, weight, dy = x.detach(), offmask.detach(), weight.detach(), dy.detach()
    inside, (ly, lx, hy, hx), corners = _deform_samples(x, offmask)
    zero = torch.zeros_like(ly)
    masked = lambda ts: [torch.where(inside, t, zero) for t in ts]
    wt = masked((hy * hx, hy * lx, ly * hx, ly * lx))
    gy = masked((-hx, -lx, hx, lx))
    gx = masked((-hy, hy, -ly, ly))
    m = torch.sigmoid(offmask[:, 18:])
    G = torch.einsum("bohw,ock->bckhw", dy, weight.reshape(Cout, Cin, 9))
    S = sum(w.unsqueeze(1) * v for w, (_, _, v) in zip(wt, corners))
    d_logit = m * (1 - m) * (G * S).sum(1)
    d_dy = m * (G * sum(w.unsqueeze(1) * v for w, (_, _, v) in zip(gy, corners))).sum(1)
    d_dx = m * (G * sum(w.unsqueeze(1) * v for w, (_, _, v) in zip(gx, corners))).sum(1)
    d_offmask = torch.cat((torch.stack((d_dy, d_dx), 2).reshape(B, 18, H, W), d_logit), 1)
    d_x = torch.zeros(B, Cin, H * W, dtype=x.dtype, device=x.device)
    for w, (idx, valid, _) in zip(wt, corners):
        coef = torch.where(valid, m * w, zero)
        d_x.scatter_add_(2, idx.unsqueeze(1).expand(B, Cin, 9 * H * W), (coef.unsqueeze(1) * G).reshape(B, Cin, 9 * H * W))
    d_weight = torch.einsum("bohw,bckhw->ock", dy, m.unsqueeze(1) * S).reshape(Cout, Cin, 3, 3)
    return d_x.view(B, Cin, H, W), d_offmask, d_weight, dy.sum((0, 2, 3))


def _deform_torch(x, offmask, weight, bias):
    return deform_conv2d_torch(x, offmask[:, :18], weight, bias, (1, 1), (1, 1), (1, 1), mask=torch.sigmoid(offmask[:, 18:]))


def deform_gate(x, offmask, weight, bias=None):
    """Whether deform_conv3x3 runs the kernels: float32 HIP tensors inside diner_deform_conv3x3_grad_f32's limits."""
    tensors = [x, offmask, weight] + ([] if bias is None else [bias])
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in tensors):
        return False
    if x.dim() != 4 or weight.dim() != 4 or offmask.dim() != 4 or tuple(weight.shape[1:]) != (x.shape[1], 3, 3):
        return False
    B, Cin, H, W = (int(n) for n in x.shape)
    Cout = int(weight.shape[0])
    if tuple(offmask.shape) != (B, 27, H, W) or (bias is not None and tuple(bias.shape) != (Cout,)):
        return False
    return _ops().deform_grad_supported(Cin, Cout) and 1 <= B <= 65535 and 1 <= H <= 1 << 14 and 1 <= W <= 1 << 14


class _DeformConv3x3(torch.autograd.Function):
    """diner_deform_conv3x3_f32 / diner_deform_conv3x3_grad_f32.  Saves its inputs x, offmask and the weight and nothing else: no sampled
    matrix, no index tensors.  The backward pass is a kernel on detached tensors and computes only the gradients that are needed; asked
    for a graph of its own (a second derivative) it differentiates deform_conv2d_torch on the saved inputs instead."""

    @staticmethod
    def forward(ctx, x, offmask, weight, bias):
        ops = _ops()
        x_cl = x.detach().permute(0, 2, 3, 1).contiguous()
        om_cl = offmask.detach().permute(0, 2, 3, 1).contiguous()
        w = weight.detach().contiguous()
        y = ops.deform_conv3x3(x_cl, om_cl, ops.pack_deform_conv3x3(w), None if bias is None else bias.detach().contiguous(), int(w.shape[0]))
        ctx.save_for_backward(x, offmask, weight)
        ctx.has_bias = bias is not None
        return y.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad):
        x, offmask, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():                 # create_graph=True: the torch restatement carries the second derivative
            with torch.enable_grad():
                bias = torch.zeros(weight.shape[0], dtype=weight.dtype, device=weight.device, requires_grad=True) if ctx.has_bias else None
                inputs = [t for t, n in zip((x, offmask, weight, bias), need) if n]
                got = iter(torch.autograd.grad(_deform_torch(x, offmask, weight, bias), inputs, grad, create_graph=True))
            return tuple(next(got) if n else None for n in need)
        want = (need[0], need[1], need[2], ctx.has_bias and need[3])
        d_x, d_om, d_w, d_b = _ops().deform_conv3x3_grad(x.detach().permute(0, 2, 3, 1).contiguous(), offmask.detach().permute(0, 2, 3, 1).contiguous(),
                                                         weight.detach().contiguous(), grad.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous(),
                                                         want=want)
        return (None if d_x is None else d_x.permute(0, 3, 1, 2), None if d_om is None else d_om.permute(0, 3, 1, 2), d_w, d_b)


def deform_conv3x3(x, offmask, weight, bias=None):
    """The modulated deformable 3 x 3 convolution (stride 1, padding 1, one offset group) of a DCN layer, differentiable: x (B,Cin,H,W),
    offmask (B,27,H,W) the raw conv_offset_mask output (channel 2 k the row and 2 k + 1 the column offset of tap k, 18 + k the logit of its
    modulation), weight (Cout,Cin,3,3) -> (B,Cout,H,W).  On float32 HIP tensors with Cin a multiple of 8 up to 64 and Cout up to 64 it is
    one autograd Function: diner_deform_conv3x3_f32 forward (the result is a PERMUTED VIEW OF CHANNELS-LAST MEMORY), in the backward pass
    diner_deform_conv3x3_grad_f32, which computes only the gradients that are needed; d_x comes from float atomic adds and is not
    bit-reproducible.  Anything else (CPU tensors, other dtypes, other sizes, a second derivative) runs deform_conv2d_torch."""
    if not deform_gate(x, offmask, weight, bias):
        return _deform_torch(x, offmask, weight, bias)
    return _DeformConv3x3.apply(x, offmask, weight, bias)


class _Conv2dBnReLU(nn.Module):
    """The reference's Conv2d block (models/module.py:24-62) with BatchNorm and ReLU, under its state-dict keys (conv.weight, bn.*)."""

    def __init__(self, cin, cout, kernel, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, momentum=0.1)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)), inplace=True)


class _DCN(nn.Module):
    """The reference's DCN (models/dcn.py) under its state-dict keys (weight, bias, conv_offset_mask.*), on deform_conv2d_torch; with
    deform_kernels set (default False: bit for bit as it was) on deform_conv3x3, whose backward pass is a kernel."""

    def __init__(self, cin, cout):
        super().__init__()
        self.deform_kernels = False
        self.weight = nn.Parameter(torch.empty(cout, cin, 3, 3))
        self.bias = nn.Parameter(torch.zeros(cout))
        self.conv_offset_mask = nn.Conv2d(cin, 27, 3, stride=1, padding=1, bias=True)
        stdv = 1.0 / np.sqrt(cin * 9)
        nn.init.uniform_(self.weight, -stdv, stdv)
        nn.init.zeros_(self.conv_offset_mask.weight)
        nn.init.zeros_(self.conv_offset_mask.bias)

    def forward(self, x):
        out = self.conv_offset_mask(x)
        if self.deform_kernels:
            return deform_conv3x3(x, out, self.weight, self.bias)       # falls back to deform_conv2d_torch by itself
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        return deform_conv2d_torch(x, torch.cat((o1, o2), dim=1), self.weight, self.bias, (1, 1), (1, 1), (1, 1), mask=torch.sigmoid(mask))


def _fold_bn2d(weight, bias, sd, bn):
    """A 2-D convolution (bias or None) followed by the BatchNorm under prefix `bn` of sd as one convolution with a bias, fold_conv_bn's
    idiom: float64 on the tensors' own device, rounded once: s = gamma / sqrt(var + eps), w' = w s, b' = (b - mean) s + beta."""
    s = sd[bn + "weight"].detach().double() / torch.sqrt(sd[bn + "running_var"].detach().double() + BN_EPS)
    b = 0.0 if bias is None else bias.detach().double()
    return ((weight.detach().double() * s.view(-1, 1, 1, 1)).to(torch.float32),
            ((b - sd[bn + "running_mean"].detach().double()) * s + sd[bn + "bias"].detach().double()).to(torch.float32))


def _pad_bias(b, n=64):
    out = b.new_zeros(-(-b.shape[0] // n) * n)
    out[:b.shape[0]] = b
    return out


FEATURENET_HEADS = (("out1", "stage1", 32), ("out2", "stage2", 16), ("out3", "stage3", 8))


class DeviceFeatureNet(nn.Module):
    """A replacement for the reference's FeatureNet (models/module.py:343-421): the same state-dict keys (conv0.0.conv.weight,
    conv0.0.bn.*, ... out1.1.weight, out1.1.bias, out1.1.conv_offset_mask.*, out1.2.*, ... inner1.*, inner2.*), the same forward():
    images (B,3,H,W) -> {"stage1": (B,32,H/4,W/4), "stage2": (B,16,H/2,W/2), "stage3": (B,8,H,W)}.  On float32 HIP tensors and
    parameters, in eval mode, with gradients disabled, base_channels 8 and H, W multiples of 4 (the only sizes at which the reference's
    own upsample-and-add matches) it runs the kernels: diner_encoder_input_f32 (C 4), diner_conv3x3_f32, diner_conv5x5_s2_f32,
    diner_conv1x1_f32, diner_fpn_lateral_f32 and, for each of the nine deformable convolutions, diner_conv3x3_f32 (the 27 offset and
    modulation channels) followed by diner_deform_conv3x3_f32; BatchNorm is folded into the weights.  Its results then have the
    reference's shapes but are PERMUTED VIEWS OF CHANNELS-LAST MEMORY, which DeviceFMTWithPathway takes unchanged.  Otherwise it runs
    the reference's operations in the reference's order, the deformable convolution as deform_conv2d_torch: differentiable, on batch
    statistics in training mode.  No torchvision anywhere.  `mvs.to_device(model)` switches a loaded TransMVSNet over.

    deform_kernels (default False: every route is as it was, bit for bit).  When True, the nine deformable convolutions of the torch
    route run deform_conv3x3: diner_deform_conv3x3_f32 forward and diner_deform_conv3x3_grad_f32 in the backward pass, with no gathered
    tensors kept for it; conv_offset_mask, the BatchNorms and the plain convolutions stay torch operations, and any input outside the
    kernels' limits takes deform_conv2d_torch silently.  The kernel route of eval mode does not look at the switch."""

    def __init__(self, base_channels=8):
        super().__init__()
        c = self.base_channels = int(base_channels)
        self.conv0 = nn.Sequential(_Conv2dBnReLU(3, c, 3, 1, 1), _Conv2dBnReLU(c, c, 3, 1, 1))
        self.conv1 = nn.Sequential(_Conv2dBnReLU(c, 2 * c, 5, 2, 2), _Conv2dBnReLU(2 * c, 2 * c, 3, 1, 1), _Conv2dBnReLU(2 * c, 2 * c, 3, 1, 1))
        self.conv2 = nn.Sequential(_Conv2dBnReLU(2 * c, 4 * c, 5, 2, 2), _Conv2dBnReLU(4 * c, 4 * c, 3, 1, 1), _Conv2dBnReLU(4 * c, 4 * c, 3, 1, 1))
        f = 4 * c

        def head(first, cout):
            return nn.Sequential(first, _DCN(f, f), nn.BatchNorm2d(f), nn.ReLU(inplace=True), _DCN(f, f), nn.BatchNorm2d(f),
                                 nn.ReLU(inplace=True), _DCN(f, cout))
        self.out1 = head(_Conv2dBnReLU(f, f, 1), f)
        self.inner1 = nn.Conv2d(2 * c, f, 1, bias=True)
        self.inner2 = nn.Conv2d(c, f, 1, bias=True)
        self.out2 = head(_Conv2dBnReLU(f, f, 3, 1, 1), 2 * c)
        self.out3 = head(_Conv2dBnReLU(f, f, 3, 1, 1), c)
        self.out_channels = [4 * c, 2 * c, c]
        self._packed, self._packed_key = None, None

    @property
    def deform_kernels(self):
        return all(m.deform_kernels for m in self.modules() if isinstance(m, _DCN))

    @deform_kernels.setter
    def deform_kernels(self, value):
        for m in self.modules():
            if isinstance(m, _DCN):
                m.deform_kernels = bool(value)

    @classmethod
    def from_module(cls, feature):
        sd = feature.state_dict()
        w = sd["conv0.0.conv.weight"]
        new = cls(int(w.shape[0]))
        new.to(device=w.device, dtype=w.dtype)
        new.load_state_dict(sd)
        new.train(feature.training)
        return new

    def invalidate(self):
        """Forget the packed weights: call after writing a parameter or buffer through `.data`, which bumps no version counter."""
        self._packed_key = None

    def packed(self):
        """name -> (packed weight, bias) of every layer of the kernel route, BatchNorm folded, of the current parameters; a deformable
        layer "outX.i" has a second entry "outX.i.offset" for its conv_offset_mask.  Packed again only after a parameter or buffer
        changed (no host read-back either way)."""
        sd = self.state_dict()
        key = tuple((k, v.data_ptr(), v._version, str(v.device)) for k, v in sd.items())
        if key != self._packed_key:
            ops = _ops()
            P = {}
            for name, kind in (("conv0.0", 3), ("conv0.1", 3), ("conv1.0", 5), ("conv1.1", 3), ("conv1.2", 3), ("conv2.0", 5), ("conv2.1", 3),
                               ("conv2.2", 3), ("out1.0", 1), ("out2.0", 3), ("out3.0", 3)):
                w, b = _fold_bn2d(sd[name + ".conv.weight"], None, sd, name + ".bn.")
                if kind == 3:
                    cin = 4 if name == "conv0.0" else None                   # the input relayout writes four channels, the fourth zero
                    P[name] = (ops.pack_conv3x3(w, Cin=cin), _pad_bias(b))
                else:
                    P[name] = ((ops.pack_conv5x5 if kind == 5 else ops.pack_conv1x1)(w), b.contiguous())
            for head, _, _ in FEATURENET_HEADS:
                for i in (1, 4, 7):
                    d = f"{head}.{i}."
                    P[d + "offset"] = (ops.pack_conv3x3(sd[d + "conv_offset_mask.weight"].detach().float()),
                                       _pad_bias(sd[d + "conv_offset_mask.bias"].detach().float()))
                    if i < 7:
                        w, b = _fold_bn2d(sd[d + "weight"], sd[d + "bias"], sd, f"{head}.{i + 1}.")
                    else:
                        w, b = sd[d + "weight"].detach().float(), sd[d + "bias"].detach().float()
                    P[d[:-1]] = (ops.pack_deform_conv3x3(w.contiguous()), b.contiguous())
            for name in ("inner1", "inner2"):
                P[name] = (sd[name + ".weight"].detach().float().contiguous(), sd[name + ".bias"].detach().float().contiguous())
            self._packed, self._packed_key = P, key
        return self._packed

    def uses_kernels(self, x):
        """The gate.  Parameters of another dtype than float32 leave it closed, so that a float32 input then fails in torch's own
        convolution as it does in the reference."""
        return (x.is_cuda and x.dtype == torch.float32 and self.inner1.weight.dtype == torch.float32 and not self.training
                and not torch.is_grad_enabled() and self.base_channels == 8 and x.dim() == 4 and x.shape[1] == 3 and x.shape[0] >= 1
                and x.shape[2] >= 4 and x.shape[3] >= 4 and x.shape[2] % 4 == 0 and x.shape[3] % 4 == 0)

    def forward_torch(self, x):
        conv0 = self.conv0(x)
        conv1 = self.conv1(conv0)
        conv2 = self.conv2(conv1)
        intra_feat = conv2
        outputs = {"stage1": self.out1(intra_feat)}
        intra_feat = F.interpolate(intra_feat, scale_factor=2, mode="nearest") + self.inner1(conv1)
        outputs["stage2"] = self.out2(intra_feat)
        intra_feat = F.interpolate(intra_feat, scale_factor=2, mode="nearest") + self.inner2(conv0)
        outputs["stage3"] = self.out3(intra_feat)
        return outputs

    def forward_cl(self, x):
        """The kernel route on images (N,3,H,W) -> channels-last (stage 1 (N,H/4,W/4,32), stage 2 (N,H/2,W/2,16), stage 3 (N,H,W,8))."""
        ops, P = _ops(), self.packed()
        conv = lambda t, name, cout: ops.conv3x3(t, *P[name], cout, relu=True)

        def head(t, name, cout):
            for i, (co, relu) in ((1, (32, True)), (4, (32, True)), (7, (cout, False))):
                offmask = ops.conv3x3(t, *P[f"{name}.{i}.offset"], 27)
                t = ops.deform_conv3x3(t, offmask, *P[f"{name}.{i}"], co, relu=relu)
            return t
        x = ops.encoder_input(x.detach().contiguous(), pad=0, C=4)
        conv0 = conv(conv(x, "conv0.0", 8), "conv0.1", 8)
        conv1 = conv(conv(ops.conv5x5_s2(conv0, *P["conv1.0"], 16, relu=True), "conv1.1", 16), "conv1.2", 16)
        conv2 = conv(conv(ops.conv5x5_s2(conv1, *P["conv2.0"], 32, relu=True), "conv2.1", 32), "conv2.2", 32)
        s1 = head(ops.conv1x1(conv2, *P["out1.0"], 32, relu=True), "out1", 32)
        intra = ops.fpn_lateral(conv2, conv1, *P["inner1"])
        s2 = head(conv(intra, "out2.0", 32), "out2", 16)
        intra = ops.fpn_lateral(intra, conv0, *P["inner2"])
        s3 = head(conv(intra, "out3.0", 32), "out3", 8)
        return s1, s2, s3

    def forward(self, x):
        if not self.uses_kernels(x):
            return self.forward_torch(x)
        return {k: t.permute(0, 3, 1, 2) for k, t in zip(("stage1", "stage2", "stage3"), self.forward_cl(x))}

    def forward_views(self, imgs):
        """imgs (B,NV,3,H,W) -> the per-view list of dicts FMT_with_pathway takes.  On the kernel route all NV B images run as one batch
        (view-major); otherwise view by view, as TransMVSNet.forward calls the module."""
        if imgs.dim() != 5 or imgs.shape[2] != 3:
            raise ValueError(f"diner_amd: DeviceFeatureNet.forward_views expects imgs (B,NV,3,H,W), got {tuple(imgs.shape)}")
        B, NV = int(imgs.shape[0]), int(imgs.shape[1])
        if not self.uses_kernels(imgs[:, 0]):
            return [self.forward(img) for img in torch.unbind(imgs, 1)]
        out = self.forward(imgs.detach().transpose(0, 1).reshape(NV * B, *imgs.shape[2:]))
        return [{k: t[v * B:(v + 1) * B] for k, t in out.items()} for v in range(NV)]


def depth_from_images(imgs, proj_matrices, depth_values, feature, fmt_with_pathway, depthnet, cost_regularization, **kwargs):
    """TransMVSNet.forward up to the stage outputs: imgs (B,NV,3,H,W), reference view first -> feature (a DeviceFeatureNet, or the
    reference's FeatureNet called view by view) -> fmt_with_pathway -> coarse_to_fine with its keywords (image_hw defaults to the images'
    size).  With the device modules and float32 HIP tensors under torch.no_grad() everything from the images to the depth maps runs on
    this library's kernels."""
    if imgs.dim() != 5:
        raise ValueError(f"diner_amd: depth_from_images expects imgs (B,NV,3,H,W), got {tuple(imgs.shape)}")
    if hasattr(feature, "forward_views"):
        features = feature.forward_views(imgs)
    else:
        features = [feature(img) for img in torch.unbind(imgs, 1)]
    features = fmt_with_pathway(features)
    kwargs.setdefault("image_hw", tuple(int(n) for n in imgs.shape[-2:]))
    return coarse_to_fine(features, proj_matrices, depth_values, depthnet, cost_regularization, **kwargs)


def to_device(model):
    """A loaded TransMVSNet -> the same model with model.DepthNet a DeviceDepthNet, model.cost_regularization a DeviceCostRegNet (one
    shared module, or a ModuleList of one per stage, as share_cr made it), model.FMT_with_pathway a DeviceFMTWithPathway and model.feature
    a DeviceFeatureNet, each carrying the original's state, device and training flag.  A model without FMT_with_pathway or without
    feature keeps what it has."""
    model.DepthNet = DeviceDepthNet.from_module(model.DepthNet)
    cr = model.cost_regularization
    if isinstance(cr, nn.ModuleList):
        model.cost_regularization = nn.ModuleList([DeviceCostRegNet.from_module(m) for m in cr])
    else:
        model.cost_regularization = DeviceCostRegNet.from_module(cr)
    if getattr(model, "FMT_with_pathway", None) is not None:
        model.FMT_with_pathway = DeviceFMTWithPathway.from_module(model.FMT_with_pathway)
    if getattr(model, "feature", None) is not None:
        model.feature = DeviceFeatureNet.from_module(model.feature)
    return model


# ---- bridges to the renderer's batches ------------------------------------------------------------------------------------------------
def proj_matrices_from_cameras(extrinsics, intrinsics, scales=STAGE_SCALES):
    """A batch's cameras, reference view first -- extrinsics (B,NV,4,4) world -> camera, intrinsics (B,NV,3,3) of the full image -- ->
    {"stage1": (B,NV,2,4,4), ...}: per view the pair (extrinsics, intrinsics in the top-left 3x3 of a zero 4x4) with the intrinsics' first
    two rows divided by the stage's scale (datasets/dtu_yao.py:170-200 states the same from the quarter-size camera upwards)."""
    if extrinsics.dim() != 4 or tuple(extrinsics.shape[2:]) != (4, 4) or tuple(intrinsics.shape) != tuple(extrinsics.shape[:2]) + (3, 3):
        raise ValueError(f"diner_amd: proj_matrices_from_cameras expects extrinsics (B,NV,4,4) and intrinsics (B,NV,3,3), got "
                         f"{tuple(extrinsics.shape)}, {tuple(intrinsics.shape)}")
    B, NV = extrinsics.shape[:2]
    out = {}
    for i, s in enumerate(scales):
        pair = torch.zeros(B, NV, 2, 4, 4, device=extrinsics.device, dtype=torch.float32)
        pair[:, :, 0] = extrinsics
        pair[:, :, 1, :3, :3] = intrinsics
        pair[:, :, 1, :2, :] = pair[:, :, 1, :2, :] / float(s)
        out[f"stage{i + 1}"] = pair
    return out


def to_source_maps(depth, confidence, law="dtu", dtu_rescale=False):
    """The estimator's depth and photometric confidence (..,H,W), on any device -> (src_depths, src_depth_stds) as the data sets deliver
    them after the PNG round trip, minus its 1e-4 quantisation: depth [/ (0.7 / 872) with dtu_rescale], std = formats.conf_to_std."""
    if law not in formats.CONF_TO_STD:
        raise ValueError(f"diner_amd: to_source_maps law must be one of {sorted(formats.CONF_TO_STD)}, got {law!r}")
    depth = depth.to(torch.float32)
    if dtu_rescale:
        depth = depth / np.float32(formats.DTU_DEPTH_RESCALE)
    return depth, formats.conf_to_std(confidence.to(torch.float32), law, depth=depth)
