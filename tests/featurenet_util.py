"""Shared by tools/make_golden_featurenet.py, tests/test_featurenet_cpu.py and tests/test_featurenet_gpu.py: the seeded weights and images
of fixture G31 (regenerated, never stored), the case table, an independent restatement of the deformable convolution on grid_sample and the
float64 restatements of the single kernels.

Weights keep the reference's own initialisation -- torch's Conv2d default, U(+- 1 / sqrt(fan-in)), which is also DCNv2.reset_parameters'
law for the deformable weights -- except that
  * BatchNorm's running statistics and affine terms are random (gamma in [0.5, 1.5], beta 0.3 N(0,1), mean 0.2 N(0,1), variance in
    [0.1, 0.3]: the variance a default-initialised convolution of a unit-scale input actually leaves, so that the signal neither dies nor
    grows through the fourteen layers and a late layer still sees a map that varies from pixel to pixel);
  * every bias is 0.2 N(0,1);
  * conv_offset_mask is NOT zero, as the reference initialises it (which would test a plain convolution): its weights are
    OFFSET_WEIGHT_STD N(0,1), which leaves offsets with a standard deviation of about 1.5 px (the generator prints and asserts it) and
    modulation logits of the same spread.
Images: per case a smooth random texture plus noise, in [0, 1] like a loaded image."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests import mvs_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g31_featurenet.npz")
BAR_FACTOR, GAP_FACTOR = MU.BAR_FACTOR, MU.GAP_FACTOR
STAGES = ("stage1", "stage2", "stage3")
STAGE_CHANNELS = {"stage1": 32, "stage2": 16, "stage3": 8}
HEADS = ("out1", "out2", "out3")
DCN_LAYERS = tuple(f"{h}.{i}" for h in HEADS for i in (1, 4, 7))
OFFSET_WEIGHT_STD = 0.12

# name: B, NV, image (H, W), seed -- the smallest images at which each thing can go wrong
CASES = {
    "tiny": dict(B=1, NV=1, hw=(16, 24), seed=3101),        # every level (4 x 6, 8 x 12, 16 x 24) is a single partial tile of every kernel
    "ragged": dict(B=2, NV=2, hw=(36, 52), seed=3102),      # ragged at all three levels: 9 x 13, 18 x 26, 36 x 52; two batch elements, two views
    "tiles": dict(B=1, NV=1, hw=(80, 112), seed=3103),      # several tiles a level: 20 x 28 = 560 pixels at stage 1, 8960 at stage 3
}
STAGE_RUN_SEED = 3111               # the three-stage scene on mvs_util.stage_inputs()' cameras: B 2, four views, a 24 x 40 image


def featurenet_state_dict(seed, base=8):
    """A seeded state dict of FeatureNet(base) under the reference's keys."""
    from diner_amd import mvs
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, p in mvs.DeviceFeatureNet(base).state_dict().items():
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.tensor(100)
        elif "conv_offset_mask.weight" in key:
            sd[key] = OFFSET_WEIGHT_STD * torch.randn(p.shape, generator=g)
        elif p.dim() == 4:
            bound = float(1.0 / np.sqrt(p.shape[1] * p.shape[2] * p.shape[3]))
            sd[key] = (torch.rand(p.shape, generator=g) * 2 - 1) * bound
        elif key.endswith("running_var"):
            sd[key] = 0.1 + 0.2 * torch.rand(p.shape, generator=g)
        elif key.endswith("running_mean"):
            sd[key] = 0.2 * torch.randn(p.shape, generator=g)
        elif key.endswith("bn.weight") or (key.split(".")[-2].isdigit() and key.split(".")[0].startswith("out") and key.endswith(".weight")):
            sd[key] = 0.5 + torch.rand(p.shape, generator=g)                # BatchNorm's gamma, in a Conv2d block or bare in a head
        elif key.endswith("bn.bias") or (key.split(".")[-2] in ("2", "5") and key.split(".")[0].startswith("out")):
            sd[key] = 0.3 * torch.randn(p.shape, generator=g)                # BatchNorm's beta
        else:
            sd[key] = 0.2 * torch.randn(p.shape, generator=g)                # a convolution's bias
    return sd


def texture(g, n, hw):
    """n images (n,3,H,W) in [0, 1]: a coarse random field upsampled smoothly, plus pixel noise."""
    H, W = hw
    coarse = torch.rand(n, 3, max(2, H // 6), max(2, W // 6), generator=g)
    img = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True) + 0.08 * torch.randn(n, 3, H, W, generator=g)
    return img.clamp(0.0, 1.0).contiguous()


def case_images(name):
    """-> (B,NV,3,H,W) float32."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    return texture(g, c["B"] * c["NV"], c["hw"]).view(c["B"], c["NV"], 3, *c["hw"])


def make_module(name_or_seed, dtype=torch.float32):
    """The DeviceFeatureNet of a case (or of a seed), in eval mode, on the CPU."""
    from diner_amd import mvs
    seed = CASES[name_or_seed]["seed"] + 50 if isinstance(name_or_seed, str) else name_or_seed
    net = mvs.DeviceFeatureNet(8)
    net.load_state_dict(featurenet_state_dict(seed))
    return net.to(dtype).eval()


def run_case(net, imgs):
    """The module on (B,NV,3,H,W) -> {stage: (NV,B,C,h,w) contiguous on the CPU}."""
    with torch.no_grad():
        views = net.forward_views(imgs)
    return {k: torch.stack([v[k].detach().cpu().contiguous() for v in views], 0) for k in STAGES}


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    """The torch route of a case on the CPU in `dtype`, computed once per session and shared; treat it as read-only."""
    return run_case(make_module(name, dtype), case_images(name).to(dtype))


def expected64(name):
    return expected(name, torch.float64)


def expected32(name):
    return expected(name, torch.float32)


def subsample(t):
    return MU.subsample(t)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


# ---- the three-stage run from images ------------------------------------------------------------------------------------------------------
def stage_run_images():
    """mvs_util's three-stage cameras looking at its textured plane, three of its sine channels as the colours -> (B,NV,3,H,W) in [0, 1]."""
    s, inp = MU.STAGES, MU.stage_inputs()
    rng = np.random.default_rng(STAGE_RUN_SEED)
    f = MU.plane_features(inp["extrinsics"], inp["intrinsics"], s["image"], 3, rng)         # (NV,B,3,H,W) in [-1, 1]
    return torch.from_numpy(0.5 + 0.5 * f).to(torch.float32).transpose(0, 1).contiguous()


def stage_run_modules(dtype, device=None):
    from diner_amd import mvs
    from tests import fmt_util as FU
    inp = MU.stage_inputs()
    feature, fmt = make_module(STAGE_RUN_SEED, dtype), FU.make_module(STAGE_RUN_SEED + 1, dtype)
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(inp["state_dict"])
    dn = dn.to(dtype).eval()
    if device is not None:
        feature, fmt, dn = feature.to(device), fmt.to(device), dn.to(device)
    return feature, fmt, dn


def stage_run(dtype, device=None):
    """mvs.depth_from_images on the three-stage scene -> coarse_to_fine's outputs.  On the CPU the torch routes; on a HIP device (under
    torch.no_grad(), in eval mode) the kernels from the images to the depth maps."""
    from diner_amd import mvs
    s, inp = MU.STAGES, MU.stage_inputs()
    feature, fmt, dn = stage_run_modules(dtype, device)
    x = MU.cast({"imgs": stage_run_images(), "proj": inp["proj"], "depth_values": inp["depth_values"]}, dtype, device)
    with torch.no_grad():
        return mvs.depth_from_images(x["imgs"], x["proj"], x["depth_values"], feature, fmt, dn, MU.regulariser, ndepths=s["ndepths"],
                                     ratios=s["ratios"], depth_interval=s["depth_interval"], scales=s["scales"])


@functools.lru_cache(maxsize=None)
def stage_run_expected(dtype):
    return stage_run(dtype)


# ---- restatements ---------------------------------------------------------------------------------------------------------------------------
def deform_conv2d_grid(x, offset, weight, bias=None, mask=None):
    """The 3 x 3, stride 1, padding 1 deformable convolution stated on F.grid_sample(bilinear, zeros, align_corners=True), which shares no
    code with mvs.deform_conv2d_torch: with align_corners=True a grid value g maps to the pixel coordinate (g + 1) / 2 (size - 1), and a
    corner outside the image contributes zero -- torchvision's rule, including its "fully outside" cases, since beyond (-1, size) every
    corner is outside.  x (B,C,H,W), offset (B,18,H,W), mask (B,9,H,W) -> (B,Cout,H,W).  (Needs H, W >= 2 and finite offsets.)"""
    B, C, H, W = x.shape
    ys = torch.arange(H, dtype=x.dtype).view(1, H, 1)
    xs = torch.arange(W, dtype=x.dtype).view(1, 1, W)
    out = 0
    for k in range(9):
        ky, kx = divmod(k, 3)
        py, px = ys + (ky - 1) + offset[:, 2 * k], xs + (kx - 1) + offset[:, 2 * k + 1]
        grid = torch.stack([px / (W - 1) * 2 - 1, py / (H - 1) * 2 - 1], -1)
        s = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        if mask is not None:
            s = s * mask[:, k:k + 1]
        out = out + torch.einsum("oc,bchw->bohw", weight[:, :, ky, kx], s)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


def deform_restated(x_cl, offmask_cl, weight, bias, relu):
    """diner_deform_conv3x3_f32's formula on channels-last tensors, in their dtype, through mvs.deform_conv2d_torch."""
    from diner_amd import mvs
    om = offmask_cl.permute(0, 3, 1, 2)
    y = mvs.deform_conv2d_torch(x_cl.permute(0, 3, 1, 2), om[:, :18], weight, bias, 1, 1, 1, mask=torch.sigmoid(om[:, 18:]))
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()


def conv_restated(x_cl, weight, bias, stride, padding, relu):
    y = F.conv2d(x_cl.permute(0, 3, 1, 2), weight, bias, stride=stride, padding=padding)
    return (F.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()


def lateral_restated(top_cl, lat_cl, weight, bias):
    """nearest2x(top) + conv1x1(lateral) on channels-last tensors."""
    up = F.interpolate(top_cl.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return (up + F.conv2d(lat_cl.permute(0, 3, 1, 2), weight, bias)).permute(0, 2, 3, 1).contiguous()


def dcn_inputs(net, imgs):
    """The inputs of the nine deformable layers on a batch of images (N,3,H,W), by forward hooks -> {layer: (x, raw conv_offset_mask(x))}."""
    got, hooks = {}, []
    for name in DCN_LAYERS:
        mod = net.get_submodule(name)
        hooks.append(mod.register_forward_hook(lambda m, inp, out, name=name: got.__setitem__(name, (inp[0].detach(), m.conv_offset_mask(inp[0]).detach()))))
    with torch.no_grad():
        net.forward_torch(imgs)
    for h in hooks:
        h.remove()
    return got


def sample_coverage(offmask, H, W):
    """The raw conv_offset_mask output (N,27,H,W) -> counts of the samples that lie fully outside on each of the four sides, that have
    exactly one corner row or column missing, and that lie inside with a fractional part."""
    ys = torch.arange(H, dtype=offmask.dtype).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=offmask.dtype).view(1, 1, 1, W)
    k = torch.arange(9)
    py = ys + (k // 3 - 1).view(1, 9, 1, 1).to(offmask.dtype) + offmask[:, 0:18:2]
    px = xs + (k % 3 - 1).view(1, 9, 1, 1).to(offmask.dtype) + offmask[:, 1:18:2]
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    frac = (py != py.floor()) & (px != px.floor())
    return dict(above=int((py <= -1).sum()), below=int((py >= H).sum()), left=int((px <= -1).sum()), right=int((px >= W).sum()),
                row_missing=int((inside & ((py < 0) | (py > H - 1)) & (px >= 0) & (px <= W - 1)).sum()),
                col_missing=int((inside & ((px < 0) | (px > W - 1)) & (py >= 0) & (py <= H - 1)).sum()),
                interior=int((inside & frac & (py > 0) & (py < H - 1) & (px > 0) & (px < W - 1)).sum()))
