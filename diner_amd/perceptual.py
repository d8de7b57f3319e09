"""The perceptual network on the device: the VGG convolution stack (csrc/conv2d.hip, csrc/perceptual.hip) behind the reference's LPIPS score
(eval_suite.py:52,75-77, lpips.LPIPS(net="vgg")) and its VGG loss (vggloss.py:59-69).

    lp = Lpips(lpips.LPIPS(net="vgg").state_dict())            # evaluate_folder(lpips_fn=lp), or --lpips_weights FILE
    vgg = VggLoss(torchvision.models.vgg19(pretrained=True).features)      # calc_losses(vgg_fn=vgg)

The weights are not part of this project and are never fetched: the caller hands over a torchvision-style feature stack or a state
dict.  Everything is fp32 on the HIP device, activations channels-last; the weights are frozen, so the loss needs the data gradient
alone, which is the same convolution kernel on a second packed weight set.  There is no CPU path."""
import collections
import re

import torch

# torchvision's feature indices: the 3 x 3 convolutions (each followed by a ReLU), the 2 x 2 max-pools in between, and the convolutions
# whose ReLU output is tapped -- vgg16 as lpips slices it (relu1_2, 2_2, 3_3, 4_3, 5_3), vgg19 up to relu4_1 as vggloss.py:25-32 does
ARCHS = {
    "vgg16": dict(convs=(0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), pools=(4, 9, 16, 23), taps=(2, 7, 14, 21, 28)),
    "vgg19": dict(convs=(0, 2, 5, 7, 10, 12, 14, 16, 19), pools=(4, 9, 18), taps=(0, 5, 10, 19)),
}
VGG_MEAN, VGG_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)              # vggloss.py:59-61
LPIPS_SHIFT, LPIPS_SCALE = (-.030, -.088, -.188), (.458, .448, .450)          # lpips.ScalingLayer
VGG_LOSS_WEIGHTS = (1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0)                          # vggloss.py:33
PIXELS_PER_PASS = 1 << 21        # Lpips: images of one pass through the stack (about 1 GiB per 64-channel activation of both sides)

# index: torchvision's feature index; w_fwd / w_bwd: ops.pack_conv3x3 of the weight and of its transpose; bias: zero-padded to the packed
# width; pool_before: a max-pool sits between the previous convolution and this one; tap: this convolution's ReLU output is a tap
Layer = collections.namedtuple("Layer", "index Cin Cout w_fwd bias w_bwd pool_before tap")
_CONV_KEY = re.compile(r"(?:^|\.)(\d+)\.(weight|bias)$")
_LIN_KEY = re.compile(r"(?:^|\.)lin(\d+)\.model\.1\.weight$")
_LIN_ANY = re.compile(r"(?:^|\.)lins?[.\d]")


def _conv_tensors(state, arch):
    """{feature index: (weight, bias)} of the convolutions `arch` needs, from a feature stack or a state-dict-like mapping."""
    spec = ARCHS[arch]
    if isinstance(state, torch.nn.Module):
        mods = list(state)
        out = {}
        for i in spec["convs"]:
            m = mods[i] if i < len(mods) else None
            if not isinstance(m, torch.nn.Conv2d):
                raise ValueError(f"diner_amd.perceptual: {arch} needs a Conv2d at feature index {i}, the stack has "
                                 f"{type(m).__name__ if m is not None else 'nothing'} there")
            if tuple(m.kernel_size) != (3, 3) or tuple(m.stride) != (1, 1) or m.padding not in ((1, 1), 1) or tuple(m.dilation) != (1, 1) \
                    or m.groups != 1 or m.bias is None or m.padding_mode != "zeros":
                raise ValueError(f"diner_amd.perceptual: feature index {i} must be a 3 x 3 convolution with stride 1, zero padding 1 and a bias")
            out[i] = (m.weight, m.bias)
        for i in spec["pools"]:
            m = mods[i] if i < len(mods) else None
            if not isinstance(m, torch.nn.MaxPool2d) or m.kernel_size not in (2, (2, 2)) or m.stride not in (2, (2, 2)) \
                    or m.padding not in (0, (0, 0)) or m.ceil_mode:
                raise ValueError(f"diner_amd.perceptual: {arch} needs a MaxPool2d(2, 2) at feature index {i}")
        return out
    if not hasattr(state, "items"):
        raise ValueError(f"diner_amd.perceptual: expected a feature stack (nn.Sequential) or a state-dict-like mapping, got {type(state).__name__}")
    found = {}
    for key, t in state.items():
        m = _CONV_KEY.search(key)
        if m is None or _LIN_ANY.search(key) or int(m.group(1)) not in spec["convs"]:
            continue
        found.setdefault(int(m.group(1)), {}).setdefault(m.group(2), t)
    out = {}
    for i in spec["convs"]:
        if i not in found or "weight" not in found[i] or "bias" not in found[i]:
            raise ValueError(f"diner_amd.perceptual: {arch} needs keys ending in '{i}.weight' and '{i}.bias' (a convolution is missing)")
        out[i] = (found[i]["weight"], found[i]["bias"])
    return out


def load_layers(state, arch):
    """Validate `state` (see VggFeatures) for `arch` and pack both weight sets: -> [Layer] on the CPU.  Channel widths are read from the
    tensors.  Needs no device."""
    from . import ops
    if arch not in ARCHS:
        raise ValueError(f"diner_amd.perceptual: arch must be one of {sorted(ARCHS)}, got {arch!r}")
    spec = ARCHS[arch]
    tensors = _conv_tensors(state, arch)
    layers, prev, width = [], None, 3
    for i in spec["convs"]:
        w, b = (torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous() for t in tensors[i])
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] != width or b.dim() != 1 or b.shape[0] != w.shape[0]:
            raise ValueError(f"diner_amd.perceptual: feature index {i}: expected weight (Cout,{width},3,3) and bias (Cout,), got "
                             f"{tuple(w.shape)} and {tuple(b.shape)}")
        Cout = int(w.shape[0])
        w_fwd = ops.pack_conv3x3(w)
        bias = torch.zeros(w_fwd.shape[3], dtype=torch.float32)
        bias[:Cout] = b
        layers.append(Layer(i, width, Cout, w_fwd, bias, ops.pack_conv3x3(w, transpose=True),
                            prev is not None and any(prev < p < i for p in spec["pools"]), i in spec["taps"]))
        prev, width = i, Cout
    return layers


def load_lins(state, layers):
    """The five lin{k}.model.1.weight tensors (1,C,1,1) of an lpips state dict as (C,) float32 CPU tensors, checked against the taps."""
    if not hasattr(state, "items"):
        raise ValueError("diner_amd.perceptual: Lpips needs a state-dict-like mapping that holds the lin{k}.model.1.weight tensors")
    found = {}
    for key, t in state.items():
        m = _LIN_KEY.search(key)
        if m is not None:
            found.setdefault(int(m.group(1)), t)
    taps = [L for L in layers if L.tap]
    lins = []
    for k, L in enumerate(taps):
        if k not in found:
            raise ValueError(f"diner_amd.perceptual: Lpips needs a key ending in 'lin{k}.model.1.weight'")
        t = torch.as_tensor(found[k]).detach().to("cpu", torch.float32)
        if tuple(t.shape) != (1, L.Cout, 1, 1):
            raise ValueError(f"diner_amd.perceptual: lin{k}.model.1.weight must be (1,{L.Cout},1,1), the width of tap {k}, got {tuple(t.shape)}")
        lins.append(t.reshape(-1).contiguous())
    return lins


def _hip_device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("diner_amd.perceptual: no HIP device; the network runs on the device and there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"diner_amd.perceptual: device {device} is not a HIP device; there is no CPU fallback")
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _check_pair(who, x, y, min_hw):
    """(N,3,H,W) float32 tensors of one shape with H, W >= min_hw, on a HIP device."""
    for name, t in (("first", x), ("second", y)):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
            raise ValueError(f"diner_amd.perceptual: {who} expects (N,3,H,W) tensors, the {name} is "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"diner_amd.perceptual: {who} expects float32, the {name} argument is {t.dtype}")
    if x.shape != y.shape:
        raise ValueError(f"diner_amd.perceptual: {who} expects two tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[2] < min_hw or x.shape[3] < min_hw:
        raise ValueError(f"diner_amd.perceptual: {who} needs H, W >= {min_hw} (the stack halves the size {min_hw.bit_length() - 1} times), got "
                         f"{tuple(x.shape[2:])}")
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError(f"diner_amd.perceptual: {who} expects tensors on the HIP device; there is no CPU fallback")


class VggFeatures:
    """The convolution stack of `arch` ("vgg16": taps after relu1_2, 2_2, 3_3, 4_3, 5_3; "vgg19": taps after relu1_1, 2_1, 3_1, 4_1) with
    both packed weight sets on the HIP device `device` (None: the current one).  `state` is a torchvision-style feature stack (an
    nn.Sequential with Conv2d modules at the usual indices) or a state-dict-like mapping whose keys end in `<N>.weight` / `<N>.bias` with
    torchvision's feature index N (`features.N.*`, or the lpips package's `net.sliceK.N.*`).  Channel widths are read from the tensors."""

    def __init__(self, state, arch, device=None):
        layers = load_layers(state, arch)
        self.arch = arch
        self.device = _hip_device(device)
        self.layers = [L._replace(w_fwd=L.w_fwd.to(self.device), bias=L.bias.to(self.device), w_bwd=L.w_bwd.to(self.device)) for L in layers]
        self.min_size = 2 ** len(ARCHS[arch]["pools"])
        self.tap_widths = [L.Cout for L in self.layers if L.tap]

    def forward(self, z, on_tap, keep=False):
        """z: the channels-last input of ops.image_in (M,H,W,4).  Calls on_tap(k, layer number, activation) at the k-th tap; -> the ReLU
        output of every convolution if keep, else None."""
        from . import ops
        acts, k = [], 0
        for j, L in enumerate(self.layers):
            if L.pool_before:
                z = ops.maxpool2(z)
            z = ops.conv3x3(z, L.w_fwd, L.bias, L.Cout, relu=True)
            if keep:
                acts.append(z)
            if L.tap:
                on_tap(k, j, z)
                k += 1
        return acts if keep else None


class Lpips:
    """lpips.LPIPS(net="vgg") on the device: VggFeatures("vgg16") plus the five lin{k}.model.1.weight tensors (1,C,1,1) of the same
    mapping.  __call__(pred, gt): (N,3,H,W) float32 device tensors in [-1, 1] -> (N,1,1,1), the shape lpips.LPIPS returns, so it fits
    evaluate_folder(lpips_fn=...).  Enqueue-only, no gradient; H, W >= 16.  An image's score does not depend on the batch around it."""

    def __init__(self, state, device=None):
        self.features = VggFeatures(state, "vgg16", device)
        self.lins = [t.to(self.features.device) for t in load_lins(state, self.features.layers)]

    @torch.no_grad()
    def __call__(self, pred, gt):
        from . import ops
        _check_pair("Lpips", pred, gt, self.features.min_size)
        N, _, H, W = pred.shape
        step = max(1, PIXELS_PER_PASS // (H * W))
        outs = []
        with torch.cuda.device(pred.device):
            for a in range(0, N, step):
                n = min(step, N - a)
                z = ops.image_in(torch.cat([pred[a:a + n], gt[a:a + n]]), LPIPS_SHIFT, LPIPS_SCALE)
                acc = []

                def on_tap(k, j, f):
                    acc[:] = [ops.lpips_layer(f[:n], f[n:], self.lins[k], out=acc[0] if acc else None)]

                self.features.forward(z, on_tap)
                outs.append(acc[0])
        return torch.cat(outs).to(torch.float32).view(N, 1, 1, 1)


class _VggLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, features):
        from . import ops
        N = x.shape[0]
        need = ctx.needs_input_grad[0]
        layers = features.layers
        last = max(j for j, L in enumerate(layers) if L.tap)
        planes, terms = {}, []

        def on_tap(k, j, f):
            mean, planes[j] = ops.feature_l1(f[:N], f[N:], weight=VGG_LOSS_WEIGHTS[k], want_grad=need, mask_by_fx=j == last)
            terms.append(mean * VGG_LOSS_WEIGHTS[k])

        with torch.cuda.device(x.device):
            z = ops.image_in(torch.cat([x.detach(), y.detach()]), VGG_MEAN, VGG_STD)
            acts = features.forward(z, on_tap, keep=need)
            loss = terms[0]
            for t in terms[1:]:
                loss = loss + t
        if need:
            ctx.features, ctx.acts, ctx.planes, ctx.N, ctx.last = features, acts, planes, N, last
        return loss.to(torch.float32).reshape(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        from . import ops
        layers, acts, planes, N = ctx.features.layers, ctx.acts, ctx.planes, ctx.N
        with torch.cuda.device(go.device):
            g = planes[ctx.last]                     # already masked by the last tap's own ReLU
            for j in range(ctx.last, 0, -1):
                L = layers[j]
                below = acts[j - 1][:N]              # the x half of the activation this convolution (or its pool) read
                if L.pool_before:
                    g = ops.conv3x3(g, L.w_bwd, None, L.Cin)
                    g = ops.maxpool2_bwd(below, g, addend=planes.get(j - 1), relu_mask=True)
                else:
                    g = ops.conv3x3(g, L.w_bwd, None, L.Cin, addend=planes.get(j - 1), mask=below)
            g = ops.conv3x3(g, layers[0].w_bwd, None, 3)
            gx = ops.image_in_bwd(g, VGG_STD) * go
        return gx, None, None


class VggLoss(torch.nn.Module):
    """The reference's VGGLoss.forward (vggloss.py:59-69) on the device: VggFeatures("vgg19"), L1 mean per tap with the weights 1/16, 1/8,
    1/4, 1, y detached.  forward(x, y): (N,3,H,W) float32 device tensors, H, W >= 8 -> a scalar that is differentiable in x through one
    autograd.Function, so it works as calc_losses(vgg_fn=...).  x and y go through the stack as one batch of 2 N images; the backward walks
    only the x half."""

    def __init__(self, state, device=None):
        super().__init__()
        self.features = VggFeatures(state, "vgg19", device)

    def forward(self, x, y):
        _check_pair("VggLoss", x, y, self.features.min_size)
        return _VggLossFn.apply(x, y.detach(), self.features)
