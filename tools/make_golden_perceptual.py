"""Fixture G26 (tests/golden/g26_perceptual.npz): LPIPS and the VGG loss on seeded weights, restated in float64 torch.

    python tools/make_golden_perceptual.py            # rewrites the fixture

The two quantities are written out here from their definitions -- lpips.LPIPS(net="vgg") (scaling layer, VGG-16 taps after relu1_2,
2_2, 3_3, 4_3, 5_3, unit-normalise over channels, squared difference, 1 x 1 `lin` convolution, spatial mean, sum over the taps) and the
reference's VGGLoss.forward (vggloss.py:59-69: ImageNet normalisation, VGG-19 taps after relu1_1, 2_1, 3_1, 4_1, L1 mean per tap with the
weights 1/16, 1/8, 1/4, 1) -- as plain functional torch, so that tests/test_perceptual_gpu.py can evaluate them in float64 on the CPU at
run time.  Nothing is read from outside this repository.  The fixture holds the small inputs of the narrow cases, the float64 results,
the distance of torch's own float32 CPU evaluation from them (the yardstick DESIGN.md 8j quotes) and a float64 checksum of the seeded
weights (diner_amd.synthetic.make_vgg_state_dict) instead of the weights."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# torchvision's feature indices, written out again (diner_amd.perceptual.ARCHS is the code under test)
CONVS = {"vgg16": (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28), "vgg19": (0, 2, 5, 7, 10, 12, 14, 16, 19)}
POOLS = {"vgg16": (4, 9, 16, 23), "vgg19": (4, 9, 18)}
TAPS = {"vgg16": (3, 8, 15, 22, 29), "vgg19": (1, 6, 11, 20)}          # the ReLU modules whose output is tapped
SEEDS = {"vgg16": 16, "vgg19": 19}
NARROW = 8                                                              # width_div of the narrow stacks
# (arch, width_div, N, H, W, input seed)
LPIPS_CASES = (("vgg16", NARROW, 2, 37, 45, 101), ("vgg16", 1, 2, 33, 47, 102))
# The gradient of the loss is piecewise constant in the signs of the tap differences, the ReLU masks and the pools' choices: inputs on
# which a float64 value sits within float32 rounding of such a switch cannot tell two float32 evaluations apart (seed 203 at full width
# is one: torch's own float32 gradient is 7.6e-3 off there).  The seeds below are well away from one; the GPU test asserts that.
LOSS_CASES = (("vgg19", NARROW, 2, 37, 45, 201), ("vgg19", NARROW, 2, 32, 32, 202), ("vgg19", 1, 2, 37, 45, 205), ("vgg19", 1, 2, 32, 32, 204))


def sequential_from(sd, arch):
    """A torchvision-style feature stack (Conv2d / ReLU / MaxPool2d at the usual indices) holding the weights of `sd`."""
    mods = []
    for i in range(TAPS[arch][-1] + 1):
        if i in CONVS[arch]:
            w = sd[f"features.{i}.weight"]
            m = torch.nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
            with torch.no_grad():
                m.weight.copy_(w)
                m.bias.copy_(sd[f"features.{i}.bias"])
        elif i in POOLS[arch]:
            m = torch.nn.MaxPool2d(2, 2)
        else:
            m = torch.nn.ReLU()
        mods.append(m)
    return torch.nn.Sequential(*mods)


def taps(sd, arch, z):
    """The tapped activations of the stack on the normalised input z (N,3,H,W), in z's dtype."""
    out = []
    for i in range(TAPS[arch][-1] + 1):
        if i in CONVS[arch]:
            z = F.conv2d(z, sd[f"features.{i}.weight"].to(z.dtype), sd[f"features.{i}.bias"].to(z.dtype), padding=1)
        elif i in POOLS[arch]:
            z = F.max_pool2d(z, 2, 2)
        else:
            z = F.relu(z)
        if i in TAPS[arch]:
            out.append(z)
    return out


def lpips_restated(sd, pred, gt, dtype=torch.float64):
    """lpips.LPIPS(net="vgg")(pred, gt) for inputs in [-1, 1] -> (N,) in `dtype`."""
    shift = torch.tensor([-.030, -.088, -.188], dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=dtype).view(1, 3, 1, 1)
    fx = taps(sd, "vgg16", (pred.to(dtype) - shift) / scale)
    fy = taps(sd, "vgg16", (gt.to(dtype) - shift) / scale)
    total = 0
    for k, (a, b) in enumerate(zip(fx, fy)):
        a = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
        b = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
        lin = sd[f"lin{k}.model.1.weight"].to(dtype)
        total = total + F.conv2d((a - b) ** 2, lin).mean(dim=(2, 3)).view(-1)
    return total


def vgg_loss_restated(sd, x, y, dtype=torch.float64):
    """The reference's VGGLoss.forward(x, y) and its gradient with respect to x -> (loss, grad) in `dtype`."""
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=dtype).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=dtype).view(1, 3, 1, 1)
    x = x.detach().to(dtype).requires_grad_(True)
    fx = taps(sd, "vgg19", (x - mean) / std)
    with torch.no_grad():
        fy = taps(sd, "vgg19", (y.to(dtype) - mean) / std)
    loss = 0
    for w, a, b in zip((1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0), fx, fy):
        loss = loss + w * (a - b).abs().mean()
    grad, = torch.autograd.grad(loss, x)
    return loss.detach(), grad


def weights_checksum(sd):
    """float64 [sum, sum of absolute values] over all tensors, keys sorted."""
    s = [0.0, 0.0]
    for k in sorted(sd):
        t = sd[k].double()
        s[0] += float(t.sum())
        s[1] += float(t.abs().sum())
    return np.array(s, dtype=np.float64)


def lpips_inputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(N, 3, H, W, generator=g) * 2 - 1
    gt = (pred + 0.3 * torch.randn(N, 3, H, W, generator=g)).clamp(-1, 1)
    return pred, gt


def loss_inputs(N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, H, W, generator=g)
    y = (x + 0.2 * torch.randn(N, 3, H, W, generator=g)).clamp(0, 1)
    return x, y


def state_dict(arch, width_div):
    from diner_amd.synthetic import make_vgg_state_dict
    return make_vgg_state_dict(arch, SEEDS[arch], width_div=width_div, with_lins=arch == "vgg16")


def main():
    out = {}
    for arch in ("vgg16", "vgg19"):
        for div in (NARROW, 1):
            out[f"checksum_{arch}_div{div}"] = weights_checksum(state_dict(arch, div))
    for c, (arch, div, N, H, W, seed) in enumerate(LPIPS_CASES):
        sd = state_dict(arch, div)
        pred, gt = lpips_inputs(N, H, W, seed)
        s64 = lpips_restated(sd, pred, gt)
        s32 = lpips_restated(sd, pred, gt, torch.float32)
        out[f"lpips{c}_score64"] = s64.numpy()
        out[f"lpips{c}_f32_rel"] = ((s32.double() - s64).abs() / s64.abs()).numpy()
        if div != 1:
            out[f"lpips{c}_pred"], out[f"lpips{c}_gt"] = pred.numpy(), gt.numpy()
        print(f"lpips case {c} {arch} / {div} {N}x3x{H}x{W}: {s64.tolist()}, float32 torch rel {out[f'lpips{c}_f32_rel'].tolist()}")
    for c, (arch, div, N, H, W, seed) in enumerate(LOSS_CASES):
        sd = state_dict(arch, div)
        x, y = loss_inputs(N, H, W, seed)
        l64, g64 = vgg_loss_restated(sd, x, y)
        l32, g32 = vgg_loss_restated(sd, x, y, torch.float32)
        out[f"loss{c}_loss64"] = np.float64(l64)
        out[f"loss{c}_f32_rel"] = np.float64(abs(float(l32) - float(l64)) / abs(float(l64)))
        out[f"loss{c}_grad_f32_rel"] = np.float64((g32.double() - g64).norm() / g64.norm())
        if div != 1:
            out[f"loss{c}_x"], out[f"loss{c}_y"], out[f"loss{c}_grad64"] = x.numpy(), y.numpy(), g64.numpy()
        print(f"vgg loss case {c} {arch} / {div} {N}x3x{H}x{W}: {float(l64):.12g}, float32 torch rel {float(out[f'loss{c}_f32_rel']):.2e}, "
              f"gradient {float(out[f'loss{c}_grad_f32_rel']):.2e}")
    path = os.path.join(ROOT, "tests", "golden", "g26_perceptual.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
