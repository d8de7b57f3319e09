"""Time FeatureNet's modulated deformable convolutions in training -- forward and backward -- on the kernels (csrc/deform.hip:
diner_deform_conv3x3_f32; csrc/deform_grad.hip: diner_deform_conv3x3_grad_f32) and on the torch route that training ran before
(mvs.deform_conv2d_torch under autograd), on the same device.

    python tools/time_deform_train.py                    # three layer shapes, FeatureNet on five views, one fit step at 256 x 320
    python tools/time_deform_train.py --calls 5 --skip-fit

In one process.  Per layer shape -- (5,32,64,80), (5,32,128,160), (5,32,256,320), with Cout 32 and with the head's last Cout (32, 16, 8)
-- one DCN's deformable convolution forward + backward under a fixed upstream gradient, mvs.deform_conv3x3 against mvs.deform_conv2d_torch,
with HIP events, 3 warm-up calls a route, then torch / kernels / torch / kernels ... alternating, the median with min - max, the torch
route's two halves against each other (A/A), and torch.cuda.max_memory_allocated of one call of each route above what was allocated
before.  Then the gradient entry alone (the median of `calls` back-to-back calls after 3 warm-up calls, not alternating): all four
outputs, and d_x, d_offmask and d_weight + d_bias each alone, beside the float-atomic bound of d_x (N H W x 9 taps x 4 corners x Cin
floats at 1.3 TB/s, an upper bound: every corner of every tap) and the fp32 matrix peak (2 N H W 9 Cin Cout flops for G, as many for
d_weight, at 157.3 TFLOPS).  Then DeviceFeatureNet forward + backward in training mode on five 256 x 320 views (one batch), the switch
off against on.  Then one fine-tuning step of DeviceTransMVSNet (forward in training mode, focal_loss_bld, backward, DeviceAdam;
fused_readout and match_kernels on in both) with and without deform_kernels, alternating.  Inputs are seeded noise; needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import estimator, mvs, ops                                      # noqa: E402
from tools.time_mvs import NS, alternate, cameras, fmt, peak_of, report, timed      # noqa: E402

ATOMIC_RATE = 1.3e12               # bytes/s of float atomic adds, chip-wide
MATRIX_PEAK = 157.3e12             # fp32 MFMA flops/s
LAYERS = (((5, 32, 64, 80), 32), ((5, 32, 128, 160), 32), ((5, 32, 128, 160), 16), ((5, 32, 256, 320), 32), ((5, 32, 256, 320), 8))


def layer(shape, Cout, calls, dev, g):
    N, Cin, H, W = shape
    x = torch.randn(N, H, W, Cin, generator=g).to(dev).permute(0, 3, 1, 2).requires_grad_(True)          # channels-last memory, as the net hands it
    om = torch.cat((1.5 * torch.randn(N, H, W, 18, generator=g), torch.randn(N, H, W, 9, generator=g)), 3).to(dev).permute(0, 3, 1, 2).requires_grad_(True)
    w = ((torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) / (9 * Cin) ** 0.5).to(dev).requires_grad_(True)
    b = torch.zeros(Cout, device=dev, requires_grad=True)
    up = torch.randn(N, H, W, Cout, generator=g).to(dev).permute(0, 3, 1, 2)

    def run(fn):
        for t in (x, om, w, b):
            t.grad = None
        fn(x, om, w, b).backward(up)

    print(f"layer {shape} -> Cout {Cout}", flush=True)
    report("deformable conv fwd + bwd", lambda: run(mvs.deform_conv3x3), lambda: run(mvs._deform_torch), calls)
    x_cl, om_cl, dy_cl = (t.detach().permute(0, 2, 3, 1).contiguous() for t in (x, om, up))
    wd = w.detach().contiguous()
    med = lambda fn: statistics.median(([fn() for _ in range(3)], timed(fn, calls))[1])
    nbytes = N * H * W * 9 * 4 * Cin * 4
    flops = 2 * N * H * W * 9 * Cin * Cout
    print(f"    the gradient entry alone, medians of {calls} back-to-back calls; d_x adds at most {nbytes / 1e9:.3f} GB: {nbytes / ATOMIC_RATE * 1e3:.3f} ms at "
          f"{ATOMIC_RATE / 1e12:.1f} TB/s; G and d_weight are {flops / 1e9:.2f} GFLOP each: {flops / MATRIX_PEAK * 1e3:.4f} ms at the fp32 matrix peak", flush=True)
    for label, want in (("all four outputs", (True, True, True, True)), ("d_x alone (G + scatter)", (True, False, False, False)),
                        ("d_offmask alone (G + dot products)", (False, True, False, False)), ("d_x + d_offmask (the data kernel)", (True, True, False, False)),
                        ("d_weight + d_bias (the weight kernel)", (False, False, True, True))):
        ms = med(lambda: ops.deform_conv3x3_grad(x_cl, om_cl, wd, dy_cl, want=want))
        line = f"    {label:40s} {ms:8.3f} ms"
        if want[0]:
            line += f"  {100 * nbytes / ATOMIC_RATE * 1e3 / ms:5.1f} % of the atomic bound"
        n_mm = (1 if want[0] or want[1] else 0) + (1 if want[2] else 0)
        line += f"  matrix part {100 * n_mm * flops / MATRIX_PEAK * 1e3 / ms:5.2f} % of the fp32 matrix peak's time"
        print(line, flush=True)
    ms = med(lambda: ops.deform_conv3x3(x_cl, om_cl, ops.pack_deform_conv3x3(wd), None, Cout))
    print(f"    {'forward kernel (with the weight packing)':40s} {ms:8.3f} ms", flush=True)


def featurenet(calls, dev, g, hw=(256, 320), nv=NS + 1):
    H, W = hw
    torch.manual_seed(0)
    net = mvs.DeviceFeatureNet(8).to(dev).train()
    for m in net.modules():                                   # offsets away from zero, as in a trained net
        if isinstance(m, mvs._DCN):
            torch.nn.init.normal_(m.conv_offset_mask.weight, std=0.12)
    imgs = torch.rand(nv, 3, H, W, generator=g).to(dev)
    ups = [torch.randn(nv, c, H // s, W // s, generator=g).to(dev) for c, s in ((32, 4), (16, 2), (8, 1))]

    def run(switch):
        net.deform_kernels = switch
        net.zero_grad(set_to_none=True)
        out = net.forward_torch(imgs)
        torch.autograd.backward([out["stage1"], out["stage2"], out["stage3"]], ups)

    print(f"FeatureNet forward + backward, training mode, {nv} views of {H} x {W} as one batch", flush=True)
    report("FeatureNet fwd + bwd", lambda: run(True), lambda: run(False), calls)
    net.deform_kernels = False


def fit_step(calls, dev, g, hw=(256, 320), nv=NS + 1):
    from diner_amd.optim import DeviceAdam
    H, W = hw
    torch.manual_seed(0)
    model = estimator.DeviceTransMVSNet().to(dev).train()
    model.fused_readout, model.match_kernels = True, True
    opt = DeviceAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4, skip_nonfinite=True)
    imgs = torch.rand(1, nv, 3, H, W, generator=g).to(dev)
    proj = {f"stage{i + 1}": cameras(1, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    gts = {f"stage{i + 1}": (1.2 + 0.7 * torch.rand(1, H // s, W // s, generator=g)).to(dev) for i, s in enumerate((4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}

    def step(deform):
        model.deform_kernels = deform
        out = model(imgs, proj, depth_values, depth_interval=0.7 / 192)
        terms = estimator.focal_loss_bld(out, gts, masks, 0.7 / 192, dlossw=(1, 1, 1))
        terms[0].backward()
        opt.step(zero_grads=True)

    def feature_only(deform):
        model.deform_kernels = deform
        out = [model.feature(img) for img in torch.unbind(imgs, 1)]
        torch.autograd.backward([o[k] for o in out for k in ("stage1", "stage2", "stage3")], [torch.ones_like(o[k]) for o in out for k in ("stage1", "stage2", "stage3")])
        model.zero_grad(set_to_none=True)

    print(f"one fine-tuning step: {nv} views of {H} x {W} (FeatureNet runs them one view at a time), ndepths {model.ndepths}, training mode, "
          f"fused_readout, match_kernels, DeviceAdam", flush=True)
    t = alternate({"default": lambda: step(False), "deform": lambda: step(True)}, 2 * calls)
    ta, tb = t["default"][0::2], t["default"][1::2]
    aa = abs(statistics.median(ta) - statistics.median(tb)) / statistics.median(t["default"])
    print(f"  default {fmt(t['default'])}  deform_kernels {fmt(t['deform'])}  default / deform {statistics.median(t['default']) / statistics.median(t['deform']):5.3f}"
          f"  default A/A {100 * aa:.1f} %  peak default {peak_of(lambda: step(False)):8.1f} MiB  deform_kernels {peak_of(lambda: step(True)):8.1f} MiB",
          flush=True)
    t = alternate({"default": lambda: feature_only(False), "deform": lambda: feature_only(True)}, 2 * calls)
    print(f"  FeatureNet's share of that step (its forward + backward alone, view by view): default {fmt(t['default'])}  deform_kernels {fmt(t['deform'])}",
          flush=True)
    model.deform_kernels = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_deform_train.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max)")
    if not args.skip_layers:
        for shape, cout in LAYERS:
            layer(shape, cout, args.calls, dev, g)
    featurenet(args.calls, dev, g)
    if not args.skip_fit:
        fit_step(args.calls, dev, g)


if __name__ == "__main__":
    main()
