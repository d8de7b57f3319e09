"""Time the depth estimator's FeatureNet on the kernels (csrc/deform.hip, csrc/conv2d.hip) and on torch, on the same device.

    python tools/time_featurenet.py                  # five 512 x 640 views, B 1 (the DTU shape)
    python tools/time_featurenet.py --calls 5 --skip-whole

The parent of this feature has no route for FeatureNet (torchvision, which the reference's deformable convolutions need, is not
installed), so the baseline is DeviceFeatureNet held on its torch route: the reference's own operations in the reference's order with
mvs.deform_conv2d_torch as the deformable convolution, eval mode, float32, run by torch on the device, view by view as
TransMVSNet.forward calls it.  In one process:

  * forward_views: HIP events around the call, 3 warm-up calls a route, then torch / kernels / torch / kernels ... alternating, the median
    of `--calls` with min - max; the torch route is timed twice over (A/A: its two halves' medians) so a difference can be held against
    the route's own spread; torch.cuda.max_memory_allocated of one call of each route above what was allocated before;
  * per launch on the kernels: FLOPs and bytes computed from the shapes (inputs + outputs + weights, each once), the median time of the
    launch alone, and the share of whichever bounds it -- the fp32 matrix peak or the HBM bandwidth -- it reaches; the deformable kernel
    and the 27-channel offset convolution in front of it side by side;
  * FeatureNet + FMT_with_pathway + the three stages of coarse_to_fine with the real regulariser as one figure (mvs.depth_from_images),
    on both routes.

The images and weights are seeded noise; the offset convolutions are scaled so that offsets spread over about 1.5 px, as in fixture G31
(with the reference's zero initialisation every sample would sit on a pixel).  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs, ops                                                 # noqa: E402
from tests import featurenet_util as FU                                        # noqa: E402
from tools.time_costreg import BASE, seeded, _TorchCostReg                     # noqa: E402
from tools.time_fmt import _TorchPathway, randomised                           # noqa: E402
from tools.time_mvs import DTU_STAGES, NS, cameras, fmt, report, timed, _TorchRoute      # noqa: E402

PEAK_FP32_MATRIX = 157.3e12        # MI355X: v_mfma_f32_16x16x4_f32 runs at the fp32 vector rate
PEAK_HBM = 6.3e12                  # bytes/s a streaming kernel reaches
H, W = 512, 640


class _TorchFeatureNet(mvs.DeviceFeatureNet):
    """The drop-in held on its torch route, whatever the tensors."""

    def uses_kernels(self, x):
        return False


def line(name, flop, nbytes, ms):
    t_flop, t_mem = flop / PEAK_FP32_MATRIX * 1e3, nbytes / PEAK_HBM * 1e3
    bound, t_bound = ("matrix", t_flop) if t_flop >= t_mem else ("HBM", t_mem)
    print(f"    {name:44s} {flop / 1e9:8.3f} GFLOP  {nbytes / 1e6:8.1f} MB  {ms:8.3f} ms  {flop / ms / 1e9:7.2f} TFLOP/s  {nbytes / ms / 1e9:6.2f} TB/s  "
          f"{100 * t_bound / ms:5.1f} % of the {bound} bound ({t_bound:.3f} ms)", flush=True)
    return ms


def per_launch(net, N, calls, dev):
    """The kernels' launches one by one at the shapes of one forward of N images."""
    P = net.packed()
    med = lambda fn: statistics.median(([fn() for _ in range(3)], timed(fn, calls))[1])
    rnd = lambda h, w, c: torch.randn(N, h, w, c, device=dev)
    total, by_kind = 0.0, {}

    def add(kind, count, ms):
        nonlocal total
        total += count * ms
        by_kind[kind] = by_kind.get(kind, 0.0) + count * ms

    img = torch.rand(N, 3, H, W, device=dev)
    add("relayout", 1, line(f"input relayout {N} x 3 x {H} x {W} -> C 4", 0, 4 * N * H * W * 7, med(lambda: ops.encoder_input(img, pad=0, C=4))))
    for name, h, w, cin, cout, count in (("conv0.0", H, W, 4, 8, 1), ("conv0.1", H, W, 8, 8, 1), ("conv1.1/2", H // 2, W // 2, 16, 16, 2),
                                         ("conv2.1/2", H // 4, W // 4, 32, 32, 2), ("out2.0", H // 2, W // 2, 32, 32, 1), ("out3.0", H, W, 32, 32, 1)):
        x, key = rnd(h, w, cin), name.split("/")[0]
        add("conv3x3", count, line(f"{name} 3 x 3 {cin} -> {cout} at {h} x {w}" + (f" (x{count})" if count > 1 else ""), 2 * 9 * cin * cout * N * h * w,
                                   4 * N * h * w * (cin + cout), med(lambda: ops.conv3x3(x, *P[key], cout, relu=True))))
    for name, h, w, cin, cout in (("conv1.0", H, W, 8, 16), ("conv2.0", H // 2, W // 2, 16, 32)):
        x = rnd(h, w, cin)
        add("conv5x5", 1, line(f"{name} 5 x 5 stride 2 {cin} -> {cout} from {h} x {w}", 2 * 25 * cin * cout * N * h * w // 4,
                               4 * N * h * w * (cin + cout // 4), med(lambda: ops.conv5x5_s2(x, *P[name], cout, relu=True))))
    x = rnd(H // 4, W // 4, 32)
    add("conv1x1", 1, line(f"out1.0 1 x 1 32 -> 32 at {H // 4} x {W // 4}", 2 * 32 * 32 * N * H * W // 16, 4 * N * H * W // 16 * 64,
                           med(lambda: ops.conv1x1(x, *P["out1.0"], 32, relu=True))))
    for name, h, w, cl in (("inner1", H // 2, W // 2, 16), ("inner2", H, W, 8)):
        top, lat = rnd(h // 2, w // 2, 32), rnd(h, w, cl)
        add("lateral", 1, line(f"lateral {name} {cl} -> 32 at {h} x {w}", 2 * cl * 32 * N * h * w, 4 * N * h * w * (8 + cl + 32),
                               med(lambda: ops.fpn_lateral(top, lat, *P[name]))))
    for head, h, w, last in (("out1", H // 4, W // 4, 32), ("out2", H // 2, W // 2, 16), ("out3", H, W, 8)):
        x = rnd(h, w, 32)
        om = ops.conv3x3(x, *P[f"{head}.1.offset"], 27)
        om[..., :18] = 1.5 * torch.randn(N, h, w, 18, device=dev)             # the spread of fixture G31, whatever the noise input gives
        add("offset conv", 3, line(f"{head} offsets 3 x 3 32 -> 27 at {h} x {w} (x3)", 2 * 9 * 32 * 27 * N * h * w, 4 * N * h * w * (32 + 27),
                                   med(lambda: ops.conv3x3(x, *P[f"{head}.1.offset"], 27))))
        add("deform", 2, line(f"{head} deform 32 -> 32 at {h} x {w} (x2)", 2 * 9 * 32 * 32 * N * h * w + 9 * 32 * 8 * N * h * w,
                              4 * N * h * w * (32 + 27 + 32), med(lambda: ops.deform_conv3x3(x, om, *P[f"{head}.1"], 32, relu=True))))
        add("deform", 1, line(f"{head} deform 32 -> {last} at {h} x {w}", 2 * 9 * 32 * last * N * h * w + 9 * 32 * 8 * N * h * w,
                              4 * N * h * w * (32 + 27 + last), med(lambda: ops.deform_conv3x3(x, om, *P[f"{head}.7"], last))))
    print(f"    sum over one forward's 34 launches: {total:.3f} ms one by one; by kind: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(by_kind.items(), key=lambda kv: -kv[1])), flush=True)


def whole(calls, dev, g, kf, tf, imgs):
    B = 1
    proj = {f"stage{i + 1}": cameras(B, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    ndepths = tuple(D for _, D, _, _ in DTU_STAGES.values())
    dn, td = mvs.DeviceDepthNet().to(dev).eval(), _TorchRoute().to(dev).eval()
    td.load_state_dict(dn.state_dict())
    kr = seeded(mvs.DeviceCostRegNet(1, BASE), g).to(dev).eval()
    tr = _TorchCostReg(1, BASE).to(dev).eval()
    tr.load_state_dict(kr.state_dict())
    kp = randomised(mvs.DeviceFMTWithPathway(8), g).to(dev).eval()
    tp = _TorchPathway(8).to(dev).eval()
    tp.load_state_dict(kp.state_dict())

    def run(feature, pathway, net, reg):
        return mvs.depth_from_images(imgs, proj, depth_values, feature, pathway, net, reg, ndepths=ndepths, depth_interval=0.7 / 192)

    print(f"depth_from_images on {NS + 1} views of {H} x {W}, ndepths {ndepths}, the real regulariser (base {BASE})", flush=True)
    report("FeatureNet + FMT + three stages", lambda: run(kf, kp, dn, kr), lambda: run(tf, tp, td, tr), calls)
    t = timed(lambda: run(tf, kp, dn, kr), calls)
    print(f"  torch FeatureNet, everything behind it on the kernels: {fmt(t)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-whole", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_featurenet.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max); bounds: fp32 matrix "
          f"{PEAK_FP32_MATRIX / 1e12:.1f} TFLOP/s, HBM {PEAK_HBM / 1e12:.1f} TB/s")
    kf = mvs.DeviceFeatureNet(8)
    kf.load_state_dict(FU.featurenet_state_dict(0))
    kf = kf.to(dev).eval()
    tf = _TorchFeatureNet(8).to(dev).eval()
    tf.load_state_dict(kf.state_dict())
    with torch.no_grad():
        imgs = FU.texture(g, NS + 1, (H, W)).view(1, NS + 1, 3, H, W).to(dev)
        assert kf.uses_kernels(imgs[:, 0]) and not tf.uses_kernels(imgs[:, 0])
        print(f"FeatureNet: {NS + 1} views of {H} x {W}, B 1", flush=True)
        report("FeatureNet forward_views", lambda: kf.forward_views(imgs), lambda: tf.forward_views(imgs), args.calls)
        per_launch(kf, NS + 1, args.calls, dev)
        if not args.skip_whole:
            whole(args.calls, dev, g, kf, tf, imgs)


if __name__ == "__main__":
    main()
