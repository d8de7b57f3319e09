"""Time the depth estimator's cost regulariser on the kernels (csrc/costreg.hip) and on torch / MIOpen, on the same device.

    python tools/time_costreg.py                  # the three DTU stage volumes at base 8 and the whole coarse_to_fine at 512 x 640
    python tools/time_costreg.py --calls 10 --skip-whole

The parent of this feature has no route for CostRegNet, so the baseline is DeviceCostRegNet held on its torch route: the reference's own
module structure (Conv3d / ConvTranspose3d, BatchNorm3d on the running statistics, ReLU, the skip additions) in eval mode, float32, run
by torch on the device.  Per volume, B 1:

  * the whole net: HIP events around forward(), 3 warm-up calls a route, then torch / kernels / torch / kernels ... alternating in one
    process, the median of `--calls` with min - max; the torch route is timed twice over (A/A: its two halves' medians) so a difference
    can be held against the route's own spread; torch.cuda.max_memory_allocated of one call of each route above what was allocated before;
  * per layer on the kernels: FLOPs and bytes computed from the shapes (input + output + addend + packed weights, each once), the median
    time of the launch alone, and the share of whichever bounds that layer -- the fp32 matrix peak or the HBM bandwidth -- it reaches;
  * the whole coarse_to_fine (three stages, one reference and four source views) with the real regulariser on both routes.

The volumes are seeded noise: the time does not depend on their values.  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs, ops                                                 # noqa: E402
from tools.time_mvs import DTU_STAGES, NS, cameras, report, timed, _TorchRoute      # noqa: E402

PEAK_FP32_MATRIX = 157.3e12        # MI355X: fp32 matrix FLOP/s (256 CUs x 256 FLOP/clk at 2.4 GHz)
PEAK_HBM = 8.0e12                  # bytes/s
BASE = 8
VOLUMES = {name: (D, H, W) for name, (_, D, H, W) in DTU_STAGES.items()}


class _TorchCostReg(mvs.DeviceCostRegNet):
    """The drop-in held on its torch route, whatever the tensors."""

    def uses_kernels(self, x):
        return False


def seeded(net, g):
    """Weights of unit gain and BatchNorm statistics away from the identity: the time does not depend on them, the values stay finite."""
    sd = net.state_dict()
    for k, v in sd.items():
        if k.endswith("conv.weight") or k == "prob.weight":
            fan = 27 * (v.shape[0] if "conv7" in k or "conv9" in k or "conv11" in k else v.shape[1])
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / fan) ** 0.5)
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith("running_mean") or k.endswith("bn.bias"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
    return net


def layer_table(D, H, W, base=BASE):
    """-> per layer (name, kind, stride, Cin, Cout, input (D,H,W), output (D,H,W), has addend)."""
    rows, dims = [], (D, H, W)
    for name, kind, ci, co, stride in mvs.COSTREG_LAYERS:
        cin, cout = (1 if ci == 0 else ci * base), co * base
        odims = tuple(2 * n for n in dims) if kind == "deconv" else tuple((n - 1) // stride + 1 for n in dims)
        rows.append((name, kind, stride, cin, cout, dims, odims, kind == "deconv"))
        dims = odims
    rows.append(("prob", "conv", 1, base, 1, dims, dims, False))
    return rows


def layer_work(row):
    name, kind, stride, cin, cout, idims, odims, addend = row
    vin, vout = idims[0] * idims[1] * idims[2], odims[0] * odims[1] * odims[2]
    flop = 2 * 27 * cin * cout * (vin if kind == "deconv" else vout)
    nbytes = 4 * (vin * cin + vout * cout * (2 if addend else 1) + (-(-cin // 8)) * 27 * 8 * ops.conv3d_cout_pad(cout))
    return flop, nbytes


def per_layer(net, x, calls):
    """The kernels' launches one by one on the volumes the net's own forward left in its workspace."""
    B, _, D, H, W = x.shape
    net(x)                                                                       # fills the workspace
    ws = net._workspace(B, D, H, W, x.device)
    cur = x.contiguous().view(B, D, H, W, 1)
    inputs = {"conv0": cur, "conv1": ws["conv0"], "conv2": ws["conv1"], "conv3": ws["conv2"], "conv4": ws["conv3"], "conv5": ws["conv4"],
              "conv6": ws["conv5"], "conv7": ws["conv6"], "conv9": ws["conv4"], "conv11": ws["conv2"], "prob": ws["conv0"]}
    skip = {"conv7": "conv4", "conv9": "conv2", "conv11": "conv0"}
    tot_flop = tot_bytes = tot_ms = 0.0
    for row, (name, kind, stride, cout, pack, bias, relu) in zip(layer_table(D, H, W, net.base_channels), net.packed()):
        xin = inputs[name]
        if kind == "deconv":
            out = torch.empty_like(ws[skip[name]])
            fn = lambda: ops.deconv3d_s2(xin, pack, bias, cout, relu=relu, addend=ws[skip[name]], out=out)
        else:
            out = torch.empty(ops._check_conv3d_args("conv3d", xin, pack, bias, cout, stride, None, None)[5], device=x.device)
            fn = lambda: ops.conv3d(xin, pack, bias, cout, stride=stride, relu=relu, out=out)
        for _ in range(3):
            fn()
        ms = statistics.median(timed(fn, calls))
        flop, nbytes = layer_work(row)
        t_flop, t_mem = flop / PEAK_FP32_MATRIX * 1e3, nbytes / PEAK_HBM * 1e3
        bound, t_bound = ("matrix", t_flop) if t_flop >= t_mem else ("HBM", t_mem)
        print(f"    {name:7s} {kind:6s} s{stride} {row[3]:3d} -> {row[4]:3d}  {'x'.join(map(str, row[5])):>12s} -> {'x'.join(map(str, row[6])):>12s}  "
              f"{flop / 1e9:7.2f} GFLOP  {nbytes / 1e6:7.1f} MB  {ms:7.3f} ms  {flop / ms / 1e9:7.1f} TFLOP/s  {nbytes / ms / 1e9:6.2f} TB/s  "
              f"{100 * t_bound / ms:5.1f} % of the {bound} bound", flush=True)
        tot_flop, tot_bytes, tot_ms = tot_flop + flop, tot_bytes + nbytes, tot_ms + ms
    print(f"    sum: {tot_flop / 1e9:.2f} GFLOP, {tot_bytes / 1e6:.1f} MB, {tot_ms:.3f} ms of launches one by one", flush=True)
    return tot_flop, tot_bytes


def whole(calls, dev, g, kn, tn):
    H, W = 512, 640
    B = 1
    stages = DTU_STAGES
    feats = [{f"stage{i + 1}": torch.randn(B, C, h, w, generator=g).to(dev) for i, (C, _, h, w) in enumerate(stages.values())}
             for _ in range(NS + 1)]
    proj = {f"stage{i + 1}": cameras(B, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    ndepths = tuple(D for _, D, _, _ in stages.values())
    dn = mvs.DeviceDepthNet().to(dev).eval()
    td = _TorchRoute().to(dev).eval()
    td.load_state_dict(dn.state_dict())

    def run(net, reg):
        return mvs.coarse_to_fine(feats, proj, depth_values, net, reg, ndepths=ndepths, image_hw=(H, W), depth_interval=0.7 / 192)

    print(f"coarse_to_fine on a {H} x {W} image, ndepths {ndepths}, {NS} source views, the real regulariser (base {BASE}) on both routes", flush=True)
    report("three stages", lambda: run(dn, kn), lambda: run(td, tn), calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-whole", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_costreg.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max); bounds: fp32 matrix "
          f"{PEAK_FP32_MATRIX / 1e12:.1f} TFLOP/s, HBM {PEAK_HBM / 1e12:.1f} TB/s")
    kn = seeded(mvs.DeviceCostRegNet(1, BASE), g).to(dev).eval()
    tn = _TorchCostReg(1, BASE).to(dev).eval()
    tn.load_state_dict(kn.state_dict())
    flop = nbytes = 0.0
    with torch.no_grad():
        for name, (D, H, W) in VOLUMES.items():
            x = (0.5 * torch.rand(1, 1, D, H, W, generator=g)).to(dev)
            print(f"{name}: volume {D} x {H} x {W}, base {BASE}, B 1", flush=True)
            report("CostRegNet forward", lambda: kn(x), lambda: tn(x), args.calls)
            f, b = per_layer(kn, x, args.calls)
            flop, nbytes = flop + f, nbytes + b
        print(f"three volumes: {flop / 1e9:.1f} GFLOP ({flop / PEAK_FP32_MATRIX * 1e3:.2f} ms at the fp32 matrix peak), {nbytes / 1e9:.2f} GB "
              f"({nbytes / PEAK_HBM * 1e3:.2f} ms at the HBM bandwidth)", flush=True)
        if not args.skip_whole:
            whole(args.calls, dev, g, kn, tn)


if __name__ == "__main__":
    main()
