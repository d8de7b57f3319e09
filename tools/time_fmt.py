"""Time the depth estimator's feature transformer on the kernels (csrc/fmt.hip) and on torch, on the same device.

    python tools/time_fmt.py                  # FMT_with_pathway at the DTU shape (512 x 640 image, stage 1 of 128 x 160, B 1, five views)
    python tools/time_fmt.py --calls 10 --skip-whole

The parent of this feature has no route for the FMT, so the baseline is DeviceFMTWithPathway held on its torch route: the reference's own
operations (Linear, elu, the three einsums, LayerNorm, Conv2d, F.interpolate) in the reference's order, eval mode, float32, run by torch
on the device.  In one process:

  * the whole FMT_with_pathway, the FMT alone (DeviceFMT.encode) and the pathway alone: HIP events around the call, 3 warm-up calls a
    route, then torch / kernels / torch / kernels ... alternating, the median of `--calls` with min - max; the torch route is timed twice
    over (A/A: its two halves' medians) so a difference can be held against the route's own spread;
    torch.cuda.max_memory_allocated of one call of each route above what was allocated before;
  * per launch on the kernels: FLOPs and bytes computed from the shapes (inputs + outputs + weights, each once), the median time of the
    launch alone, and the share of whichever bounds it -- the fp32 vector peak or the HBM bandwidth -- it reaches;
  * the three stages of coarse_to_fine with the real regulariser, with the module in front of them, on both routes.

The features are seeded noise: the time does not depend on their values.  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs, ops                                                 # noqa: E402
from tools.time_costreg import BASE, seeded, _TorchCostReg                     # noqa: E402
from tools.time_mvs import DTU_STAGES, NS, cameras, fmt, report, timed, _TorchRoute      # noqa: E402

PEAK_FP32_VECTOR = 157.3e12        # MI355X: fp32 vector FLOP/s (256 CUs x 128 lanes x 2 FLOP at 2.4 GHz): what plain fmaf chains can reach
PEAK_HBM = 8.0e12                  # bytes/s
H1, W1 = 128, 160


class _TorchFMT(mvs.DeviceFMT):
    def uses_kernels(self, x):
        return False


class _TorchPathway(mvs.DeviceFMTWithPathway):
    """The drop-in held on its torch route, whatever the tensors."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.FMT.__class__ = _TorchFMT

    def uses_kernels(self, features):
        return False


def randomised(net, g):
    """Biases and LayerNorm terms away from their defaults: the time does not depend on them, the values stay finite."""
    for k, v in net.state_dict().items():
        if v.dim() == 1:
            v.copy_(0.5 + torch.rand(v.shape, generator=g) if ".norm" in k and k.endswith("weight") else 0.2 * torch.randn(v.shape, generator=g))
    return net


def features(B, g, dev):
    return [{"stage1": torch.randn(B, 32, H1, W1, generator=g).to(dev), "stage2": torch.randn(B, 16, 2 * H1, 2 * W1, generator=g).to(dev),
             "stage3": torch.randn(B, 8, 4 * H1, 4 * W1, generator=g).to(dev)} for _ in range(NS + 1)]


def line(name, flop, nbytes, ms):
    t_flop, t_mem = flop / PEAK_FP32_VECTOR * 1e3, nbytes / PEAK_HBM * 1e3
    bound, t_bound = ("vector", t_flop) if t_flop >= t_mem else ("HBM", t_mem)
    print(f"    {name:34s} {flop / 1e9:7.3f} GFLOP  {nbytes / 1e6:7.1f} MB  {ms:7.3f} ms  {flop / ms / 1e9:7.2f} TFLOP/s  {nbytes / ms / 1e9:6.2f} TB/s  "
          f"{100 * t_bound / ms:5.1f} % of the {bound} bound", flush=True)
    return ms


def per_launch(net, feats, calls):
    """The kernels' launches one by one at the shapes of one forward."""
    dev = feats[0]["stage1"].device
    NV, B, L = len(feats), feats[0]["stage1"].shape[0], H1 * W1
    maps = torch.stack([f["stage1"] for f in feats], 0)
    packs = net.FMT.packed()
    tok = ops.fmt_tokenise(maps.view(NV * B, 32, H1, W1), net.FMT.pe[0])
    ref, src = tok[:B].contiguous(), tok[B:].contiguous()
    st_ref, st_src = ops.fmt_kv(ref, packs[0]), ops.fmt_kv(src, packs[0])
    med = lambda fn: statistics.median(([fn() for _ in range(3)], timed(fn, calls))[1])
    w = 4 * ops.FMT_PACK_FLOATS
    kv_flop = lambda n: n * L * (2 * 2 * 32 * 32 + 2 * 160)
    layer_flop = lambda n: n * L * (2 * (3 * 32 * 32 + 2 * 32 * 64) + 2 * 8 * 20)
    total = 0.0
    total += line(f"tokenise {NV * B} x {L}", NV * B * L * 32, 4 * 2 * NV * B * L * 32, med(lambda: ops.fmt_tokenise(maps.view(NV * B, 32, H1, W1), net.FMT.pe[0], out=tok)))
    t_kv_ref = line(f"attention state {B} x {L} (2 launches)", kv_flop(B), 4 * B * L * 32 + w, med(lambda: ops.fmt_kv(ref, packs[0])))
    t_kv_src = line(f"attention state {NS * B} x {L} (2 launches)", kv_flop(NS * B), 4 * NS * B * L * 32 + w, med(lambda: ops.fmt_kv(src, packs[0])))
    out_ref, out_src = torch.empty_like(ref), torch.empty_like(src)
    t_l_ref = line(f"layer {B} x {L}", layer_flop(B), 4 * 2 * B * L * 32 + w, med(lambda: ops.fmt_layer(ref, packs[0], st_ref, out=out_ref)))
    t_l_src = line(f"layer {NS * B} x {L}", layer_flop(NS * B), 4 * 2 * NS * B * L * 32 + w, med(lambda: ops.fmt_layer(src, packs[0], st_src, out=out_src)))
    t_l_x = line(f"cross layer {NS * B} x {L}", layer_flop(NS * B), 4 * 2 * NS * B * L * 32 + w, med(lambda: ops.fmt_layer(src, packs[1], st_ref, out=out_src)))
    total += 8 * t_kv_ref + 4 * t_l_ref + 4 * t_kv_src + 4 * t_l_src + 4 * t_l_x
    N = NV * B
    p1, p2 = net.packed()
    for tag, (h, wd, ct, cl, pk) in (("stage 2", (H1, W1, 32, 16, p1)), ("stage 3", (2 * H1, 2 * W1, 16, 8, p2))):
        top, lat = torch.randn(N, h, wd, ct, device=dev), torch.randn(N, 2 * h, 2 * wd, cl, device=dev)
        wt = (net.dim_reduction_1 if ct == 32 else net.dim_reduction_2).weight.detach()
        out = torch.empty_like(lat)
        fine = N * 4 * h * wd * cl
        total += line(f"merge {ct} -> {cl} to {tag} (2 launches)", 2 * N * h * wd * ct * cl + 8 * fine, 4 * (N * h * wd * (ct + 2 * cl) + 3 * fine),
                      med(lambda: ops.fpn_merge(top, wt, lat, out=out)))
        total += line(f"smooth 3 x 3, {cl} -> {cl}, {tag}", 2 * 9 * cl * fine, 4 * 2 * fine, med(lambda: ops.conv3x3(lat, pk, None, cl, out=out)))
    print(f"    sum over one forward's launches (8 + 4 states and 4 + 8 layers): {total:.3f} ms one by one", flush=True)


def whole(calls, dev, g, kn, tn, feats):
    H, W, B = 512, 640, 1
    proj = {f"stage{i + 1}": cameras(B, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    ndepths = tuple(D for _, D, _, _ in DTU_STAGES.values())
    dn, td = mvs.DeviceDepthNet().to(dev).eval(), _TorchRoute().to(dev).eval()
    td.load_state_dict(dn.state_dict())
    kr = seeded(mvs.DeviceCostRegNet(1, BASE), g).to(dev).eval()
    tr = _TorchCostReg(1, BASE).to(dev).eval()
    tr.load_state_dict(kr.state_dict())

    def run(module, net, reg):
        f = [dict(x) for x in feats] if module is None else module([dict(x) for x in feats])
        return mvs.coarse_to_fine(f, proj, depth_values, net, reg, ndepths=ndepths, image_hw=(H, W), depth_interval=0.7 / 192)

    print(f"coarse_to_fine on a {H} x {W} image, ndepths {ndepths}, {NS} source views, the real regulariser (base {BASE})", flush=True)
    report("three stages, features as given", lambda: run(None, dn, kr), lambda: run(None, td, tr), calls)
    report("FMT_with_pathway + three stages", lambda: run(kn, dn, kr), lambda: run(tn, td, tr), calls)
    t = timed(lambda: run(tn, dn, kr), calls)
    print(f"  torch FMT_with_pathway + three stages on the kernels: {fmt(t)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-whole", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_fmt.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max); bounds: fp32 vector "
          f"{PEAK_FP32_VECTOR / 1e12:.1f} TFLOP/s, HBM {PEAK_HBM / 1e12:.1f} TB/s")
    kn = randomised(mvs.DeviceFMTWithPathway(8), g).to(dev).eval()
    tn = _TorchPathway(8).to(dev).eval()
    tn.load_state_dict(kn.state_dict())
    with torch.no_grad():
        feats = features(1, g, dev)
        fresh = lambda: [dict(f) for f in feats]
        print(f"FMT_with_pathway: stage 1 of {H1} x {W1}, B 1, {NS + 1} views", flush=True)
        assert kn.uses_kernels(feats) and not tn.uses_kernels(feats)
        report("FMT_with_pathway forward", lambda: kn(fresh()), lambda: tn(fresh()), args.calls)
        ref, srcs = feats[0]["stage1"], [f["stage1"] for f in feats[1:]]
        report("FMT alone (encode)", lambda: kn.FMT.encode(ref, srcs), lambda: tn.FMT.encode(ref, srcs), args.calls)
        N = NS + 1
        tok = torch.randn(N, H1, W1, 32, device=dev)
        lat2, lat3 = torch.randn(N, 2 * H1, 2 * W1, 16, device=dev), torch.randn(N, 4 * H1, 4 * W1, 8, device=dev)
        nchw = [t.permute(0, 3, 1, 2).contiguous() for t in (tok, lat2, lat3)]

        def torch_pathway():
            s2 = tn.smooth_1(tn._upsample_add(tn.dim_reduction_1(nchw[0]), nchw[1]))
            return s2, tn.smooth_2(tn._upsample_add(tn.dim_reduction_2(s2), nchw[2]))
        report("pathway alone (all views, one batch)", lambda: kn.pathway(tok, lat2.clone(), lat3.clone()), torch_pathway, args.calls)
        per_launch(kn, feats, args.calls)
        if not args.skip_whole:
            whole(args.calls, dev, g, kn, tn, feats)


if __name__ == "__main__":
    main()
