"""Time the depth estimator's matching stage on the kernels (csrc/mvs.hip) and on the torch restatement, on the same device.

    python tools/time_mvs.py                      # the three DTU stage shapes and the DINER-sized 256 x 320 image
    python tools/time_mvs.py --calls 10 --only dtu

The parent of this feature has no route for the matching stage, so the baseline is the torch restatement of diner_amd.mvs: the
reference's own operations (torch.inverse, the sampling grid, F.grid_sample, the (B,C,D,H,W) warped volume, Conv3d / BatchNorm3d for the
view weights) run by torch on the device, untuned.  Per shape, with one reference and four source views at B 1:

  * cost volume with the pixelwise net, cost volume with given view weights, depth read-out, hypotheses: HIP events around each entry,
    3 warm-up calls a route, then torch / kernels / torch / kernels ... alternating in one process, the median of `--calls` with min - max;
    the torch route is timed twice over (A/A: its two halves' medians) so a difference can be held against the route's own spread;
  * torch.cuda.max_memory_allocated of one call of each route above what was allocated before it;
  * the whole coarse_to_fine (three stages) with an identity-gain regulariser on both routes.

The features are seeded noise: the time does not depend on their values (every sample takes the same four taps).  Needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import mvs                     # noqa: E402

NS = 4
# name: (C, D, H, W)
DTU_STAGES = {"dtu stage1": (32, 48, 128, 160), "dtu stage2": (16, 32, 256, 320), "dtu stage3": (8, 8, 512, 640)}
DINER_STAGES = {"diner stage1": (32, 48, 64, 80), "diner stage2": (16, 32, 128, 160), "diner stage3": (8, 8, 256, 320)}
IMAGES = {"dtu": ((512, 640), DTU_STAGES), "diner": ((256, 320), DINER_STAGES)}


def cameras(B, H, W, scale, dev, g):
    """Reference-first camera pairs (B,NS+1,2,4,4): focal 0.9 W of the full image, source cameras shifted by up to 0.15 in x and y."""
    pair = torch.zeros(B, NS + 1, 2, 4, 4)
    pair[:, :, 0] = torch.eye(4)
    pair[:, 1:, 0, :2, 3] = (torch.rand(B, NS, 2, generator=g) - 0.5) * 0.3
    f = 0.9 * W * scale
    pair[:, :, 1, :3, :3] = torch.tensor([[f, 0, (W * scale - 1) / 2], [0, f, (H * scale - 1) / 2], [0, 0, 1]])
    pair[:, :, 1, :2] /= scale
    return pair.to(dev)


def timed(fn, calls):
    """-> list of ms per call (HIP events)."""
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(routes, calls, warm=3):
    """routes: {name: fn}; each is warmed, then they run in turn, one call at a time -> {name: [ms]}."""
    for fn in routes.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for _ in range(calls):
        for k, fn in routes.items():
            out[k] += timed(fn, 1)
    return out


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def fmt(ms):
    return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f} - {max(ms):.3f})"


def report(title, kernel_fn, torch_fn, calls):
    t = alternate({"torch": torch_fn, "kernels": kernel_fn}, 2 * calls)
    ta, tb = t["torch"][0::2], t["torch"][1::2]
    tk = t["kernels"]
    aa = abs(statistics.median(ta) - statistics.median(tb)) / statistics.median(t["torch"])
    ratio = statistics.median(t["torch"]) / statistics.median(tk)
    print(f"  {title:34s} torch {fmt(t['torch'])}  kernels {fmt(tk)}  torch / kernels {ratio:6.2f}  torch A/A {100 * aa:.1f} %  "
          f"peak torch {peak_of(torch_fn):8.1f} MiB  kernels {peak_of(kernel_fn):7.1f} MiB", flush=True)


def entries(name, shape, calls, dev, g):
    C, D, H, W = shape
    B = 1
    feats = [torch.randn(B, C, H, W, generator=g).to(dev) for _ in range(NS + 1)]
    proj = cameras(B, H, W, 1, dev, g)
    hyp = (torch.linspace(1.2, 1.9, D).view(1, D, 1, 1) + 0.03 * torch.rand(B, 1, H, W, generator=g)).to(dev).contiguous()
    weights = torch.rand(B, NS, H, W, generator=g).to(dev)
    cost = torch.randn(B, D, H, W, generator=g).to(dev)
    dn = mvs.DeviceDepthNet().to(dev).eval()
    pw = dn.pixelwise()
    prev = torch.rand(B, max(H // 2, 1), max(W // 2, 1), generator=g).to(dev) + 1.2
    print(f"{name}: C {C}, D {D}, {H} x {W}, {NS} source views, B {B}", flush=True)
    with torch.no_grad():
        report("cost volume + pixelwise net", lambda: mvs.cost_volume(feats, proj, hyp, pw, None),
               lambda: mvs.cost_volume_torch(feats, proj, hyp, pw, None), calls)
        report("cost volume, given view weights", lambda: mvs.cost_volume(feats, proj, hyp, None, weights),
               lambda: mvs.cost_volume_torch(feats, proj, hyp, None, weights), calls)
        report("select depth (with prob volume)", lambda: mvs.select_depth(cost, hyp), lambda: mvs.select_depth_torch(cost, hyp), calls)
        report("hypotheses (scale 1 of this size)", lambda: mvs.depth_hypotheses(prev, D, 0.01, (H, W), 1) if D > 1 else None,
               lambda: mvs.depth_hypotheses_torch(prev, D, 0.01, (H, W), 1) if D > 1 else None, calls)


class _TorchRoute(mvs.DeviceDepthNet):
    """The drop-in held on its torch route (cost volume, read-out and hypotheses), whatever the tensors."""

    def uses_kernels(self, features):
        return False


def whole(tag, image, stages, calls, dev, g):
    H, W = image
    B = 1
    feats = [{f"stage{i + 1}": torch.randn(B, C, h, w, generator=g).to(dev) for i, (C, _, h, w) in enumerate(stages.values())}
             for _ in range(NS + 1)]
    proj = {f"stage{i + 1}": cameras(B, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    ndepths = tuple(D for _, D, _, _ in stages.values())
    dn = mvs.DeviceDepthNet().to(dev).eval()
    tn = _TorchRoute().to(dev).eval()
    tn.load_state_dict(dn.state_dict())
    gain = lambda s: 1.0 * s

    def run(net):
        return mvs.coarse_to_fine(feats, proj, depth_values, net, gain, ndepths=ndepths, image_hw=image, depth_interval=0.7 / 192)

    print(f"{tag}: coarse_to_fine on a {H} x {W} image, ndepths {ndepths}, identity-gain regulariser", flush=True)
    with torch.no_grad():
        report("three stages", lambda: run(dn), lambda: run(tn), calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--only", choices=sorted(IMAGES), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_mvs.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max)")
    for tag, (image, stages) in IMAGES.items():
        if args.only and tag != args.only:
            continue
        for name, shape in stages.items():
            entries(name, shape, args.calls, dev, g)
        whole(tag, image, stages, args.calls, dev, g)


if __name__ == "__main__":
    main()
