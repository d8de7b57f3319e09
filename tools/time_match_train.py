"""Time the matching stage in training -- the cost volume's forward and backward -- on the kernels (csrc/mvs.hip: diner_mvs_similarity_f32,
diner_mvs_cost_volume_f32, diner_mvs_similarity_grad_f32) and on the torch route that training ran before (mvs.cost_volume_torch under
autograd), on the same device.

    python tools/time_match_train.py                     # the three DTU stage shapes, B 1, four source views, and one fit step at 256 x 320
    python tools/time_match_train.py --calls 10 --skip-fit

In one process, per stage shape (C32 D48 128 x 160 with the view weights from the pixelwise module in training mode; C16 D32 256 x 320 and
C8 D8 512 x 640 with given weights): cost volume forward + backward under a fixed upstream gradient, mvs.cost_volume_train against
mvs.cost_volume_torch, with HIP events, 3 warm-up calls a route, then torch / kernels / torch / kernels ... alternating, the median with
min - max, the torch route's two halves against each other (A/A), and torch.cuda.max_memory_allocated of one call of each route above
what was allocated before.  Then the gradient kernel alone in both upstream forms (the median of `calls` back-to-back calls after 3
warm-up calls, not alternating): its atomic bytes (4 taps x C floats per sample with a
non-zero weight, counted on the host from the forward's geometry as an upper bound: every sample, every tap) over its time beside the
chip-wide float-atomic rate, and the bytes it gathers (the same count) beside the cache rate DESIGN.md 8m measured for the forward's
gathers.  Then one fine-tuning step of DeviceTransMVSNet (forward in training mode, focal_loss_bld, backward, DeviceAdam; fused_readout
on) with and without match_kernels, alternating, as many calls a route as the stages get.  Inputs are seeded noise; needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import estimator, mvs, ops                                      # noqa: E402
from tools.time_mvs import DTU_STAGES, NS, alternate, cameras, fmt, peak_of, report, timed      # noqa: E402

ATOMIC_RATE = 1.3e12               # bytes/s of float atomic adds, chip-wide
GATHER_RATE = 4.8e12               # bytes/s the forward kernel's tap gathers reach out of the caches
GIVEN = {"dtu stage1": False, "dtu stage2": True, "dtu stage3": True}


def stage(name, shape, calls, dev, g):
    C, D, H, W = shape
    B = 1
    feats = [torch.randn(B, C, H, W, generator=g).to(dev).requires_grad_(True) for _ in range(NS + 1)]
    proj = cameras(B, H, W, 1, dev, g)
    hyp = (torch.linspace(1.2, 1.9, D).view(1, D, 1, 1) + 0.03 * torch.rand(B, 1, H, W, generator=g)).to(dev).contiguous()
    weights = torch.rand(B, NS, H, W, generator=g).to(dev) if GIVEN[name] else None
    up = torch.randn(B, 1, D, H, W, generator=g).to(dev)
    net = None if GIVEN[name] else mvs.DeviceDepthNet().to(dev).train().pixel_wise_net

    def run(fn):
        for f in feats:
            f.grad = None
        sim, _ = fn(feats, proj, hyp, net, weights)
        sim.backward(up)

    print(f"{name}: C {C}, D {D}, {H} x {W}, {NS} source views, B {B}, view weights {'given' if GIVEN[name] else 'from the pixelwise module'}",
          flush=True)
    report("cost volume fwd + bwd", lambda: run(mvs.cost_volume_train), lambda: run(mvs.cost_volume_torch), calls)
    # the gradient kernel alone
    cl = torch.stack([f.detach() for f in feats], 0).permute(0, 1, 3, 4, 2).contiguous()
    s, hom = ops.mvs_similarity(cl[0], cl[1:], proj, hyp)
    G = torch.randn(B, NS, D, H, W, generator=g).to(dev)
    vw = weights if weights is not None else torch.rand(B, NS, H, W, generator=g).to(dev)
    med = lambda fn: statistics.median(([fn() for _ in range(3)], timed(fn, calls))[1])
    live = float((s != 0).float().mean())                             # the share of samples with a tap inside the map
    nbytes = NS * D * H * W * 4 * C * 4
    print(f"    the kernels alone, medians of {calls} back-to-back calls; samples with a tap inside the map: {100 * live:.1f} %; upper bound of {nbytes / 1e9:.3f} GB added and as many gathered", flush=True)
    for label, fn in (("gradient kernel, per-view upstream", lambda: ops.mvs_similarity_grad(cl[0], cl[1:], hom, hyp, grad_views=G)),
                      ("gradient kernel, aggregated upstream", lambda: ops.mvs_similarity_grad(cl[0], cl[1:], hom, hyp, grad_aggregated=up[:, 0],
                                                                                                view_weights=vw)),
                      ("similarity kernel (forward)", lambda: ops.mvs_similarity(cl[0], cl[1:], proj, hyp))):
        ms = med(fn)
        line = f"    {label:38s} {ms:8.3f} ms"
        if "gradient" in label:
            line += (f"  atomics at most {nbytes / ms / 1e9:6.3f} TB/s of {ATOMIC_RATE / 1e12:.1f} ({100 * nbytes / ATOMIC_RATE * 1e3 / ms:5.1f} % of that bound, "
                     f"{nbytes / ATOMIC_RATE * 1e3:.3f} ms)  gathers {nbytes / ms / 1e9:6.3f} TB/s of {GATHER_RATE / 1e12:.1f}")
        print(line, flush=True)


def fit_step(calls, dev, g, hw=(256, 320), nv=NS + 1):
    from diner_amd.optim import DeviceAdam
    H, W = hw
    torch.manual_seed(0)
    model = estimator.DeviceTransMVSNet().to(dev).train()
    model.fused_readout = True
    opt = DeviceAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4, skip_nonfinite=True)
    imgs = torch.rand(1, nv, 3, H, W, generator=g).to(dev)
    proj = {f"stage{i + 1}": cameras(1, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    gts = {f"stage{i + 1}": (1.2 + 0.7 * torch.rand(1, H // s, W // s, generator=g)).to(dev) for i, s in enumerate((4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}

    def step(match):
        model.match_kernels = match
        out = model(imgs, proj, depth_values, depth_interval=0.7 / 192)
        terms = estimator.focal_loss_bld(out, gts, masks, 0.7 / 192, dlossw=(1, 1, 1))
        terms[0].backward()
        opt.step(zero_grads=True)

    print(f"one fine-tuning step: {nv} views of {H} x {W}, ndepths {model.ndepths}, training mode, fused_readout, DeviceAdam", flush=True)
    t = alternate({"default": lambda: step(False), "match": lambda: step(True)}, 2 * calls)
    ta, tb = t["default"][0::2], t["default"][1::2]
    aa = abs(statistics.median(ta) - statistics.median(tb)) / statistics.median(t["default"])
    print(f"  default {fmt(t['default'])}  match_kernels {fmt(t['match'])}  default / match {statistics.median(t['default']) / statistics.median(t['match']):5.3f}"
          f"  default A/A {100 * aa:.1f} %  peak default {peak_of(lambda: step(False)):8.1f} MiB  match_kernels {peak_of(lambda: step(True)):8.1f} MiB",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_match_train.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max)")
    for name, shape in DTU_STAGES.items():
        stage(name, shape, args.calls, dev, g)
    if not args.skip_fit:
        fit_step(args.calls, dev, g)


if __name__ == "__main__":
    main()
