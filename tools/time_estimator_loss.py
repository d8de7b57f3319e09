"""Time the depth estimator's fine-tuning objective on the kernels (csrc/mvsloss.hip) and on torch, on the same device.

    python tools/time_estimator_loss.py                  # the three DTU stage shapes, B 1, and one fit step at 256 x 320
    python tools/time_estimator_loss.py --calls 10 --skip-fit

The parent of this feature has no objective for the estimator, so the baseline is estimator.focal_loss_bld_torch: the reference's own
operations in the reference's order, float32, run by torch on the device.  In one process, per stage shape:

  * loss forward + backward from the regulariser's cost (a leaf): the kernels on {"cost"} against torch on prob_volume =
    exp(log_softmax(cost)) -- what a fused_readout model and a default model hand to the loss -- with HIP events, 3 warm-up calls a route,
    then torch / kernels / torch / kernels ... alternating, the median with min - max, the torch route's two halves against each other
    (A/A), and torch.cuda.max_memory_allocated of one call of each route above what was allocated before;
  * the same with the kernels on the reference's call signature (torch forms prob_volume, the FROM_PROB kernels take it);
  * each launch alone against its byte bound: the bytes its volumes hold (each volume once) over the HBM rate a streaming kernel reaches.

Then one fine-tuning step (forward in training mode, focal_loss_bld, backward, DeviceAdam) of DeviceTransMVSNet with and without
fused_readout, alternating.  Inputs are seeded noise with a planted winner; needs a HIP device."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diner_amd import estimator, ops                                           # noqa: E402
from tools.time_mvs import DTU_STAGES, NS, alternate, cameras, fmt, peak_of, report, timed      # noqa: E402

PEAK_HBM = 6.3e12                  # bytes/s a streaming kernel reaches


def problem(D, H, W, dev, g, B=1):
    hyp = (torch.linspace(425.0, 935.0, D).view(1, D, 1, 1) + 2.0 * torch.rand(B, 1, H, W, generator=g)).contiguous()
    idx = torch.randint(0, D, (B, 1, H, W), generator=g)
    gt = torch.gather(hyp, 1, idx).squeeze(1) + (torch.rand(B, H, W, generator=g) - 0.5)
    cost = torch.randn(B, D, H, W, generator=g)
    cost.scatter_(1, (idx + torch.randint(-1, 2, idx.shape, generator=g)).clamp(0, D - 1), 6.0)
    mask = (torch.rand(B, H, W, generator=g) < 0.8).float()
    return cost.to(dev), hyp.to(dev), gt.to(dev), mask.to(dev)


def bound_line(name, nbytes, ms):
    t = nbytes / PEAK_HBM * 1e3
    print(f"    {name:44s} {nbytes / 1e6:8.1f} MB  {ms:8.3f} ms  {nbytes / ms / 1e9:6.2f} TB/s  {100 * t / ms:5.1f} % of the HBM bound ({t:.3f} ms)",
          flush=True)


def stage(name, D, H, W, calls, dev, g):
    cost, hyp, gt, mask = problem(D, H, W, dev, g)
    leaf = cost.clone().requires_grad_(True)
    gts, masks = {"stage3": gt}, {"stage3": mask}
    depth = torch.gather(hyp, 1, cost.argmax(1, keepdim=True)).squeeze(1)

    def run(kernels, from_cost):
        leaf.grad = None
        stage_in = {"depth_values": hyp, "depth": depth}
        if from_cost:
            stage_in.update(cost=leaf, prob_volume=None)
        else:
            stage_in["prob_volume"] = torch.exp(torch.log_softmax(leaf, dim=1))
        out = estimator.focal_loss_bld({"stage3": stage_in}, gts, masks, 2.5, force_torch=not kernels)
        out[0].backward()
        return out

    print(f"{name}: D {D}, {H} x {W}, B 1 ({4 * D * H * W / 2 ** 20:.1f} MiB a volume)", flush=True)
    a, b = run(True, True), run(False, False)
    print(f"  total kernels {float(a[0].detach()):.6f}  torch {float(b[0].detach()):.6f}; epe {float(a[2]):.6f} / {float(b[2]):.6f}", flush=True)
    report("loss fwd + bwd, cost route", lambda: run(True, True), lambda: run(False, False), calls)
    report("loss fwd + bwd, prob_volume route", lambda: run(True, False), lambda: run(False, False), calls)
    vol = 4 * D * H * W
    med = lambda fn: statistics.median(([fn() for _ in range(3)], timed(fn, calls))[1])
    unit = torch.full((1,), 3.75, dtype=torch.float64, device=dev)
    r = ops.mvs_stage_loss(cost, hyp, gt, mask, unit=unit, thresholds=(1.0, 3.0))
    up = torch.ones((), device=dev)
    prob = torch.exp(torch.log_softmax(cost, 1))
    bound_line("stage loss forward (cost, hyp; maps, record)", 2 * vol + 4 * H * W * 8,
               med(lambda: ops.mvs_stage_loss(cost, hyp, gt, mask, unit=unit, thresholds=(1.0, 3.0))))
    bound_line("stage loss forward, FROM_PROB", 2 * vol + 4 * H * W * 8,
               med(lambda: ops.mvs_stage_loss(prob, hyp, gt, mask, from_prob=True, unit=unit, thresholds=(1.0, 3.0))))
    bound_line("gradient (cost in, gradient out; record)", 2 * vol + 4 * H * W * 5,
               med(lambda: ops.mvs_stage_loss_grad(cost, None, False, mask, r["record"], r["factors"], up)))
    bound_line("gradient, FROM_PROB (gradient out; record)", vol + 4 * H * W * 5,
               med(lambda: ops.mvs_stage_loss_grad(prob, None, True, mask, r["record"], r["factors"], up)))
    bound_line("depth scores (three maps)", 4 * H * W * 3, med(lambda: ops.depth_scores(r["depth"], gt, mask, (1.5, 5.0), (0.5, 6.0))))


def fit_step(calls, dev, g, hw=(256, 320), nv=NS + 1):
    from diner_amd.optim import DeviceAdam
    H, W = hw
    torch.manual_seed(0)
    model = estimator.DeviceTransMVSNet().to(dev).train()
    opt = DeviceAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4, skip_nonfinite=True)
    imgs = torch.rand(1, nv, 3, H, W, generator=g).to(dev)
    proj = {f"stage{i + 1}": cameras(1, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    gts = {f"stage{i + 1}": (1.2 + 0.7 * torch.rand(1, H // s, W // s, generator=g)).to(dev) for i, s in enumerate((4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}

    def step(fused):
        model.fused_readout = fused
        out = model(imgs, proj, depth_values, depth_interval=0.7 / 192)
        terms = estimator.focal_loss_bld(out, gts, masks, 0.7 / 192, dlossw=(1, 1, 1))
        terms[0].backward()
        opt.step(zero_grads=True)

    print(f"one fine-tuning step: {nv} views of {H} x {W}, ndepths {model.ndepths}, training mode, DeviceAdam", flush=True)
    t = alternate({"default": lambda: step(False), "fused": lambda: step(True)}, 2 * calls)
    ta, tb = t["default"][0::2], t["default"][1::2]
    aa = abs(statistics.median(ta) - statistics.median(tb)) / statistics.median(t["default"])
    print(f"  default {fmt(t['default'])}  fused_readout {fmt(t['fused'])}  default / fused {statistics.median(t['default']) / statistics.median(t['fused']):5.3f}"
          f"  default A/A {100 * aa:.1f} %  peak default {peak_of(lambda: step(False)):8.1f} MiB  fused {peak_of(lambda: step(True)):8.1f} MiB", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_estimator_loss.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max); HBM bound at {PEAK_HBM / 1e12:.1f} TB/s")
    for name, (_, D, H, W) in DTU_STAGES.items():
        stage(name, D, H, W, args.calls, dev, g)
    if not args.skip_fit:
        fit_step(max(2, args.calls // 2), dev, g)


if __name__ == "__main__":
    main()
