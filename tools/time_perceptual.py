"""What the perceptual network costs on the device, beside the torch / MIOpen route on the same weights and inputs.

    python tools/time_perceptual.py [--reps 10] [--skip-batch16]

Seeded full-width weights (diner_amd.synthetic.make_vgg_state_dict: the real ones are not part of this project; the cost does not depend
on the values).  Three workloads:
  - LPIPS on 800 x 600 pairs at batch 1 and at batch 16: diner_amd.perceptual.Lpips against the torch restatement of lpips.LPIPS(net="vgg")
    (torch.nn.functional convolutions in float32 on the same device, written out below);
  - one VGG-loss forward plus backward at 4 x 3 x 64 x 64, the patch of the shipped training step: diner_amd.perceptual.VggLoss against
    src.losses.VGGLoss around the same stack.
Each workload: 3 warm-up calls of both routes, then --reps timed calls of each, the two routes alternating, HIP events around every
call; the median, the fastest and the slowest are reported, and the outputs of the two routes are compared.  The FLOP count is that of
the convolutions alone (2 x 9 x Cin x Cout per output pixel; the data gradient costs the same again for every layer but none of it is
skipped for the first), computed from the shapes.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def conv_flops(layers, n_images, H, W):
    total = 0
    for L in layers:
        if L.pool_before:
            H, W = H // 2, W // 2
        total += 2 * 9 * L.Cin * L.Cout * H * W * n_images
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-batch16", action="store_true")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    assert torch.cuda.is_available(), "needs a HIP device"
    from diner_amd import perceptual as P
    from diner_amd.synthetic import make_vgg_state_dict
    from src.losses import VGGLoss
    dev = torch.device("cuda", 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def compare(routes, reps):
        """routes: {name: fn}; alternating timed calls -> {name: {median_ms, min_ms, max_ms}}, the last outputs."""
        for _ in range(3):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        ms, outs = {k: [] for k in routes}, {}
        for _ in range(reps):
            for k, fn in routes.items():
                t, outs[k] = timed(fn)
                ms[k].append(t)
        return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}, outs

    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps}

    # ---- LPIPS ----
    sd16 = make_vgg_state_dict("vgg16", 16, with_lins=True)
    lp = P.Lpips(sd16, device=dev)
    sdd = {k: v.to(dev) for k, v in sd16.items()}
    spec = P.ARCHS["vgg16"]
    tap_relu = [i + 1 for i in spec["taps"]]
    shift = torch.tensor(P.LPIPS_SHIFT, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(P.LPIPS_SCALE, device=dev).view(1, 3, 1, 1)

    def torch_taps(z):
        out = []
        for i in range(tap_relu[-1] + 1):
            if i in spec["convs"]:
                z = F.conv2d(z, sdd[f"features.{i}.weight"], sdd[f"features.{i}.bias"], padding=1)
            elif i in spec["pools"]:
                z = F.max_pool2d(z, 2, 2)
            else:
                z = F.relu(z)
            if i in tap_relu:
                out.append(z)
        return out

    @torch.no_grad()
    def torch_lpips(pred, gt):
        total = 0
        for k, (a, b) in enumerate(zip(torch_taps((pred - shift) / scale), torch_taps((gt - shift) / scale))):
            a = a / (torch.sqrt(torch.sum(a ** 2, dim=1, keepdim=True)) + 1e-10)
            b = b / (torch.sqrt(torch.sum(b ** 2, dim=1, keepdim=True)) + 1e-10)
            total = total + F.conv2d((a - b) ** 2, sdd[f"lin{k}.model.1.weight"]).mean(dim=(2, 3), keepdim=True)
        return total

    g = torch.Generator().manual_seed(7)
    H, W = 600, 800
    for N in (1,) if args.skip_batch16 else (1, 16):
        pred = (torch.rand(N, 3, H, W, generator=g) * 2 - 1).to(dev)
        gt = (pred + 0.3 * torch.randn(N, 3, H, W, generator=g).to(dev)).clamp(-1, 1)
        t, outs = compare({"device": lambda: lp(pred, gt), "torch": lambda: torch_lpips(pred, gt)}, args.reps if N == 1 else max(3, args.reps // 2))
        flops = conv_flops(lp.features.layers, 2 * N, H, W)
        rel = float(((outs["device"] - outs["torch"]).abs() / outs["torch"].abs()).max())
        result[f"lpips_800x600_batch{N}"] = dict(**t, ratio_torch_over_device=t["torch"]["median_ms"] / t["device"]["median_ms"],
                                                  conv_tflop=flops / 1e12, device_tflops=flops / t["device"]["median_ms"] / 1e9,
                                                  max_rel_difference=rel)
        del pred, gt, outs
        torch.cuda.empty_cache()

    # ---- the VGG loss of the training step ----
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden_perceptual import sequential_from
    sd19 = make_vgg_state_dict("vgg19", 19)
    stack = sequential_from(sd19, "vgg19")
    mine = P.VggLoss(stack, device=dev)
    theirs = VGGLoss(features=stack).to(dev)
    x = torch.rand(4, 3, 64, 64, generator=g).to(dev)
    y = (x + 0.2 * torch.randn(4, 3, 64, 64, generator=g).to(dev)).clamp(0, 1)

    def step(fn):
        def run():
            xd = x.clone().requires_grad_(True)
            loss = fn(xd, y)
            loss.backward()
            return loss.detach(), xd.grad
        return run

    t, outs = compare({"device": step(mine), "torch": step(theirs)}, max(args.reps, 20))
    flops = conv_flops(mine.features.layers, 8, 64, 64) + conv_flops(mine.features.layers, 4, 64, 64)
    result["vgg_loss_4x64x64_fwd_bwd"] = dict(
        **t, ratio_torch_over_device=t["torch"]["median_ms"] / t["device"]["median_ms"], conv_tflop=flops / 1e12,
        device_tflops=flops / t["device"]["median_ms"] / 1e9,
        loss_rel_difference=float((outs["device"][0] - outs["torch"][0]).abs() / outs["torch"][0].abs()),
        grad_rel_difference_l2=float((outs["device"][1] - outs["torch"][1]).norm() / outs["torch"][1].norm()))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
