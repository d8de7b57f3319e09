"""Time the depth estimator's feature transformer in training -- forward and backward -- on the kernels (csrc/fmt.hip: diner_fmt_kv_f32,
diner_fmt_layer_f32; csrc/fmt_grad.hip: diner_fmt_layer_grad_f32) and on the torch route that training ran before (DeviceFMT.forward
under autograd, view by view), on the same device.

    python tools/time_fmt_train.py                    # the FMT at the training step's shape, the entry's kernels, one fit step at 256 x 320
    python tools/time_fmt_train.py --calls 5 --skip-fit

In one process.  The FMT's forward + backward at the step's shape -- stage 1 of 64 x 80 (5120 tokens), five views, B 1 -- under fixed
upstream gradients, DeviceFMT.encode with fmt_kernels against the same call with the switch off (the reference's schedule, one view at
a time), with HIP events, 3 warm-up calls a route, then torch / kernels / torch / kernels ... alternating, the median with min - max, the
torch route's two halves against each other (A/A), and torch.cuda.max_memory_allocated of one call of each route above what was
allocated before.  Then the gradient entry alone on the reference view's self layer (1 x 5120) and on the source views' cross layer
(4 x 5120 reading 1 x 5120): the median of `calls` back-to-back calls after 3 warm-up calls, all outputs and each output alone, beside
the bytes the call must move (x, dy, d_x, the source and d_source once each) at 4 TB/s -- a bound the kernels are not expected to be
near at this size: the call is four launches of at most 160 workgroups.  Then one fine-tuning step of DeviceTransMVSNet (forward in
training mode, focal_loss_bld, backward, DeviceAdam; fused_readout, match_kernels and deform_kernels on in both) with and without
fmt_kernels, alternating, and FMT_with_pathway's share of that step on both routes.  Inputs are seeded noise; needs a HIP device."""
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

HBM_RATE = 4.0e12                  # bytes/s, the streaming rate the byte bound is stated at


def transformer(calls, dev, g, hw=(64, 80), nv=NS + 1):
    H, W = hw
    torch.manual_seed(0)
    net = mvs.DeviceFMT().to(dev).train()
    maps = [torch.randn(1, 32, H, W, generator=g).to(dev).requires_grad_(True) for _ in range(nv)]
    ups = [torch.randn(1, 32, H, W, generator=g).to(dev) for _ in range(nv)]

    def run(switch):
        net.fmt_kernels = switch
        net.zero_grad(set_to_none=True)
        for m in maps:
            m.grad = None
        ref, sources = net.encode(maps[0], maps[1:])
        torch.autograd.backward([ref] + list(sources), ups)

    print(f"FMT forward + backward, {nv} views of {H} x {W} ({H * W} tokens), B 1: 4 self layers on the reference view, 8 layers on each source view",
          flush=True)
    report("FMT fwd + bwd", lambda: run(True), lambda: run(False), calls)
    net.fmt_kernels = False


def entry(calls, dev, g, L=5120, ns=NS):
    torch.manual_seed(0)
    layer = mvs._EncoderLayer(32, 8).to(dev)
    pack = ops.pack_fmt_layer(layer.state_dict())
    med = lambda fn: statistics.median(([fn() for _ in range(3)], timed(fn, calls))[1])
    for label, N, R in (("self layer, the reference view", 1, 1), ("self layer, the source views", ns, ns), ("cross layer, the source views", ns, 1)):
        x = torch.randn(N, L, 32, generator=g).to(dev)
        source = x if N == R else torch.randn(R, L, 32, generator=g).to(dev)
        dy = torch.randn(N, L, 32, generator=g).to(dev)
        state = ops.fmt_kv(source, pack)
        tokens = 4 * 32 * L
        nbytes = 3 * N * tokens + (0 if source is x else 2 * R * tokens)
        tq, ts = ops.fmt_grad_slabs(N, L, R, L)
        print(f"  {label}: x ({N},{L},32), source ({R},{L},32); {N * -(-L // ops.FMT_GRAD_TOKENS)} + {R * -(-L // ops.FMT_GRAD_TOKENS)} tiles in {tq} + {ts} "
              f"workgroups; x, dy, d_x (and the source, d_source) once each are {nbytes / 1e6:.2f} MB: {nbytes / HBM_RATE * 1e6:.2f} us at "
              f"{HBM_RATE / 1e12:.0f} TB/s", flush=True)
        for what, want in (("all outputs (query, state, source, finish)", (True, True, True)), ("d_x alone", (True, False, False)),
                           ("d_source alone", (False, True, False)), ("the parameter block alone", (False, False, True))):
            ms = med(lambda: ops.fmt_layer_grad(x, source, pack, state, dy, want=want))
            print(f"    {what:46s} {ms * 1e3:9.1f} us  {100 * nbytes / HBM_RATE * 1e3 / ms:5.2f} % of the byte bound", flush=True)
        ms = med(lambda: ops.fmt_layer(x, pack, ops.fmt_kv(source, pack)))
        print(f"    {'forward (fmt_kv + fmt_layer, out of place)':46s} {ms * 1e3:9.1f} us", flush=True)


def fit_step(calls, dev, g, hw=(256, 320), nv=NS + 1):
    from diner_amd.optim import DeviceAdam
    H, W = hw
    torch.manual_seed(0)
    model = estimator.DeviceTransMVSNet().to(dev).train()
    model.fused_readout, model.match_kernels, model.deform_kernels = True, True, True
    opt = DeviceAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-4, skip_nonfinite=True)
    imgs = torch.rand(1, nv, 3, H, W, generator=g).to(dev)
    proj = {f"stage{i + 1}": cameras(1, H // s, W // s, s, dev, g) for i, s in enumerate((4, 2, 1))}
    depth_values = torch.linspace(1.2, 1.9, 192).view(1, -1).to(dev)
    gts = {f"stage{i + 1}": (1.2 + 0.7 * torch.rand(1, H // s, W // s, generator=g)).to(dev) for i, s in enumerate((4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}
    feats = [{k: torch.randn(1, c, H // s, W // s, generator=g).to(dev) for k, c, s in (("stage1", 32, 4), ("stage2", 16, 2), ("stage3", 8, 1))}
             for _ in range(nv)]

    def step(switch):
        model.fmt_kernels = switch
        out = model(imgs, proj, depth_values, depth_interval=0.7 / 192)
        terms = estimator.focal_loss_bld(out, gts, masks, 0.7 / 192, dlossw=(1, 1, 1))
        terms[0].backward()
        opt.step(zero_grads=True)

    def fmt_only(switch):
        model.fmt_kernels = switch
        out = model.FMT_with_pathway([dict(f) for f in feats])
        keys = ("stage1", "stage2", "stage3")
        torch.autograd.backward([o[k] for o in out for k in keys], [torch.ones_like(o[k]) for o in out for k in keys])
        model.zero_grad(set_to_none=True)

    print(f"one fine-tuning step: {nv} views of {H} x {W}, ndepths {model.ndepths}, training mode, fused_readout, match_kernels, deform_kernels, "
          f"DeviceAdam", flush=True)
    t = alternate({"default": lambda: step(False), "fmt": lambda: step(True)}, 2 * calls)
    ta, tb = t["default"][0::2], t["default"][1::2]
    aa = abs(statistics.median(ta) - statistics.median(tb)) / statistics.median(t["default"])
    print(f"  default {fmt(t['default'])}  fmt_kernels {fmt(t['fmt'])}  default / fmt_kernels {statistics.median(t['default']) / statistics.median(t['fmt']):5.3f}"
          f"  default A/A {100 * aa:.1f} %  peak default {peak_of(lambda: step(False)):8.1f} MiB  fmt_kernels {peak_of(lambda: step(True)):8.1f} MiB",
          flush=True)
    t = alternate({"default": lambda: fmt_only(False), "fmt": lambda: fmt_only(True)}, 2 * calls)
    print(f"  FMT_with_pathway's share of that step (its forward + backward alone, the pathway on torch in both): default {fmt(t['default'])}  "
          f"fmt_kernels {fmt(t['fmt'])}", flush=True)
    model.fmt_kernels = False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/time_fmt_train.py needs a HIP device"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    print(f"device {torch.cuda.get_device_name(0)}; medians of {2 * args.calls} alternating calls (min - max)")
    transformer(args.calls, dev, g)
    entry(args.calls, dev, g)
    if not args.skip_fit:
        fit_step(args.calls, dev, g)


if __name__ == "__main__":
    main()
