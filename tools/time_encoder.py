"""Time the image encoder's trunk on the torch / MIOpen route and on the device route (diner_amd.encoder.DeviceTrunk).

    python tools/time_encoder.py                  # 4 x 800x600 and 16 x 400x300, the two routes alternating
    python tools/time_encoder.py --shapes 1x4x600x800 --calls 10

Per shape (SB x NV x H x W): HIP events around SpatialEncoder.forward in eval mode under no_grad, 3 warm-up calls a route, then the two
routes alternating, the median of `--calls` with min - max; torch.cuda.max_memory_allocated of one call of each route; the trunk's
FLOPs (2 K Cout per output pixel of every convolution, counted from the shapes) over the device route's time beside the 157 TFLOP/s
fp32 matrix peak; the device route's launches timed one by one (events around each), summed per kind; and the first call of each route
in a fresh process (host clock around the call and a synchronise: it holds the weight packing or MIOpen's kernel search).  The weights
are seeded, not trained: the time does not depend on them.  Needs a HIP device; there is no CPU path."""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3              # fp32 matrix peak of the MI355X


def parse_shape(s):
    sb, nv, h, w = (int(v) for v in s.split("x"))
    return sb, nv, h, w


def make_encoder(seed=0):
    from src.models.image_encoder import SpatialEncoder
    torch.manual_seed(seed)
    enc = SpatialEncoder(pretrained=False, image_padding=64, padding_pe=4)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.uniform_(0.5, 1.5)
                m.running_mean.normal_(0.0, 0.1)
    return enc.cuda().eval()


def trunk_flops(N, H, W, pad=64, stem_cin=21):
    """2 x multiply-adds of the 29 convolutions of resnet34 up to layer3 on N images of H x W padded by `pad`."""
    h, w = (H + 2 * pad - 1) // 2 + 1, (W + 2 * pad - 1) // 2 + 1
    total = 2 * 49 * stem_cin * 64 * h * w
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cin = 64
    for c, blocks in ((64, 3), (128, 4), (256, 6)):
        if c != 64:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            total += 2 * cin * c * h * w                        # the 1 x 1 downsample
        total += 2 * 9 * cin * c * h * w + 2 * 9 * c * c * h * w * (2 * blocks - 1)
        cin = c
    return N * total


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(enc, imgs):
    """The device route's launches of one call, each between two events: {kind: (count, ms)}."""
    from diner_amd import ops
    log, saved = [], {}

    def wrap(name):
        fn = getattr(ops, name)

        def inner(x, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = fn(x, *a, **k)
            e1.record()
            kind = name
            if name == "conv_s2":
                kind = f"conv_s2 {a[3]}x{a[3]} {x.shape[3]}->{a[2]}"
            elif name == "conv3x3":
                kind = f"conv3x3 {x.shape[3]}->{a[2]}"
            elif name == "pyramid_level":
                kind = f"pyramid_level {x.shape[3]} ch"
            log.append((kind, e0, e1))
            return y
        saved[name] = fn
        setattr(ops, name, inner)

    for name in ("encoder_input", "conv_s2", "conv3x3", "maxpool3s2", "pyramid_level"):
        wrap(name)
    try:
        with torch.no_grad():
            enc(imgs, None, None, None)
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    out = collections.OrderedDict()
    for kind, e0, e1 in log:
        n, ms = out.get(kind, (0, 0.0))
        out[kind] = (n + 1, ms + e0.elapsed_time(e1))
    return out


def first_call(route, shape):
    sb, nv, h, w = shape
    enc = make_encoder()
    enc.device_trunk = route == "device"
    imgs = torch.rand(sb, nv, 3, h, w, device="cuda") * 2 - 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        enc(imgs, None, None, None)
    torch.cuda.synchronize()
    print(json.dumps({"first_call_ms": (time.perf_counter() - t0) * 1e3, "route": route}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="1x4x600x800,4x4x300x400", help="comma-separated SBxNVxHxW")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--first-call", choices=("torch", "device"), default=None, help="(internal) time the first call of a route and exit")
    ap.add_argument("--no-first-call", action="store_true", help="skip the two fresh-process runs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_encoder.py needs a HIP device: a time taken anywhere else says nothing")
    shapes = [parse_shape(s) for s in args.shapes.split(",")]
    if args.first_call:
        return first_call(args.first_call, shapes[0])
    enc = make_encoder()
    results = []
    for sb, nv, h, w in shapes:
        imgs = torch.rand(sb, nv, 3, h, w, device="cuda") * 2 - 1

        def run(route):
            enc.device_trunk = route == "device"
            with torch.no_grad():
                enc(imgs, None, None, None)

        ms, peak = {"torch": [], "device": []}, {}
        for route in ms:
            for _ in range(args.warmup):
                run(route)
        torch.cuda.synchronize()
        for _ in range(args.calls):
            for route in ms:
                ms[route].append(timed(lambda: run(route)))
        for route in ms:
            enc.latent = torch.empty(1, 1, 1, 1, device="cuda")
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            run(route)
            torch.cuda.synchronize()
            peak[route] = (torch.cuda.max_memory_allocated(), base)
        run("device")
        lat_dev = enc.latent.clone()
        run("torch")
        diff = float((lat_dev - enc.latent).abs().max() / enc.latent.abs().max())
        flops = trunk_flops(sb * nv, h, w)
        res = dict(shape=f"{sb}x{nv}x{h}x{w}", calls=args.calls, flops=flops, routes_max_rel_diff=diff)
        print(f"== {sb} x {nv} images of {w} x {h}: trunk {flops / 1e12:.3f} TFLOP, latent {tuple(enc.latent.shape)}, routes differ by {diff:.2e} of the maximum")
        for route in ms:
            med = statistics.median(ms[route])
            res[route] = dict(median_ms=med, min_ms=min(ms[route]), max_ms=max(ms[route]), peak_bytes=peak[route][0], resident_before_bytes=peak[route][1])
            print(f"   {route:6s}  median {med:8.3f} ms  (min {min(ms[route]):8.3f} - max {max(ms[route]):8.3f})  peak {peak[route][0] / 2 ** 20:8.1f} MiB "
                  f"(resident before the call {peak[route][1] / 2 ** 20:7.1f} MiB)  {flops / med / 1e9:6.1f} TFLOP/s = "
                  f"{100 * flops / med / 1e9 / PEAK_TFLOPS:4.1f} % of the fp32 matrix peak")
        enc.device_trunk = True
        per = launches(enc, imgs)
        total = sum(v[1] for v in per.values())
        print(f"   device route, launches one by one ({sum(v[0] for v in per.values())} launches, {total:.3f} ms between their events):")
        for kind, (n, t) in sorted(per.items(), key=lambda kv: -kv[1][1]):
            print(f"      {kind:28s} x {n:2d}  {t:8.3f} ms  {100 * t / total:5.1f} %")
        res["launches"] = {k: dict(count=n, ms=t) for k, (n, t) in per.items()}
        results.append(res)
    if not args.no_first_call:
        for route in ("torch", "device"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-call", route, "--shapes", args.shapes.split(",")[0]],
                                 capture_output=True, text=True, timeout=400)
            line = [l for l in out.stdout.splitlines() if l.startswith("{")]
            if out.returncode != 0 or not line:
                raise SystemExit(f"the first-call child of the {route} route failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
            fc = json.loads(line[-1])
            print(f"== first call in a fresh process, {args.shapes.split(',')[0]}, {route} route: {fc['first_call_ms']:.1f} ms")
            results.append(fc)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
