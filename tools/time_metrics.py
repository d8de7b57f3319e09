"""Time the image-metric kernels (diner_amd.metrics.image_metrics, uint8 route) against the host restatement (tests/metrics_host.py).

    python tools/time_metrics.py [--reps 20]

Per configuration (800x600 and 1024x1024 pairs, batches of 1 and 16) it prints one JSON line: the device time per pair (HIP events
around `reps` calls after warm-up, kernels + workspace allocation) and the host restatement's time per pair (numpy, one pass)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diner_amd.metrics import image_metrics          # noqa: E402
from diner_amd.synthetic import metric_pair          # noqa: E402
from tests.metrics_host import host_metrics          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-pairs", type=int, default=2, help="pairs the host restatement is timed on")
    a = ap.parse_args()
    for H, W in ((600, 800), (1024, 1024)):
        for N in (1, 16):
            pairs = [metric_pair("smooth", H, W, 500 + i) for i in range(N)]
            P = torch.from_numpy(np.stack([p for p, _ in pairs])).cuda()
            G = torch.from_numpy(np.stack([g for _, g in pairs])).cuda()
            for _ in range(3):
                image_metrics(P, G)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                image_metrics(P, G)
            e1.record()
            torch.cuda.synchronize()
            dev_us = e0.elapsed_time(e1) * 1e3 / a.reps / N
            t = time.perf_counter()
            for p, g in pairs[:a.host_pairs]:
                host_metrics(p, g)
            host_us = (time.perf_counter() - t) * 1e6 / min(a.host_pairs, N)
            print(json.dumps(dict(H=H, W=W, batch=N, device_us_per_pair=round(dev_us, 2), host_us_per_pair=round(host_us, 1),
                                  reps=a.reps, device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
