"""HIP-event timing of the compositor on one 800 x 600 frame (480 000 rays x 128 samples) through diner_amd.ops: the plain entry, the aux
entry (opacity + depth spread) and the route the aux entry replaces (weights written out + a torch sum); three
alternating rounds, median / min / max of 20 calls each (host enqueue and the output allocations included)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diner_amd import ops
NR, K = 480000, 128
g = torch.Generator().manual_seed(1)
field = torch.rand(NR, K, 4, generator=g).cuda(); field[..., 3] *= 20
z = (0.5 + torch.rand(NR, K, generator=g)).sort(-1).values.cuda()
rays = torch.zeros(NR, 8).cuda(); rays[:, 6] = 0.5; rays[:, 7] = 1.5
def t(fn, n=20):
    for _ in range(5): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(n):
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    ts.sort(); return ts[len(ts) // 2], ts[0], ts[-1]
for rnd in range(3):
    for name, fn in (("plain", lambda: ops.composite(field, z, rays, True, want_weights=False)),
                     ("aux", lambda: ops.composite(field, z, rays, True, want_weights=False, want_aux=True)),
                     ("weights+sum", lambda: ops.composite(field, z, rays, True, want_weights=True)[0].sum(-1))):
        med, lo, hi = t(fn)
        print(f"round {rnd} {name}: median {med*1e3:.1f} us (min {lo*1e3:.1f}, max {hi*1e3:.1f})", flush=True)
