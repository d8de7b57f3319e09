"""The yardstick of the optimiser tests: torch.optim.Adam / AdamW's update (torch/optim/adam.py, single-tensor route) restated in float64,
with the gradient statistics, clip_grad_norm_'s clipping and the skip of a non-finite step, and the inputs the GPU tests share."""
import math

import torch

CHUNK = 4096          # DINER_OPTIM_CHUNK
SIZES = [1, 3, 4, 5, 512, 4 * 512, 55 * 512, 3 * CHUNK + 5, 512 * 512, 0]          # the last one is empty
HYPERS = [dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False),          # the reference's
          dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=False),
          dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=True)]


def adam64(p, g, m, v, t, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None,
           skip_nonfinite=False):
    """One step t (1-based, the step being taken) over lists of float64 tensors -> (p, m, v, info); inputs are not modified.
    info: grad_norm, nonfinite, clip, skipped."""
    p, g, m, v = ([x.detach().to(torch.float64).clone() for x in xs] for xs in (p, g, m, v))
    sumsq = sum(float((x * x).sum()) for x in g)
    nonfinite = sum(int((~torch.isfinite(x)).sum()) for x in g)
    norm = math.sqrt(sumsq) if sumsq == sumsq else float("nan")
    info = dict(grad_norm=norm, nonfinite=nonfinite, clip=1.0, skipped=False)
    if skip_nonfinite and nonfinite:
        info.update(skipped=True, clip=0.0)
        return p, m, v, info
    if max_grad_norm is not None:
        info["clip"] = min(1.0, max_grad_norm / (norm + 1e-6))
        g = [x * info["clip"] for x in g]
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for k in range(len(p)):
        if decoupled:
            p[k] = p[k] * (1.0 - lr * weight_decay)
        elif weight_decay != 0:
            g[k] = g[k] + weight_decay * p[k]
        m[k] = m[k] + (g[k] - m[k]) * (1.0 - b1)
        v[k] = b2 * v[k] + (1.0 - b2) * g[k] * g[k]
        p[k] = p[k] - (lr / bc1) * m[k] / (v[k].sqrt() / math.sqrt(bc2) + eps)
    return p, m, v, info


def make_inputs(seed, sizes=SIZES, steps=3):
    """-> (params, grads): params N(0,1) with a few at +-50; grads[s][k] for step s: magnitudes 10^U(-12, 2), random signs, ~1 % exact
    zeros.  float32 CPU tensors; the test moves them."""
    gen = torch.Generator().manual_seed(seed)
    params, grads = [], [[] for _ in range(steps)]
    for n in sizes:
        p = torch.randn(n, generator=gen)
        if n >= 512:
            idx = torch.randint(0, n, (4,), generator=gen)
            p[idx] = torch.tensor([50.0, -50.0, 50.0, -50.0])
        params.append(p)
        for s in range(steps):
            mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 14.0 - 12.0)
            sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).to(torch.float64)
            g = (mag * sign).to(torch.float32)
            g[torch.rand(n, generator=gen) < 0.01] = 0.0
            grads[s].append(g)
    return params, grads


def errors(p, m, v, p64, m64, v64, lr):
    """(e_p, e_m, e_v) over lists of tensors: max |p - p64| / lr; max-norm relative error of the moments."""
    cat = lambda xs: torch.cat([x.detach().reshape(-1).cpu().to(torch.float64) for x in xs])
    P, M, V, P64, M64, V64 = (cat(x) for x in (p, m, v, p64, m64, v64))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    return float((P - P64).abs().max()) / lr, rel(M, M64), rel(V, V64)


def floors(p64, lr):
    """float32 rounding of the stored values: 2^-22 max|p64| / lr for e_p, 2^-22 for e_m and e_v."""
    pmax = max(float(x.abs().max()) for x in p64 if x.numel())
    return 2.0 ** -22 * pmax / lr, 2.0 ** -22, 2.0 ** -22
