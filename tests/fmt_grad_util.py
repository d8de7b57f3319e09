"""Shared by tools/make_golden_fmt_grad.py, tests/test_fmt_grad_cpu.py and tests/test_fmt_grad_gpu.py: the seeded inputs of fixture G35
(regenerated, never stored), the case tables, the runs that turn a case into the feature transformer's gradients, and the condition on
the inputs.

Single-layer cases: one encoder layer of fmt_util.fmt_state_dict(seed + 50) (every bias and LayerNorm affine non-trivial) on N(0,1)
tokens under a seeded N(0,1) cotangent; all eighteen gradients (d_x, d_source, the sixteen parameters).  Whole-stack cases: the FMT's
reference view and source views (and, for the pathway runs, the two finer stages) under seeded cotangents at every output.

The condition on the inputs: the ReLU is a kink.  Where float32 and float64 disagree on the sign of a linear1 output the gradient jumps
and no bar means anything, so every case must keep the smallest |linear1 output| in float64 at least KINK_FACTOR times the largest
|float32 - float64| of those outputs, with nothing excluded (kink_ratio >= 1).  The seeds below were picked for it; see DESIGN.md 8t."""
import functools
import os

import numpy as np
import torch

from tests import fmt_util as FU
from tests import mvs_util as MU

FIXTURE = os.path.join(MU.ROOT, "tests", "golden", "g35_fmt_grad.npz")
BAR_FACTOR = MU.BAR_FACTOR
KINK_FACTOR = 4.0
SEED_OFFSET = 3500                  # the cotangents' generator: the case's seed + this
SHORT = ("wq", "wk", "wv", "wo", "w1", "w2", "bq", "bk", "bv", "bo", "g1", "be1", "b1", "b2", "g2", "be2")     # mvs.FMT_LAYER_SHORT
LAYER_OUTPUTS = ("d_x", "d_source") + SHORT

# name: x (N, L), source (R, S) or None for a self layer, the layer of the stack whose weights it takes, seed, the slab counts it is run with
LAYER_CASES = {
    "self_tiny": dict(N=1, L=35, source=None, layer=0, seed=3521, slabs=(0,)),             # fewer tokens than a tile, both paths into one d_x
    "self_ragged": dict(N=2, L=851, source=None, layer=2, seed=3535, slabs=(0,)),          # 7 tiles, the last of 83 tokens; two images
    "cross_views": dict(N=6, L=129, source=(2, 600), layer=1, seed=3542, slabs=(0,)),      # L != S, one token alone in tile 2, 3 images a row
    "cross_blocks": dict(N=1, L=2080, source=(1, 2080), layer=3, seed=3557, slabs=(0, 3, 1)),   # 17 tiles, the last of 32 tokens; forced slabs
}
# name: B, NV, stage-1 (H, W), seed
STACK_CASES = {
    "stack_tiny": dict(B=1, NV=2, hw=(5, 7), seed=3101),
    "stack_views": dict(B=2, NV=3, hw=(9, 15), seed=3103),
}


# ---- single layers -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_inputs(name):
    """-> dict of float32 CPU tensors x (N,L,32), source (R,S,32) or None (a self layer), dy (N,L,32) and the layer's state dict under
    ops.FMT_LAYER_KEYS.  Treat it as read-only."""
    c = LAYER_CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    x = torch.randn(c["N"], c["L"], 32, generator=g)
    source = None if c["source"] is None else torch.randn(*c["source"], 32, generator=g)
    dy = torch.randn(c["N"], c["L"], 32, generator=torch.Generator().manual_seed(c["seed"] + SEED_OFFSET))
    prefix = f"FMT.layers.{c['layer']}."
    sd = {k[len(prefix):]: v for k, v in FU.fmt_state_dict(c["seed"] + 50).items() if k.startswith(prefix)}
    return dict(x=x, source=source, dy=dy, state_dict=sd)


def _leaf(t, dtype, device):
    return t.to(dtype=dtype, device=device).clone().requires_grad_(True)


def make_layer(name, dtype=torch.float32, device=None, cls=None):
    """The case's encoder layer (mvs._EncoderLayer, or `cls(32, 8)` with the same keys) in `dtype`."""
    from diner_amd import mvs
    layer = (cls or mvs._EncoderLayer)(32, 8)
    layer.load_state_dict(layer_inputs(name)["state_dict"])
    return layer.to(dtype=dtype, device=device)


def layer_parameters(layer):
    a = layer.attention
    return (a.query_projection.weight, a.key_projection.weight, a.value_projection.weight, a.out_projection.weight, layer.linear1.weight,
            layer.linear2.weight, a.query_projection.bias, a.key_projection.bias, a.value_projection.bias, a.out_projection.bias,
            layer.norm1.weight, layer.norm1.bias, layer.linear1.bias, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias)


def run_layer(name, dtype=torch.float64, device=None, fn=None, layer=None, hidden=None):
    """fn(x, source, layer) (default: the layer's own forward with the source repeated over the images that share it) on the case in
    `dtype`, and its backward under dy -> dict(y, d_x, d_source (absent for a self layer), the sixteen parameter gradients).  hidden: a
    list that receives the linear1 outputs."""
    inp = layer_inputs(name)
    layer = layer if layer is not None else make_layer(name, dtype, device)
    x = _leaf(inp["x"], dtype, device)
    source = x if inp["source"] is None else _leaf(inp["source"], dtype, device)
    handle = layer.linear1.register_forward_hook(lambda m, i, o: hidden.append(o.detach())) if hidden is not None else None
    if fn is None:
        fn = lambda x, s, ly: ly(x, s if s is x else s.repeat(x.shape[0] // s.shape[0], 1, 1))
    y = fn(x, source, layer)
    if handle is not None:
        handle.remove()
    params = layer_parameters(layer)
    leaves = [x] + ([] if source is x else [source]) + list(params)
    grads = torch.autograd.grad(y, leaves, inp["dy"].to(dtype=dtype, device=device))
    out = dict(y=y.detach(), d_x=grads[0])
    if source is not x:
        out["d_source"] = grads[1]
    out.update(zip(SHORT, grads[-16:]))
    return out


def closed_form(name, dtype=torch.float64, device=None):
    from diner_amd import mvs
    inp = layer_inputs(name)
    layer = make_layer(name, dtype, device)
    x = inp["x"].to(dtype=dtype, device=device)
    source = x if inp["source"] is None else inp["source"].to(dtype=dtype, device=device)
    d_x, d_source, grads = mvs.fmt_layer_grad_torch(x, source, dict(zip(SHORT, layer_parameters(layer))), inp["dy"].to(dtype=dtype, device=device))
    out = dict(d_x=d_x, **grads)
    if d_source is not None:
        out["d_source"] = d_source
    return out


def layer_outputs(name):
    return tuple(k for k in LAYER_OUTPUTS if k != "d_source" or LAYER_CASES[name]["source"] is not None)


@functools.lru_cache(maxsize=None)
def layer_expected64(name):
    """Float64 autograd through the layer on the CPU, computed once per session and shared; treat it as read-only."""
    return run_layer(name, torch.float64)


def kink_ratio(hidden32, hidden64):
    """min |linear1 output| in float64 over KINK_FACTOR max |float32 - float64| of those outputs, over all the calls of a run: the condition
    holds where this is >= 1."""
    assert len(hidden32) == len(hidden64) and len(hidden64) > 0
    smallest = min(float(h.abs().min()) for h in hidden64)
    apart = max(float((a.double() - b).abs().max()) for a, b in zip(hidden32, hidden64))
    return smallest / (KINK_FACTOR * apart)


def layer_kink_ratio(name):
    h32, h64 = [], []
    run_layer(name, torch.float32, hidden=h32)
    run_layer(name, torch.float64, hidden=h64)
    return kink_ratio(h32, h64)


# ---- the whole stack -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stack_inputs(name):
    """-> (state dict of the 132 keys, per view {"stage1", "stage2", "stage3"}, per view the cotangents under the same keys), float32 on
    the CPU.  The stage-1 features come view by view from Generator(seed), the finer stages from Generator(seed + 1000), the weights are
    fmt_util.fmt_state_dict(seed + 50)."""
    c = STACK_CASES[name]
    B, (H, W) = c["B"], c["hw"]
    g, fine = torch.Generator().manual_seed(c["seed"]), torch.Generator().manual_seed(c["seed"] + 1000)
    feats = [{"stage1": torch.randn(B, 32, H, W, generator=g), "stage2": torch.randn(B, 16, 2 * H, 2 * W, generator=fine),
              "stage3": torch.randn(B, 8, 4 * H, 4 * W, generator=fine)} for _ in range(c["NV"])]
    g = torch.Generator().manual_seed(c["seed"] + SEED_OFFSET)
    ups = [{k: torch.randn(v.shape, generator=g) for k, v in f.items()} for f in feats]
    return FU.fmt_state_dict(c["seed"] + 50), feats, ups


def make_stack(name, dtype=torch.float32, device=None, module=None):
    from diner_amd import mvs
    net = module if module is not None else mvs.DeviceFMTWithPathway(8)
    net.load_state_dict(stack_inputs(name)[0])
    return net.to(dtype=dtype, device=device).train()


def _hook_hidden(fmt, hidden):
    return [ly.linear1.register_forward_hook(lambda m, i, o: hidden.append(o.detach())) for ly in fmt.layers]


def run_encode(name, dtype=torch.float64, device=None, fmt_kernels=False, module=None, hidden=None):
    """The transformer alone, in training mode: DeviceFMT.encode (or, for `module` = the reference's FMT_with_pathway, its FMT called view
    by view as FMT_with_pathway.forward calls it) and the backward under the stage-1 cotangents -> {"out_<v>": output, "in_<v>": the
    gradient at view v's input map, "param_<key>": the gradient at each of the 128 FMT parameters}."""
    _, feats, ups = stack_inputs(name)
    net = make_stack(name, dtype, device, module)
    fmt = net.FMT
    if module is None:
        net.fmt_kernels = fmt_kernels
    handles = _hook_hidden(fmt, hidden) if hidden is not None else []
    maps = [_leaf(f["stage1"], dtype, device) for f in feats]
    if module is None:
        ref, sources = fmt.encode(maps[0], maps[1:])
        outs = [ref] + list(sources)
    else:
        refs = fmt(maps[0].clone(), feat="ref")
        outs = [refs[-1]] + [fmt([r.clone() for r in refs], m.clone(), feat="src") for m in maps[1:]]
    for h in handles:
        h.remove()
    sum((o * u["stage1"].to(dtype=dtype, device=device)).sum() for o, u in zip(outs, ups)).backward()
    res = {f"out_{v}": o.detach() for v, o in enumerate(outs)}
    res.update({f"in_{v}": m.grad for v, m in enumerate(maps)})
    res.update({"param_" + k: p.grad for k, p in fmt.named_parameters()})
    return res


def run_pathway(name, dtype=torch.float64, device=None, fmt_kernels=False, module=None):
    """DeviceFMTWithPathway.forward (or the reference's FMT_with_pathway as `module`) in training mode and the backward under the
    cotangents of all three stages of every view -> {"<stage>_<v>": output, "in_<stage>_<v>": the gradient at that input, "param_<key>":
    the gradient at each of the 132 parameters}."""
    _, feats, ups = stack_inputs(name)
    net = make_stack(name, dtype, device, module)
    if module is None:
        net.fmt_kernels = fmt_kernels
    leaves = [{k: _leaf(v, dtype, device) for k, v in f.items()} for f in feats]
    out = net([dict(f) for f in leaves])
    sum((o[k] * u[k].to(dtype=dtype, device=device)).sum() for o, u in zip(out, ups) for k in FU.STAGES).backward()
    res = {f"{k}_{v}": o[k].detach() for v, o in enumerate(out) for k in FU.STAGES}
    res.update({f"in_{k}_{v}": f[k].grad for v, f in enumerate(leaves) for k in FU.STAGES})
    res.update({"param_" + k: p.grad for k, p in net.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def encode_expected64(name):
    return run_encode(name, torch.float64)


@functools.lru_cache(maxsize=None)
def pathway_expected64(name):
    return run_pathway(name, torch.float64)


def stack_kink_ratio(name):
    h32, h64 = [], []
    run_encode(name, torch.float32, hidden=h32)
    run_encode(name, torch.float64, hidden=h64)
    return kink_ratio(h32, h64)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def bar(fx, name, key):
    return BAR_FACTOR * float(fx[f"{name}_err_{key}"])


def stack_bars(fx, name, kind):
    """kind "encode" or "pathway" -> {output: bar}."""
    return {str(k): BAR_FACTOR * float(e) for k, e in zip(fx[f"{name}_{kind}_keys"], fx[f"{name}_{kind}_errs"])}


SAMPLES = 24


def sample(t):
    """A strided sub-sample of at most SAMPLES + 8 values, as a float64 array."""
    flat = t.detach().cpu().double().reshape(-1).numpy()
    return flat[::max(1, flat.size // SAMPLES) | 1].copy()


def input_hash():
    """sha256 over every case's regenerated inputs."""
    from tools.make_golden_mvs import sha256_of
    layers = [{k: v for k, v in layer_inputs(n).items() if v is not None} for n in LAYER_CASES]
    return sha256_of(layers + [list(stack_inputs(n)) for n in STACK_CASES])
