"""Shared by tools/make_golden_deform_grad.py, tests/test_deform_grad_cpu.py and tests/test_deform_grad_gpu.py: the seeded inputs of fixture
G34 (regenerated, never stored), the case table, the runs that turn a case into the deformable convolution's gradients, and the names
under which the fixture keeps them.

Layer cases: the inputs of the LAST deformable layer of each head (out1.7: Cout 32, out2.7: Cout 16, out3.7: Cout 8, all Cin 32) on
featurenet_util's "tiny" and "ragged" images -- the activations and the raw conv_offset_mask output a seeded FeatureNet really hands that
layer, with the layer's own weight -- under a seeded normal upstream gradient.  Synthetic cases: the other channel counts, a forced slab
count, the fresh layer (offmask zero) and planted non-finite offsets.  Net cases: one whole FeatureNet training step (batch statistics),
loss = sum over the stages of sum(g_stage output_stage), gradients at every parameter."""
import functools
import os

import numpy as np
import torch

from tests import featurenet_util as FU
from tests import mvs_util as MU

FIXTURE = os.path.join(MU.ROOT, "tests", "golden", "g34_deform_grad.npz")
BAR_FACTOR = MU.BAR_FACTOR
SEED_OFFSET = 3400                  # the upstream gradients' generator: the case's seed + this
OUTPUTS = ("d_x", "d_offmask", "d_weight", "d_bias")
LAYER_OF_COUT = {32: "out1.7", 16: "out2.7", 8: "out3.7"}
# the seeded FeatureNet whose layers the images run through: chosen so that, on all three layers, float32 and float64 agree on `inside`
# and on both floors of every sample (margin_holds) -- on "ragged", featurenet_util's own seed 3152 leaves one sample of out2.7 that does not
LAYER_NET_SEED = {"tiny": 3151, "ragged": 3422}

# synthetic: N, (H, W), Cin, Cout, seed, slabs (0: the default), kind
SYNTHETIC = {
    "syn_8_1": dict(N=2, hw=(7, 9), Cin=8, Cout=1, seed=3411, slabs=0, kind="random"),          # one partial tile an image, PER = 8 rows an add
    "syn_16_27": dict(N=1, hw=(17, 18), Cin=16, Cout=27, seed=3412, slabs=3, kind="random"),    # 306 pixels: 5 tiles, walked 2 + 2 + 1
    "syn_64_64": dict(N=1, hw=(5, 13), Cin=64, Cout=64, seed=3413, slabs=0, kind="random"),     # 65 pixels: a tile of one pixel; the largest
    "zero": dict(N=1, hw=(6, 10), Cin=32, Cout=32, seed=3414, slabs=0, kind="zero"),            # the fresh DCN: integer coordinates, m = 0.5
    "planted": dict(N=2, hw=(6, 10), Cin=32, Cout=16, seed=3415, slabs=0, kind="planted"),      # NaN, +-inf, +-1e30 under finite logits
}
LAYER_CASES = tuple(f"{img}_{cout}" for img in ("tiny", "ragged") for cout in (32, 16, 8))
CASE_NAMES = LAYER_CASES + tuple(SYNTHETIC)
NET_CASES = ("tiny", "ragged")
# (image, pixel row, pixel column, tap, which offset: 0 row / 1 column, the value planted)
PLANTED = ((0, 0, 0, 0, 0, float("nan")), (0, 2, 3, 4, 1, float("nan")), (0, 5, 9, 8, 0, float("inf")), (0, 3, 0, 2, 1, float("-inf")),
           (1, 1, 7, 6, 0, 1e30), (1, 4, 4, 4, 1, -1e30), (1, 0, 9, 1, 0, float("nan")), (1, 5, 0, 7, 1, float("inf")))


@functools.lru_cache(maxsize=None)
def _layer_source(img):
    net = FU.make_module(LAYER_NET_SEED[img])
    return net, FU.dcn_inputs(net, FU.case_images(img).flatten(0, 1))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict of float32 CPU tensors x (N,Cin,H,W), offmask (N,27,H,W), weight (Cout,Cin,3,3), bias (Cout), dy (N,Cout,H,W), and slabs.
    Treat it as read-only."""
    if name in SYNTHETIC:
        c = SYNTHETIC[name]
        g = torch.Generator().manual_seed(c["seed"])
        N, (H, W), Cin, Cout = c["N"], c["hw"], c["Cin"], c["Cout"]
        x = torch.randn(N, Cin, H, W, generator=g)
        offmask = torch.cat((1.5 * torch.randn(N, 18, H, W, generator=g), torch.randn(N, 9, H, W, generator=g)), 1)
        if c["kind"] == "zero":
            offmask = torch.zeros_like(offmask)
        if c["kind"] == "planted":
            for n, h, w, k, which, value in PLANTED:
                offmask[n, 2 * k + which, h, w] = value
        bound = 1.0 / np.sqrt(9 * Cin)
        weight = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * bound
        bias = 0.2 * torch.randn(Cout, generator=g)
        seed, slabs = c["seed"], c["slabs"]
    else:
        img, cout = name.rsplit("_", 1)
        layer = LAYER_OF_COUT[int(cout)]
        net, got = _layer_source(img)
        x, offmask = (t.contiguous() for t in got[layer])
        mod = net.get_submodule(layer)
        weight, bias = mod.weight.detach().clone(), mod.bias.detach().clone()
        seed, slabs = LAYER_NET_SEED[img] + int(cout), 0
    g = torch.Generator().manual_seed(seed + SEED_OFFSET)
    dy = torch.randn(x.shape[0], weight.shape[0], *x.shape[2:], generator=g)
    return dict(x=x, offmask=offmask, weight=weight, bias=bias, dy=dy, slabs=slabs)


def tensors(name):
    inp = inputs(name)
    return {k: inp[k] for k in ("x", "offmask", "weight", "bias", "dy")}


def run_layer(inp, dtype=torch.float64, device=None, fn=None):
    """fn (default mvs.deform_conv3x3) on the case in `dtype` and its backward under dy -> dict(y, d_x, d_offmask, d_weight, d_bias)."""
    from diner_amd import mvs
    t = {k: inp[k].to(dtype=dtype, device=device) for k in ("x", "offmask", "weight", "bias", "dy")}
    leaves = [t[k].clone().requires_grad_(True) for k in ("x", "offmask", "weight", "bias")]
    y = (fn or mvs.deform_conv3x3)(*leaves)
    (y * t["dy"]).sum().backward()
    return dict(y=y.detach(), **{k: leaf.grad for k, leaf in zip(OUTPUTS, leaves)})


def closed_form(inp, dtype=torch.float64, device=None):
    from diner_amd import mvs
    t = {k: inp[k].to(dtype=dtype, device=device) for k in ("x", "offmask", "weight", "dy")}
    return dict(zip(OUTPUTS, mvs.deform_conv3x3_grad_torch(t["x"], t["offmask"], t["weight"], t["dy"])))


@functools.lru_cache(maxsize=None)
def expected64(name):
    """The float64 restatement (autograd through mvs.deform_conv2d_torch) of a case on the CPU, computed once per session and shared; treat
    it as read-only."""
    from diner_amd import mvs
    return run_layer(inputs(name), torch.float64, fn=mvs._deform_torch)


def sample_geometry(offmask, H, W):
    """The raw offmask (N,27,H,W) in its dtype -> (inside, floor(py), floor(px)), each (N,9,H,W); the floors are 0 outside.  NaN is outside."""
    dt = offmask.dtype
    k = torch.arange(9)
    py = ((torch.arange(H) - 1).view(1, H, 1) + (k // 3).view(9, 1, 1)).to(dt).unsqueeze(0) + offmask[:, 0:18:2]
    px = ((torch.arange(W) - 1).view(1, 1, W) + (k % 3).view(9, 1, 1)).to(dt).unsqueeze(0) + offmask[:, 1:18:2]
    inside = (py > -1) & (py < H) & (px > -1) & (px < W)
    zero = torch.zeros_like(py)
    return inside, torch.floor(torch.where(inside, py, zero)).double(), torch.floor(torch.where(inside, px, zero)).double()


def margin_holds(offmask):
    """Whether float32 and float64 agree, for every sample, on `inside` and on both floors: the kernel forms py, px by the same single
    fp32 addition as the float32 run, so only float64 can floor differently -- and there the offset gradient jumps."""
    H, W = offmask.shape[2:]
    a, b = sample_geometry(offmask.float(), H, W), sample_geometry(offmask.double(), H, W)
    return all(bool((p == q).all()) for p, q in zip(a, b))


def planted_taps():
    """-> [(n, h, w, k)]: the taps whose gradients must be exactly 0."""
    return [(n, h, w, k) for n, h, w, k, _, _ in PLANTED]


# ---- the whole FeatureNet training step ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_inputs(name):
    """-> (state dict, images (N,3,H,W), {stage: upstream gradient}) of a net case, float32 on the CPU."""
    c = FU.CASES[name]
    imgs = FU.case_images(name).flatten(0, 1)
    H, W = c["hw"]
    g = torch.Generator().manual_seed(c["seed"] + SEED_OFFSET + 50)
    ups = {s: torch.randn(imgs.shape[0], FU.STAGE_CHANNELS[s], H // d, W // d, generator=g) for s, d in zip(FU.STAGES, (4, 2, 1))}
    return FU.featurenet_state_dict(c["seed"] + 50), imgs, ups


def run_net(name, dtype=torch.float64, device=None, deform_kernels=False, module=None, dy_sums=None):
    """One training-mode forward and backward of DeviceFeatureNet (or `module`, which takes the same state dict) -> {stage: output,
    "param_<key>": gradient}.  dy_sums: a dict that receives, per deformable layer "outX.i", the per-channel sum over the pixels of the
    magnitudes of the upstream gradient that reaches the layer's output."""
    from diner_amd import mvs
    sd, imgs, ups = net_inputs(name)
    net = module if module is not None else mvs.DeviceFeatureNet(8)
    net.load_state_dict(sd)
    net = net.to(dtype=dtype, device=device).train()
    if module is None:
        net.deform_kernels = deform_kernels
    if dy_sums is not None:
        for layer in FU.DCN_LAYERS:
            net.get_submodule(layer).register_full_backward_hook(
                lambda m, gin, gout, layer=layer: dy_sums.__setitem__(layer, gout[0].detach().abs().double().sum((0, 2, 3)).cpu()))
    out = net.forward_torch(imgs.to(dtype=dtype, device=device)) if module is None else net(imgs.to(dtype=dtype, device=device))
    sum((out[s] * ups[s].to(dtype=dtype, device=device)).sum() for s in FU.STAGES).backward()
    res = {s: out[s].detach() for s in FU.STAGES}
    res.update({"param_" + k: p.grad for k, p in net.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def net_expected64(name):
    return run_net(name, torch.float64)


# the DCN biases in front of a BatchNorm: their gradient is mathematically zero
BN_FED_BIASES = tuple(f"param_{h}.{i}.bias" for h in FU.HEADS for i in (1, 4))


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


def bar(fx, name, key):
    return BAR_FACTOR * float(fx[f"{name}_err_{key}"])


def input_hash():
    """sha256 over every case's regenerated inputs."""
    from tools.make_golden_mvs import sha256_of
    return sha256_of([tensors(n) for n in CASE_NAMES] + [list(net_inputs(n)) for n in NET_CASES])
