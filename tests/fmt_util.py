"""Shared by tools/make_golden_fmt.py, tests/test_fmt_cpu.py and tests/test_fmt_gpu.py: the seeded weights and inputs of fixture G30
(regenerated, never stored), the case table and the float64 restatements of the single kernels.

Weights: the matrices keep the reference's own initialisation -- Xavier-uniform for the transformer's Linear weights (FMT._reset_parameters),
torch's Conv2d default (uniform within 1 / sqrt(fan-in)) for the pathway's four convolutions.  Every 1-D parameter is non-trivial, because
a default LayerNorm (gamma 1, beta 0) and zero-mean biases would hide a dropped affine or bias: biases and LayerNorm beta 0.2 N(0,1),
LayerNorm gamma in [0.5, 1.5].  Features: N(0,1) per stage."""
import functools
import os

import numpy as np
import torch

from tests import mvs_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g30_fmt.npz")
BAR_FACTOR, GAP_FACTOR = MU.BAR_FACTOR, MU.GAP_FACTOR
STAGES = ("stage1", "stage2", "stage3")
STAGE_CHANNELS = {"stage1": 32, "stage2": 16, "stage3": 8}
KV_TOKENS = 512                    # DINER_FMT_KV_TOKENS: the run of tokens one workgroup of k_fmt_kv sums (checked against ops in the tests)

# name: B, NV, stage-1 (H, W), seed, whether the pathway runs -- the smallest shapes at which each thing can go wrong
CASES = {
    "tiny": dict(B=1, NV=2, hw=(5, 7), seed=3001, pathway=True),          # fewer tokens than a tile, one partial block, the edge clamp nearly everywhere
    "ragged": dict(B=2, NV=4, hw=(23, 37), seed=3002, pathway=True),      # 851 tokens: partly filled last tile and block; 2 batch elements x 3 sources; H != W
    "blocks": dict(B=1, NV=2, hw=(40, 52), seed=3003, pathway=True),      # 2080 tokens: five partial blocks, the last holding 32
    "dtu_tokens": dict(B=1, NV=2, hw=(128, 160), seed=3004, pathway=False),   # the workload's own token count through the reduction
}
# the attention state of "blocks" is summed from at least three partial blocks, the last one partly filled
_L = CASES["blocks"]["hw"][0] * CASES["blocks"]["hw"][1]
assert -(-_L // KV_TOKENS) >= 3 and _L % KV_TOKENS != 0, (_L, KV_TOKENS)
# the three-stage run behind the device module: mvs_util's G28-style scene (B 2, three sources, a 24 x 40 image, stage 1 of 6 x 10)
STAGE_RUN_SEED = 3011


def fmt_state_dict(seed, base=8):
    """A seeded state dict of FMT_with_pathway(base) under the reference's 132 keys."""
    from diner_amd import mvs
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, p in mvs.DeviceFMTWithPathway(base).state_dict().items():
        if p.dim() == 2:                                           # Linear: Xavier-uniform, as FMT._reset_parameters leaves it
            bound = float(np.sqrt(6.0 / (p.shape[0] + p.shape[1])))
            sd[key] = (torch.rand(p.shape, generator=g) * 2 - 1) * bound
        elif p.dim() == 4:                                         # Conv2d: torch's default, kaiming_uniform(a = sqrt 5) = U(+- 1 / sqrt(fan-in))
            bound = float(1.0 / np.sqrt(p.shape[1] * p.shape[2] * p.shape[3]))
            sd[key] = (torch.rand(p.shape, generator=g) * 2 - 1) * bound
        elif ".norm" in key and key.endswith(".weight"):
            sd[key] = 0.5 + torch.rand(p.shape, generator=g)
        else:
            sd[key] = 0.2 * torch.randn(p.shape, generator=g)
    return sd


def case_features(name):
    """-> per view {"stage1": (B,32,H,W), "stage2": (B,16,2H,2W), "stage3": (B,8,4H,4W)} float32 (stage 1 alone without the pathway)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    B, (H, W) = c["B"], c["hw"]
    out = []
    for _ in range(c["NV"]):
        f = {"stage1": torch.randn(B, 32, H, W, generator=g)}
        if c["pathway"]:
            f["stage2"], f["stage3"] = torch.randn(B, 16, 2 * H, 2 * W, generator=g), torch.randn(B, 8, 4 * H, 4 * W, generator=g)
        out.append(f)
    return out


def make_module(name_or_seed, dtype=torch.float32):
    """The DeviceFMTWithPathway of a case (or of a seed), in eval mode, on the CPU."""
    from diner_amd import mvs
    seed = CASES[name_or_seed]["seed"] + 50 if isinstance(name_or_seed, str) else name_or_seed
    net = mvs.DeviceFMTWithPathway(8)
    net.load_state_dict(fmt_state_dict(seed))
    return net.to(dtype).eval()


def case_stages(name):
    return STAGES if CASES[name]["pathway"] else STAGES[:1]


def run_case(net, feats, pathway=True):
    """The module on a list of per-view feature dicts (copied: the module rewrites them) -> {stage: [view 0, view 1, ...]}."""
    feats = [dict(f) for f in feats]
    with torch.no_grad():
        if pathway:
            out = net(feats)
            return {k: [f[k] for f in out] for k in STAGES}
        ref, srcs = net.FMT.encode(feats[0]["stage1"], [f["stage1"] for f in feats[1:]])
        return {"stage1": [ref] + list(srcs)}


@functools.lru_cache(maxsize=None)
def expected(name, dtype):
    """The torch route of a case on the CPU in `dtype`, computed once per session and shared; treat it as read-only."""
    return run_case(make_module(name, dtype), MU.cast(case_features(name), dtype), CASES[name]["pathway"])


def expected64(name):
    return expected(name, torch.float64)


def expected32(name):
    return expected(name, torch.float32)


def stacked(views):
    """[view (B,C,H,W), ...] -> (NV,B,C,H,W) contiguous, on the CPU."""
    return torch.stack([v.detach().cpu().contiguous() for v in views], 0)


def subsample(t):
    return MU.subsample(t)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))


# ---- the three-stage run behind the module ------------------------------------------------------------------------------------------------
def stage_run(dtype, device=None, use_module=True):
    """mvs_util's three-stage scene with its features sent through the module first -> coarse_to_fine's outputs.  On the CPU the module's
    torch route; on a HIP device its kernels, or with use_module=False its torch route there."""
    from diner_amd import mvs
    s, inp = MU.STAGES, MU.stage_inputs()
    net = make_module(STAGE_RUN_SEED, dtype)
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(inp["state_dict"])
    dn = dn.to(dtype).eval()
    if device is not None:
        net, dn = net.to(device), dn.to(device)
    x = MU.cast({k: inp[k] for k in ("features", "proj", "depth_values")}, dtype, device)
    with torch.no_grad():
        feats = net([dict(f) for f in x["features"]]) if use_module else net.forward_torch([dict(f) for f in x["features"]])
        return mvs.coarse_to_fine(feats, x["proj"], x["depth_values"], dn, MU.regulariser, ndepths=s["ndepths"], ratios=s["ratios"],
                                  image_hw=s["image"], depth_interval=s["depth_interval"], scales=s["scales"])


@functools.lru_cache(maxsize=None)
def stage_run_expected(dtype):
    return stage_run(dtype)


# ---- float64 restatements of the single kernels' own formulas -------------------------------------------------------------------------------
def layer_weights(net, i, dtype=torch.float64):
    """Layer i's sixteen tensors under short names, in `dtype`."""
    ly = net.FMT.layers[i]
    a = ly.attention
    w = dict(wq=a.query_projection.weight, bq=a.query_projection.bias, wk=a.key_projection.weight, bk=a.key_projection.bias,
             wv=a.value_projection.weight, bv=a.value_projection.bias, wo=a.out_projection.weight, bo=a.out_projection.bias,
             g1=ly.norm1.weight, be1=ly.norm1.bias, w1=ly.linear1.weight, b1=ly.linear1.bias, w2=ly.linear2.weight, b2=ly.linear2.bias,
             g2=ly.norm2.weight, be2=ly.norm2.bias)
    return {k: v.detach().to(dtype) for k, v in w.items()}


def kv_restated(src, w):
    """src (N,S,32) -> the attention state (N,160): KV as [h][m][d], then Ksum [h][d]."""
    N, S, _ = src.shape
    K = (torch.nn.functional.elu(src @ w["wk"].T + w["bk"]) + 1).view(N, S, 8, 4)
    V = (src @ w["wv"].T + w["bv"]).view(N, S, 8, 4)
    kv = (K.unsqueeze(3) * V.unsqueeze(4)).sum(1)                  # (N, h, m, d) = sum_s K[s,h,d] V[s,h,m]
    return torch.cat([kv.reshape(N, 128), K.sum(1).reshape(N, 32)], 1)


def layer_norm_restated(x, gamma, beta):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5) * gamma + beta


def layer_restated(x, state, w):
    """x (N,L,32), state (R,160) with image n reading row n mod R -> the layer's output (N,L,32)."""
    N, L, _ = x.shape
    st = state[torch.arange(N) % state.shape[0]]
    kv, ksum = st[:, :128].view(N, 1, 8, 4, 4), st[:, 128:].view(N, 1, 8, 4)
    Q = (torch.nn.functional.elu(x @ w["wq"].T + w["bq"]) + 1).view(N, L, 8, 4)
    Z = 1 / ((Q * ksum).sum(-1) + 1e-6)
    A = ((Q.unsqueeze(3) * kv).sum(-1) * Z.unsqueeze(-1)).reshape(N, L, 32)
    x1 = layer_norm_restated(x + A @ w["wo"].T + w["bo"], w["g1"], w["be1"])
    y = torch.relu(x1 @ w["w1"].T + w["b1"]) @ w["w2"].T + w["b2"]
    return layer_norm_restated(x1 + y, w["g2"], w["be2"])


def merge_restated(top, weight, lateral):
    """Channels-last top (N,H,W,Ctop), weight (Clat,Ctop,1,1), lateral (N,2H,2W,Clat) -> bilinear2x(conv1x1(top)) + lateral, channels-last."""
    red = torch.nn.functional.conv2d(top.permute(0, 3, 1, 2), weight)
    up = torch.nn.functional.interpolate(red, size=lateral.shape[1:3], mode="bilinear", align_corners=False)
    return up.permute(0, 2, 3, 1) + lateral
