"""Shared by tools/make_golden_costreg.py, tests/test_costreg_cpu.py and tests/test_costreg_gpu.py: the seeded weights and inputs of fixture
G29 (regenerated, never stored), the case table and the single-layer shapes.

Weights: every convolution weight is normal with variance 2 / fan-in (fan-in = 27 Cin); BatchNorm has gamma in [0.5, 1.5], beta and the
running mean 0.2 N(0,1) and the running variance in [0.5, 1.5], nothing a folding mistake could cancel against.  Input: a similarity
volume peaked on a slanted plane, 0.5 exp(-0.5 ((d - plane(h, w)) / 1.2)^2) + 0.05 N(0,1), built in float64 and rounded once."""
import functools
import os

import numpy as np
import torch

from tests import mvs_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g29_costreg.npz")
BAR_FACTOR, GAP_FACTOR, EXCLUDED_CAP = MU.BAR_FACTOR, MU.GAP_FACTOR, MU.EXCLUDED_CAP

# name: (base, B, D, H, W), seed -- the smallest shapes at which each thing can go wrong
CASES = {
    "one_voxel": dict(shape=(4, 1, 8, 8, 8), seed=2901),      # the bottom level is one voxel: every tap but the centre is padding; Cout 4 < the N tile
    "batch": dict(shape=(8, 2, 8, 16, 24), seed=2902),        # the shipped width, two samples, tiles partly outside the volume
    "long": dict(shape=(8, 1, 16, 8, 40), seed=2903),         # a long axis against a short one
    "stage1": dict(shape=(8, 1, 48, 32, 40), seed=2904),      # stage 1's depth count
}
# DeviceDepthNet with the real regulariser: a G28-style scene (tests/mvs_util.py) at sizes the kernels' gate takes
DEPTHNET = dict(B=2, NS=3, C=8, D=8, hw=(24, 40), seed=2911, base=8)

# single layers: every Cin x Cout, on every volume (D, H, W): one voxel; odd sizes at stride 2; the transposed layer's last odd index
LAYER_CIN, LAYER_COUT = (1, 8, 12, 64), (1, 8, 20, 64)
LAYER_VOLUMES = ((1, 1, 1), (3, 5, 18), (2, 9, 17))
LAYER_KINDS = ("conv1", "conv2", "deconv")


def costreg_state_dict(base, seed, in_channels=1):
    """A seeded state dict of CostRegNet(in_channels, base) under the reference's keys."""
    from diner_amd import mvs
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, kind, ci, co, _ in mvs.COSTREG_LAYERS:
        cin, cout = (in_channels if ci == 0 else ci * base), co * base
        shape = (cin, cout, 3, 3, 3) if kind == "deconv" else (cout, cin, 3, 3, 3)
        sd[f"{name}.conv.weight"] = torch.randn(shape, generator=g) * float(np.sqrt(2.0 / (27 * cin)))
        sd[f"{name}.bn.weight"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.2 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.2 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(100)
    sd["prob.weight"] = torch.randn(1, base, 3, 3, 3, generator=g) * float(np.sqrt(2.0 / (27 * base)))
    return sd


def case_input(name):
    """-> the similarity volume (B,1,D,H,W) float32 of a case."""
    c = CASES[name]
    _, B, D, H, W = c["shape"]
    rng = np.random.default_rng(c["seed"])
    d = np.arange(D, dtype=np.float64).reshape(1, D, 1, 1)
    h = np.linspace(-0.5, 0.5, H).reshape(1, 1, H, 1)
    w = np.linspace(-0.5, 0.5, W).reshape(1, 1, 1, W)
    slope = rng.uniform(-0.5, 0.5, (B, 2, 1, 1, 1))
    plane = (D - 1) * (0.5 + slope[:, 0] * w + slope[:, 1] * h)
    vol = 0.5 * np.exp(-0.5 * ((d - plane) / 1.2) ** 2) + 0.05 * rng.normal(0.0, 1.0, (B, D, H, W))
    return torch.from_numpy(vol).to(torch.float32).unsqueeze(1)


def make_net(name_or_base, dtype=torch.float32, seed=None):
    """The DeviceCostRegNet of a case (or of a base width and a seed), in eval mode, on the CPU."""
    from diner_amd import mvs
    base, seed = (CASES[name_or_base]["shape"][0], CASES[name_or_base]["seed"] + 50) if isinstance(name_or_base, str) else (name_or_base, seed)
    net = mvs.DeviceCostRegNet(1, base)
    net.load_state_dict(costreg_state_dict(base, seed))
    return net.to(dtype).eval()


@functools.lru_cache(maxsize=None)
def expected64(name):
    """The float64 torch route of a case on the CPU, computed once per session and shared; treat it as read-only."""
    with torch.no_grad():
        return make_net(name, torch.float64)(case_input(name).double())


@functools.lru_cache(maxsize=None)
def expected32(name):
    with torch.no_grad():
        return make_net(name, torch.float32)(case_input(name))


def softmax_d(cost):
    """(B,1,D,H,W) -> (B,D,H,W): the prob volume select_depth forms of a cost."""
    return torch.exp(torch.nn.functional.log_softmax(cost.squeeze(1), dim=1))


def depthnet_inputs():
    """The G28-style scene of DEPTHNET -> features, proj, depth_values (float32) and the two state dicts."""
    c = DEPTHNET
    rng = np.random.default_rng(c["seed"])
    B, NS, C, D, (H, W) = c["B"], c["NS"], c["C"], c["D"], c["hw"]
    E, K = MU.make_cameras(rng, B, NS, (H, W))
    feats = MU.plane_features(E, K, (H, W), C, rng)
    depth = np.linspace(1.2, 1.9, D).reshape(1, D, 1, 1) + rng.uniform(0.0, 0.03, (B, 1, H, W))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
    return dict(features=[f32(f) for f in feats], proj=f32(MU.proj_pairs(E, K)), depth_values=f32(depth),
                pixelwise=MU.pixelwise_state_dict(c["seed"] + 50), costreg=costreg_state_dict(c["base"], c["seed"] + 60))


def run_depthnet(inp, dtype, device=None):
    """DeviceDepthNet.forward with a DeviceCostRegNet as the regulariser -> (outputs dict, view weights)."""
    from diner_amd import mvs
    dn, cr = mvs.DeviceDepthNet(), mvs.DeviceCostRegNet(1, DEPTHNET["base"])
    dn.pixel_wise_net.load_state_dict(inp["pixelwise"])
    cr.load_state_dict(inp["costreg"])
    dn, cr = dn.to(dtype).eval(), cr.to(dtype).eval()
    if device is not None:
        dn, cr = dn.to(device), cr.to(device)
    x = MU.cast({k: inp[k] for k in ("features", "proj", "depth_values")}, dtype, device)
    with torch.no_grad():
        return dn(x["features"], x["proj"], x["depth_values"], DEPTHNET["D"], cr)


@functools.lru_cache(maxsize=None)
def depthnet_expected(dtype):
    return run_depthnet(depthnet_inputs(), dtype)


def subsample(t):
    return MU.subsample(t)


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(FIXTURE))
