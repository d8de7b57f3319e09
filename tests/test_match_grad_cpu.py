"""The matching stage's backward pass (diner_amd.mvs.match_similarity / cost_volume_train, DeviceDepthNet.match_kernels) without a device:
the torch restatement's float64 autograd against fixture G33 (tests/golden/g33_match_grad.npz, whose float64 values the generator trusts
only after finding the restatement's float32 run equal to the reference's own homo_warping / PixelwiseNet under autograd), the C symbols,
the argument checks, the closed gate on CPU tensors, the switches' defaults and the host program around the tap geometry."""
import ctypes
import importlib.util
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from diner_amd import _lib, estimator, mvs, ops
from tests import match_grad_util as U
from tests import mvs_util as MU

ROOT = MU.ROOT
NEW_SYMBOLS = ("diner_mvs_similarity_f32", "diner_mvs_similarity_grad_f32")


@pytest.mark.parametrize("run", ["sim", "cv"])
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_float64_restatement_matches_the_fixture(name, run):
    fx, got = U.fixture(), U.outputs(U.expected64(name, run))
    zero = set(fx[f"{name}_{run}_zero"].tolist())
    assert zero == ({"d_src1"} if name == "turned" else set())
    for key, val in got.items():
        if key in zero:
            assert not bool(val.any()), (name, run, key)
            continue
        assert float(fx[f"{name}_{run}_err_{key}"]) > 0.0, (name, run, key)
        want = fx[f"{name}_{run}_{key}64"]
        assert np.abs(MU.subsample(val) - want).max() <= 1e-12, (name, run, key)
    if run == "cv":
        assert ("param_conv2.bias" in got) == (name not in U.GIVEN)


def test_generator_imports():
    spec = importlib.util.spec_from_file_location("_g33_generator", os.path.join(ROOT, "tools", "make_golden_match_grad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.main) and mod.U.FIXTURE == U.FIXTURE and os.path.getsize(U.FIXTURE) < 400 * 1024


def test_new_symbols_and_abi():
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    assert re.search(r"#define DINER_ABI_VERSION 6\b", header) and _lib.ABI_VERSION == 6
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.diner_abi_version() == 6
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\(", header) and hasattr(lib, name), name


def _args(B=1, NS=2, C=8, D=4, H=5, W=6):
    return (torch.zeros(B, H, W, C), torch.zeros(NS, B, H, W, C), torch.zeros(B, NS + 1, 2, 4, 4), torch.zeros(B, D, H, W))


def test_refusals_without_a_device():
    for kw, word in ((dict(NS=16), "source views"), (dict(C=6), "multiple of 4"), (dict(C=68), "multiple of 4"), (dict(D=257), "depth")):
        ref, src, proj, depth = _args(**kw)
        with pytest.raises(ValueError, match=word):
            ops.mvs_similarity(ref, src, proj, depth)
        with pytest.raises(ValueError, match=word):
            ops.mvs_similarity_grad(ref, src, torch.zeros(ref.shape[0], src.shape[0], 12), depth, grad_views=torch.zeros(1))
    big = torch.zeros(1).expand(1, 256, 4096, 2048)                # B D H W = 2^31, no memory behind it
    with pytest.raises(ValueError, match="2\\^31"):
        ops.mvs_similarity(torch.zeros(1).expand(1, 4096, 2048, 4), torch.zeros(1).expand(1, 1, 4096, 2048, 4), torch.zeros(1, 2, 2, 4, 4), big)
    ref, src, proj, depth = _args()
    hom, G, g, w = torch.zeros(1, 2, 12), torch.zeros(1, 2, 4, 5, 6), torch.zeros(1, 4, 5, 6), torch.zeros(1, 2, 5, 6)
    with pytest.raises(ValueError, match="shapes disagree"):
        ops.mvs_similarity(ref, src[:, :, :4], proj, depth)
    with pytest.raises(ValueError, match="proj"):
        ops.mvs_similarity(ref, src, proj[:, :2], depth)
    with pytest.raises(ValueError, match="homography"):
        ops.mvs_similarity_grad(ref, src, hom[:, :1], depth, grad_views=G)
    with pytest.raises(ValueError, match="either"):
        ops.mvs_similarity_grad(ref, src, hom, depth)
    with pytest.raises(ValueError, match="either"):
        ops.mvs_similarity_grad(ref, src, hom, depth, grad_views=G, grad_aggregated=g, view_weights=w)
    with pytest.raises(ValueError, match="view_weights"):
        ops.mvs_similarity_grad(ref, src, hom, depth, grad_aggregated=g)
    with pytest.raises(ValueError, match="view_weights"):
        ops.mvs_similarity_grad(ref, src, hom, depth, grad_views=G, view_weights=w)
    with pytest.raises(ValueError, match="grad_views"):
        ops.mvs_similarity_grad(ref, src, hom, depth, grad_views=G[:, :1])
    with pytest.raises(ValueError, match="grad_aggregated"):
        ops.mvs_similarity_grad(ref, src, hom, depth, grad_aggregated=g, view_weights=w[:, :1])
    # in range and well-formed: only the missing device stops them
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mvs_similarity(ref, src, proj, depth)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.mvs_similarity_grad(ref, src, hom, depth, grad_aggregated=g, view_weights=w)
    with pytest.raises(ValueError, match="either"):
        mvs.cost_volume_train([torch.zeros(1, 8, 5, 6)] * 3, proj, depth)


def _depthnet_step(match_kernels, name="probe", dtype=torch.float32):
    inp = U.inputs(name)
    dn = mvs.DeviceDepthNet()
    dn.pixel_wise_net.load_state_dict(inp["state_dict"])
    dn = dn.to(dtype).train()
    dn.match_kernels = match_kernels
    feats = U.leaves(inp, dtype)
    x = MU.cast(dict(proj=inp["proj"], depth=inp["depth_values"], vw=inp["view_weights"]), dtype)
    res = dn(feats, x["proj"], x["depth"], x["depth"].shape[1], MU.regulariser, view_weights=x["vw"])
    out = res if x["vw"] is not None else res[0]
    out["prob_volume"].square().sum().backward()
    return out, [f.grad for f in feats], dn


@pytest.mark.parametrize("name", ["probe", "shifted"])
def test_match_kernels_on_cpu_tensors_is_the_torch_route(name):
    a, ga, dna = _depthnet_step(True, name)
    b, gb, dnb = _depthnet_step(False, name)
    assert torch.equal(a["prob_volume"], b["prob_volume"]) and torch.equal(a["depth"], b["depth"])
    assert all(torch.equal(p, q) for p, q in zip(ga, gb))
    assert all(torch.equal(p, q) for p, q in zip(dna.state_dict().values(), dnb.state_dict().values()))
    inp = U.inputs(name)
    assert not mvs.match_gate(inp["features"], inp["proj"], inp["depth_values"])
    s = mvs.match_similarity(inp["features"], inp["proj"], inp["depth_values"])
    assert torch.equal(s, mvs.match_similarity_torch(inp["features"], inp["proj"], inp["depth_values"]))


def test_switches_default_to_off():
    assert mvs.DeviceDepthNet().match_kernels is False
    model = estimator.DeviceTransMVSNet(ndepths=(8, 4, 2))
    assert model.match_kernels is False
    model.match_kernels = 1
    assert model.DepthNet.match_kernels is True and model.fused_readout is False
    assert inspect.signature(estimator.fit_estimator).parameters["match_kernels"].default is False
    assert not [k for k in model.state_dict() if "match" in k]                 # a plain attribute: the state-dict keys stay the reference's


def test_tap_geometry_under_the_sanitizers(tmp_path):
    """tools/mvs_geom_check.cpp, built for the host with AddressSanitizer, UBSan and the float-cast-overflow check, run as a program of its
    own (nothing is loaded into this process): NaN, infinite, huge and denormal depths and homographies never yield an index outside
    the map, and outside or invalid taps carry zero weights."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) to build tools/mvs_geom_check.cpp with")
    exe = str(tmp_path / "mvs_geom_check")
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        built = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                                "-fno-sanitize-recover=all", *static, os.path.join(ROOT, "tools", "mvs_geom_check.cpp"), "-o", exe],
                               capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "every index in range" in run.stdout, run.stdout + run.stderr
