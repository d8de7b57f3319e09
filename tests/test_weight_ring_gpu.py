"""GPU: the four-wave f16x3 field kernels after the weight ring's address change (csrc/mlp_h3n.hip, ARing: the lane offset is kept a
32-bit value where the loads are issued, so every fragment load is `scalar base + lane offset + immediate`; the per-view training
instance stores its saved activations in the same form).  Addressing only: the arithmetic is what it was, so the bars are the existing ones -- the stage
tolerance of tests/test_hip_parity.py for the two parity-grade modes on G6 (the exact-fp32 mode is the anchor), bit-identity between
replicas, and the forward bar of tests/test_train_gpu.py for the storing variants against the layer-wise training forward.  Point
counts: 1, one 16-point tile, a ragged second tile, and 4115 = 258 tiles of the per-view kernel over 256 workgroups, so that some
workgroup runs a second tile (the case a spilled accumulator inside a GEMM broke: DESIGN_HISTORY.md, "a hazard worth recording")."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import load, oracle_setup, max_norm_rel

pytestmark = pytest.mark.gpu
TOL_STAGE = 2e-5          # tests/test_hip_parity.py: what either mode is held to on G6


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def hip_scene(ops, sc):
    K = sc["src_intrinsics"]
    return ops.HipScene(sc["latent"].cuda(), sc["depths"].cuda(), sc["depths_std"].cuda(), sc["normals"].cuda(),
                        sc["src_extrinsics"], K[:, [0, 1], [0, 1]], K[:, :2, -1], sc["image_shape"], sc["feature_padding"])


def spread(g, P):
    """P distinct points from the 512 of G6: the repeats are scaled by 1 + 1e-3 k (as tests/test_train_gpu.py does)."""
    n = g["pts"].shape[0]
    reps = (P + n - 1) // n
    jit = 1.0 + 1e-3 * torch.arange(reps).repeat_interleave(n)[:P, None]
    return (T(g["pts"]).repeat(reps, 1)[:P] * jit).contiguous(), T(g["dirs"]).repeat(reps, 1)[:P].contiguous()


@pytest.fixture(scope="module")
def g6(ops):
    g = load("g6_pixelnerf.npz")
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]))
    return dict(g=g, sc=sc, msd=msd, hs=hip_scene(ops, sc), hm=ops.HipMlp({k: v.cuda() for k, v in msd.items()}))


def both_modes(ops, hs, hm, pts, dirs):
    hm.fallback_launches(reset=True)
    got = ops.field_from_points(hs, hm, pts, dirs, precision="f16x3")
    fb = hm.fallback_launches(reset=True)
    exact = ops.field_from_points(hs, hm, pts, dirs, precision="fp32")
    return got, exact, fb


@pytest.mark.parametrize("P", [1, 16, 17, 4115])
def test_f16x3_against_exact_fp32(ops, g6, P):
    pts, dirs = spread(g6["g"], P)
    got, exact, fb = both_modes(ops, g6["hs"], g6["hm"], pts.cuda(), dirs.cuda())
    rel = max_norm_rel(got, exact)
    print(f"P={P}: f16x3 vs fp32 {rel:.3e} (max-norm-rel), fall-back launches {fb}")
    assert got.shape == (P, 4) and torch.isfinite(got).all()
    assert rel < TOL_STAGE
    assert fb == 0


def test_replicas_at_4115_points_are_bit_identical(ops, g6):
    """4115 = 5 x 823: 823 distinct points five times over.  A replica starts at point 823 r, which is no multiple of 16 for r > 0: the same
    point sits in another lane, tile and workgroup (and in some workgroup's second tile) in every replica."""
    R, n = 5, 823
    p1, d1 = spread(g6["g"], n)
    hs, hm = g6["hs"], g6["hm"]
    hm.fallback_launches(reset=True)
    out = ops.field_from_points(hs, hm, p1.repeat(R, 1).cuda(), d1.repeat(R, 1).cuda(), precision="f16x3").cpu().view(R, n, 4)
    assert hm.fallback_launches(reset=True) == 0
    exact = ops.field_from_points(hs, hm, p1.cuda(), d1.cuda(), precision="fp32").cpu()
    assert max_norm_rel(out[0], exact) < TOL_STAGE
    for r in range(1, R):
        assert torch.equal(out[r], out[0]), f"replica {r} differs from replica 0"


@pytest.mark.parametrize("nv", [3, 5])
def test_view_group_instance(ops, g6, nv):
    """k_field_views_h3n: one partial group (3 views), a whole group and a later group that adds into the hand-over planes (5)."""
    g = g6["g"]
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]), nv=nv)
    hs, hm = hip_scene(ops, sc), ops.HipMlp({k: v.cuda() for k, v in msd.items()})
    pts, dirs = spread(g, 17)
    got, exact, fb = both_modes(ops, hs, hm, pts.cuda(), dirs.cuda())
    rel = max_norm_rel(got, exact)
    print(f"NV={nv}, 17 points: f16x3 vs fp32 {rel:.3e} (max-norm-rel), fall-back launches {fb}")
    assert torch.isfinite(got).all()
    assert rel < TOL_STAGE
    assert fb == 0


def test_fused_training_forward_against_the_layerwise_one(ops, g6, monkeypatch):
    """k_train_fwd_pre / k_train_fwd_post at the smallest point count that the host routes to them by size, plus a ragged tile: outputs and
    every saved pre-activation (diner_field_train_ws_layout) against the layer-wise forward, at the forward bar of tests/test_train_gpu.py."""
    from diner_amd import train, _lib
    from tests.tests_train_util import module_param_list
    monkeypatch.delenv("DINER_TRAIN_FUSED_FWD", raising=False)
    lo, hi = 1, 1 << 20                            # the threshold of fused_forward_enabled (16384 points per object)
    assert not train.fused_forward_enabled(lo) and train.fused_forward_enabled(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if train.fused_forward_enabled(mid) else (mid, hi)
    P = hi + 7
    g, sc, hs = g6["g"], g6["sc"], g6["hs"]
    xyz, dirs = spread(g, P)
    xyz, dirs = xyz.cuda(), dirs.cuda()
    params, names = module_param_list(g6["msd"])
    lib = _lib.load()
    off = (C.c_longlong * 12)()
    _lib.check(lib.diner_field_train_ws_layout(P, 4, off, 12))
    regions = [(f"X[{b}]", off[b], (4 if b < 3 else 1) * P * 512) for b in range(5)]
    regions += [(f"H[{b}]", off[5 + b], (4 if b < 3 else 1) * P * 512) for b in range(5)]
    regions += [("x_last", off[10], P * 512), ("raw", off[11], P * 4)]

    def run(env):
        if env is not None:
            monkeypatch.setenv("DINER_TRAIN_FUSED_FWD", env)
        latent = sc["latent"].detach().cuda().requires_grad_(True)
        out = train.field_train(hs, xyz, dirs, latent, params)
        ws = out.grad_fn.saved_tensors[0].view(torch.float32)
        return out, ws

    assert train.fused_forward_enabled(P, hs)
    out_f, ws_f = run(None)
    ovf = C.c_int(-1)
    _lib.check(lib.diner_field_train_fused_overflowed(out_f.grad_fn.saved_tensors[0].data_ptr(), P, 4, C.byref(ovf), None))
    assert ovf.value == 0, "the fused kernels raised their range flag: what follows would compare the layer-wise repeat with itself"
    assert train._step_handle(params, 6.28).fallback_launches() == 0
    out_l, ws_l = run("0")
    e_out = max_norm_rel(out_f.detach(), out_l.detach())
    print(f"P={P}: fused vs layer-wise training forward {e_out:.3e} (max-norm-rel)")
    worst = ("", 0.0)
    for name, o, n in regions:
        e = max_norm_rel(ws_f[o:o + n], ws_l[o:o + n])
        print(f"   saved {name}: {e:.3e}")
        worst = max(worst, (name, e), key=lambda t: t[1])
    assert torch.isfinite(out_f).all()
    assert e_out < 2e-5
    assert worst[1] < 2e-5, worst
