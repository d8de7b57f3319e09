"""GPU: the f16x3 field kernels with block 2's fc_1 behind the view mean (csrc/mlp_h3n.hip; tests/test_mean_first_cpu.py has the identity).
The per-view kernel stops behind block 2's fc_0 and hands over two planes per point -- the view means of the residual stream (caller's
workspace) and of relu(h) (a library-owned buffer per stream) --, the post kernel runs the layer once per point.  G6 scene (16 x 16 maps,
512 points); the exact-fp32 mode, which keeps the reference's order, is the anchor; bound: the stage tolerance of test_hip_parity.py."""
import numpy as np
import pytest
import torch

from tests.helpers import load, oracle_setup, max_norm_rel

pytestmark = pytest.mark.gpu
TOL_STAGE = 2e-5


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


def hip_mlp(ops, msd):
    return ops.HipMlp({k: v.cuda() for k, v in msd.items()})


@pytest.fixture(scope="module")
def g6(ops):
    """(scene dict, mlp state dict, points, directions) of G6 and the scene / MLP handles of the four-view scene."""
    g = load("g6_pixelnerf.npz")
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]))
    return dict(g=g, sc=sc, msd=msd, pts=T(g["pts"]).cuda(), dirs=T(g["dirs"]).cuda(), hs=hip_scene(ops, sc), hm=hip_mlp(ops, msd))


def planted(msd):
    """Block 2's hidden activation beyond the fp16 range in every seventh feature: the mean of relu(h) that crosses the hand-over leaves
    the range (65504) while the residual stream stays small."""
    big = {k: v.clone() for k, v in msd.items()}
    big["blocks.2.fc_0.bias"] = big["blocks.2.fc_0.bias"] + 3.0e5 * (torch.arange(512) % 7 == 0)
    return big


@pytest.mark.parametrize("P", [7, 83, 213, 512])
def test_f16x3_against_exact_fp32(ops, g6, P):
    """A ragged 16-point group (7), a ragged 64-point post tile with empty column groups (83), both (213), whole tiles (512)."""
    hs, hm, pts, dirs = g6["hs"], g6["hm"], g6["pts"][:P].contiguous(), g6["dirs"][:P].contiguous()
    hm.fallback_launches(reset=True)
    got = ops.field_from_points(hs, hm, pts, dirs, precision="f16x3")
    fb = hm.fallback_launches(reset=True)
    exact = ops.field_from_points(hs, hm, pts, dirs, precision="fp32")
    rel = max_norm_rel(got, exact)
    print(f"P={P}: f16x3 vs fp32 {rel:.3e} (max-norm-rel), vs the reference {max_norm_rel(got, g6['g']['out'][:P]):.3e}, fall-back launches {fb}")
    assert torch.isfinite(got).all()
    assert rel < TOL_STAGE
    assert fb == 0


@pytest.mark.parametrize("P", [512, 83, 7])
def test_range_flag_across_the_handover(ops, g6, P):
    hs, pts, dirs = g6["hs"], g6["pts"][:P].contiguous(), g6["dirs"][:P].contiguous()
    hm = hip_mlp(ops, planted(g6["msd"]))
    assert hm.h3_ok
    exact = ops.field_from_points(hs, hm, pts, dirs, precision="fp32")
    hm.fallback_launches(reset=True)
    got = ops.field_from_points(hs, hm, pts, dirs, precision="f16x3")
    fb = hm.fallback_launches(reset=True)
    print(f"P={P}: fall-back launches {fb}, equal to fp32: {torch.equal(got, exact)}")
    assert torch.isfinite(got).all() and torch.equal(got, exact)
    assert fb == 1


def test_range_flag_across_the_handover_six_views(ops, g6):
    """The same plant through the views entry (two groups: four live views, then two)."""
    g = g6["g"]
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]), nv=6)
    hs, hm = hip_scene(ops, sc), hip_mlp(ops, planted(msd))
    pts, dirs = g6["pts"][:83].contiguous(), g6["dirs"][:83].contiguous()
    exact = ops.field_from_points(hs, hm, pts, dirs, precision="fp32")
    hm.fallback_launches(reset=True)
    got = ops.field_from_points(hs, hm, pts, dirs, precision="f16x3")
    fb = hm.fallback_launches(reset=True)
    print(f"NV=6: fall-back launches {fb}, equal to fp32: {torch.equal(got, exact)}")
    assert torch.isfinite(got).all() and torch.equal(got, exact)
    assert fb == 1


@pytest.mark.parametrize("nv", [1, 3, 5, 6])
def test_view_groups(ops, g6, nv):
    """First-group write, later-group add and partial groups, for both hand-over planes."""
    g = g6["g"]
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]), nv=nv)
    hs, hm = hip_scene(ops, sc), hip_mlp(ops, msd)
    pts, dirs = g6["pts"][:83].contiguous(), g6["dirs"][:83].contiguous()
    hm.fallback_launches(reset=True)
    got = ops.field_from_points(hs, hm, pts, dirs, precision="f16x3")
    fb = hm.fallback_launches(reset=True)
    exact = ops.field_from_points(hs, hm, pts, dirs, precision="fp32")
    rel = max_norm_rel(got, exact)
    print(f"NV={nv}: f16x3 vs fp32 {rel:.3e} (max-norm-rel), fall-back launches {fb}")
    assert torch.isfinite(got).all()
    assert rel < TOL_STAGE
    assert fb == 0


def test_side_buffer_grows_per_stream_and_is_released(ops, g6):
    """The library-owned plane: grown on one stream (83, 512, 83 points), a second stream's own, released and allocated again -- every
    result equals the first call of its size bit for bit."""
    hs, hm = g6["hs"], g6["hm"]
    call = lambda P: ops.field_from_points(hs, hm, g6["pts"][:P].contiguous(), g6["dirs"][:P].contiguous(), precision="f16x3")
    first = {83: call(83).clone()}
    first[512] = call(512).clone()
    assert torch.equal(call(83), first[83])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = call(512).clone()
    side.synchronize()
    assert torch.equal(other, first[512])
    torch.cuda.synchronize()
    assert ops.lib.diner_field_release_buffers() == 0
    for P in (83, 512):
        assert torch.equal(call(P), first[P]), P
    torch.cuda.synchronize()
    assert ops.lib.diner_field_release_buffers() == 0
    assert max_norm_rel(first[512], g6["g"]["out"]) < TOL_STAGE
