"""CPU: scenes with up to 16 source views (DINER_MAX_VIEWS; the reference's PixelNeRF takes any number, pixelnerf.py:67).

  1. the oracle against the reference at NV = 6, 8 and 16 (tests/golden/g23_many_views.npz, tools/make_golden_many_views.py):
     depth-guided picks, filled samples and renderer.forward's colours and depths, and one grad-mode step at NV = 6;
  2. the C ABI's view limits, before any device work (dummy pointers, never dereferenced): nv outside [1, 16] is DINER_E_INVALID for
     the NV-generic entries (sampler, diner_index_f32, the generic inputs and their adjoint); 5..16 views are DINER_E_UNSUPPORTED, with a
     message naming the 4-view limit, for every entry built for the fused kernels; the size queries of those entries return 0;
  3. ops.HipScene refuses 17 views with a ValueError before it touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, sha, selection_diff, SAT_L, max_norm_rel
from diner_amd.synthetic import realistic_mlp_state_dict


def T(a):
    return torch.from_numpy(np.asarray(a))


def g23():
    return load("g23_many_views.npz")


def nv_inputs(g, nv):
    """-> (scene dict, oracle scene, weights, the reference's rays (NR, 8), {K: (nc, ng, nf)}) of G23 at nv views."""
    W, H, NR, n_cand = int(g["W"]), int(g["H"]), int(g["NR"]), int(g["n_cand"])
    sc, scene, w, msd, rays = oracle_setup(W, H, int(g["scene_seed"]), nv=nv)
    assert sha(sc["latent"][:, :4, :8, :8], sc["latent"][:, -4:, -8:, -8:]) == str(g[f"latent_sha_{nv}"])
    sel = torch.randperm(W * H, generator=torch.Generator().manual_seed(int(g["ray_seed"])))[:NR].sort().values
    assert torch.equal(sel, T(g["ray_idx"]))
    # the reference's rays (gen_rays through host trigonometry: the last bit of a direction can differ between hosts)
    rs = T(g[f"rays_{nv}"])
    assert torch.allclose(rays[sel], rs, rtol=0, atol=1e-6)
    gn = torch.Generator().manual_seed(int(g["noise_seed"]) + nv)
    cfgs = [(int(g["K"]), int(g["G"]))] + ([(int(g["K_wide"]), int(g["G_wide"]))] if nv == int(g["nv_wide"]) else [])
    noises = {}
    for K, G in cfgs:
        noises[K] = (torch.rand(NR, n_cand, generator=gn), torch.randn(NR, G, generator=gn), torch.rand(NR, K, generator=gn))
        assert sha(*noises[K]) == str(g[f"in_sha_{nv}_{K}"]), "seeded noise not reproducible on this host"
    return sc, scene, w, rs, noises


@pytest.mark.parametrize("nv", [6, 8, 16])
def test_oracle_reproduces_reference_many_views(nv):
    g = g23()
    sc, scene, w, rs, noises = nv_inputs(g, nv)
    n_cand, NR = int(g["n_cand"]), rs.shape[0]
    for K, (nc, ng, nf) in noises.items():
        G = ng.shape[1]
        z0, aux = O.sample_depthguided(scene, rs, K, n_cand, G, nc, ng, return_aux=True)
        z = O.fill_up_uniform_samples(z0, rs, nf)
        ref_z0, ref_z = T(g[f"z_unfilled_{nv}_{K}"]), T(g[f"z_{nv}_{K}"])
        if not torch.equal(z0, ref_z0):
            # a host whose erf kernel differs from the pinning host's in the last bit (tests/helpers.py selection_diff)
            bad, worst = selection_diff(ref_z0.sort(-1).values, z0.sort(-1).values, aux["L"], aux["z_cand"], K - G)
            assert worst < SAT_L and len(bad) <= 0.05 * NR
            good = torch.ones(NR, dtype=torch.bool)
            good[bad] = False
            assert torch.allclose(z[good], ref_z[good], rtol=3e-6, atol=1e-7)
        else:
            assert torch.equal(z, ref_z)
        # the likelihood row sums: host erf kernels differ in the last bit (a few 1e-7 of a row sum)
        np.testing.assert_allclose(aux["L"].sum(-1).numpy(), g[f"L_sum_{nv}_{K}"], rtol=1e-5)
    # renderer.forward at K = 64 (the field through MKL GEMMs: host-dependent association, as G22's compositor check)
    K = int(g["K"])
    nc, ng, nf = noises[K]
    out = O.render(scene, w, rs, K, n_cand, int(g["G"]), False, nc, ng, nf)
    same = torch.isclose(out["z"], T(g[f"z_{nv}_{K}"]), rtol=3e-6, atol=1e-7).all(-1)
    assert int(same.sum()) >= NR - 3
    for name in ("rgb", "depth"):
        ref = T(g[f"{name}_{nv}"])
        e = ((out[name][same] - ref[same]).abs().max() / ref.abs().max()).item()
        assert e < 1e-5, (name, e)


def test_oracle_reproduces_reference_grad_step():
    """The NV = 6 grad-mode step of G23: the oracle's autograd on the reference's samples gives its loss and gradients."""
    g = g23()
    W, H, nv, K = int(g["W"]), int(g["H"]), int(g["nv_t"]), int(g["K_t"])
    sc, scene, _, _, rays = oracle_setup(W, H, int(g["scene_seed"]), nv=nv)
    rsd = realistic_mlp_state_dict(int(g["mlp_seed"]))
    assert sha(*[rsd[k] for k in sorted(rsd)]) == str(g["t_mlp_sha"])
    rs = T(g["t_rays"])
    assert torch.allclose(rays[T(g["t_ray_idx"])], rs, rtol=0, atol=1e-6)
    w = O.MLPWeights.from_state_dict(rsd)
    w.lin_out_w.requires_grad_()
    w.fc0_w[0].requires_grad_()
    scene.latent = scene.latent.clone().requires_grad_()
    z = T(g["t_z"])
    xyz = (rs[:, None, :3] + z[..., None] * rs[:, None, 3:6]).reshape(-1, 3)
    dirs = rs[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3)
    f = O.pixelnerf_forward(scene, w, xyz, dirs).view(rs.shape[0], K, 4)
    _, rgb, _ = O.composite_from_field(f, rs, z, False)
    loss = torch.nn.functional.mse_loss(rgb, T(g["t_target"]))
    loss.backward()
    assert abs(loss.item() - float(g["t_loss"])) <= 1e-5 * abs(float(g["t_loss"]))
    assert max_norm_rel(w.lin_out_w.grad, T(g["t_g_lin_out_w"])) < 1e-5
    assert max_norm_rel(w.fc0_w[0].grad[::8], T(g["t_g_fc0_w_rows8"])) < 1e-5
    tx = T(g["t_g_lat_texels"])
    gl = scene.latent.grad[tx[:, 0], :, tx[:, 1], tx[:, 2]]
    assert ((gl - T(g["t_g_lat"])).abs().max() / float(g["t_g_lat_absmax"])).item() < 1e-5


# ---- the C ABI's limits ------------------------------------------------------------------------------------------------------------
def _scene(nv):
    from diner_amd import _lib
    s = _lib.DinerScene()
    s.nv, s.C, s.Hf, s.Wf, s.Hs, s.Ws = nv, 512, 8, 8, 8, 8
    s.img_w, s.img_h = 8.0, 8.0
    return s


def test_max_views_constant():
    from diner_amd import _lib
    import os
    lib = _lib.load()
    assert _lib.MAX_VIEWS == 16 and lib.diner_abi_version() == 6
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diner_hip.h")).read()
    assert "#define DINER_MAX_VIEWS 16" in hdr


@pytest.mark.parametrize("nv", [0, 17, -1, 64])
def test_generic_route_refuses_nv_outside_1_16(nv):
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(8)                 # never dereferenced: the checks run before any device work
    s = _scene(nv)
    sc = C.byref(s)
    calls = {
        "sample_depthguided": lambda: lib.diner_sample_depthguided_f32(sc, p, 4, 1000, 64, 24, 0.05, p, None, None, None, 0, 0, p, None, None),
        "sample_depthguided_long": lambda: lib.diner_sample_depthguided_long_f32(sc, p, 4, 1000, 320, 96, 0.05, p, None, None, None, 0, 0, p,
                                                                                 None, None),
        "sample_depthguided_long (bounded sizes)": lambda: lib.diner_sample_depthguided_long_f32(sc, p, 4, 1000, 64, 24, 0.05, p, None, None,
                                                                                                 None, 0, 0, p, None, None),
        "index latent": lambda: lib.diner_index_f32(sc, 0, p, 16, p, None),
        "index depth": lambda: lib.diner_index_f32(sc, 1, p, 16, p, None),
        "field_inputs_generic": lambda: lib.diner_field_inputs_generic_f32(sc, None, None, 0, p, p, 16, 6, 1, 6.28, p, None),
        "field_inputs_generic rays": lambda: lib.diner_field_inputs_generic_f32(sc, p, p, 8, None, None, 16, 6, 1, 6.28, p, None),
        "field_inputs_generic_bwd": lambda: lib.diner_field_inputs_generic_bwd_f32(sc, p, p, 16, 567, p, p, None),
    }
    for name, call in calls.items():
        assert call() == _lib.E_INVALID, name
        msg = lib.diner_last_error()
        assert f"nv={nv} outside [1,16]".encode() in msg, (name, msg)


def test_fused_entries_refuse_5_to_16_views():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(8)                 # never dereferenced: the view check comes before the handle, the parameters or the device
    prm = _lib.DinerMlpParams()       # zeroed: an unsupported configuration, which the view check must report first
    for nv in (5, 6, 16):
        s = _scene(nv)
        sc = C.byref(s)
        sps = (C.POINTER(_lib.DinerScene) * 2)(C.pointer(s), C.pointer(s))
        u, v = C.c_size_t(0), C.c_size_t(0)
        offs = (C.c_longlong * 12)()
        flag = C.c_int(0)
        lats = (C.c_void_p * 2)(None, None)
        calls = {
            "field_from_rays": lambda: lib.diner_field_from_rays_f32(sc, p, p, p, 4, 8, 0, p, p, None),
            "field_from_points": lambda: lib.diner_field_from_points_f32(sc, p, p, p, 32, 1, p, p, None),
            "render": lambda: lib.diner_render_f32(sc, p, p, p, 4, 8, 0, 0, p, p, None, p, p, None),
            "scene_prepare_f32": lambda: lib.diner_scene_prepare_f32(sc, p, p, None),
            "scene_prepare_f16": lambda: lib.diner_scene_prepare_f16(sc, p, None),
            "train_inputs": lambda: lib.diner_train_inputs_f32(sc, p, p, 32, 6.28, p, p, p, p, None),
            "field_train_forward": lambda: lib.diner_field_train_forward_f32(sc, C.byref(prm), p, p, 32, p, p, None),
            "field_train_forward_s": lambda: lib.diner_field_train_forward_s_f32(sc, C.byref(prm), p, p, 32, p, p, p, None),
            "field_train_backward": lambda: lib.diner_field_train_backward_f32(sc, C.byref(prm), C.byref(prm), 32, p, p, p, None),
            "field_train_backward_s": lambda: lib.diner_field_train_backward_s_f32(sc, C.byref(prm), C.byref(prm), 32, p, p, p, p, None),
            "field_train_forward_fused": lambda: lib.diner_field_train_forward_fused_f32(sc, p, C.byref(prm), p, p, 32, p, p, p, p, None),
            "field_train_forward_batch": lambda: lib.diner_field_train_forward_batch_f32(sps, 2, p, C.byref(prm), p, p, 32, p, p, p, p, None),
            "field_train_backward_batch": lambda: lib.diner_field_train_backward_batch_f32(sps, 2, C.byref(prm), C.byref(prm), 32, p, p, p,
                                                                                           lats, None, None),
            "field_train_workspace_split": lambda: lib.diner_field_train_workspace_split(32, nv, C.byref(u), C.byref(v)),
            "field_train_batch_workspace_split": lambda: lib.diner_field_train_batch_workspace_split(32, nv, 2, C.byref(u), C.byref(v)),
            "field_train_ws_layout": lambda: lib.diner_field_train_ws_layout(32, nv, offs, 12),
            "field_train_fused_overflowed": lambda: lib.diner_field_train_fused_overflowed(p, 32, nv, C.byref(flag), None),
        }
        for name, call in calls.items():
            assert call() == _lib.E_UNSUPPORTED, (nv, name)
            msg = lib.diner_last_error()
            assert f"nv={nv}".encode() in msg and b"at most 4" in msg and b"4-view limit" in msg, (nv, name, msg)
        assert lib.diner_scene_proj_bytes(sc) == 0 and lib.diner_scene_proj_f16_bytes(sc) == 0
        assert lib.diner_field_train_workspace_bytes(32, nv) == 0
    # the four-view sizes are what they were
    s4 = _scene(4)
    assert lib.diner_scene_proj_bytes(C.byref(s4)) == 3 * 4 * 8 * 8 * 512 * 4
    assert lib.diner_field_train_workspace_bytes(32, 4) > 0
    # nv outside [1, 16] stays DINER_E_INVALID on these entries as well
    for nv in (0, 17):
        s = _scene(nv)
        assert lib.diner_field_from_points_f32(C.byref(s), p, p, p, 32, 1, p, p, None) == _lib.E_INVALID
        assert lib.diner_train_inputs_f32(C.byref(s), p, p, 32, 6.28, p, p, p, p, None) == _lib.E_INVALID
        assert lib.diner_field_train_workspace_split(32, nv, C.byref(C.c_size_t()), C.byref(C.c_size_t())) == _lib.E_INVALID


def test_hip_scene_refuses_17_views_before_device_work():
    from diner_amd import ops
    nv = 17
    with pytest.raises(ValueError, match="1 to 16 source views"):
        # CPU tensors: a scene that got as far as the device check would raise another error
        ops.HipScene(torch.zeros(nv, 8, 4, 4), torch.zeros(nv, 1, 4, 4), torch.zeros(nv, 1, 4, 4), torch.zeros(nv, 3, 4, 4),
                     torch.eye(4).repeat(nv, 1, 1), torch.ones(nv, 2), torch.ones(nv, 2), torch.tensor([4.0, 4.0]), 32.0)


def test_generic_chunking_scales_with_views():
    from diner_amd import ops
    base = ops.GENERIC_POINTS_PER_LAUNCH
    for nv in (1, 2, 3, 4):
        assert ops.generic_points_per_launch(nv) == base
    assert ops.generic_points_per_launch(8) == base // 2
    assert ops.generic_points_per_launch(16) == base // 4
    assert ops.generic_points_per_launch(6) * 6 <= base * 4
