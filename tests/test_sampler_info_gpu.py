"""GPU: the info entries of the depth-guided sampler (diner_sample_depthguided_info_f32 / _info_long_f32) -- the unfilled samples in
the reference's slot order (picks by descending surface likelihood, then the gaussian samples, nerf_renderer.py:172-190), the
likelihood and candidate index of every pick slot, and per ray (sum L, sum O, mean, sigma) of the gaussian fit -- through ops, the
drop-in NeRFRendererDGS.sample_depthguided and diner_amd.render.predict_surface_prior.

The oracle's L, O and z_cand (CPU) are the reference's on the fixtures G3 / G22 / G23, whose z_unfilled is stored in the reference's
order.  SAT_L (tests/helpers.py) bounds how far two erf implementations move a likelihood; a slot is PINNED when its oracle likelihood
is >= SAT_L and at least SAT_L away from both neighbours in the ray's descending order.  Per case:
  A  every slot: |slot_L - oracle's sorted L| <= SAT_L;
  B  pinned slots: slot_idx is the oracle's argsort index and z_ordered the fixture's z_unfilled bit for bit; pinned >= 95 % of the
     positive slots on every fixture;
  C  every positive slot: z_ordered is the oracle's candidate depth at slot_idx bit for bit; slot_L non-increasing; a slot is empty
     (idx -1, L 0, z 0) exactly when slot_L == 0; beyond the oracle's positive count a device slot is positive only below SAT_L;
  D  gaussian columns against the fixture at rtol 3e-6 / atol 1e-7 where sum O >= 1e-2;
  E  the four stats;
  F  z of the info call is the plain call's bit for bit and z_ordered is a permutation of its z_unfilled (explicit and Philox noise);
  G  edges on small seeded scenes; H the module; I predict_surface_prior."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, SAT_L

pytestmark = pytest.mark.gpu
RED = 3e-6            # reduction-order bar of the gaussian slots (test_hip_parity.py::test_sampler_and_fill)
COND = 1e-2           # sum O of a conditioned fit


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


# ---------------------------------------------------------------------------------------------------------------- the oracle's side
def oracle_slots(scene, rays, K, n_cand, G, nc):
    """The oracle's candidates in the reference's order, cut / padded to the K - G pick slots, the pinned slots and the ray stats."""
    zc = O.sample_coarse(rays, n_cand, nc)
    L, Oq = O.point_likelihood(scene, rays, zc)
    NR, want = rays.shape[0], K - G
    Ls, order = L.sort(dim=-1, descending=True, stable=True)          # equal likelihoods: lower candidate index first
    inf = torch.full((NR, 1), float("inf"))
    up = torch.cat([inf, Ls[:, :-1]], 1) - Ls
    dn = Ls - torch.cat([Ls[:, 1:], -inf], 1)
    pin = (Ls >= SAT_L) & (up >= SAT_L) & (dn >= SAT_L)
    n = min(want, n_cand)
    Lw, iw, pw = torch.zeros(NR, want), torch.full((NR, want), -1, dtype=torch.long), torch.zeros(NR, want, dtype=torch.bool)
    Lw[:, :n], iw[:, :n], pw[:, :n] = Ls[:, :n], order[:, :n], pin[:, :n]
    iw[Lw == 0] = -1
    mean, std = torch.zeros(NR), torch.zeros(NR)
    seen = (Oq != 0).any(-1)
    if seen.any():
        m, s = O.weighted_mean_n_std(zc[seen], Oq[seen])
        mean[seen], std[seen] = m[:, 0], s[:, 0]
    return types.SimpleNamespace(zc=zc, L=L, Lw=Lw, iw=iw, pinned=pw, sum_L=L.sum(-1), sum_O=Oq.sum(-1), mean=mean, std=std,
                                 npos=(L > 0).sum(-1), n_cand=n_cand)


def check_slots(tag, orc, info, K, G, ref_unfilled=None, min_pinned=None):
    """A, B, C, D of the module docstring; info: SamplerInfo on the CPU."""
    want, NR = K - G, info.z_ordered.shape[0]
    zo, sl, si = info.z_ordered, info.slot_L, info.slot_idx.long()
    assert zo.shape == (NR, K) and sl.shape == (NR, want) and si.shape == (NR, want)
    if want > 0:
        zp = zo[:, :want]
        # A
        dist = (sl - orc.Lw).abs().max().item()
        print(f"{tag}: A largest |slot_L - oracle| {dist:.2e} (SAT_L {SAT_L:.1e})")
        assert dist <= SAT_L
        # C
        pos = sl > 0
        assert (sl >= 0).all() and (sl[:, 1:] <= sl[:, :-1]).all()
        assert torch.equal(si == -1, ~pos) and torch.equal(zp == 0, ~pos)
        assert (si[pos] < orc.n_cand).all()
        rows = torch.arange(NR)[:, None].expand(NR, want)
        assert torch.equal(zp[pos], orc.zc[rows[pos], si[pos]])
        tie = pos[:, 1:] & (sl[:, 1:] == sl[:, :-1])
        assert (si[:, 1:][tie] > si[:, :-1][tie]).all()              # equal likelihood bits: lower candidate index first
        beyond = torch.arange(want)[None] >= (orc.Lw > 0).sum(-1, keepdim=True)
        assert (sl[beyond & pos] < SAT_L).all()
        # B
        n_pos, n_pin = int((orc.Lw > 0).sum()), int(orc.pinned.sum())
        share = n_pin / max(n_pos, 1)
        print(f"{tag}: B pinned {n_pin} of {n_pos} positive slots ({100 * share:.1f} %)")
        if min_pinned is not None:
            assert share >= min_pinned
        assert torch.equal(si[orc.pinned], orc.iw[orc.pinned])
        if ref_unfilled is not None:
            assert torch.equal(zp[orc.pinned], ref_unfilled[:, :want][orc.pinned])
    if ref_unfilled is not None and G > 0:
        cond = orc.sum_O >= COND                                       # D
        assert torch.allclose(zo[cond, want:], ref_unfilled[cond, want:], rtol=RED, atol=1e-7)
    if G > 0:
        assert (zo[orc.sum_O == 0, want:] == 0).all()


def check_stats(tag, orc, info, ref_sum_L=None, ref_sum_O=None):
    """E.  The float32-versus-float64 spread of the oracle's own evaluation: 1.6e-7 relative on sum L, 3e-7 on the mean,
    1.3e-7 relative on sigma."""
    ref_L = orc.sum_L if ref_sum_L is None else ref_sum_L
    ref_O = orc.sum_O if ref_sum_O is None else ref_sum_O
    slack = SAT_L * orc.npos.float()
    dL, dO = (info.sum_L - ref_L).abs(), (info.sum_O - ref_O).abs()
    cond = orc.sum_O >= COND
    dm = ((info.prior_depth - orc.mean).abs() / orc.mean.abs().clamp(min=1e-30))[cond]
    ds = ((info.prior_std - orc.std).abs() / orc.mean.abs().clamp(min=1e-30))[cond]
    rel = lambda d, r: (d / r.abs().clamp(min=1e-30))[cond].max().item() if cond.any() else 0.0
    print(f"{tag}: E on {int(cond.sum())} conditioned rays: sum_L rel {rel(dL, ref_L):.2e}, sum_O rel {rel(dO, ref_O):.2e}, "
          f"mean rel {dm.max().item() if cond.any() else 0.0:.2e}, sigma / mean {ds.max().item() if cond.any() else 0.0:.2e}")
    assert (dL <= RED * ref_L.abs() + slack).all() and (dO <= RED * ref_O.abs() + slack).all()
    assert (dm <= RED).all() and (ds <= RED).all()
    for none in (orc.sum_O == 0, info.sum_O == 0):
        for f in ("sum_L", "sum_O", "prior_depth", "prior_std"):
            assert (getattr(info, f)[none] == 0).all(), f
    assert (info.sum_O >= 0).all() and (info.prior_std >= 0).all()


def cpu(info):
    return type(info)(*[t.cpu() for t in info])


def same_info(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def check_unchanged(ops, hs, rc, K, n_cand, G, nz):
    """F: explicit noise and seed = 11 Philox noise, ray_index0 = 5, the long entry and (where it fits) the bounded one.
    -> (z, info) of the explicit-noise call on the long entry, on the CPU."""
    entries = [ops.sample_depthguided_long] + ([ops.sample_depthguided] if K <= 256 and n_cand <= 1024 else [])
    keep = None
    for noise in (nz, None):
        first = None
        for fn in entries:
            z_p, zu_p = fn(hs, rc, K, n_cand, G, 0.05, noise=noise, seed=11, want_unfilled=True, ray_index0=5)
            z_i, info = fn(hs, rc, K, n_cand, G, 0.05, noise=noise, seed=11, ray_index0=5, want_info=True)
            assert torch.equal(z_i, z_p), (fn.__name__, noise is None)
            assert torch.equal(info.z_ordered.sort(-1).values, zu_p.sort(-1).values), (fn.__name__, noise is None)
            if first is None:
                first = (z_i, info)
            else:                                                     # the long entry runs the bounded info kernel where it fits
                assert torch.equal(first[0], z_i) and same_info(first[1], info)
        if noise is not None:
            keep = (first[0].cpu(), cpu(first[1]))
    return keep


# ------------------------------------------------------------------------------------------------------- fixtures G3 / G22 / G23
@functools.lru_cache(maxsize=None)
def fixture_case(name):
    """-> (scene dict, K, n_cand, G, rays, (nc, ng, nf), the reference's z_unfilled, its sum L / sum O per ray or None, oracle slots)"""
    kind, *rest = name.split("_")
    fix_L = fix_O = None
    if kind == "g3":
        from tests.test_hip_parity import _sampler_case
        K = int(rest[0])
        g, sc, scene, rs, nz = _sampler_case(K)
        n_cand, G, ref_u = 1000, int(g["G"]), T(g["z_unfilled"])
        fix_L, fix_O = T(g["L_sum"]), T(g["O_sum"])
    elif kind == "g22":
        from tests.test_long_rays_cpu import long_inputs
        K = int(rest[0])
        g, sc, scene, _, rs, noises = long_inputs()
        n_cand, G = {int(c[0]): (int(c[1]), int(c[2])) for c in g["configs"].tolist()}[K]
        nz, ref_u = noises[K], T(g[f"z_unfilled_{K}"])
    else:
        from tests.test_many_views_cpu import nv_inputs
        nv, K = int(rest[0]), int(rest[1])
        g = load("g23_many_views.npz")
        sc, scene, _, rs, noises = nv_inputs(g, nv)
        nz = noises[K]
        n_cand, G, ref_u = int(g["n_cand"]), nz[1].shape[1], T(g[f"z_unfilled_{nv}_{K}"])
    return sc, K, n_cand, G, rs, nz, ref_u, fix_L, fix_O, oracle_slots(scene, rs, K, n_cand, G, nz[0])


FIXTURES = ["g3_64", "g3_128", "g22_512", "g22_1024", "g23_6_64", "g23_8_64", "g23_16_64", "g23_8_320"]


@pytest.mark.parametrize("name", FIXTURES)
def test_info_against_reference_fixtures(ops, name):
    """A-F on the reference's fixtures: bounded and wide kernels, 4-view and wide-scene instances.  Measured on MI355X: see DESIGN.md 8d."""
    sc, K, n_cand, G, rs, nz, ref_u, fix_L, fix_O, orc = fixture_case(name)
    hs, rc = hip_scene(ops, sc), rs.cuda()
    z, info = check_unchanged(ops, hs, rc, K, n_cand, G, tuple(t.cuda() for t in nz))
    check_slots(name, orc, info, K, G, ref_unfilled=ref_u, min_pinned=0.95)
    check_stats(name, orc, info, fix_L, fix_O)
    assert torch.equal(O.fill_up_uniform_samples(info.z_ordered, rs, nz[2]), z)


# ----------------------------------------------------------------------------------------------------------------------- G edges
@functools.lru_cache(maxsize=None)
def small_scene(nv):
    sc, scene, _, _, rays = oracle_setup(24, 24, 40 + nv, nv=nv)
    return sc, scene, rays


def edge_rays(rays, NR):
    """NR rays through the middle of the frame (they meet the surface)."""
    n = rays.shape[0]
    return rays[torch.linspace(0.3 * n, 0.7 * n, NR).long()].contiguous()


def noise_for(NR, n_cand, G, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(NR, n_cand, generator=g), torch.randn(NR, G, generator=g), torch.rand(NR, K, generator=g)


EDGES = sorted({(K, G, 1000, 4) for K in (1, 2, 63, 65, 256) for G in (0, K // 3, K)}
               | {(257, G, 1000, 4) for G in (0, 85, 257)}                                  # the wide kernel starts at K = 257
               | {(64, 21, n, 4) for n in (1, 1000, 1024, 1025)}                            # ... and at 1025 candidates
               | {(K, 21, 1000, nv) for K in (64, 257) for nv in (1, 4, 5)})


@pytest.mark.parametrize("K,G,n_cand,nv", EDGES)
def test_info_edges(ops, K, G, n_cand, nv):
    """1 / 3 / 5 rays (a partial block of the four-rays-per-workgroup kernel: dead waves shadow the last ray): A, C, E, F."""
    sc, scene, rays = small_scene(nv)
    hs = hip_scene(ops, sc)
    for NR in (1, 3, 5):
        rs = edge_rays(rays, NR)
        nz = noise_for(NR, n_cand, G, K, 1000 * K + G + NR)
        orc = oracle_slots(scene, rs, K, n_cand, G, nz[0])
        assert n_cand < 1000 or (orc.sum_O > 0).any()
        z, info = check_unchanged(ops, hs, rs.cuda(), K, n_cand, G, tuple(t.cuda() for t in nz))
        tag = f"K={K} G={G} n_cand={n_cand} NV={nv} NR={NR}"
        check_slots(tag, orc, info, K, G)
        check_stats(tag, orc, info)
        assert torch.equal(O.fill_up_uniform_samples(info.z_ordered, rs, nz[2]), z)


@pytest.mark.parametrize("K,G,n_cand", [(64, 24, 1000), (300, 100, 1000)], ids=["bounded", "wide"])
def test_info_rays_that_see_no_surface(ops, K, G, n_cand):
    """Rays that look away from every source view: all slots empty, all stats 0, z a plain stratification."""
    sc, scene, rays = small_scene(4)
    rs = edge_rays(rays, 5)
    rs[:, 3:6] = -rs[:, 3:6]
    nz = noise_for(5, n_cand, G, K, K)
    orc = oracle_slots(scene, rs, K, n_cand, G, nz[0])
    assert (orc.L == 0).all(), "the rays were meant to miss every view"
    z, info = check_unchanged(ops, hip_scene(ops, sc), rs.cuda(), K, n_cand, G, tuple(t.cuda() for t in nz))
    check_slots("away", orc, info, K, G)
    check_stats("away", orc, info)
    assert (info.z_ordered == 0).all() and (info.slot_L == 0).all() and (info.slot_idx == -1).all()
    assert all((getattr(info, f) == 0).all() for f in ("sum_L", "sum_O", "prior_depth", "prior_std"))
    assert torch.equal(z, O.fill_up_uniform_samples(torch.zeros(5, K), rs, nz[2]))


def raw_info(ops, entry, hs, rc, n_cand, K, G, nz, zo, sl, si, st):
    """The C entry with the output pointers as given (None = NULL) -> z."""
    from diner_amd import _lib
    NR = rc.shape[0]
    z = torch.empty(NR, K, device="cuda")
    _lib.check(entry(hs.ref, ops._ptr(rc), NR, n_cand, K, G, 0.05, ops._ptr(ops._t_base(n_cand, rc.device)), ops._ptr(nz[0]),
                     ops._ptr(nz[1]), ops._ptr(nz[2]), C.c_uint64(0), 0, ops._ptr(z), ops._ptr(zo), ops._ptr(sl), ops._ptr(si),
                     ops._ptr(st), ops._stream()))
    return z


@pytest.mark.parametrize("K,G,n_cand", [(65, 21, 1000), (257, 85, 1025)], ids=["bounded", "wide"])
def test_info_each_output_alone(ops, K, G, n_cand):
    """Every output pointer NULL except one, in turn (and all NULL): what is written is the full call's, z always."""
    from diner_amd import _lib
    lib = _lib.load()
    sc, scene, rays = small_scene(4)
    hs, rc = hip_scene(ops, sc), edge_rays(rays, 5).cuda()
    nz = tuple(t.cuda() for t in noise_for(5, n_cand, G, K, 9))
    z_full, full = ops.sample_depthguided_long(hs, rc, K, n_cand, G, 0.05, noise=nz, want_info=True)
    full_st = torch.stack((full.sum_L, full.sum_O, full.prior_depth, full.prior_std), -1)
    want = (full.z_ordered, full.slot_L, full.slot_idx, full_st)
    entries = [lib.diner_sample_depthguided_info_long_f32] + ([lib.diner_sample_depthguided_info_f32] if K <= 256 else [])
    for entry in entries:
        for only in (None, 0, 1, 2, 3):
            bufs = [torch.empty_like(t) if i == only else None for i, t in enumerate(want)]
            z = raw_info(ops, entry, hs, rc, n_cand, K, G, nz, *bufs)
            assert torch.equal(z, z_full), only
            if only is not None:
                assert torch.equal(bufs[only], want[only]), only


@pytest.mark.parametrize("K,n_cand", [(24, 1000), (300, 1000)], ids=["bounded", "wide"])
def test_info_no_pick_slots(ops, K, n_cand):
    """K - G = 0: nothing to order; slot_L / slot_idx buffers handed in anyway keep their sentinels."""
    from diner_amd import _lib
    lib = _lib.load()
    sc, scene, rays = small_scene(4)
    rs = edge_rays(rays, 5)
    hs, rc = hip_scene(ops, sc), rs.cuda()
    nz = noise_for(5, n_cand, K, K, 3)
    nzc = tuple(t.cuda() for t in nz)
    sl = torch.full((5, 8), -7.0, device="cuda")
    si = torch.full((5, 8), -7, device="cuda", dtype=torch.int32)
    zo, st = torch.empty(5, K, device="cuda"), torch.empty(5, 4, device="cuda")
    z = raw_info(ops, lib.diner_sample_depthguided_info_long_f32, hs, rc, n_cand, K, K, nzc, zo, sl, si, st)
    assert (sl == -7.0).all() and (si == -7).all()
    z_p, zu_p = ops.sample_depthguided_long(hs, rc, K, n_cand, K, 0.05, noise=nzc, want_unfilled=True)
    assert torch.equal(z, z_p) and torch.equal(zo, zu_p)             # gaussian slots only: the order is the plain kernel's
    z_i, info = ops.sample_depthguided_long(hs, rc, K, n_cand, K, 0.05, noise=nzc, want_info=True)
    assert info.slot_L.shape == (5, 0) and torch.equal(z_i, z) and torch.equal(info.z_ordered, zo)
    orc = oracle_slots(scene, rs, K, n_cand, K, nz[0])
    check_stats(f"K=G={K}", orc, cpu(info))
    assert torch.equal(st.cpu(), torch.stack(cpu(info)[3:], -1))


# ---------------------------------------------------------------------------------------------------------------------- H module
def test_module_sample_depthguided_reference_order(ops):
    """NeRFRendererDGS.sample_depthguided on G3 K = 64 with injected noise: the reference's z_unfilled at the pinned slots and the
    gaussian columns; return_info delivers the ops values; its fill is forward's samples."""
    from diner_amd import noise
    from diner_amd.synthetic import build_modules, make_mlp_state_dict
    sc, K, n_cand, G, rs, nz, ref_u, _, _, orc = fixture_case("g3_64")
    nerf, R = build_modules(sc, make_mlp_state_dict(), "cuda", normals=sc["normals"])
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=True)
    r = rs.cuda()[None]
    inj = tuple(t[None].cuda() for t in nz)
    with noise.inject(*inj), torch.no_grad():
        zu = ren.sample_depthguided(r, nerf, K, n_cand, n_gaussian=G)
        zu2, info = ren.sample_depthguided(r, nerf, K, n_cand, n_gaussian=G, return_info=True)
        filled = ren.fill_up_uniform_samples(zu, r)
        fwd = ren.forward(nerf, r, want_weights=True)
    assert zu.shape == (1, rs.shape[0], K) and torch.equal(zu, zu2)
    want = K - G
    z0 = zu[0].cpu()
    assert torch.equal(z0[:, :want][orc.pinned], ref_u[:, :want][orc.pinned])
    cond = orc.sum_O >= COND
    assert torch.allclose(z0[cond, want:], ref_u[cond, want:], rtol=RED, atol=1e-7)
    _, oinfo = ops.sample_depthguided_long(nerf.hip_scene(0), r[0], K, n_cand, G, 0.05, noise=tuple(t[0] for t in inj), want_info=True)
    assert torch.equal(zu[0], oinfo.z_ordered)
    for f in ("slot_L", "slot_idx", "sum_L", "sum_O", "prior_depth", "prior_std"):
        assert torch.equal(info[f][0], getattr(oinfo, f)), f
    # forward's samples: the compositor's weights are a function of them; compare the samples themselves through the plain entry
    z_fwd = ops.sample_depthguided_long(nerf.hip_scene(0), r[0], K, n_cand, G, 0.05, noise=tuple(t[0] for t in inj))
    assert torch.equal(filled[0], z_fwd)
    rgb = ops.render(nerf.hip_scene(0), nerf.hip_mlp(), r[0], filled[0], True)[1]
    assert torch.equal(rgb, fwd.fine.rgb[0])


# ------------------------------------------------------------------------------------------------------- I predict_surface_prior
def test_predict_surface_prior(ops):
    """Two objects, 64 x 48 targets: the maps are the info of the same rays sampled in one batch -- through ops for object 0, and for
    both objects through NeRFRendererDGS.sample_depthguided under the frame key (the per-object noise key is the renderer's)."""
    from tests.test_boundary_gpu import setup_model
    from diner_amd import noise
    from diner_amd.render import predict_surface_prior
    W, H = 64, 48
    sc, nerf, R, rays = setup_model(W, H, 5)
    sc2, nerf2, _, _ = setup_model(W, H, 6)
    enc, enc2 = nerf.encoder, nerf2.encoder
    for name in ("depths", "depths_std", "normals", "latent"):
        setattr(enc, name, torch.cat([getattr(enc, name), getattr(enc2, name)]))
    enc.nobjects = 2
    nerf.poses, nerf.c, nerf.focal = (torch.cat([getattr(nerf, n), getattr(nerf2, n)]) for n in ("poses", "c", "focal"))
    E = torch.stack([sc["target_extrinsics"], sc2["target_extrinsics"]]).cuda()
    Kt = torch.stack([sc["target_intrinsics"], sc2["target_intrinsics"]]).cuda()
    K, n_cand, G = 40, 1000, 15
    maps = [predict_surface_prior(nerf, E, Kt, W, H, sc["znear"], sc["zfar"], K, n_cand, G, ray_batch_size=bs, seed=321)
            for bs in (1000, 8192)]
    rl = ops.gen_rays(E, Kt, W, H, sc["znear"], sc["zfar"], "cuda")
    _, info = ops.sample_depthguided_long(nerf.hip_scene(0), rl[0], K, n_cand, G, 0.05, seed=321, ray_index0=0, want_info=True)
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=True)
    with noise.keyed(321, 0):
        _, minfo = ren.sample_depthguided(rl, nerf, K, n_cand, n_gaussian=G, return_info=True)
    assert not torch.equal(minfo.sum_O[0], minfo.sum_O[1])
    for m in maps:
        for got, ref, mref in zip(m, (info.sum_O, info.prior_depth, info.prior_std), (minfo.sum_O, minfo.prior_depth, minfo.prior_std)):
            assert got.shape == (2, 1, H, W) and torch.equal(got[0], ref.view(1, H, W)) and torch.equal(got, mref.view(2, 1, H, W))
    hit, depth, dstd = maps[0]
    assert (hit >= 0).all() and (hit <= 1).all() and (hit[0] > 0).any() and (hit[1] > 0).any()
    seen = hit > 0
    assert (depth[seen] >= sc["znear"]).all() and (depth[seen] <= sc["zfar"]).all()
    assert (depth[~seen] == 0).all() and (dstd[~seen] == 0).all() and (dstd >= 0).all()
