"""CPU: the long-ray entry points (K <= 1024 samples, n_cand <= 4096 candidates; the reference's --nsamples) -- exported, listed
in the ctypes signatures, refusing out-of-range arguments with a message before any device work -- and the oracle against the
reference's outputs at those sizes (tests/golden/g22_long_rays.npz, tools/make_golden_long_rays.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, sha, selection_diff, SAT_L

LONG = ("diner_sample_depthguided_long_f32", "diner_fill_uniform_long_f32", "diner_composite_long_f32")


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_long_entries_exported():
    from diner_amd import _lib
    lib = _lib.load()
    for name in LONG:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        # same signature as the bounded sibling
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_long", "")]
    assert lib.diner_abi_version() == 6


def test_long_entries_refuse_out_of_range_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(8)                 # never dereferenced: the checks run before any device work
    scene = _lib.DinerScene()

    def sample(n_cand, K, G, scene_=C.byref(scene), rays=p, z=p):
        return lib.diner_sample_depthguided_long_f32(scene_, rays, 4, n_cand, K, G, 0.05, p, None, None, None, 0, 0, z, None, None)

    for (n_cand, K, G, what) in ((1000, 1025, 96, b"K"), (4097, 512, 96, b"n_cand"), (1000, 512, 513, b"n_gaussian"),
                                 (0, 64, 24, b"n_cand"), (1000, 0, 0, b"K"), (1000, 64, -1, b"n_gaussian")):
        assert sample(n_cand, K, G) == _lib.E_INVALID, (n_cand, K, G)
        msg = lib.diner_last_error()
        assert what in msg and b"long" in msg, msg
    assert sample(1000, 64, 24, scene_=None) == _lib.E_INVALID and b"null" in lib.diner_last_error()
    assert sample(1000, 512, 24, rays=None) == _lib.E_INVALID and b"null" in lib.diner_last_error()
    assert sample(1000, 512, 24, z=None) == _lib.E_INVALID and b"null" in lib.diner_last_error()

    assert lib.diner_fill_uniform_long_f32(p, p, 4, 1025, None, 0, 0, p, None) == _lib.E_INVALID
    assert b"K=1025" in lib.diner_last_error()
    assert lib.diner_fill_uniform_long_f32(None, p, 4, 512, None, 0, 0, p, None) == _lib.E_INVALID
    assert b"null" in lib.diner_last_error()
    assert lib.diner_composite_long_f32(p, p, p, 4, 1025, 0, p, p, None, None) == _lib.E_INVALID
    assert b"K=1025" in lib.diner_last_error()
    assert lib.diner_composite_long_f32(p, None, p, 4, 512, 0, p, p, None, None) == _lib.E_INVALID
    assert b"null" in lib.diner_last_error()
    # the bounded entries keep their limits
    assert lib.diner_composite_f32(p, p, p, 4, 257, 0, p, p, None, None) == _lib.E_INVALID
    assert lib.diner_fill_uniform_f32(p, p, 4, 257, None, 0, 0, p, None) == _lib.E_INVALID
    assert lib.diner_sample_depthguided_f32(C.byref(scene), p, 4, 1000, 257, 24, 0.05, p, None, None, None, 0, 0, p, None,
                                            None) == _lib.E_INVALID


def long_inputs():
    """-> (fixture, scene dict, oracle Scene, weights, rays (64,8), {K: (nc, ng, nf)}) of g22_long_rays.npz."""
    g = load("g22_long_rays.npz")
    W, H = int(g["W"]), int(g["H"])
    sc, scene, w, msd, rays = oracle_setup(W, H, int(g["seed"]))
    gen = torch.Generator().manual_seed(int(g["noise_seed"]))
    NR = int(g["ray_idx"].shape[0])
    sel = torch.randperm(W * H, generator=gen)[:NR].sort().values
    assert torch.equal(sel, T(g["ray_idx"]))
    noises = {}
    for K, n_cand, G in g["configs"].tolist():
        noises[K] = (torch.rand(NR, n_cand, generator=gen), torch.randn(NR, G, generator=gen), torch.rand(NR, K, generator=gen))
        assert sha(*noises[K]) == str(g[f"in_sha_{K}"]), "seeded noise not reproducible on this host"
    return g, sc, scene, w, T(g["rays"]), noises


@pytest.mark.parametrize("K", [512, 1024])
def test_oracle_reproduces_reference_long_rays(K):
    g, sc, scene, w, rs, noises = long_inputs()
    cfg = {int(c[0]): (int(c[1]), int(c[2])) for c in g["configs"].tolist()}
    white = dict(zip([int(c[0]) for c in g["configs"].tolist()], g["white"].tolist()))[K]
    n_cand, G = cfg[K]
    nc, ng, nf = noises[K]
    NR = rs.shape[0]
    z0, aux = O.sample_depthguided(scene, rs, K, n_cand, G, nc, ng, return_aux=True)
    z = O.fill_up_uniform_samples(z0, rs, nf)
    assert z0.shape == (NR, K) and torch.all(z[:, 1:] >= z[:, :-1])
    ref_z0, ref_z = T(g[f"z_unfilled_{K}"]), T(g[f"z_{K}"])
    if not torch.equal(z0, ref_z0):
        # a host whose erf kernel differs from the pinning host's in the last bit (see selection_diff)
        bad, worst = selection_diff(ref_z0.sort(-1).values, z0.sort(-1).values, aux["L"], aux["z_cand"], K - G)
        assert worst < SAT_L and len(bad) <= 0.05 * NR
        good = torch.ones(NR, dtype=torch.bool)
        good[bad] = False
        assert torch.allclose(z[good], ref_z[good], rtol=3e-6, atol=1e-7)
    else:
        assert torch.equal(z, ref_z)
    np.testing.assert_allclose(aux["L"].sum(-1).numpy(), g[f"L_sum_{K}"], rtol=1e-6)
    # compositor on the reference's samples (field through MKL GEMMs: host-dependent association, as XHOST of test_oracle_golden)
    wo, rgbo, do, _ = O.composite(scene, w, rs, ref_z, bool(white))
    for name, got in (("rgb", rgbo), ("depth", do), ("weights", wo)):
        ref = T(g[f"{name}_{K}"])
        assert ((got - ref).abs().max() / ref.abs().max()).item() < 1e-5, name
