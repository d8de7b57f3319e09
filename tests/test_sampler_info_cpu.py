"""CPU: the info entries of the depth-guided sampler (diner_sample_depthguided_info_f32 / _info_long_f32: the sampler's z plus the
reference's slot order, per-slot likelihoods and candidate indices, per-ray stats) -- exported, listed in the ctypes signatures with
their namesakes' arguments, refusing out-of-range arguments with a message before any device work."""
import ctypes as C

import pytest

INFO = {"diner_sample_depthguided_info_f32": "diner_sample_depthguided_f32",
        "diner_sample_depthguided_info_long_f32": "diner_sample_depthguided_long_f32"}
INFO_B, INFO_L = INFO


def test_info_entries_exported():
    from diner_amd import _lib
    lib = _lib.load()
    for name, plain in INFO.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        pres, pargs = _lib.SIGNATURES[plain]
        # the namesake's arguments with z_unfilled replaced by z_ordered, slot_L, slot_idx, stats
        assert res == pres and args == pargs[:-2] + [C.c_void_p] * 4 + pargs[-1:]
    assert _lib.SIGNATURES[INFO_B] == _lib.SIGNATURES[INFO_L]
    assert lib.diner_abi_version() == 6


@pytest.mark.parametrize("name", [INFO_B, INFO_L])
def test_info_entries_refuse_out_of_range_without_gpu(name):
    from diner_amd import _lib
    lib = _lib.load()
    entry = getattr(lib, name)
    long = name == INFO_L
    p = C.c_void_p(8)                 # never dereferenced: the checks run before any device work
    scene = _lib.DinerScene()

    def sample(n_cand, K, G, scene_=C.byref(scene), rays=p, t_base=p, z=p, NR=4, r0=0):
        return entry(scene_, rays, NR, n_cand, K, G, 0.05, t_base, None, None, None, 0, r0, z, p, p, p, p, None)

    who = b"sample_depthguided_info_long" if long else b"sample_depthguided_info:"
    bad = [(1000, 64, 65, b"n_gaussian"), (1000, 64, -1, b"n_gaussian"), (0, 64, 24, b"n_cand"), (1000, 0, 0, b"K")]
    if long:
        bad += [(1000, 1025, 96, b"K=1025"), (4097, 512, 96, b"n_cand=4097"), (1000, 512, 513, b"n_gaussian")]
    else:
        bad += [(1000, 257, 24, b"K=257"), (1025, 64, 24, b"n_cand=1025")]
    for (n_cand, K, G, what) in bad:
        assert sample(n_cand, K, G) == _lib.E_INVALID, (n_cand, K, G)
        msg = lib.diner_last_error()
        assert what in msg and who in msg, msg
    for kw in (dict(scene_=None), dict(rays=None), dict(t_base=None), dict(z=None)):
        assert sample(1000, 64, 24, **kw) == _lib.E_INVALID and b"null" in lib.diner_last_error(), kw
    assert sample(1000, 64, 24, NR=0) == _lib.E_INVALID and b"NR" in lib.diner_last_error()
    assert sample(1000, 64, 24, r0=-1) == _lib.E_INVALID and b"ray_index0" in lib.diner_last_error()
    assert sample(1000, 64, 24, r0=(1 << 32) - 3) == _lib.E_INVALID and b"ray_index0" in lib.diner_last_error()
    # the same codes as the namesake on the same arguments
    plain = getattr(lib, INFO[name])
    for (n_cand, K, G, _) in bad:
        assert plain(C.byref(scene), p, 4, n_cand, K, G, 0.05, p, None, None, None, 0, 0, p, None, None) == _lib.E_INVALID
