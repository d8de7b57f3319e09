"""CPU: the opacity / depth-spread entries of the C ABI (pix_alpha of nerf_renderer.py:359, which the reference computes and drops).

  1. the four new symbols resolve and the ABI version is still 6;
  2. each refuses a null colour pointer, K = 0 and K = 1025 with DINER_E_INVALID and a message, before any device work (dummy pointers,
     never dereferenced; the render entries with a zeroed scene and no handle, which a field launch would have to refuse first);
  3. NeRFRendererDGS.forward keeps its default signature and output keys."""
import ctypes as C
import inspect

import pytest

NEW = ("diner_composite_aux_f32", "diner_render_aux_f32", "diner_render_views_aux_f32", "diner_composite_aux_bwd_f32")


def _calls(lib, _lib):
    """name -> f(colour pointer, K): the entry with dummy arguments; `colour` is rgb_out (g_rgb for the backward)."""
    p = C.c_void_p(8)
    s = _lib.DinerScene()
    s.nv = 4
    sc = C.byref(s)
    return {
        "diner_composite_aux_f32": lambda rgb, K: lib.diner_composite_aux_f32(p, p, p, 4, K, 0, rgb, p, None, p, p, None),
        "diner_render_aux_f32": lambda rgb, K: lib.diner_render_aux_f32(sc, p, p, p, 4, K, 0, 0, rgb, p, None, p, p, p, p, None),
        "diner_render_views_aux_f32": lambda rgb, K: lib.diner_render_views_aux_f32(sc, p, p, p, 4, K, 0, 0, rgb, p, None, p, p, p, p, None),
        "diner_composite_aux_bwd_f32": lambda rgb, K: lib.diner_composite_aux_bwd_f32(p, p, p, 4, K, 0, rgb, None, p, p, None),
    }


def test_aux_symbols_resolve():
    from diner_amd import _lib
    lib = _lib.load()
    assert lib.diner_abi_version() == 6
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None


@pytest.mark.parametrize("name", NEW)
def test_aux_entries_refuse_bad_arguments_before_device_work(name):
    from diner_amd import _lib
    lib = _lib.load()
    call = _calls(lib, _lib)[name]
    p = C.c_void_p(8)
    for what, rgb, K, needle in (("null colour pointer", None, 40, b"null"), ("K = 0", p, 0, b"K=0"), ("K = 1025", p, 1025, b"K=1025")):
        assert call(rgb, K) == _lib.E_INVALID, (name, what)
        msg = lib.diner_last_error()
        assert needle in msg and b"aux" in msg, (name, what, msg)


def test_forward_default_signature_and_keys():
    from src.models.nerf_renderer import NeRFRendererDGS
    sig = inspect.signature(NeRFRendererDGS.forward)
    assert list(sig.parameters) == ["self", "model", "rays", "want_weights", "want_alpha"]
    assert sig.parameters["want_weights"].default is False and sig.parameters["want_alpha"].default is False
    out = NeRFRendererDGS()._format_outputs(None, 1, 2, want_weights=False)
    assert sorted(out.keys()) == ["depth", "rgb"] and "alpha" not in out
