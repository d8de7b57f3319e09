"""CPU: the C ABI and the Python classification of the view-grouped field path -- scenes with 1 to 16 source views on the fused kernels,
four views at a time (the *_views entries of include/diner_hip.h; GPU parity: tests/test_view_groups_gpu.py).

  1. the new symbols exist and the ABI version stays 6;
  2. diner_scene_proj_views_bytes: 3 nv Hf Wf 512 4 bytes for 1 <= nv <= 16, else 0;
  3. nv outside [1, 16] is DINER_E_INVALID from every new entry before any device work (dummy pointers, never dereferenced);
  4. ops.fused_shape_any_views / fused_shape, and the modules' classification of a six-view scene;
  5. codegen: the view-group instance of the f16x3 per-view kernel carries no scratch access, like the shipped instance."""
import ctypes as C
import os

import pytest

from tests.test_many_views_cpu import _scene

NEW = ("diner_scene_proj_views_bytes", "diner_scene_prepare_views_f32", "diner_field_views_workspace_bytes",
       "diner_field_from_rays_views_f32", "diner_field_from_points_views_f32", "diner_render_views_f32")


def test_new_symbols_and_abi_version():
    from diner_amd import _lib
    lib = _lib.load()
    for sym in NEW:
        assert sym in _lib.SIGNATURES and hasattr(lib, sym), sym
    assert lib.diner_abi_version() == 6 and _lib.ABI_VERSION == 6
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diner_hip.h")).read()
    assert "#define DINER_ABI_VERSION 6" in hdr
    for sym in NEW:
        assert sym + "(" in hdr, sym


def test_scene_proj_views_bytes():
    from diner_amd import _lib
    lib = _lib.load()
    for nv in (1, 3, 4, 6, 16):
        s = _scene(nv)
        assert lib.diner_scene_proj_views_bytes(C.byref(s)) == 3 * nv * 8 * 8 * 512 * 4, nv
    for nv in (0, 17):
        s = _scene(nv)
        assert lib.diner_scene_proj_views_bytes(C.byref(s)) == 0, nv
    # the four-view query keeps its refusal of 5..16 views, and the hand-over does not depend on the view count
    assert lib.diner_scene_proj_bytes(C.byref(_scene(6))) == 0
    assert lib.diner_field_views_workspace_bytes(1000) == lib.diner_field_workspace_bytes(1000) > 0
    assert lib.diner_field_views_workspace_bytes(0) == 0


@pytest.mark.parametrize("nv", [0, 17])
def test_new_entries_refuse_nv_outside_1_16(nv):
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(8)                 # never dereferenced: the view check comes before the handle, the sizes or the device
    s = _scene(nv)
    sc = C.byref(s)
    calls = {
        "scene_prepare_views": lambda: lib.diner_scene_prepare_views_f32(sc, p, p, None),
        "field_from_rays_views": lambda: lib.diner_field_from_rays_views_f32(sc, p, p, p, 4, 8, 1, p, p, None),
        "field_from_points_views": lambda: lib.diner_field_from_points_views_f32(sc, p, p, p, 32, 1, p, p, None),
        "render_views": lambda: lib.diner_render_views_f32(sc, p, p, p, 4, 8, 0, 1, p, p, None, p, p, None),
    }
    for name, call in calls.items():
        assert call() == _lib.E_INVALID, name
        msg = lib.diner_last_error()
        assert f"nv={nv} outside [1,16]".encode() in msg, (name, msg)


def test_fused_shape_any_views():
    from diner_amd import ops
    shipped = (55, 512, 512, 4, 5, 3)
    for nv in range(1, 17):
        assert ops.fused_shape_any_views(*shipped, nv=nv), nv
    assert not ops.fused_shape_any_views(*shipped, nv=0) and not ops.fused_shape_any_views(*shipped, nv=17)
    assert not ops.fused_shape_any_views(55, 512, 256, 4, 5, 3, nv=6)           # another d_hidden
    assert not ops.fused_shape_any_views(*shipped, nv=6, num_freqs=4) and not ops.fused_shape_any_views(*shipped, nv=6, beta=1.0)
    assert ops.fused_shape(*shipped, nv=4) and not ops.fused_shape(*shipped, nv=6)


def test_resnetfc_classification_keeps_the_generic_path_for_explicit_matrices():
    from src.models.resnetfc import ResnetFC
    m = ResnetFC(d_in=55, d_latent=512, n_blocks=5, d_hidden=512, combine_layer=3)
    assert not m.is_fused_shape(nv=6) and m.is_fused_shape_any_views(nv=6) and m.is_fused_shape_any_views(nv=1)
    assert not m.is_fused_shape_any_views(nv=17)
    assert not ResnetFC(d_in=55, d_latent=512, n_blocks=5, d_hidden=128, combine_layer=3).is_fused_shape_any_views(nv=6)


def test_view_group_kernel_codegen(tmp_path):
    """The view-group instance of the f16x3 per-view kernel (k_field_views_h3n) is the shipped body plus a selected, scaled sum: as many
    MFMAs, no scratch access at all, no packed-fp32 arithmetic inside the MFMA streams beyond the shipped instance's allowance."""
    import re
    import shutil
    import subprocess
    from diner_amd import build as B
    hipcc = B._hipcc()
    if not (hipcc and (shutil.which(hipcc) or os.path.exists(hipcc))):
        pytest.skip("hipcc not available")
    out = tmp_path / "mlp_h3n.s"
    subprocess.check_call([hipcc] + B.FLAGS + ["-x", "hip", "-S", "--cuda-device-only", os.path.join(B.CSRC, "mlp_h3n.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    txt = out.read_text()
    bodies = {}
    for name in ("k_field_views_h3n", "k_field_pre_h3n"):
        m = re.search(r"^(\w*\d" + name + r"[EI]\w*):.*?\n(.*?)\.Lfunc_end", txt, re.S | re.M)
        assert m, name
        bodies[name] = m.group(2).split("\n")
    n_mfma = {k: sum("v_mfma_f32_16x16x32_f16" in l for l in b) for k, b in bodies.items()}
    assert n_mfma["k_field_views_h3n"] == n_mfma["k_field_pre_h3n"] > 1500, n_mfma
    assert not [l for l in bodies["k_field_views_h3n"] if "scratch_" in l]
