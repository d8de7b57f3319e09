"""CPU: TSDF fusion and surface nets (surface.hip, diner_amd.surface) -- the entries are declared, exported, bound and refuse bad
arguments before any device work; the Python layer is off by default and checks its arguments before touching a device; the mesh PLY
round-trips bit for bit and leaves write_ply's bytes alone; and the numpy restatement the GPU tests compare against
(tests/surface_util.py) is fit for purpose: on the analytic sphere it gives a closed, oriented mesh of Euler characteristic 2 within a
voxel of the sphere, and the share of voxels it must leave undecided stays under 2 %."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import surface_util as S
from tests.helpers import ROOT

ENTRIES = ("diner_tsdf_integrate_f32", "diner_surface_workspace_bytes", "diner_surface_count", "diner_surface_extract_f32")


def test_entries_declared_exported_and_bound():
    from diner_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "surface.hip" in build.SOURCES
    assert lib.diner_surface_workspace_bytes(16, 16, 16) == 4 * (4 + 2 * 16 + 4096)
    assert lib.diner_surface_workspace_bytes(1, 16, 16) == 0 and lib.diner_surface_workspace_bytes(16, 1025, 16) == 0


def test_entries_refuse_bad_arguments_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(16)                 # never dereferenced: the checks run before any device work
    origin = (C.c_float * 3)(0.0, 0.0, 0.0)
    Km = (C.c_float * (9 * 16))()
    E = (C.c_float * (16 * 16))()

    def integ(N=2, dims=(8, 8, 8), voxel=0.1, trunc=0.3, color4=p, color=p, tsdf=p):
        return lib.diner_tsdf_integrate_f32(tsdf, p, color4, *dims, origin, voxel, trunc, p, None, color, Km, E, N, 4, 4, 0, 0.0, None)

    for kw, what in ((dict(N=0), b"views"), (dict(N=17), b"views"), (dict(dims=(1, 8, 8)), b"dimension"), (dict(dims=(8, 1025, 8)), b"dimension"),
                     (dict(dims=(8, 8, 0)), b"dimension"), (dict(dims=(8, -8, 8)), b"dimension"),
                     (dict(dims=(1, 8, 8), N=0), b"views"), (dict(voxel=0.0), b"voxel"),
                     (dict(voxel=float("nan")), b"voxel"), (dict(trunc=0.0), b"truncation"), (dict(trunc=-1.0), b"truncation"),
                     (dict(color=None), b"color"), (dict(color4=None), b"color"), (dict(tsdf=None, color4=None, color=None), b"null")):
        assert integ(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())

    def count(dims=(8, 8, 8), ws=p, mw=0.0):
        return lib.diner_surface_count(p, p, *dims, mw, ws, p, None)

    for kw, what in ((dict(dims=(1, 8, 8)), b"dimension"), (dict(dims=(8, 8, 2048)), b"dimension"), (dict(ws=None), b"null"),
                     (dict(mw=float("nan")), b"min_weight")):
        assert count(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())

    def extract(dims=(8, 8, 8), voxel=0.1, nv=3, nq=1, verts=p, faces=p, ws=p):
        return lib.diner_surface_extract_f32(p, p, None, *dims, origin, voxel, 0.0, ws, nv, nq, verts, None, None, faces, None)

    for kw, what in ((dict(dims=(8, 1, 8)), b"dimension"), (dict(voxel=0.0), b"voxel"), (dict(nv=-1), b"counts"), (dict(nq=-1), b"counts"),
                     (dict(verts=None), b"vertices"), (dict(faces=None), b"quads"), (dict(ws=None), b"null")):
        assert extract(**kw) == _lib.E_INVALID and what in lib.diner_last_error(), (kw, lib.diner_last_error())


def test_python_surface_is_off_by_default_and_checks_before_the_device(tmp_path):
    from diner_amd import evaluate, ops, surface
    assert inspect.signature(evaluate.write_prediction_folder).parameters["write_mesh"].default is False
    sig = inspect.signature(surface.TsdfVolume.__init__).parameters
    assert (sig["trunc"].default, sig["color"].default) == (None, True)
    sig = inspect.signature(surface.TsdfVolume.integrate).parameters
    assert (sig["rgb"].default, sig["weight"].default, sig["carve"].default, sig["max_weight"].default) == (None, None, False, 0.0)
    sig = inspect.signature(surface.TsdfVolume.integrate_geometry).parameters
    assert (sig["min_alpha"].default, sig["carve"].default) == (0.5, True)
    assert inspect.signature(surface.TsdfVolume.extract).parameters["min_weight"].default == 0.0
    sig = inspect.signature(surface.mesh_from_views).parameters
    assert (sig["bounds"].default, sig["voxel"].default) == (None, None)
    assert inspect.signature(surface.mesh_from_sources).parameters["sb"].default == 0
    sig = inspect.signature(ops.tsdf_integrate).parameters
    assert (sig["weight"].default, sig["color"].default, sig["carve"].default, sig["max_weight"].default) == (None, None, False, 0.0)
    assert inspect.signature(ops.surface_extract).parameters["min_weight"].default == 0.0
    assert surface.Mesh._fields == ("vertices", "normals", "rgb", "faces")

    t, w, c4 = torch.ones(4, 5, 6), torch.zeros(4, 5, 6), torch.zeros(4, 4, 5, 6)
    d, Km, E = torch.ones(2, 3, 4), torch.eye(3).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1)
    o = (0.0, 0.0, 0.0)
    good = dict(tsdf=t, wsum=w, color4=None, origin=o, voxel=0.1, trunc=0.3, depth=d, intrinsics=Km, extrinsics=E)
    for kw, exc in ((dict(wsum=w[:3]), ValueError), (dict(tsdf=t[:1], wsum=w[:1]), ValueError), (dict(color4=c4[:3]), ValueError),
                    (dict(origin=(0.0, 0.0)), ValueError), (dict(voxel=0.0), ValueError), (dict(trunc=0.0), ValueError),
                    (dict(depth=d[0]), ValueError), (dict(depth=torch.ones(17, 3, 4), intrinsics=torch.eye(3).repeat(17, 1, 1),
                                                          extrinsics=torch.eye(4).repeat(17, 1, 1)), ValueError),
                    (dict(intrinsics=Km[:1]), ValueError), (dict(extrinsics=E[:, :3]), ValueError), (dict(weight=torch.ones(2, 3, 5)), ValueError),
                    (dict(color=torch.ones(2, 3, 3, 4)), ValueError), (dict(color4=c4), ValueError),
                    (dict(color4=c4, color=torch.ones(2, 3, 3, 5)), ValueError), ({}, RuntimeError),
                    (dict(color4=c4, color=torch.ones(2, 3, 3, 4), weight=torch.ones(2, 1, 3, 4)), RuntimeError)):
        with pytest.raises(exc):
            ops.tsdf_integrate(**{**good, **kw})                    # CPU tensors: the last ones are the "no CPU fallback" error
    for args, exc in (((t, w[:3], None, o, 0.1), ValueError), ((t, w, c4[:, :2], o, 0.1), ValueError), ((t, w, None, o, -1.0), ValueError),
                      ((t, w, None, o, 0.1), RuntimeError), ((t, w, c4, o, 0.1), RuntimeError)):
        with pytest.raises(exc):
            ops.surface_extract(*args)
    for kw, exc in ((dict(dims=(1, 4, 4)), ValueError), (dict(dims=(4, 4)), ValueError), (dict(voxel=0.0), ValueError),
                    (dict(origin=(0.0,)), ValueError), (dict(trunc=-1.0), ValueError), (dict(device="cpu"), RuntimeError)):
        with pytest.raises(exc):
            surface.TsdfVolume(**{**dict(origin=o, voxel=0.1, dims=(4, 4, 4), device="cpu"), **kw})
    with pytest.raises(RuntimeError):
        surface.mesh_from_views(None, None, E[:1], Km[:1], 4, 4, 0.5, 2.0)
    with pytest.raises(ValueError):
        surface.mesh_from_views(None, None, E[:, :3], Km, 4, 4, 0.5, 2.0)
    with pytest.raises(RuntimeError):
        surface.mesh_from_sources({}, device="cpu")


def test_volume_box():
    from diner_amd.surface import _volume_for
    origin, voxel, dims = _volume_for((0.0, 0.0, 0.0), (1.0, 0.5, 0.25), True, None, None)
    assert abs(voxel - 1.0 / 250.0) < 1e-9 and dims[0] in (257, 258) and torch.allclose(origin, torch.full((3,), -3.0 / 250.0))
    origin, voxel, dims = _volume_for((0.0, 0.0, 0.0), (1.0, 0.5, 0.25), False, None, None)
    assert voxel == 1.0 / 256.0 and dims[0] in (257, 258) and origin.tolist() == [0.0, 0.0, 0.0]
    origin, voxel, dims = _volume_for((0.0, 0.0, 0.0), (1.0, 0.5, 0.25), True, 0.125, 0.25)
    assert dims == (13, 9, 7) and origin.tolist() == [-0.25] * 3
    with pytest.raises(ValueError):
        _volume_for((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), True, None, None)


# ----------------------------------------------------------------------------------------------------------------------- PLY
@pytest.mark.parametrize("M,F", [(0, 0), (5, 0), (257, 301)])
@pytest.mark.parametrize("with_rgb,with_normals", [(False, False), (True, False), (False, True), (True, True)])
def test_mesh_ply_round_trip_is_bit_exact(tmp_path, M, F, with_rgb, with_normals):
    from diner_amd.surface import read_mesh_ply, write_mesh_ply
    g = np.random.default_rng(M + F)
    xyz = g.normal(size=(M, 3)).astype(np.float32)
    if M:
        xyz[0] = [np.float32("nan"), np.float32("inf"), -0.0]
    rgb = g.integers(0, 256, (M, 3)).astype(np.uint8) if with_rgb else None
    nrm = g.normal(size=(M, 3)).astype(np.float32) if with_normals else None
    faces = g.integers(0, max(M, 1), (F, 3)).astype(np.int32)
    path = tmp_path / "mesh.ply"
    write_mesh_ply(path, torch.from_numpy(xyz), nrm, None if rgb is None else torch.from_numpy(rgb), torch.from_numpy(faces))
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    want = ["ply", "format binary_little_endian 1.0", f"element vertex {M}", "property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] if with_normals else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_rgb else []
    want += [f"element face {F}", "property list uchar int vertex_indices", ""]
    assert head == want
    assert len(raw) == raw.index(b"end_header\n") + 11 + M * (12 + 12 * with_normals + 3 * with_rgb) + F * 13
    m = read_mesh_ply(path)
    assert m.vertices.dtype == np.float32 and m.vertices.shape == (M, 3) and m.vertices.tobytes() == xyz.tobytes()
    assert m.faces.dtype == np.int32 and m.faces.shape == (F, 3) and m.faces.tobytes() == faces.tobytes()
    assert (m.rgb is None) == (rgb is None) and (m.normals is None) == (nrm is None)
    if with_rgb:
        assert m.rgb.dtype == np.uint8 and m.rgb.tobytes() == rgb.tobytes()
    if with_normals:
        assert m.normals.dtype == np.float32 and m.normals.tobytes() == nrm.tobytes()


def test_mesh_ply_vertex_block_is_write_ply_and_bad_input_is_refused(tmp_path):
    from diner_amd.geometry import write_ply
    from diner_amd.surface import write_mesh_ply
    g = np.random.default_rng(1)
    xyz, nrm = g.normal(size=(9, 3)).astype(np.float32), g.normal(size=(9, 3)).astype(np.float32)
    rgb = g.integers(0, 256, (9, 3)).astype(np.uint8)
    write_ply(tmp_path / "cloud.ply", xyz, rgb, nrm)
    cloud = open(tmp_path / "cloud.ply", "rb").read()
    # write_ply's bytes are what they were: header, then 27-byte records
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\nproperty float z\n" \
           b"property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
    rec = b"".join(xyz[i].tobytes() + nrm[i].tobytes() + rgb[i].tobytes() for i in range(9))
    assert cloud == head + rec
    write_mesh_ply(tmp_path / "mesh.ply", xyz, nrm, rgb, np.array([[0, 1, 2]], dtype=np.int32))
    mesh = open(tmp_path / "mesh.ply", "rb").read()
    body = mesh[mesh.index(b"end_header\n") + 11:]
    assert body == rec + b"\x03" + np.array([0, 1, 2], dtype="<i4").tobytes()
    with pytest.raises(ValueError):
        write_mesh_ply(tmp_path / "a.ply", xyz, faces=np.array([[0, 1, 9]], dtype=np.int32))          # index outside the vertices
    with pytest.raises(ValueError):
        write_mesh_ply(tmp_path / "a.ply", xyz, faces=np.array([[0, 1, 2]], dtype=np.int64))
    with pytest.raises(ValueError):
        write_mesh_ply(tmp_path / "a.ply", xyz, rgb=rgb[:3])


# ------------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("n", [12, 16, 24])
def test_restatement_on_the_sphere(n):
    sc = S.main_scene(n)
    t0, w0, c0 = S.fresh_volume(sc.dims)
    r64 = S.ref_integrate(t0, w0, c0, sc.origin, sc.voxel, sc.trunc, sc.depth, None, sc.color, sc.K, sc.E, carve=True)
    r32 = S.ref_integrate(t0, w0, c0, sc.origin, sc.voxel, sc.trunc, sc.depth, None, sc.color, sc.K, sc.E, carve=True, dtype=np.float32)
    band = S.integration_band(r64, sc.W, sc.H)
    share = band.mean()
    ok = ~band
    assert np.array_equal(r32.used[:, ok], r64.used[:, ok]) and np.array_equal(r32.wsum[ok].astype(np.float64), r64.wsum[ok])
    vol32 = r64.tsdf.astype(np.float32), r64.wsum.astype(np.float32), r64.color4.astype(np.float32)
    m = S.ref_surface_nets(*vol32, sc.origin, sc.voxel)
    m32 = S.ref_surface_nets(r32.tsdf, r32.wsum, r32.color4, sc.origin, sc.voxel, dtype=np.float32)
    st = S.mesh_stats(m.vertices, m.faces)
    err = np.abs(np.linalg.norm(m.vertices, axis=1) - S.RADIUS) / float(sc.voxel)
    rel_volume = st.volume / (4.0 / 3.0 * np.pi * S.RADIUS ** 3)
    print(f"n={n}: observed {(r64.wsum > 0).sum()} / {n ** 3}; {m.n_vertices} vertices, {m.n_quads} quads, Euler {st.euler}, boundary "
          f"{st.boundary_edges}; radius error max {err.max():.2f} mean {err.mean():.2f} voxel; volume {rel_volume:.3f}; band {share:.4%}")
    assert st.closed and st.oriented and st.euler == 2 and len(m.faces) == 2 * m.n_quads
    assert err.max() <= 1.0 and share <= 0.02 and 0.8 < rel_volume < 1.0
    assert (m.n_vertices, m.n_quads) == (m32.n_vertices, m32.n_quads) and np.array_equal(m.faces, m32.faces)     # identical topology
    # the normals point away from the centre, the colours are 0.5 + 0.5 normal to within the pixel and voxel sizes
    out = m.vertices / np.linalg.norm(m.vertices, axis=1, keepdims=True)
    assert ((m.normals * out).sum(axis=1) > 0).all() and np.abs(m.rgb - (0.5 + 0.5 * out)).max() < 0.25
    if n == 16:
        assert (m.n_vertices, m.n_quads) == (502, 500) and (r64.wsum > 0).sum() == 4047


def test_restatement_without_carving_is_open_and_hand_made_volumes():
    sc = S.main_scene(16)
    t0, w0, _ = S.fresh_volume(sc.dims, color=False)
    r = S.ref_integrate(t0, w0, None, sc.origin, sc.voxel, sc.trunc, sc.depth, None, None, sc.K, sc.E, carve=False)
    m = S.ref_surface_nets(r.tsdf, r.wsum, None, sc.origin, sc.voxel)
    st = S.mesh_stats(m.vertices, m.faces)
    print(f"no carve: observed {(r.wsum > 0).sum()}, {m.n_vertices} vertices, {m.n_quads} quads, boundary edges {st.boundary_edges}")
    assert (r.wsum > 0).sum() == 1454 and st.boundary_edges == 170 and not st.closed and m.rgb is None
    # 2^3 with one negative corner: one vertex at (1/6, 1/6, 1/6) voxel, no face
    t = np.ones((2, 2, 2), np.float32)
    t[0, 0, 0] = -1.0
    w = np.ones((2, 2, 2), np.float32)
    m = S.ref_surface_nets(t, w, None, (0, 0, 0), 0.5)
    assert m.n_vertices == 1 and m.n_quads == 0 and np.allclose(m.vertices, 0.5 / 6.0) and m.faces.shape == (0, 3)
    assert np.allclose(m.normals, 1 / np.sqrt(3.0))
    # 3^3 with a negative centre: 8 vertices, 6 quads, closed; an unobserved corner takes a cell and three quads away
    t = np.ones((3, 3, 3), np.float32)
    t[1, 1, 1] = -1.0
    w = np.ones((3, 3, 3), np.float32)
    m = S.ref_surface_nets(t, w, None, (0, 0, 0), 1.0)
    st = S.mesh_stats(m.vertices, m.faces)
    assert (m.n_vertices, m.n_quads) == (8, 6) and st.closed and st.oriented and st.euler == 2 and st.volume > 0
    w[0, 0, 0] = 0.0
    m = S.ref_surface_nets(t, w, None, (0, 0, 0), 1.0)
    assert (m.n_vertices, m.n_quads) == (7, 3)
    # an exact 0 is positive; all-positive gives nothing
    t = np.ones((2, 2, 2), np.float32)
    t[0, 0, 0] = 0.0
    assert S.ref_surface_nets(t, np.ones_like(t), None, (0, 0, 0), 1.0).n_vertices == 0
    t[1, 1, 1] = -0.5
    m = S.ref_surface_nets(t, np.ones_like(t), None, (0, 0, 0), 1.0)
    assert m.n_vertices == 1 and np.isfinite(m.vertices).all()
