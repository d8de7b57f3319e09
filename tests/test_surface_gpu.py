"""GPU: TSDF fusion and surface nets -- diner_tsdf_integrate_f32 / diner_surface_count / diner_surface_extract_f32 through ops,
diner_amd.surface and evaluate.write_prediction_folder(write_mesh=True).

  1  integration against the float64 restatement (tests/surface_util.py) on the analytic sphere: 1, 6 and 16 views, with and without
     carving, per-pixel weights and colour, and a volume whose sides are no multiple of any block; wsum and the skip decisions equal on
     every voxel outside the band the restatement cannot decide (stated, <= 2 %), tsdf and the colour sums at 4 x its float32 - float64 gap;
  2  one call with six views leaves the bits of six single-view calls, also under a weight cap; NaN and negative depths change nothing;
  3  extraction from the DEVICE's own volume: counts and faces equal the restatement's exactly, positions / normals / colours at 4 x gap;
     hand-made volumes, among them one whose block counts take more than one chunk of the scan;
  4  the sphere end to end through TsdfVolume: closed, oriented, Euler characteristic 2, within a voxel of the sphere;
  5  mesh_from_sources, mesh_from_views and write_prediction_folder(write_mesh=True) on the 48 x 40 culling scene, rendering untouched."""
import os
import types

import numpy as np
import pytest
import torch

from tests import surface_util as S

pytestmark = pytest.mark.gpu
SEED = 20261019


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def scene(N=6, dims=(16, 16, 16)):
    """The main scene with N views; the weights are the cosine on the sphere and 1 off it (an empty pixel carves at full weight)."""
    sc = S.main_scene(16, N)
    weight = np.where(sc.depth > 0, sc.weight, np.float32(1.0)).astype(np.float32)
    return sc, weight, dims


def device_integrate(ops, sc, dims, weight, color, carve, max_weight=0.0, views=None, start=None):
    """-> (tsdf, wsum, color4 | None) device tensors after one ops.tsdf_integrate call on a fresh volume (or on `start`)."""
    t0, w0, c0 = S.fresh_volume(dims, color) if start is None else start
    t, w, c4 = cuda(t0), cuda(w0), cuda(c0)
    v = slice(None) if views is None else views
    ops.tsdf_integrate(t, w, c4, sc.origin, float(sc.voxel), float(sc.trunc), cuda(sc.depth[v]), torch.from_numpy(sc.K[v]),
                       torch.from_numpy(sc.E[v]), weight=None if weight is None else cuda(weight[v]),
                       color=cuda(sc.color[v]) if color else None, carve=carve, max_weight=max_weight)
    return t, w, c4


# ------------------------------------------------------------------------------------------------------------------ 1 integration
CASES = [(N, (16, 16, 16), carve, wt, col) for N in (1, 6, 16)
         for carve, wt, col in ((False, False, False), (True, True, True), (True, False, True), (False, True, False))]
CASES.append((6, (17, 13, 9), True, True, True))
CASES.append((6, (17, 13, 9), False, False, False))


@pytest.mark.parametrize("N,dims,carve,wt,col", CASES)
def test_integration_against_restatement(ops, N, dims, carve, wt, col):
    sc, weight, dims = scene(N, dims)
    weight = weight if wt else None
    t0, w0, c0 = S.fresh_volume(dims, col)
    args = (t0, w0, c0, sc.origin, sc.voxel, sc.trunc, sc.depth, weight, sc.color if col else None, sc.K, sc.E, carve)
    r64 = S.ref_integrate(*args)
    r32 = S.ref_integrate(*args, dtype=np.float32)
    band = S.integration_band(r64, sc.W, sc.H)
    ok = ~band
    share = float(band.mean())
    t, w, c4 = device_integrate(ops, sc, dims, weight, col, carve)
    t, w = t.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(r32.used[:, ok], r64.used[:, ok])
    gap_t = float(np.abs(r32.tsdf.astype(np.float64) - r64.tsdf)[ok].max())
    gap_w = float(np.abs(r32.wsum.astype(np.float64) - r64.wsum)[ok].max())
    err_t, err_w = float(np.abs(t - r64.tsdf)[ok].max()), float(np.abs(w - r64.wsum)[ok].max())
    line = f"N={N} dims={dims} carve={carve} weight={wt} color={col}: band {share:.4%}, observed {int((w > 0).sum())}; " \
           f"tsdf err {err_t:.3e} / tol {4 * gap_t:.3e}; wsum err {err_w:.3e} / tol {4 * gap_w:.3e}"
    # wsum: the same additions in the same order as the float32 restatement -- equal bit for bit; without weights it is the number of
    # views that updated the voxel, equal to the float64 restatement's as well
    assert np.array_equal(w[ok].view(np.int32), r32.wsum[ok].view(np.int32)), line
    if not wt:
        assert np.array_equal(w[ok].astype(np.float64), r64.used.sum(axis=0)[ok].astype(np.float64)), line
    assert np.array_equal((w > 0)[ok], r64.used.any(axis=0)[ok]), line
    if col:
        c = c4.cpu().numpy()
        gap_c = float(np.abs(r32.color4.astype(np.float64) - r64.color4)[:, ok].max())
        err_c = float(np.abs(c - r64.color4)[:, ok].max())
        line += f"; colour err {err_c:.3e} / tol {4 * gap_c:.3e}"
        assert np.array_equal(c[3][ok] > 0, r64.painted.any(axis=0)[ok])
        assert err_c <= 4 * gap_c, line
    print(line)
    assert share <= 0.02, line
    assert err_t <= 4 * gap_t and err_w <= 4 * gap_w, line
    assert (t[w == 0] == 1).all()                                        # an unobserved voxel keeps the fresh value


def test_skip_decisions_per_view(ops):
    """Each view alone on a fresh volume: the voxels it updates (wsum > 0) and paints (sum w > 0) are the float64 restatement's."""
    sc, weight, dims = scene(6)
    t0, w0, c0 = S.fresh_volume(dims, True)
    r64 = S.ref_integrate(t0, w0, c0, sc.origin, sc.voxel, sc.trunc, sc.depth, weight, sc.color, sc.K, sc.E, True)
    ok = ~S.integration_band(r64, sc.W, sc.H)
    for n in range(6):
        t, w, c4 = device_integrate(ops, sc, dims, weight, True, True, views=slice(n, n + 1))
        assert np.array_equal((w.cpu().numpy() > 0)[ok], r64.used[n][ok]), n
        assert np.array_equal((c4[3].cpu().numpy() > 0)[ok], r64.painted[n][ok]), n
        assert 0 < int(r64.painted[n].sum()) < int(r64.used[n].sum()) < 4096


# ------------------------------------------------------------------------------------------------- 2 one call = N calls, bit for bit
@pytest.mark.parametrize("max_weight", [0.0, 2.5])
def test_one_call_equals_single_view_calls(ops, max_weight):
    sc, weight, dims = scene(6)
    one = device_integrate(ops, sc, dims, weight, True, True, max_weight=max_weight)
    t, w, c4 = (cuda(a) for a in S.fresh_volume(dims, True))
    for n in range(6):
        ops.tsdf_integrate(t, w, c4, sc.origin, float(sc.voxel), float(sc.trunc), cuda(sc.depth[n:n + 1]), torch.from_numpy(sc.K[n:n + 1]),
                           torch.from_numpy(sc.E[n:n + 1]), weight=cuda(weight[n:n + 1]), color=cuda(sc.color[n:n + 1]), carve=True,
                           max_weight=max_weight)
    for a, b in zip(one, (t, w, c4)):
        assert torch.equal(bits(a), bits(b))
    if max_weight > 0:
        free = device_integrate(ops, sc, dims, weight, True, True)
        assert float(w.max()) == 2.5 and float(free[1].max()) > 2.5 and (w <= 2.5).all()
        assert torch.equal(bits(w), bits(free[1].clamp(max=2.5)))           # positive weights: once at the cap, always at the cap
        assert torch.equal(bits(c4), bits(free[2]))                      # the colour sums are never clamped
    # NaN and negative depths, and a weight of zero, NaN or below zero, change nothing -- carving or not
    before = [a.clone() for a in (t, w, c4)]
    bad = sc.depth[:2].copy()
    bad[0], bad[1] = np.float32("nan"), -1.0
    for carve in (False, True):
        ops.tsdf_integrate(t, w, c4, sc.origin, float(sc.voxel), float(sc.trunc), cuda(bad), torch.from_numpy(sc.K[:2]),
                           torch.from_numpy(sc.E[:2]), color=cuda(sc.color[:2]), carve=carve)
        wbad = np.zeros_like(sc.depth[:3])
        wbad[1], wbad[2] = np.float32("nan"), -1.0
        ops.tsdf_integrate(t, w, c4, sc.origin, float(sc.voxel), float(sc.trunc), cuda(sc.depth[:3]), torch.from_numpy(sc.K[:3]),
                           torch.from_numpy(sc.E[:3]), weight=cuda(wbad), color=cuda(sc.color[:3]), carve=carve)
    for a, b in zip(before, (t, w, c4)):
        assert torch.equal(bits(a), bits(b))


# -------------------------------------------------------------------------------------------------------------------- 3 extraction
def check_extraction(ops, tsdf, wsum, color4, origin, voxel, min_weight=0.0, label=""):
    """ops.surface_extract on device tensors against the restatement on the same bits -> (device mesh as numpy, float64 restatement)."""
    m = ops.surface_extract(tsdf, wsum, color4, origin, voxel, min_weight=min_weight)
    th, wh = tsdf.cpu().numpy(), wsum.cpu().numpy()
    ch = None if color4 is None else color4.cpu().numpy()
    r64 = S.ref_surface_nets(th, wh, ch, origin, voxel, min_weight)
    r32 = S.ref_surface_nets(th, wh, ch, origin, voxel, min_weight, dtype=np.float32)
    v, n, f = m.vertices.cpu().numpy(), m.normals.cpu().numpy(), m.faces.cpu().numpy()
    assert v.shape == (r64.n_vertices, 3) and n.shape == v.shape and f.shape == (2 * r64.n_quads, 3) and f.dtype == np.int32
    assert np.array_equal(f, r64.faces)
    pairs = [("position", v, r64.vertices, r32.vertices), ("normal", n, r64.normals, r32.normals)]
    if color4 is not None:
        pairs.append(("rgb", m.rgb.cpu().numpy(), r64.rgb, r32.rgb))
    else:
        assert m.rgb is None
    line = f"{label}: {r64.n_vertices} vertices, {r64.n_quads} quads"
    for name, got, want, want32 in pairs:
        if r64.n_vertices == 0:
            continue
        gap = float(np.abs(want32.astype(np.float64) - want).max())
        err = float(np.abs(got - want).max())
        line += f"; {name} err {err:.3e} / tol {4 * gap:.3e}"
        assert err <= 4 * gap, line
    print(line)
    return types.SimpleNamespace(vertices=v, normals=n, faces=f, rgb=None if color4 is None else m.rgb.cpu().numpy()), r64


@pytest.mark.parametrize("carve,col", [(True, True), (False, False)])
def test_extraction_from_the_device_volume(ops, carve, col):
    sc, weight, dims = scene(6)
    t, w, c4 = device_integrate(ops, sc, dims, weight if col else None, col, carve)
    m, r = check_extraction(ops, t, w, c4, sc.origin, float(sc.voxel), label=f"sphere carve={carve}")
    st = S.mesh_stats(m.vertices, m.faces)
    assert (st.closed and st.euler == 2 and st.oriented) if carve else (st.boundary_edges > 0)
    # a weight threshold takes the thinly observed cells away: fewer vertices, still the restatement's
    m2, r2 = check_extraction(ops, t, w, c4, sc.origin, float(sc.voxel), min_weight=1.5, label="min_weight 1.5")
    assert 0 < r2.n_vertices < r.n_vertices


def test_extraction_hand_made_volumes(ops):
    o = (0.0, 0.0, 0.0)
    # 2^3 with one negative corner: one vertex at (1/6, 1/6, 1/6) voxel, no face
    t = np.ones((2, 2, 2), np.float32)
    t[0, 0, 0] = -1.0
    m, r = check_extraction(ops, cuda(t), cuda(np.ones_like(t)), None, o, 0.5, label="2^3")
    assert m.vertices.shape == (1, 3) and m.faces.shape == (0, 3) and np.allclose(m.vertices, 0.5 / 6.0, rtol=1e-6)
    # 3^3 with a negative centre: 8 vertices, 6 quads, closed; with an unobserved corner 7 and 3
    t = np.ones((3, 3, 3), np.float32)
    t[1, 1, 1] = -1.0
    w = np.ones((3, 3, 3), np.float32)
    m, r = check_extraction(ops, cuda(t), cuda(w), None, o, 1.0, label="3^3")
    st = S.mesh_stats(m.vertices, m.faces)
    assert m.vertices.shape == (8, 3) and m.faces.shape == (12, 3) and st.closed and st.oriented and st.euler == 2 and st.volume > 0
    w[0, 0, 0] = 0.0
    m, r = check_extraction(ops, cuda(t), cuda(w), None, o, 1.0, label="3^3 with a hole")
    assert m.vertices.shape == (7, 3) and m.faces.shape == (6, 3)
    # an exact 0 and a NaN are positive
    t = np.ones((2, 2, 2), np.float32)
    t[0, 0, 0], t[1, 1, 0] = 0.0, np.float32("nan")
    m, r = check_extraction(ops, cuda(t), cuda(np.ones_like(t)), None, o, 1.0, label="zero and NaN corners")
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)
    t[0, 0, 1] = -0.5                                                    # the +x neighbour of the exact 0: t = 0 / 0.5 on that edge
    t[1, 1, 0] = 1.0
    m, r = check_extraction(ops, cuda(t), cuda(np.ones_like(t)), None, o, 1.0, label="zero corner next to a negative one")
    assert m.vertices.shape == (1, 3) and np.isfinite(m.vertices).all() and np.isfinite(m.normals).all()
    # all positive: nothing, and empty outputs
    t = np.ones((5, 4, 3), np.float32)
    m = ops.surface_extract(cuda(t), cuda(t), cuda(np.zeros((4, 5, 4, 3), np.float32)), o, 1.0)
    assert m.vertices.shape == (0, 3) and m.normals.shape == (0, 3) and m.rgb.shape == (0, 3) and m.faces.shape == (0, 3)
    assert m.faces.dtype == torch.int32


def test_extraction_scan_runs_more_than_one_chunk(ops):
    """67 x 33 x 31 samples: 268 blocks of 256 samples, two passes of the scanning workgroup at 256 blocks a pass."""
    dims, voxel = (67, 33, 31), 0.03
    origin = (-1.0, -0.49, -0.46)
    t = S.sphere_tsdf(dims, origin, voxel, 0.4, 0.09)
    w = np.ones_like(t)
    m, r = check_extraction(ops, cuda(t), cuda(w), None, origin, voxel, label="67 x 33 x 31 sphere")
    st = S.mesh_stats(m.vertices, m.faces)
    err = np.abs(np.linalg.norm(m.vertices, axis=1) - 0.4) / voxel
    print(f"  Euler {st.euler}, radius error {err.max():.3f} voxel, {len(np.unique(np.asarray(r.cells)[:, 2]))} z-slabs of cells")
    assert st.closed and st.oriented and st.euler == 2 and err.max() < 0.5 and r.n_vertices > 2000
    assert (m.normals * m.vertices).sum(axis=1).min() > 0


def test_extract_refuses_counts_that_are_not_counts(ops):
    import ctypes as C
    from diner_amd import _lib
    lib = _lib.load()
    t = np.ones((3, 3, 3), np.float32)
    t[1, 1, 1] = -1.0
    td, wd = cuda(t), cuda(np.ones_like(t))
    ws = torch.empty(lib.diner_surface_workspace_bytes(3, 3, 3), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    origin = (C.c_float * 3)(0.0, 0.0, 0.0)
    assert lib.diner_surface_count(td.data_ptr(), wd.data_ptr(), 3, 3, 3, 0.0, ws.data_ptr(), counts.data_ptr(), st) == 0
    assert counts.tolist() == [8, 6]
    verts = torch.full((8, 3), -7.0, device="cuda")
    faces = torch.full((12, 3), -7, device="cuda", dtype=torch.int32)
    for nv, nq in ((7, 6), (8, 5), (0, 0), (9, 6)):
        rc = lib.diner_surface_extract_f32(td.data_ptr(), wd.data_ptr(), None, 3, 3, 3, origin, 1.0, 0.0, ws.data_ptr(), nv, nq,
                                           verts.data_ptr(), None, None, faces.data_ptr(), st)
        assert rc == _lib.E_INVALID and b"counts" in lib.diner_last_error(), (nv, nq)
    torch.cuda.synchronize()
    assert (verts == -7).all() and (faces == -7).all()                   # a refused call launches nothing
    assert lib.diner_surface_extract_f32(td.data_ptr(), wd.data_ptr(), None, 3, 3, 3, origin, 1.0, 0.0, ws.data_ptr(), 8, 6,
                                         verts.data_ptr(), None, None, faces.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (faces >= 0).all() and (faces < 8).all() and (verts > 0).all()


# -------------------------------------------------------------------------------------------------------------------- 4 end to end
def test_sphere_through_tsdf_volume(ops, tmp_path):
    from diner_amd.surface import Mesh, TsdfVolume, read_mesh_ply, write_mesh_ply
    sc, weight, dims = scene(6)
    vol = TsdfVolume(sc.origin, float(sc.voxel), dims, trunc=float(sc.trunc), device="cuda")
    assert vol.integrate(cuda(sc.depth)[:, None], torch.from_numpy(sc.K[0]), torch.from_numpy(sc.E), rgb=cuda(sc.color), carve=True) is vol
    mesh = vol.extract()
    assert isinstance(mesh, Mesh) and mesh.rgb.dtype == torch.uint8 and mesh.faces.dtype == torch.int32
    v, n, f = mesh.vertices.cpu().numpy().astype(np.float64), mesh.normals.cpu().numpy().astype(np.float64), mesh.faces.cpu().numpy()
    st = S.mesh_stats(v, f)
    t0, w0, c0 = S.fresh_volume(dims, True)
    r = S.ref_integrate(t0, w0, c0, sc.origin, sc.voxel, sc.trunc, sc.depth, None, sc.color, sc.K, sc.E, True)
    ref = S.ref_surface_nets(r.tsdf.astype(np.float32), r.wsum.astype(np.float32), r.color4.astype(np.float32), sc.origin, sc.voxel)
    ref_volume = S.mesh_stats(ref.vertices, ref.faces).volume
    err = np.abs(np.linalg.norm(v, axis=1) - S.RADIUS) / float(sc.voxel)
    print(f"sphere: {len(v)} vertices, {len(f) // 2} quads, Euler {st.euler}, radius error max {err.max():.3f} mean {err.mean():.3f} voxel, "
          f"volume {st.volume:.6f} (restatement {ref_volume:.6f}, sphere {4 / 3 * np.pi * S.RADIUS ** 3:.6f})")
    assert st.closed and st.euler == 2 and st.oriented and st.boundary_edges == 0
    assert ((n * v).sum(axis=1) / np.linalg.norm(v, axis=1) > 0).all()
    assert err.max() <= 1.0
    assert abs(st.volume - ref_volume) <= 0.01 * ref_volume
    out = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.abs(mesh.rgb.cpu().numpy() / 255.0 - (0.5 + 0.5 * out)).max() < 0.25
    # a second integrate call goes on where the first stopped; reset gives a fresh volume
    vol16 = TsdfVolume(sc.origin, float(sc.voxel), dims, trunc=float(sc.trunc), device="cuda")
    sc17 = S.main_scene(16, 16)
    d17 = np.concatenate((sc17.depth, sc17.depth[:1]))
    vol16.integrate(cuda(d17)[:, None], torch.from_numpy(sc17.K[0]), torch.from_numpy(np.concatenate((sc17.E, sc17.E[:1]))), carve=True)
    assert float(vol16.wsum.max()) == 17.0 and float(vol16.color4.abs().max()) == 0.0              # 17 views: two kernel calls
    vol16.reset()
    assert float(vol16.wsum.max()) == 0.0 and float(vol16.tsdf.min()) == 1.0
    # through the file
    write_mesh_ply(tmp_path / "sphere.ply", *mesh)
    back = read_mesh_ply(tmp_path / "sphere.ply")
    for a, b in zip(mesh, back):
        assert a.cpu().numpy().tobytes() == b.tobytes()


# -------------------------------------------------------------------------------------------------------- 5 on the culling scene
def test_meshes_of_the_culling_scene(ops, tmp_path):
    from diner_amd import evaluate, noise
    from diner_amd.render import predict_image
    from diner_amd.surface import mesh_from_sources, mesh_from_views, read_mesh_ply
    from tests.test_geometry_gpu import K as KS, model
    case, nerf, ren, E, Kt = model()
    sc, w, h = case.sc, case.w, case.h
    assert (w, h) == (48, 40)

    def renders():
        rays = ops.gen_rays(E, Kt, w, h, sc["znear"], sc["zfar"], "cuda")[:, 100:900].contiguous()
        with torch.no_grad(), noise.keyed(SEED, 100):
            f = ren.forward(nerf, rays, want_alpha=True).fine
        return predict_image(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED), f

    before = renders()
    g = torch.Generator().manual_seed(3)
    nv = sc["depths"].shape[0]
    batch = dict(src_depths=sc["depths"][None], src_rgbs=torch.rand(1, nv, 3, h, w, generator=g), src_intrinsics=sc["src_intrinsics"][None],
                 src_extrinsics=sc["src_extrinsics"][None], target_rgb=torch.rand(1, 3, h, w, generator=g), sample_name=["view0"],
                 target_extrinsics=sc["target_extrinsics"][None], target_intrinsics=case.Kt[None])

    def check(mesh, label):
        nvert = mesh.vertices.shape[0]
        print(f"{label}: {nvert} vertices, {mesh.faces.shape[0]} triangles")
        assert mesh.vertices.shape == mesh.normals.shape == mesh.rgb.shape == (nvert, 3) and mesh.faces.shape[1] == 3
        assert mesh.faces.shape[0] % 2 == 0 and mesh.rgb.dtype == torch.uint8 and mesh.faces.dtype == torch.int32
        if mesh.faces.shape[0]:
            assert int(mesh.faces.min()) >= 0 and int(mesh.faces.max()) < nvert
        assert torch.isfinite(mesh.vertices).all()
        return nvert

    mesh, vol = mesh_from_sources(batch, voxel=0.02)
    assert check(mesh, f"mesh_from_sources, volume {vol.dims}") > 0 and mesh.faces.shape[0] > 0
    lo = vol.origin
    hi = lo + torch.tensor([d - 1 for d in vol.dims]) * vol.voxel
    assert (mesh.vertices.cpu() >= lo).all() and (mesh.vertices.cpu() <= hi).all()
    turn = torch.eye(4)
    a = 0.06
    turn[0, 0], turn[0, 2], turn[2, 0], turn[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    Es = torch.stack((E[0].cpu(), turn @ E[0].cpu(), turn.T @ E[0].cpu())).cuda()
    mesh, vol, views = mesh_from_views(nerf, ren, Es, Kt[0], w, h, sc["znear"], sc["zfar"], voxel=0.02, seed=SEED)
    assert len(views) == 3 and check(mesh, f"mesh_from_views, volume {vol.dims}") >= 0
    assert float(vol.wsum.max()) > 0

    encode, nerf.encode = nerf.encode, lambda **kw: None               # the scene is injected, as everywhere in this suite
    import diner_amd.datasets as datasets
    orig, datasets.encode_args = datasets.encode_args, lambda b, dev: {}
    try:
        torch.manual_seed(5)
        evaluate.write_prediction_folder(nerf, ren, [batch], str(tmp_path / "plain"), sc["znear"], sc["zfar"])
        torch.manual_seed(5)
        evaluate.write_prediction_folder(nerf, ren, [batch], str(tmp_path / "mesh"), sc["znear"], sc["zfar"], write_mesh=True)
    finally:
        datasets.encode_args = orig
        nerf.encode = encode
    plain, with_mesh = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(tmp_path / "mesh"))
    assert "view0-mesh.ply" not in plain and with_mesh == sorted(plain + ["view0-mesh.ply"])
    for name in plain:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "mesh" / name, "rb").read(), name
    m = read_mesh_ply(tmp_path / "mesh" / "view0-mesh.ply")
    assert m.vertices.shape[0] > 0 and m.faces.shape[0] > 0 and m.faces.max() < m.vertices.shape[0] and m.rgb.shape == m.vertices.shape
    assert np.isfinite(m.vertices).all()

    after = renders()
    for a_, b_ in zip(before[0], after[0]):
        assert torch.equal(a_, b_)
    assert sorted(before[1].keys()) == sorted(after[1].keys())
    for k in before[1]:
        assert torch.equal(bits(before[1][k]), bits(after[1][k])), k
