"""GPU: the ray's opacity (pix_alpha = weights.sum(-1), nerf_renderer.py:359 -- computed by the reference and dropped) and the depth spread
as outputs of the compositor, through the C ABI, ops, the autograd node, the drop-in renderer, the image harness and the objective.

The aux compositor must leave rgb / depth / weights bit-equal to the existing entries; alpha and depth_var are held to a float64 torch
evaluation of the compositing formula (nerf_renderer.py:299-301, :341-360) written out below, with the float32 torch evaluation of the
same expression on the CPU as the yardstick where the per-stage bar does not cover a float32 evaluation at all (long rays)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, max_norm_rel
from tests.test_hip_parity import TOL, TOL_STAGE, hip_scene, hip_mlp
from tests.test_train_gpu import TOL_GRAD          # the bar of test_composite_backward_against_oracle_autograd (tests/test_train_gpu.py:206)

pytestmark = pytest.mark.gpu


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


def formula(field, z, rays, white):
    """nerf_renderer.py:299-301, :341-360 in the dtype of its inputs -> weights, rgb, depth, alpha, depth_var (the spread around the
    unnormalised depth, centred form; reported as 0 where a negative weight -- a sample beyond `far` -- makes the sum negative)."""
    deltas = torch.cat((z[:, 1:] - z[:, :-1], rays[:, 7:8] - z[:, -1:]), -1)
    a = 1 - torch.exp(-deltas * torch.relu(field[..., 3]))
    t = torch.cat((torch.ones_like(a[:, :1]), 1 - a + 1e-10), -1)
    w = a * torch.cumprod(t, -1)[:, :-1]
    rgb = (w[..., None] * field[..., :3]).sum(-2)
    depth = (w * z).sum(-1)
    alpha = w.sum(-1)
    if white:
        rgb = rgb + 1 - alpha[:, None]
    var = (w * (z - depth[:, None]) ** 2).sum(-1).clamp(min=0)
    return w, rgb, depth, alpha, var


def rel(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max().clamp(min=1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------ 1 fixture parity
@pytest.fixture(scope="module")
def g7(ops):
    g = load("g7_composite.npz")
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]))
    return g, hip_scene(ops, sc), hip_mlp(ops, msd), T(g["rays"]).cuda(), T(g["z"]).cuda(), T(g["field"]).cuda()


def test_fixture_parity(ops, g7):
    g, hs, hm, r7, z7, field = g7
    for wb in (0, 1):
        want = T(g[f"weights_{wb}"]).double().sum(-1)           # the reference's own weights, summed in float64
        base = ops.composite(field, z7, r7, bool(wb))
        wts, rgb, depth, alpha, var = ops.composite(field, z7, r7, bool(wb), want_aux=True)
        assert all(torch.equal(a, b) for a, b in zip((wts, rgb, depth), base))
        e = rel(alpha, want)
        print(f"composite white={wb} alpha: {e:.3e}")
        assert e < TOL_STAGE and (var >= 0).all()
        base = ops.render(hs, hm, r7, z7, bool(wb), want_weights=True)
        wts, rgb, depth, alpha, var = ops.render(hs, hm, r7, z7, bool(wb), want_weights=True, want_aux=True)
        assert all(torch.equal(a, b) for a, b in zip((wts, rgb, depth), base))
        e = rel(alpha, want)
        print(f"render    white={wb} alpha: {e:.3e}")
        assert e < TOL and (var >= 0).all()


@pytest.mark.parametrize("views_entry", [False, True])
def test_render_entries_equal_the_compositor_on_their_field(ops, g7, views_entry):
    """diner_render_aux_f32 / diner_render_views_aux_f32 directly: their outputs are those of diner_composite_aux_f32 on the field they
    left in the scratch buffer, bit for bit (K <= 256), and their colours those of the entries without the aux outputs."""
    from diner_amd import _lib
    lib = ops.lib
    g, hs, hm, r7, z7, _ = g7
    NR, K = z7.shape
    assert K <= 256
    hs.prepare(hm)
    new = lambda *s: torch.empty(*s, device="cuda")
    fws, ws = new(NR, K, 4), ops._workspace(lib.diner_field_workspace_bytes(NR * K), r7.device)
    rgb, depth, wts, alpha, var = new(NR, 3), new(NR), new(NR, K), new(NR), new(NR)
    entry, plain = (lib.diner_render_views_aux_f32, lib.diner_render_views_f32) if views_entry else (lib.diner_render_aux_f32, lib.diner_render_f32)
    p = ops._ptr
    _lib.check(entry(hs.ref, hm.handle, p(r7), p(z7), NR, K, 1, ops.get_precision(), p(rgb), p(depth), p(wts), p(fws), p(ws), p(alpha),
                     p(var), ops._stream()))
    w2, rgb2, depth2, alpha2, var2 = ops.composite(fws, z7, r7, True, want_aux=True)
    for a, b in ((rgb, rgb2), (depth, depth2), (wts, w2), (alpha, alpha2), (var, var2)):
        assert torch.equal(a, b)
    rgb3, depth3 = new(NR, 3), new(NR)
    _lib.check(plain(hs.ref, hm.handle, p(r7), p(z7), NR, K, 1, ops.get_precision(), p(rgb3), p(depth3), None, p(fws), p(ws), ops._stream()))
    assert torch.equal(rgb, rgb3) and torch.equal(depth, depth3)
    assert rel(alpha, T(g["weights_1"]).double().sum(-1)) < TOL


# ------------------------------------------------------------------------------------------------------------------ 2 edge shapes
KS = (1, 2, 63, 64, 65, 256, 257, 1024)       # one lane, a full wave, the first second slot, the per-lane width switch, the cap
NEAR, FAR = 0.5, 1.5


def edge_case(K):
    """Seven rays: 0 has z_K > far (and density there: a negative weight), 1 has sigma <= 0 everywhere, 2 has sigma = 1e4 everywhere,
    3..6 are plain.  The density scale follows K below 40 samples, so that a ray of one or two samples is not simply opaque (its depth
    spread would be nothing but rounding)."""
    gen = torch.Generator().manual_seed(7000 + K)
    field = torch.rand(7, K, 4, generator=gen)
    dens = 30.0 * min(1.0, K / 40)
    field[..., 3] = torch.relu(torch.randn(7, K, generator=gen)) * dens
    field[0, -1, 3] = dens
    field[1, :, 3] = -torch.rand(K, generator=gen)
    field[1, ::2, 3] = 0.0
    field[2, :, 3] = 1e4
    rays = torch.zeros(7, 8)
    rays[:, 3:6] = torch.nn.functional.normalize(torch.randn(7, 3, generator=gen), dim=-1)
    rays[:, 6], rays[:, 7] = NEAR, FAR
    z = (NEAR + (FAR - NEAR) * torch.rand(7, K, generator=gen)).sort(-1).values.clamp(max=FAR - 0.01)
    z[0, -1] = FAR + 0.02
    return field, z, rays


_refs = {}


def edge_reference(K, white):
    """(inputs, float64 outputs, float32-torch-on-the-CPU outputs) of the case, computed once."""
    if (K, white) not in _refs:
        field, z, rays = edge_case(K)
        _refs[(K, white)] = ((field, z, rays), formula(field.double(), z.double(), rays.double(), white), formula(field, z, rays, white))
    return _refs[(K, white)]


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("K", KS)
def test_edge_shapes(ops, K, white):
    """NR = 7, 5 (partial workgroups of four rays) and 1 (each of rays 0..3 alone) against the float64 formula.  Bar per output: TOL_STAGE
    where the float32 torch evaluation of the same expression (the yardstick, same max-norm) fits in it, 4 x the yardstick above (the
    kernel's wave-tree summation order differs from torch's)."""
    (field, z, rays), ref64, ref32 = edge_reference(K, white)
    names = ("weights", "rgb", "depth", "alpha", "depth_var")
    for rows in (slice(0, 7), slice(0, 5), slice(0, 1), slice(1, 2), slice(2, 3), slice(3, 4)):
        f, zz, rr = (t[rows].contiguous().cuda() for t in (field, z, rays))
        got = ops.composite(f, zz, rr, white, want_aux=True)
        base = ops.composite(f, zz, rr, white)
        assert all(torch.equal(a, b) for a, b in zip(got[:3], base)), (K, rows)
        for name, g_, r64, r32 in zip(names, got, ref64, ref32):
            if name not in ("alpha", "depth_var"):
                continue
            want = r64[rows]
            scale = r64.abs().max().clamp(min=1e-30)            # one scale per case: that of the seven-ray launch
            yard = ((r32.double() - r64).abs().max() / scale).item()
            err = ((g_.double().cpu() - want).abs().max() / scale).item()
            bar = TOL_STAGE if yard <= TOL_STAGE else 4 * yard
            print(f"K={K} white={white} rays {rows.start}:{rows.stop} {name}: {err:.2e} (float32 torch {yard:.2e}, bar {bar:.2e})")
            assert err < bar, (K, rows, name, err, yard)
        alpha, var = got[3].cpu(), got[4].cpu()
        assert (var >= 0).all() and torch.isfinite(var).all() and torch.isfinite(alpha).all()
        if rows.start <= 1 < rows.stop:                          # no density anywhere: nothing absorbed, the background shows through
            i = 1 - rows.start
            assert alpha[i].item() == 0.0 and var[i].item() == 0.0
            assert (got[1][i].cpu() == (1.0 if white else 0.0)).all()
        if rows.start <= 2 < rows.stop and K > 1:                # opaque at the first sample
            assert abs(alpha[2 - rows.start].item() - 1.0) < 1e-6


# ------------------------------------------------------------------------------------------------------------------ 3 null pointers
@pytest.mark.parametrize("K", [40, 300])
def test_either_aux_pointer_may_be_null(ops, K):
    from diner_amd import _lib
    lib, p = ops.lib, ops._ptr
    (field, z, rays), _, _ = edge_reference(64, True)
    gen = torch.Generator().manual_seed(K)
    field = torch.rand(7, K, 4, generator=gen).cuda()
    field[..., 3] *= 20
    z = (NEAR + torch.rand(7, K, generator=gen)).sort(-1).values.clamp(max=FAR - 0.01).cuda()
    rays = rays.cuda()
    _, rgb0, depth0, alpha0, var0 = ops.composite(field, z, rays, True, want_weights=False, want_aux=True)
    for which in ("alpha", "depth_var"):
        rgb, depth, out = torch.empty(7, 3, device="cuda"), torch.empty(7, device="cuda"), torch.full((7,), -7.0, device="cuda")
        a, v = (p(out), None) if which == "alpha" else (None, p(out))
        _lib.check(lib.diner_composite_aux_f32(p(field), p(z), p(rays), 7, K, 1, p(rgb), p(depth), None, a, v, ops._stream()))
        assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)
        assert torch.equal(out, alpha0 if which == "alpha" else var0)


# ------------------------------------------------------------------------------------------------------------------ 4 many views
def test_many_views_nv6(ops):
    from tests.test_many_views_cpu import nv_inputs
    g = load("g23_many_views.npz")
    sc, scene, w, rs, noises = nv_inputs(g, 6)
    _, _, _, msd, _ = oracle_setup(int(g["W"]), int(g["H"]), int(g["scene_seed"]), nv=6)
    K = int(g["K"])
    hs, hm = hip_scene(ops, sc), hip_mlp(ops, msd)
    assert hs.nv == 6
    r, z = rs.cuda(), T(g[f"z_6_{K}"]).cuda()
    _, rgb0, depth0 = ops.render(hs, hm, r, z, False)
    wts, rgb, depth, alpha, var = ops.render(hs, hm, r, z, False, want_weights=True, want_aux=True)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)
    e = rel(alpha, wts.double().cpu().sum(-1))
    print(f"NV=6 alpha against the weights of the same call: {e:.2e}")
    assert e < TOL_STAGE and (var >= 0).all()


# ------------------------------------------------------------------------------------------------------------------ 5 backward
@pytest.mark.parametrize("K", [1, 40, 65])
def test_backward_against_float64_autograd(ops, K):
    from diner_amd import _lib, train
    lib, p = ops.lib, ops._ptr
    NR = 5
    gen = torch.Generator().manual_seed(500 + K)
    field = torch.rand(NR, K, 4, generator=gen)
    field[..., 3] = torch.relu(torch.randn(NR, K, generator=gen)) * 30
    rays = torch.zeros(NR, 8); rays[:, 6] = NEAR; rays[:, 7] = FAR
    z = (NEAR + torch.rand(NR, K, generator=gen)).sort(-1).values.clamp(max=FAR - 0.01)
    z[3, -1] = FAR + 0.1                                                # a sample beyond `far`: negative delta (:301)
    Grgb, Gd, Ga = torch.randn(NR, 3, generator=gen), torch.randn(NR, generator=gen), torch.randn(NR, generator=gen)
    fc, zc, rc = field.cuda(), z.cuda(), rays.cuda()
    Grgb_c, Gd_c, Ga_c = Grgb.cuda(), Gd.cuda(), Ga.cuda()               # named: a raw pointer does not keep a temporary's memory alive
    for white in (False, True):
        f64 = field.double().requires_grad_(True)
        _, rgb_o, d_o, a_o, _ = formula(f64, z.double(), rays.double(), white)
        ((rgb_o * Grgb.double()).sum() + (d_o * Gd.double()).sum() + (a_o * Ga.double()).sum()).backward()
        d_field = torch.empty_like(fc)
        _lib.check(lib.diner_composite_aux_bwd_f32(p(fc), p(zc), p(rc), NR, K, int(white), p(Grgb_c), p(Gd_c), p(Ga_c), p(d_field),
                                                   ops._stream()))
        e = max_norm_rel(d_field.cpu(), f64.grad)
        # the autograd node: the same gradient from rgb / depth / alpha as outputs of one Function
        fh = fc.clone().requires_grad_(True)
        rgb, dep, alpha = train.composite_train(fh, zc, rc, white, want_alpha=True)
        assert max_norm_rel(alpha.detach().cpu(), a_o.detach()) < TOL_STAGE
        ((rgb * Grgb_c).sum() + (dep * Gd_c).sum() + (alpha * Ga_c).sum()).backward()
        assert torch.equal(fh.grad, d_field)
        print(f"aux compositor adjoint K={K} white={white}: {e:.2e}")
        assert e < TOL_GRAD
        # without an opacity gradient: the existing entry's bits
        a, b = torch.empty_like(fc), torch.empty_like(fc)
        _lib.check(lib.diner_composite_aux_bwd_f32(p(fc), p(zc), p(rc), NR, K, int(white), p(Grgb_c), p(Gd_c), None, p(a), ops._stream()))
        _lib.check(lib.diner_composite_bwd_f32(p(fc), p(zc), p(rc), NR, K, int(white), p(Grgb_c), p(Gd_c), p(b), ops._stream()))
        assert torch.equal(a, b)
        if K > 1:
            assert not torch.equal(a, d_field)


# ------------------------------------------------------------------------------------------------------------------ 6 modules
def test_renderer_forward_want_alpha(ops):
    """128 rays x 40 samples through the drop-in renderer, without grad and in grad mode.  The weights `want_weights` returns in grad mode
    are detached, so the gradient of alpha.sum() is held to the oracle's autograd of weights.sum() on the same samples, at the bar of
    tests/test_train_gpu.py::test_module_training_step_against_oracle_autograd (1e-4, or twice float32 torch autograd's own distance
    from the float64 gradient where that is larger)."""
    import copy
    from tests.test_boundary_gpu import setup_model
    from tests.tests_train_util import oracle_key
    from diner_amd import noise
    sc, nerf, R, rays = setup_model(32, 32, 4)
    NR, K, G, n_cand, seed = 128, 40, 15, 1000, 20261018
    r = rays[torch.linspace(0, rays.shape[0] - 1, NR).long()].cuda()[None]
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=True)
    with torch.no_grad(), noise.keyed(seed, 0):
        base = ren.forward(nerf, r)
        out = ren.forward(nerf, r, want_alpha=True)
        both = ren.forward(nerf, r, want_weights=True, want_alpha=True)
    assert sorted(base.fine.keys()) == ["depth", "rgb"]
    assert sorted(out.fine.keys()) == ["alpha", "depth", "depth_var", "rgb"]
    assert torch.equal(out.fine.rgb, base.fine.rgb) and torch.equal(out.fine.depth, base.fine.depth)
    assert tuple(out.fine.alpha.shape) == (1, NR) and tuple(out.fine.depth_var.shape) == (1, NR) and (out.fine.depth_var >= 0).all()
    assert rel(out.fine.alpha, both.fine.weights.double().cpu().sum(-1)) < TOL_STAGE
    # grad mode
    nerf.train()
    nerf.encoder.latent = nerf.encoder.latent.detach().requires_grad_(True)
    assert nerf.needs_grad()
    with noise.keyed(seed, 0):
        base_t = ren.forward(nerf, r)
        out_t = ren.forward(nerf, r, want_alpha=True)
    assert sorted(base_t.fine.keys()) == ["depth", "rgb"] and sorted(out_t.fine.keys()) == ["alpha", "depth", "rgb"]
    assert torch.equal(out_t.fine.rgb, base_t.fine.rgb) and out_t.fine.alpha.requires_grad
    assert max_norm_rel(out_t.fine.alpha.detach().cpu(), out.fine.alpha.cpu()) < TOL_STAGE
    # the gradient of the opacity, on injected noise (so that the oracle gets the same sample positions)
    gen = torch.Generator().manual_seed(61)
    inj = (torch.rand(1, NR, n_cand, generator=gen).cuda(), torch.randn(1, NR, G, generator=gen).cuda(), torch.rand(1, NR, K, generator=gen).cuda())
    with noise.inject(*inj):
        with torch.no_grad():
            z = ren.fill_up_uniform_samples(ren.sample_depthguided(r, nerf, K, n_cand, n_gaussian=G), r)
        alpha = ren.forward(nerf, r, want_alpha=True).fine.alpha
    alpha.sum().backward()
    # the oracle on the same samples: float32 autograd and float64 autograd of weights.sum()
    _, scene, w, msd, _ = oracle_setup(32, 32, 4)
    rc, zc = r[0].cpu(), z[0].cpu()
    xyz = (rc[:, None, :3] + zc[..., None] * rc[:, None, 3:6]).reshape(-1, 3)
    dirs = rc[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3)

    def leaves_of(scene_, w_, dt):
        s2, w2, leaves = copy.copy(scene_), copy.copy(w_), {}
        for k, v in vars(scene_).items():
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(s2, k, v.detach().to(dt))
        for k, v in vars(w_).items():
            if isinstance(v, (list, tuple)):
                new = [t.detach().to(dt).requires_grad_(True) for t in v]
                setattr(w2, k, new)
                leaves.update({(k, i): t for i, t in enumerate(new)})
            elif torch.is_tensor(v) and v.is_floating_point():
                leaves[(k, None)] = v.detach().to(dt).requires_grad_(True)
                setattr(w2, k, leaves[(k, None)])
        return s2, w2, leaves

    grads = {}
    for dt in (torch.float32, torch.float64):
        s2, w2, leaves = leaves_of(scene, w, dt)
        f = O.pixelnerf_forward(s2, w2, xyz.to(dt), dirs.to(dt)).view(NR, K, 4)
        wts, _, _ = O.composite_from_field(f, rc.to(dt), zc.to(dt), True)
        wts.sum().backward()
        grads[dt] = leaves
    worst, worst_o = ("", 0.0), ("", 0.0)
    for name, prm in nerf.mlp_fine.named_parameters():
        exact = grads[torch.float64][oracle_key(name)].grad
        worst = max(worst, (name, max_norm_rel(prm.grad.cpu().double(), exact)), key=lambda t: t[1])
        worst_o = max(worst_o, (name, max_norm_rel(grads[torch.float32][oracle_key(name)].grad.double(), exact)), key=lambda t: t[1])
    print(f"d alpha.sum() / d MLP parameters vs float64 autograd of weights.sum(): HIP {worst[0]} {worst[1]:.2e}; float32 torch autograd "
          f"itself {worst_o[0]} {worst_o[1]:.2e}")
    assert worst[1] < max(TOL_GRAD, 2.0 * worst_o[1])
    assert nerf.encoder.latent.grad is not None and float(nerf.encoder.latent.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 7 image harness
IW = IH = 16
IK, IG, ISEED = 40, 15, 20261019
_MODEL = {}


def _predict(rank, world, return_alpha):
    from diner_amd.render import predict_image
    from tests.test_boundary_gpu import setup_model
    if "m" not in _MODEL:
        _MODEL["m"] = setup_model(IW, IH, 3)
    sc, nerf, R, _ = _MODEL["m"]
    ren = R(n_samples=IK, n_depth_candidates=1000, n_gaussian=IG, white_bkgd=True)
    E, Km = sc["target_extrinsics"][None].cuda(), sc["target_intrinsics"][None].cuda()
    kw = dict(return_alpha=True) if return_alpha else {}
    return predict_image(nerf, ren, E, Km, IW, IH, sc["znear"], sc["zfar"], ray_batch_size=100, rank=rank, world=world, seed=ISEED, **kw)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(max(1, torch.get_num_threads() // world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = _predict(rank, world, True)
        if rank == 0:
            q.put(tuple(t.cpu().numpy() for t in out))
        else:
            assert len(out) == 3 and all(t is None for t in out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_predict_image_return_alpha(ops):
    rgb0, depth0 = _predict(0, 1, False)
    rgb, depth, alpha = _predict(0, 1, True)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)
    assert tuple(alpha.shape) == (1, 1, IH, IW) and alpha[0].shape == (1, IH, IW) and torch.isfinite(alpha).all()
    assert float(alpha.min()) > -1e-5 and float(alpha.max()) < 1 + 1e-5
    # two gloo ranks on the one device: the gathered tiles carry the fifth channel
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(rk, 2, port, q)) for rk in range(2)]
    for pr in procs:
        pr.start()
    try:
        got = [torch.from_numpy(a) for a in q.get(timeout=300)]
        for pr in procs:
            pr.join(timeout=120)
            assert pr.exitcode == 0
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.kill()
    assert torch.equal(got[0], rgb.cpu()) and torch.equal(got[1], depth.cpu()) and torch.equal(got[2], alpha.cpu())


def test_write_prediction_folder_alpha_png(ops, tmp_path):
    """<stem>-alpha.png: 8-bit grey, save_image's quantisation of the opacity map; the default folder has no such file."""
    from diner_amd import evaluate
    from diner_amd.png import read_png
    from diner_amd.render import predict_image
    from tests.test_boundary_gpu import setup_model
    if "m" not in _MODEL:
        _MODEL["m"] = setup_model(IW, IH, 3)
    sc, nerf, R, _ = _MODEL["m"]
    ren = R(n_samples=IK, n_depth_candidates=1000, n_gaussian=IG, white_bkgd=True)
    encode, nerf.encode = nerf.encode, lambda **kw: None               # the scene is injected (setup_model), as everywhere in this suite
    try:
        batch = dict(target_rgb=torch.rand(1, 3, IH, IW), src_rgbs=torch.rand(1, 4, 3, IH, IW), sample_name=["view0"],
                     target_extrinsics=sc["target_extrinsics"][None], target_intrinsics=sc["target_intrinsics"][None])
        import diner_amd.datasets as datasets
        orig, datasets.encode_args = datasets.encode_args, lambda b, dev: {}
        try:
            torch.manual_seed(5)
            evaluate.write_prediction_folder(nerf, ren, [batch], str(tmp_path / "plain"), sc["znear"], sc["zfar"])
            torch.manual_seed(5)
            evaluate.write_prediction_folder(nerf, ren, [batch], str(tmp_path / "matte"), sc["znear"], sc["zfar"], write_alpha=True)
            torch.manual_seed(5)
            _, _, alpha = predict_image(nerf, ren, batch["target_extrinsics"].cuda(), batch["target_intrinsics"].cuda(), IW, IH, sc["znear"],
                                        sc["zfar"], return_alpha=True)
        finally:
            datasets.encode_args = orig
    finally:
        nerf.encode = encode
    plain, matte = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(tmp_path / "matte"))
    assert "view0-alpha.png" not in plain and matte == sorted(plain + ["view0-alpha.png"])
    for name in plain:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "matte" / name, "rb").read(), name
    img = read_png(str(tmp_path / "matte" / "view0-alpha.png"))
    assert img.shape == (IH, IW) and img.dtype == np.uint8
    want = (alpha[0, 0].cpu() * 255 + 0.5).clamp(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(img, want)


# ------------------------------------------------------------------------------------------------------------------ 8 objective
def test_calc_losses_w_alpha(ops):
    from diner_amd import noise, objective
    from diner_amd.synthetic import build_modules, make_scene, make_mlp_state_dict
    W = H = 64
    SB, B, K, G, n_cand = 2, 128, 40, 15, 1000
    scs = [make_scene(W, H, seed=31 + i) for i in range(SB)]
    nerf, R = build_modules(scs, make_mlp_state_dict(), torch.device("cuda", 0))
    nerf.train()
    latent0 = nerf.encoder.latent.detach().clone()

    def encode(images, depths, depths_std, extrinsics, intrinsics):       # stands in for the ResNet trunk: a fresh leaf latent per call
        nerf.encoder.latent = latent0.clone().requires_grad_(True)
        nerf._scenes = {}

    nerf.encode = encode
    gen = torch.Generator().manual_seed(12)
    st = lambda k: torch.stack([sc[k] for sc in scs]).cuda()
    batch = dict(src_rgbs=torch.rand(SB, 4, 3, H, W, generator=gen).cuda(), src_depths=st("depths"), src_depth_stds=st("depths_std"),
                 src_extrinsics=st("src_extrinsics"), src_intrinsics=st("src_intrinsics"), target_rgb=torch.rand(SB, 3, H, W, generator=gen).cuda(),
                 target_alpha=torch.rand(SB, 1, H, W, generator=gen).cuda(), target_extrinsics=torch.stack([sc["target_extrinsics"] for sc in scs]),
                 target_intrinsics=torch.stack([sc["target_intrinsics"] for sc in scs]))
    znear, zfar = scs[0]["znear"], scs[0]["zfar"]
    ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=True)
    inj = (torch.rand(SB, B, n_cand, generator=gen).cuda(), torch.randn(SB, B, G, generator=gen).cuda(), torch.rand(SB, B, K, generator=gen).cuda())
    params = dict(nerf.mlp_fine.named_parameters())

    def step(**kw):
        for prm in nerf.parameters():
            prm.grad = None
        info = {}
        torch.manual_seed(77)                                             # the same loose pixels in every call
        with noise.inject(*inj):
            ld = objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, ray_batch_size=B, info=info, **kw)
        ld["total"].backward()
        return ld, info, {k: prm.grad.clone() for k, prm in params.items()}

    ld0, info0, g0 = step()
    ldz, _, gz = step(w_alpha=0.)
    assert set(ld0) == set(ldz) == {"rgb_fine", "vgg_fine", "antibias", "total"}
    assert torch.equal(ld0["total"], ldz["total"])
    assert max(max_norm_rel(gz[k].cpu(), g0[k].cpu()) for k in g0) < 1e-5         # (the weight gradients sum with atomics: not bit-stable)
    lda, infoa, ga = step(w_alpha=0.5)
    assert set(lda) == {"rgb_fine", "vgg_fine", "antibias", "total", "alpha"}
    assert torch.equal(infoa["pix"], info0["pix"]) and torch.equal(infoa["pred"].detach(), info0["pred"].detach())
    assert torch.equal(lda["rgb_fine"], ld0["rgb_fine"])
    # the term itself, from a render of the same rays on the same (grad-mode) path, evaluated in float64
    from diner_amd.ops import gen_rays_at
    rays = gen_rays_at(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, infoa["pix"])
    assert nerf.needs_grad()
    with noise.inject(*inj):
        alpha = ren.forward(nerf, rays, want_alpha=True).fine.alpha.detach()
    gt = batch["target_alpha"][:, 0].reshape(SB, H * W).gather(1, infoa["pix"].long())
    want = (alpha.double() - gt.double()).square().mean().item()
    assert float(lda["alpha"].detach()) > 0 and abs(float(lda["alpha"].detach()) - want) <= 1e-6 * want      # a float32 mean of SB x B squares
    old, new = float(ld0["total"].detach()), float(lda["total"].detach())
    assert abs(new - (old + 0.5 * float(lda["alpha"].detach()))) <= 4 * 2.0 ** -24 * new        # a float32 sum of two float32 terms
    assert max(max_norm_rel(ga[k].cpu(), g0[k].cpu()) for k in ga) > 1e-4               # the opacity term reached the parameters
