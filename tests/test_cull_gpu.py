"""GPU: empty-ray culling -- diner_compact_live_f32 / diner_expand_live_f32 through ops, predict_image(cull_empty=True), the renderer's
cull_empty attribute and two ranks sharing the device.

  1  the compaction against the Python reference (tests/cull_util.py), byte for byte: sizes around the 64-lane wave and the 256-ray
     block and several blocks, vector and scalar row lengths, flag patterns, NaN / +inf, two thresholds, split lists, a short capacity;
  2  the expansion against the indexing expression;
  3  the culled frame is the plain frame at the live pixels (torch.equal: a ray's result does not depend on its launch) and exactly the
     compositor's zero-density row elsewhere, for three batch sizes, both backgrounds and a six-view scene; the live mask holds every
     ray the oracle pins live and none it pins dead (same candidate jitter, injected);
  4  the field kernels process n_live * K points, not 1920 * K;
  5  edges: a camera that sees nothing, the scene's own focal length, cull_below;
  6  NeRFRendererDGS.cull_empty through forward, ignored in grad mode;
  7  two ranks on one device render the single-process culled frame."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from tests import cull_util as U

pytestmark = pytest.mark.gpu
K, G, N_CAND, SEED = 40, 15, U.N_CAND, 20261018


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from diner_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------------ 1 compaction
def flag_patterns(NR):
    g = torch.Generator().manual_seed(NR)
    alt = torch.arange(NR) % 2 == 0
    first, last = torch.zeros(NR, dtype=torch.bool), torch.zeros(NR, dtype=torch.bool)
    first[0], last[-1] = True, True
    return {"all_dead": torch.zeros(NR, dtype=torch.bool), "all_live": torch.ones(NR, dtype=torch.bool), "alternating": alt,
            "p0.4": torch.rand(NR, generator=g) < 0.4, "first": first, "last": last}


def stats_for(live, threshold, seed):
    """(NR,4) stats whose column 1 realises the flags at this threshold: dead values at and below it (both zeros), live values above it,
    a NaN and a +inf among the live ones; the other columns are noise the kernel must not look at."""
    g = torch.Generator().manual_seed(seed)
    NR = live.shape[0]
    dead_vals = torch.tensor([0.0, -0.0] if threshold == 0 else [0.0, 0.5, 0.25, -1.0])
    live_vals = torch.tensor([1e-30, 0.75, 1.0, float("inf"), float("nan")] if threshold == 0 else
                             [0.50000006, 0.75, 1.0, float("inf"), float("nan")])
    st = torch.randn(NR, 4, generator=g)
    pick = torch.randint(0, 1 << 30, (NR,), generator=g)
    st[:, 1] = torch.where(live, live_vals[pick % len(live_vals)], dead_vals[pick % len(dead_vals)])
    return st


def gpu_compact(ops, st, thr, rays, z, cuts, cap_rows, capacity, base=0):
    """The list in consecutive calls at `cuts` into sentinel-filled buffers of cap_rows rows, of which the first `capacity` are handed
    to the entry -> CPU (rays_out, z_out, live_idx, slot, counter)."""
    Kz = z.shape[1]
    ro = torch.full((cap_rows, 8), -7.0, device="cuda")
    zo = torch.full((cap_rows, Kz), -7.0, device="cuda")
    li = torch.full((cap_rows,), -7, device="cuda", dtype=torch.int32)
    n = torch.full((1,), base, device="cuda", dtype=torch.int32)
    std, rd, zd = st.cuda(), rays.cuda(), z.cuda()
    slots = []
    edges = [0] + list(cuts) + [st.shape[0]]
    for a, b in zip(edges[:-1], edges[1:]):
        slot, n_ret = ops.compact_live(std[a:b], thr, rd[a:b], zd[a:b], 100 + a, ro[:capacity], zo[:capacity], li[:capacity], n)
        assert n_ret is n
        slots.append(slot)
    return ro.cpu(), zo.cpu(), li.cpu(), torch.cat(slots).cpu(), int(n.item())


def same(a, b):
    return all(torch.equal(U.bits(x), U.bits(y)) if torch.is_tensor(x) else x == y for x, y in zip(a, b))


@pytest.mark.parametrize("Kz", [1, 40, 129])
@pytest.mark.parametrize("NR", [1, 63, 64, 65, 255, 256, 257, 1000, 8197])
def test_compaction_against_python_reference(ops, NR, Kz):
    g = torch.Generator().manual_seed(1000 * NR + Kz)
    rays, z = torch.randn(NR, 8, generator=g), torch.randn(NR, Kz, generator=g)
    for thr in (0.0, 0.5):
        for name, live in flag_patterns(NR).items():
            st = stats_for(live, thr, NR + Kz)
            ro, zo, li = torch.full((NR + 3, 8), -7.0), torch.full((NR + 3, Kz), -7.0), torch.full((NR + 3,), -7, dtype=torch.int32)
            slot, n = U.ref_compact(st, thr, rays, z, 100, 2, ro, zo, li)
            assert n == 2 + int(live.sum()), (name, thr)               # the flags are the pattern's: NaN and +inf count as live
            want = (ro, zo, li, slot, n)
            one = gpu_compact(ops, st, thr, rays, z, (), NR + 3, NR + 3, base=2)
            assert same(one, want), (name, thr)
            for cuts in ((NR // 2,), (NR // 3, 2 * NR // 3 + 1)):
                cuts = [c for c in cuts if 0 < c < NR]
                if cuts:
                    assert same(gpu_compact(ops, st, thr, rays, z, cuts, NR + 3, NR + 3, base=2), want), (name, thr, cuts)


@pytest.mark.parametrize("NR,Kz", [(257, 40), (1000, 129), (8197, 1)])
def test_compaction_capacity_below_the_live_count(ops, NR, Kz):
    g = torch.Generator().manual_seed(NR)
    rays, z = torch.randn(NR, 8, generator=g), torch.randn(NR, Kz, generator=g)
    live = flag_patterns(NR)["p0.4"]
    st = stats_for(live, 0.0, NR)
    n_true = int(live.sum())
    cap = n_true // 2
    ro, zo, li = torch.full((NR, 8), -7.0), torch.full((NR, Kz), -7.0), torch.full((NR,), -7, dtype=torch.int32)
    slot, n = U.ref_compact(st, 0.0, rays, z, 100, 0, ro[:cap], zo[:cap], li[:cap])
    assert n == n_true and (ro[cap:] == -7).all()
    first = gpu_compact(ops, st, 0.0, rays, z, (NR // 2,), NR, cap)
    assert same(first, (ro, zo, li, slot, n_true))                     # rows beyond the capacity keep the sentinel, the counter is true
    assert (first[3] < cap).all() and int((first[3] >= 0).sum()) == cap
    assert same(gpu_compact(ops, st, 0.0, rays, z, (NR // 2,), NR, cap), first)
    none = gpu_compact(ops, st, 0.0, rays, z, (), NR, 0)                # capacity 0: nothing written, everything counted
    assert none[4] == n_true and (none[3] == -1).all() and (none[0] == -7).all()


# ------------------------------------------------------------------------------------------------------------------- 2 expansion
@pytest.mark.parametrize("N", [1, 65, 1920])
@pytest.mark.parametrize("C", [1, 4, 5, 8])
def test_expansion_against_indexing(ops, C, N):
    g = torch.Generator().manual_seed(10 * N + C)
    bg = torch.randn(C, generator=g)
    live = torch.rand(N, generator=g) < 0.4
    for flags in (torch.zeros(N, dtype=torch.bool), torch.ones(N, dtype=torch.bool), live):
        n = int(flags.sum())
        slot = torch.full((N,), -1, dtype=torch.int32)
        slot[flags] = torch.arange(n, dtype=torch.int32)
        tiles = torch.randn(n, C, generator=g)
        out = ops.expand_live(tiles.cuda(), slot.cuda(), bg.cuda())
        assert out.shape == (N, C) and torch.equal(U.bits(out), U.bits(U.ref_expand(tiles, slot, bg)))
    # a tile list with spare rows: only the first n_tiles count, a slot beyond them reads nothing
    spare = torch.randn(N + 2, C, generator=g)
    slot = torch.arange(N, dtype=torch.int32)
    out = ops.expand_live(spare.cuda(), slot.cuda(), bg.cuda(), n_tiles=N // 2)
    want = torch.where((slot < N // 2)[:, None], spare[:N], bg[None])
    assert torch.equal(U.bits(out), U.bits(want))


# ------------------------------------------------------------------------------------------------------------------ 3 the frame
_MODELS = {}


def model(nv=4, w=U.W, h=U.H, focal_scale=0.5):
    """(scene case, PixelNeRF on the device, renderer class, E (1,4,4), Kt (1,3,3)), built once per process."""
    key = (nv, w, h, focal_scale)
    if key not in _MODELS:
        from diner_amd.synthetic import build_modules
        case = U.scene_case(nv, w, h, focal_scale)
        nerf, R = build_modules(case.sc, case.msd, "cuda", normals=case.sc["normals"])
        _MODELS[key] = (case, nerf, R, case.sc["target_extrinsics"][None].cuda(), case.Kt[None].cuda())
    return _MODELS[key]


def frames(nerf, ren, E, Kt, w, h, sc, batch=8192, seed=SEED, **kw):
    from diner_amd.render import predict_image
    return predict_image(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], ray_batch_size=batch, seed=seed, return_alpha=True, **kw)


def hit_map(nerf, E, Kt, w, h, sc, seed=SEED):
    from diner_amd.render import predict_surface_prior
    hit = predict_surface_prior(nerf, E, Kt, w, h, sc["znear"], sc["zfar"], K, N_CAND, G, seed=seed)[0]
    assert not torch.isnan(hit).any()
    return hit


def check_culled_against_plain(culled, plain, live, white):
    """live (1,1,H,W) bool: there the culled frame is the plain one bit for bit, elsewhere the compositor's zero-density row."""
    for c, p in zip(culled, plain):
        m = live.expand_as(c)
        assert c.shape == p.shape and torch.equal(c[m], p[m])
    rgb, depth, alpha = culled
    dead = ~live
    assert (rgb[dead.expand_as(rgb)] == (1.0 if white else 0.0)).all()
    assert (depth[dead] == 0).all() and (alpha[dead] == 0).all()


@pytest.mark.parametrize("nv,white", [(4, True), (4, False), (6, True)])
def test_culled_frame_is_the_plain_frame_where_it_renders(ops, nv, white):
    case, nerf, R, E, Kt = model(nv)
    sc, w, h = case.sc, case.w, case.h
    ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=white)
    mlp = nerf.hip_mlp()
    mlp.fallback_launches(reset=True)
    plain = frames(nerf, ren, E, Kt, w, h, sc)
    live = hit_map(nerf, E, Kt, w, h, sc) > 0
    n_live = int(live.sum())
    print(f"NV={nv}: {n_live} of {w * h} rays live")
    assert 0.2 * w * h <= n_live <= 0.8 * w * h
    culled = frames(nerf, ren, E, Kt, w, h, sc, cull_empty=True)
    check_culled_against_plain(culled, plain, live, white)
    for batch in (777, 64):
        again = frames(nerf, ren, E, Kt, w, h, sc, batch=batch, cull_empty=True)
        assert all(torch.equal(a, c) for a, c in zip(again, culled)), batch
    assert mlp.fallback_launches() == 0            # a range fall-back is per launch: with one, equality across launches would not follow
    # without alpha: the same colour and depth
    from diner_amd.render import predict_image
    rgb, depth = predict_image(nerf, ren, E, Kt, w, h, sc["znear"], sc["zfar"], seed=SEED, cull_empty=True)
    assert torch.equal(rgb, culled[0]) and torch.equal(depth, culled[1])
    # the oracle's verdict, under the oracle's candidate jitter
    from diner_amd import noise
    inj = tuple(t.cuda() for t in U.frame_noise(w * h, K, G))
    assert torch.equal(inj[0][0].cpu(), case.coarse)
    with noise.inject(*inj):
        plain_i = frames(nerf, ren, E, Kt, w, h, sc)
        live_i = hit_map(nerf, E, Kt, w, h, sc) > 0
        culled_i = frames(nerf, ren, E, Kt, w, h, sc, batch=777, cull_empty=True)
    check_culled_against_plain(culled_i, plain_i, live_i, white)
    flat = live_i.view(-1).cpu()
    v = case.verdict
    assert flat[v.pinned_live].all(), "a ray the oracle pins live was culled"
    assert not flat[v.pinned_dead].any(), "a ray the oracle pins dead was rendered"


# ----------------------------------------------------------------------------------------------------------- 4 the work is skipped
def test_field_kernels_run_on_live_rays_only(ops):
    case, nerf, R, E, Kt = model(4)
    sc, w, h = case.sc, case.w, case.h
    ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=True)
    n_live = int((hit_map(nerf, E, Kt, w, h, sc) > 0).sum())
    assert 0 < n_live < w * h
    ops.profile_enable()
    try:
        ops.profile_collect()
        frames(nerf, ren, E, Kt, w, h, sc, batch=777)
        plain_points = ops.profile_collect()["points"]
        frames(nerf, ren, E, Kt, w, h, sc, batch=777, cull_empty=True)
        culled_points = ops.profile_collect()["points"]
    finally:
        ops.profile_enable(False)
    assert plain_points == w * h * K
    assert culled_points == n_live * K


# ------------------------------------------------------------------------------------------------------------------------ 5 edges
def test_camera_turned_away_launches_no_field_kernel(ops):
    case, nerf, R, E, Kt = model(4)
    sc, w, h = case.sc, case.w, case.h
    flip = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0])).cuda()       # half a turn about the camera's y axis: same position, looking away
    E_away = (flip @ E[0])[None]
    for white in (True, False):
        ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=white)
        assert int((hit_map(nerf, E_away, Kt, w, h, sc) > 0).sum()) == 0
        ops.profile_enable()
        try:
            ops.profile_collect()
            rgb, depth, alpha = frames(nerf, ren, E_away, Kt, w, h, sc, cull_empty=True)
            prof = ops.profile_collect()
        finally:
            ops.profile_enable(False)
        assert prof["points"] == 0 and prof["launches"] == 0
        assert rgb.shape == (1, 3, h, w) and (rgb == (1.0 if white else 0.0)).all() and (depth == 0).all() and (alpha == 0).all()


def test_own_focal_length_almost_all_live(ops):
    case, nerf, R, E, Kt = model(4, 64, 64, 1.0)
    sc = case.sc
    ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=True)
    live = hit_map(nerf, E, Kt, 64, 64, sc) > 0
    n_dead = int((~live).sum())
    print(f"own focal length, 64 x 64: {n_dead} of 4096 rays empty")
    assert 0 < n_dead <= 0.05 * 4096
    plain = frames(nerf, ren, E, Kt, 64, 64, sc, batch=1000)
    culled = frames(nerf, ren, E, Kt, 64, 64, sc, batch=1000, cull_empty=True)
    check_culled_against_plain(culled, plain, live, True)


def test_cull_below(ops):
    case, nerf, R, E, Kt = model(4)
    sc, w, h = case.sc, case.w, case.h
    ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=False)
    hit = hit_map(nerf, E, Kt, w, h, sc)
    live = hit > 0.5
    assert 0 < int(live.sum()) < int((hit > 0).sum()), "the threshold was meant to cull some rays that see a surface"
    plain = frames(nerf, ren, E, Kt, w, h, sc)
    ops.profile_enable()
    try:
        ops.profile_collect()
        culled = frames(nerf, ren, E, Kt, w, h, sc, cull_empty=True, cull_below=0.5)
        points = ops.profile_collect()["points"]
    finally:
        ops.profile_enable(False)
    assert points == int(live.sum()) * K                               # the live mask is hit > 0.5 ...
    check_culled_against_plain(culled, plain, live, False)             # ... and those are the rays that were rendered


# --------------------------------------------------------------------------------------------------------------- 6 the attribute
def test_renderer_attribute_through_forward(ops):
    from diner_amd import noise
    case, nerf, R, E, Kt = model(4)
    sc, w, h = case.sc, case.w, case.h
    rays = ops.gen_rays(E, Kt, w, h, sc["znear"], sc["zfar"], "cuda")
    live = (hit_map(nerf, E, Kt, w, h, sc) > 0).view(1, -1)
    for white in (True, False):
        ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=white)
        with torch.no_grad(), noise.keyed(SEED, 0):
            plain = ren.forward(nerf, rays, want_alpha=True).fine
            ren.cull_empty = True
            got = ren.forward(nerf, rays, want_alpha=True).fine
            bare = ren.forward(nerf, rays).fine
            ren.cull_below = 0.5
            half = ren.forward(nerf, rays).fine
        for f in ("rgb", "depth", "alpha", "depth_var"):
            assert got[f].shape == plain[f].shape and torch.equal(got[f][live], plain[f][live]), f
        assert (got.rgb[~live] == (1.0 if white else 0.0)).all()
        assert all((got[f][~live] == 0).all() for f in ("depth", "alpha", "depth_var"))
        assert torch.equal(bare.rgb, got.rgb) and torch.equal(bare.depth, got.depth) and "alpha" not in bare
        assert not torch.equal(half.rgb, got.rgb)


def test_renderer_attribute_is_ignored_in_grad_mode(ops):
    from diner_amd import noise
    case, nerf, R, E, Kt = model(4)
    sc, w, h = case.sc, case.w, case.h
    rays = ops.gen_rays(E, Kt, w, h, sc["znear"], sc["zfar"], "cuda")[:, 20 * w:20 * w + 256].contiguous()   # rows that cross the object
    ren = R(n_samples=8, n_depth_candidates=N_CAND, n_gaussian=3, white_bkgd=True)
    assert nerf.needs_grad()
    outs = []
    for cull in (False, True):
        ren.cull_empty = cull
        with noise.keyed(SEED, 20 * w):
            outs.append(ren.forward(nerf, rays).fine)
    assert outs[1].rgb.requires_grad
    assert torch.equal(outs[0].rgb, outs[1].rgb) and torch.equal(outs[0].depth, outs[1].depth)
    with torch.no_grad(), noise.keyed(SEED, 20 * w):                    # ... and the same call without grad does cull
        culled = ren.forward(nerf, rays).fine
    assert (culled.depth == 0).any() and not torch.equal(culled.rgb, outs[0].rgb.detach())


# --------------------------------------------------------------------------------------------------------------------- 7 two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _culled_frame(rank, world):
    case, nerf, R, E, Kt = model(4)
    ren = R(n_samples=K, n_depth_candidates=N_CAND, n_gaussian=G, white_bkgd=True)
    return frames(nerf, ren, E, Kt, case.w, case.h, case.sc, batch=300, cull_empty=True, rank=rank, world=world)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(max(1, torch.get_num_threads() // world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = _culled_frame(rank, world)
        if rank == 0:
            q.put(tuple(t.cpu().numpy() for t in out))
        else:
            assert all(t is None for t in out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_sharing_one_gpu_render_the_culled_frame():
    assert torch.cuda.is_available()
    ref = _culled_frame(0, 1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = [torch.from_numpy(a) for a in q.get(timeout=600)]
        for p in procs:
            p.join(timeout=300)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert len(got) == 3 and all(torch.equal(g, r.cpu()) for g, r in zip(got, ref)), "2-rank culled frame differs from the single-process one"
