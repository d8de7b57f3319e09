"""The kernels of csrc/fmt.hip on the device against float64 on the host and fixture G30's yardsticks (tests/golden/g30_fmt.npz).

Whole cases are held against the float64 torch route (which tests/test_fmt_cpu.py holds against the fixture) with fmt_util.BAR_FACTOR (4)
times the case's recorded distance between the reference's float32 and float64, for all stages and all views, no pixel excluded.  Each
kernel alone is held against a float64 restatement of its own formula (tests/fmt_util.py); its bar is 4 x the distance the same
restatement in float32 on the CPU keeps from float64 on the same inputs (tokenise: bit-equal to torch's float32 add).  The three
determinism properties are bit-equalities.

Measured on an MI355X (max |kernel - float64| / bar): see DESIGN.md section 8o."""
import pytest
import torch

from diner_amd import mvs, ops
from tests import fmt_util as U
from tests import mvs_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SINGLE = ("tiny", "ragged")


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _device_module(name_or_seed):
    return U.make_module(name_or_seed).to(DEV)


def _run_device(net, feats, pathway=True):
    return U.run_case(net, MU.cast(feats, torch.float32, DEV), pathway)


@pytest.mark.parametrize("name", list(U.CASES))
def test_cases_against_float64(name):
    fx, c = U.fixture(), U.CASES[name]
    net = _device_module(name)
    feats = MU.cast(U.case_features(name), torch.float32, DEV)
    with torch.no_grad():
        assert net.uses_kernels(feats) if c["pathway"] else net.FMT.uses_kernels(feats[0]["stage1"])
    got, want = U.run_case(net, feats, c["pathway"]), U.expected64(name)
    for stage in U.case_stages(name):
        assert len(got[stage]) == c["NV"] and all(g.shape == w.shape and g.is_cuda and g.dtype == torch.float32
                                                  for g, w in zip(got[stage], want[stage]))
        e, bar = _err(U.stacked(got[stage]), U.stacked(want[stage])), U.BAR_FACTOR * float(fx[f"{name}_err_{stage}"])
        print(f"{name} {stage}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
        assert e <= bar, (name, stage, e, bar)


def _case_tokens(name):
    """The case's stage-1 maps of all views as (N = NV B, 32, H, W) view-major, float32 on the CPU, and the position-encoded tokens."""
    net = U.make_module(name)
    x = torch.stack([f["stage1"] for f in U.case_features(name)], 0).flatten(0, 1)
    tok = mvs._tokens(net.FMT.pos_encoding(x)).contiguous()
    return net, x, tok


@pytest.mark.parametrize("name", SINGLE)
def test_tokenise_is_torchs_add(name):
    net, x, tok = _case_tokens(name)
    got = ops.fmt_tokenise(x.to(DEV), net.FMT.pe[0].to(DEV))
    assert got.shape == tok.shape and torch.equal(got.cpu(), tok)
    H, W = x.shape[2:]
    small = net.FMT.pe[0, :, :H + 1, :W + 2].contiguous()                  # another row pitch of the encoding: the crop is indexed, not assumed
    assert torch.equal(ops.fmt_tokenise(x.to(DEV), small.to(DEV)).cpu(), tok)


@pytest.mark.parametrize("name", SINGLE + ("blocks",))
def test_attention_state_against_float64(name):
    net, _, tok = _case_tokens(name)
    pack = ops.pack_fmt_layer(net.FMT.state_dict(), "layers.1.").to(DEV)
    want = U.kv_restated(tok.double(), U.layer_weights(net, 1))
    e32 = _err(U.kv_restated(tok, U.layer_weights(net, 1, torch.float32)), want)
    got = ops.fmt_kv(tok.to(DEV), pack)
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"attention state {name}: {tok.shape[1]} tokens, {ops.fmt_kv_blocks(tok.shape[1])} blocks, kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == (tok.shape[0], 160) and e <= bar
    ws = torch.empty(tok.shape[0] * ops.fmt_kv_blocks(tok.shape[1]) * 160 + 7, dtype=torch.float64, device=DEV)
    out = torch.empty(tok.shape[0], 160, device=DEV)
    assert ops.fmt_kv(tok.to(DEV), pack, ws, out) is out and torch.equal(out, got)          # a caller's workspace: the same bits


@pytest.mark.parametrize("kind", ["self", "cross"])
@pytest.mark.parametrize("name", SINGLE)
def test_one_layer_against_float64(name, kind):
    """A self layer reads its own image's state; a cross layer on view-major images reads row n mod B."""
    net, _, tok = _case_tokens(name)
    B = U.CASES[name]["B"]
    i = 2 if kind == "self" else 3
    w64, w32 = U.layer_weights(net, i), U.layer_weights(net, i, torch.float32)
    src = tok if kind == "self" else tok[:B]                               # the reference view's images are the first B
    state = U.kv_restated(src.double(), w64).to(torch.float32)              # one float32 state for all three evaluations
    want = U.layer_restated(tok.double(), state.double(), w64)
    e32 = _err(U.layer_restated(tok, state, w32), want)
    pack = ops.pack_fmt_layer(net.FMT.state_dict(), f"layers.{i}.").to(DEV)
    xd = tok.to(DEV)
    got = ops.fmt_layer(xd, pack, state.to(DEV))
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"{kind} layer {name}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == tok.shape and e <= bar and torch.equal(xd.cpu(), tok)
    assert ops.fmt_layer(xd, pack, state.to(DEV), out=xd) is xd and torch.equal(xd, got)      # in place: the same bits


@pytest.mark.parametrize("channels", [(32, 16), (16, 8)])
@pytest.mark.parametrize("name", SINGLE)
def test_merge_against_float64(name, channels):
    c = U.CASES[name]
    (H, W), N, (Ctop, Clat) = c["hw"], c["B"] * c["NV"], channels
    if Ctop == 16:
        H, W = 2 * H, 2 * W
    g = torch.Generator().manual_seed(c["seed"] + Ctop)
    top, lat = torch.randn(N, H, W, Ctop, generator=g), torch.randn(N, 2 * H, 2 * W, Clat, generator=g)
    w = (torch.rand(Clat, Ctop, 1, 1, generator=g) * 2 - 1) / Ctop ** 0.5
    want = U.merge_restated(top.double(), w.double(), lat.double())
    e32 = _err(U.merge_restated(top, w, lat), want)
    latd = lat.to(DEV)
    got = ops.fpn_merge(top.to(DEV), w.to(DEV), latd)
    e, bar = _err(got, want), U.BAR_FACTOR * e32
    print(f"merge {Ctop} -> {Clat} {name}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got.shape == want.shape and e <= bar and torch.equal(latd.cpu(), lat)
    assert ops.fpn_merge(top.to(DEV), w.to(DEV), latd, out=latd) is latd and torch.equal(latd, got)


def test_an_image_does_not_depend_on_its_batch_position():
    net = _device_module("ragged")
    feats = U.case_features("ragged")                                      # B = 2
    a = _run_device(net, feats)
    b = _run_device(net, [{k: v.flip(0) for k, v in f.items()} for f in feats])
    for stage in U.STAGES:
        for v in range(len(feats)):
            assert torch.equal(a[stage][v][0], b[stage][v][1]) and torch.equal(a[stage][v][1], b[stage][v][0]), (stage, v)


def test_a_source_view_does_not_depend_on_how_many_are_batched_with_it():
    net = _device_module("ragged")
    feats = U.case_features("ragged")                                      # NS = 3
    full = _run_device(net, feats)
    for v in (1, 3):
        alone = _run_device(net, [feats[0], feats[v]])                     # NS = 1
        for stage in U.STAGES:
            assert torch.equal(alone[stage][0], full[stage][0]) and torch.equal(alone[stage][1], full[stage][v]), (stage, v)


def test_two_runs_give_the_same_bits():
    net = _device_module("blocks")
    feats = U.case_features("blocks")
    a, b = _run_device(net, feats), _run_device(net, feats)
    assert all(torch.equal(x, y) for stage in U.STAGES for x, y in zip(a[stage], b[stage]))
    big = U.case_features("dtu_tokens")
    c, d = _run_device(net, big, False), _run_device(net, big, False)
    assert all(torch.equal(x, y) for x, y in zip(c["stage1"], d["stage1"]))


def test_outputs_are_channels_last_views_and_inputs_stay():
    net = _device_module("tiny")
    feats = MU.cast(U.case_features("tiny"), torch.float32, DEV)
    keep = [{k: v.clone() for k, v in f.items()} for f in feats]
    work = [dict(f) for f in feats]
    with torch.no_grad():
        out = net(work)
    assert out is work
    for f, k0, o in zip(feats, keep, out):
        for stage in U.STAGES:
            assert torch.equal(f[stage], k0[stage])                        # the caller's tensors are not written
            assert o[stage].shape == f[stage].shape and o[stage].permute(0, 2, 3, 1).is_contiguous()


def test_closed_gate_takes_the_torch_route_on_the_device(monkeypatch):
    fx = U.fixture()
    net = _device_module("tiny")
    feats = MU.cast(U.case_features("tiny"), torch.float32, DEV)

    def no_kernels():
        raise AssertionError("the kernel route was taken")
    monkeypatch.setattr(mvs, "_ops", no_kernels)
    assert not net.uses_kernels(feats)                                     # gradients are enabled here
    got = net([dict(f) for f in feats])
    with torch.no_grad():
        odd = [dict(f) for f in feats]
        for f in odd:
            f["stage2"], f["stage3"] = torch.zeros(1, 16, 15, 21, device=DEV), torch.zeros(1, 8, 30, 42, device=DEV)
        assert not net.uses_kernels(odd) and net(odd)[1]["stage3"].shape == (1, 8, 30, 42)        # a 3 x stage 2: torch resizes it
        with pytest.raises(AssertionError):
            net.eval()([dict(f) for f in feats])                           # the open gate would have reached the kernels
    want = U.expected64("tiny")
    for stage in U.STAGES:
        e, bar = _err(torch.stack([f[stage] for f in got], 0), U.stacked(want[stage])), U.BAR_FACTOR * float(fx[f"tiny_err_{stage}"])
        assert got[0][stage].requires_grad and e <= bar, (stage, e, bar)


def _clean_footprint(agree, size):
    """(B,h,w) bool -> (B,H,W) bool: the pixels of the next stage whose bilinear footprint in the previous stage agrees everywhere."""
    up = torch.nn.functional.interpolate(agree.float().unsqueeze(1), size, mode="bilinear", align_corners=False).squeeze(1)
    return up == 1.0


def test_coarse_to_fine_behind_the_device_module():
    """The three-stage run with its features from the device module, and from the torch route on the device, against the float64 run:
    the prob volumes within the stored bars, and the same winners wherever the top-2 gap rule keeps the pixel.  A later stage is compared
    where the stages before it picked float64's plane throughout the pixel's footprint, as tests/test_mvs_gpu.py does."""
    fx, s = U.fixture(), MU.STAGES
    want = U.stage_run_expected(torch.float64)
    runs = {"kernels": U.stage_run(torch.float32, DEV, True), "torch": U.stage_run(torch.float32, DEV, False)}
    for route, got in runs.items():
        clean = torch.ones(want["stage1"]["depth"].shape, dtype=torch.bool)
        for i, stage in enumerate(U.STAGES):
            err = float(fx[f"run_err_{stage}"])
            diff = (got[stage]["prob_volume"].cpu().double() - want[stage]["prob_volume"]).abs()
            e, bar = float(diff[clean.unsqueeze(1).expand_as(diff)].max()), U.BAR_FACTOR * err
            keep, excluded = MU.excluded_share(want[stage]["prob_volume"], err)
            agree = got[stage]["prob_volume"].cpu().argmax(1) == want[stage]["prob_volume"].argmax(1)
            print(f"{route} {stage}: prob {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}) on {100 * float(clean.double().mean()):.1f} % of the pixels, "
                  f"excluded {100 * excluded:.2f} %, winners that differ {int((~agree & clean).sum())}")
            assert e <= bar and bool(agree[keep & clean].all()), (route, stage)
            same = (got[stage]["depth"].cpu().double() - want[stage]["depth"]).abs()[agree & clean]
            # the same plane is the same hypothesis: depths near 1.5 (float32 spacing 1.2e-7) through the dozen float32 operations of the
            # hypothesis chain stay well within 4e-6 of float64's
            assert float(same.max()) <= 4e-6, (route, stage)
            if i + 1 < len(U.STAGES):
                nxt = s["scales"][i + 1]
                full = _clean_footprint(agree & clean, s["image"])
                clean = torch.nn.functional.avg_pool2d(full.float().unsqueeze(1), nxt).squeeze(1) == 1.0 if nxt > 1 else full
    assert runs["kernels"]["depth"].is_cuda and runs["kernels"]["stage3"]["depth"].shape == (2, 24, 40)
