"""The kernels of csrc/costreg.hip on the device against float64 on the host and fixture G29's yardsticks (tests/golden/g29_costreg.npz).

Single layers are held against float64 F.conv3d / F.conv_transpose3d on the host; the bar is costreg_util.BAR_FACTOR (4) times the
distance torch's own float32 CPU result keeps from float64 on that layer (one weight set and one set of options; the maximum over the
three volumes, computed here: the 1 x 1 x 1 volume has one or two outputs a channel, whose float32 error can be exactly zero): the
kernels are one fmaf chain per output in an order of their own.  The whole net is held against the float64 torch route (which tests/test_costreg_cpu.py holds against the fixture) with 4 x the case's recorded reference distance.  With
the regulariser inside DeviceDepthNet the argmax must equal float64's wherever the float64 top-2 gap exceeds GAP_FACTOR (3) x the
reference float32's prob error; the excluded share is printed and must stay under EXCLUDED_CAP (2 %).

Measured on an MI355X (max |kernel - float64| / bar): see DESIGN.md section 8n."""
import pytest
import torch
import torch.nn.functional as F

from diner_amd import mvs, ops
from tests import costreg_util as U
from tests import mvs_util as MU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3).contiguous()


def _layer_host(kind, x, w, b, relu, addend):
    """The layer in x's dtype with torch's operations: convolution [+ bias], ReLU, + addend."""
    if kind == "deconv":
        y = F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)
    else:
        y = F.conv3d(x, w, b, stride=1 if kind == "conv1" else 2, padding=1)
    if relu:
        y = F.relu(y)
    return y if addend is None else y + addend


def _layer_device(kind, x, w, b, relu, addend, out=None):
    xd = _ndhwc(x).to(DEV)
    bd = None if b is None else b.to(DEV)
    ad = None if addend is None else _ndhwc(addend).to(DEV)
    Cout = w.shape[1] if kind == "deconv" else w.shape[0]
    if kind == "deconv":
        return ops.deconv3d_s2(xd, ops.pack_deconv3d(w).to(DEV), bd, Cout, relu=relu, addend=ad, out=out)
    return ops.conv3d(xd, ops.pack_conv3d(w).to(DEV), bd, Cout, stride=1 if kind == "conv1" else 2, relu=relu, addend=ad, out=out)


def _out_shape(kind, vol):
    return tuple(2 * n for n in vol) if kind == "deconv" else tuple(n if kind == "conv1" else (n - 1) // 2 + 1 for n in vol)


@pytest.mark.parametrize("Cin", U.LAYER_CIN)
@pytest.mark.parametrize("kind", U.LAYER_KINDS)
def test_single_layers_against_float64(kind, Cin):
    worst = 0.0
    for Cout in U.LAYER_COUT:
        g = torch.Generator().manual_seed(1000 * Cin + Cout)
        w = torch.randn((Cin, Cout, 3, 3, 3) if kind == "deconv" else (Cout, Cin, 3, 3, 3), generator=g) * (2.0 / (27 * Cin)) ** 0.5
        bias = 0.3 * torch.randn(Cout, generator=g)
        worst = max(worst, _check_layer(kind, w, bias, g))
    print(f"{kind} Cin {Cin}: largest kernel error / bar = {worst:.3f}")


# plain; bias, ReLU and addend each alone (an addend without the ReLU before it, a bias without either); all three
OPTION_SETS = ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True))


def _check_layer(kind, w, bias, g, volumes=U.LAYER_VOLUMES):
    """One weight set on every volume under every option set against float64 -> the largest error / bar."""
    Cin, Cout = (w.shape[0], w.shape[1]) if kind == "deconv" else (w.shape[1], w.shape[0])
    worst = 0.0
    for with_bias, relu, with_addend in OPTION_SETS:
        runs, e32 = [], 0.0
        for vol in volumes:
            x = torch.randn((2, Cin) + vol, generator=g)
            addend = torch.randn((2, Cout) + _out_shape(kind, vol), generator=g) if with_addend else None
            b = bias if with_bias else None
            y64 = _layer_host(kind, x.double(), w.double(), None if b is None else b.double(), relu, None if addend is None else addend.double())
            e32 = max(e32, _err(_layer_host(kind, x, w, b, relu, addend), y64))
            got = _ncdhw(_layer_device(kind, x, w, b, relu, addend))
            assert got.shape == y64.shape and got.dtype == torch.float32
            runs.append((vol, _err(got, y64)))
        bar = U.BAR_FACTOR * e32
        for vol, e in runs:
            worst = max(worst, e / bar)
            assert e <= bar, (kind, Cin, Cout, vol, (with_bias, relu, with_addend), e, bar)
    return worst


@pytest.mark.parametrize("Cout", [5, 12, 16])
def test_one_input_channel_at_other_widths(Cout):
    """Cin 1 at stride 1 runs k_conv3d_cin1<4 | 8 | 16>: Cout 5 takes <8>'s scalar epilogue, 12 <16>'s, 16 <16>'s vector epilogue."""
    g = torch.Generator().manual_seed(300 + Cout)
    w = torch.randn(Cout, 1, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    worst = _check_layer("conv1", w, 0.3 * torch.randn(Cout, generator=g), g)
    print(f"conv1 Cin 1 Cout {Cout}: largest kernel error / bar = {worst:.3f}")


# name: kind, Cin, input volume -- per kind one volume of exactly 1024 tiles and one of 512, both with tiles partly outside.  The launcher
# keeps NT as wide as CoutPad allows while tiles x column groups >= 1024, so (tiles, Cout) -> (NT, groups): (1024, 128) -> (4, 2),
# (1024, 64) -> (4, 1), (1024, 32) -> (2, 1), (512, 128) -> (4, 2), (512, 64) -> (2, 2), (512, 32) -> (1, 2), and Cout 16 -> (1, 1) always.
WIDE = {
    "conv1 1024 tiles": ("conv1", 8, (31, 62, 63)),         # ceil(31 / 2) ceil(62 / 4) ceil(63 / 16) = 16 x 16 x 4
    "conv1 512 tiles": ("conv1", 12, (15, 62, 63)),         # Cin 12: the scalar staging path, two chunks
    "conv2 1024 tiles": ("conv2", 8, (31, 125, 127)),       # output 16 x 63 x 64: 8 x 32 x 4 tiles of 2 x 2 x 16
    "conv2 512 tiles": ("conv2", 12, (15, 125, 127)),
    "deconv 1024 tiles": ("deconv", 8, (16, 31, 31)),       # 8 x 8 x 2 tiles of the input grid x 8 parity classes
    "deconv 512 tiles": ("deconv", 12, (8, 31, 31)),
}


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_column_tiles(name):
    """NT 2 and NT 4, one and two column groups: against float64, and bit-equal to the same layer computed sixteen output channels at a
    time (CoutPad 16: NT 1) -- an output's chain does not depend on how many column tiles its workgroup runs."""
    kind, Cin, vol = WIDE[name]
    g = torch.Generator().manual_seed(sum(vol) + Cin)
    Cmax = 128
    w = torch.randn((Cin, Cmax, 3, 3, 3) if kind == "deconv" else (Cmax, Cin, 3, 3, 3), generator=g) * (2.0 / (27 * Cin)) ** 0.5
    bias, x = 0.3 * torch.randn(Cmax, generator=g), torch.randn((1, Cin) + vol, generator=g)
    addend = torch.randn((1, Cmax) + _out_shape(kind, vol), generator=g)
    cut = (lambda n0, n1: w[:, n0:n1]) if kind == "deconv" else (lambda n0, n1: w[n0:n1])
    run = lambda n0, n1: _layer_device(kind, x, cut(n0, n1).contiguous(), bias[n0:n1].contiguous(), True, addend[:, n0:n1])
    narrow = torch.cat([run(n, n + 16) for n in range(0, Cmax, 16)], dim=4)          # NT 1, one group each
    y64 = _layer_host(kind, x.double(), w.double(), bias.double(), True, addend.double())
    bar = U.BAR_FACTOR * _err(_layer_host(kind, x, w, bias, True, addend), y64)
    e = _err(_ncdhw(narrow), y64)
    print(f"{name}: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert e <= bar
    for Cout in (32, 64, 128):
        assert torch.equal(run(0, Cout), narrow[..., :Cout]), (name, Cout)


@pytest.mark.parametrize("name", list(U.CASES))
def test_whole_net_against_float64(name):
    fx, x, r64 = U.fixture(), U.case_input(name), U.expected64(name)
    net = mvs.DeviceCostRegNet.from_module(U.make_net(name).to(DEV))
    with torch.no_grad():
        assert net.uses_kernels(x.to(DEV))
        got = net(x.to(DEV))
        on_device = net.forward_torch(x.to(DEV))                        # the reference's operations in float32 on the device
    e, bar, e_dev = _err(got, r64), U.BAR_FACTOR * float(fx[f"{name}_err_cost"]), _err(on_device, r64)
    print(f"{name} cost: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f}); torch on the device {e_dev:.2e}")
    assert got.shape == r64.shape and got.dtype == torch.float32 and got.is_cuda
    assert e <= bar, (name, e, bar)
    ep, barp = _err(U.softmax_d(got), U.softmax_d(r64)), U.BAR_FACTOR * float(fx[f"{name}_err_prob"])
    print(f"{name} prob: kernel {ep:.2e}, bar {barp:.2e} (x{ep / barp:.2f})")
    assert ep <= barp, (name, ep, barp)
    keep, excluded = MU.excluded_share(U.softmax_d(r64), float(fx[f"{name}_err_prob"]))
    print(f"{name}: excluded share {100 * excluded:.2f} % (cap {100 * U.EXCLUDED_CAP:.0f} %)")
    assert excluded <= U.EXCLUDED_CAP
    assert bool((U.softmax_d(got).cpu().argmax(1) == U.softmax_d(r64).argmax(1))[keep].all())


def test_depthnet_with_the_real_regulariser(monkeypatch):
    fx, inp = U.fixture(), U.depthnet_inputs()
    want, _ = U.depthnet_expected(torch.float64)
    launches = []
    for entry in ("conv3d", "deconv3d_s2"):
        monkeypatch.setattr(ops, entry, lambda *a, _f=getattr(ops, entry), **k: (launches.append(1), _f(*a, **k))[1])

    def torch_route(self, x):
        raise AssertionError("the regulariser took the torch route")
    monkeypatch.setattr(mvs.DeviceCostRegNet, "forward_torch", torch_route)
    got, weights = U.run_depthnet(inp, torch.float32, DEV)
    assert len(launches) == 11                                          # the regulariser ran on the kernels, eleven launches
    err_prob = float(fx["depthnet_err_prob"])
    e, bar = _err(got["prob_volume"], want["prob_volume"]), U.BAR_FACTOR * err_prob
    print(f"depthnet prob: kernel {e:.2e}, bar {bar:.2e} (x{e / bar:.2f})")
    assert got["prob_volume"].is_cuda and e <= bar
    keep, excluded = MU.excluded_share(want["prob_volume"], err_prob)
    print(f"depthnet: excluded share {100 * excluded:.2f} % (cap {100 * U.EXCLUDED_CAP:.0f} %)")
    assert excluded <= U.EXCLUDED_CAP
    agree = got["prob_volume"].cpu().argmax(1) == want["prob_volume"].argmax(1)
    assert bool(agree[keep].all()), f"{int((~agree & keep).sum())} pixels with a clear float64 winner got another plane"
    assert bool((got["depth"].cpu() == want["depth"].float())[keep].all())


def test_bits_do_not_depend_on_batch_position_or_run():
    name = "batch"
    x = U.case_input(name).to(DEV)
    net = mvs.DeviceCostRegNet.from_module(U.make_net(name).to(DEV))
    with torch.no_grad():
        both = net(x).clone()
        again = net(x).clone()
        alone = net(x[1:2].contiguous()).clone()
        flipped = net(x.flip(0).contiguous()).clone()
    assert torch.equal(both, again)
    assert torch.equal(alone, both[1:2])
    assert torch.equal(flipped, both.flip(0))


@pytest.mark.parametrize("kind", U.LAYER_KINDS)
def test_out_may_alias_the_addend(kind):
    g = torch.Generator().manual_seed(7)
    Cin, Cout, vol = 12, 20, (3, 5, 18)
    w = torch.randn((Cin, Cout, 3, 3, 3) if kind == "deconv" else (Cout, Cin, 3, 3, 3), generator=g) * 0.1
    x, bias = torch.randn((2, Cin) + vol, generator=g), torch.randn(Cout, generator=g)
    addend = torch.randn((2, Cout) + _out_shape(kind, vol), generator=g)
    apart = _layer_device(kind, x, w, bias, True, addend)
    buf = _ndhwc(addend).to(DEV)
    Cw = ops.pack_deconv3d(w).to(DEV) if kind == "deconv" else ops.pack_conv3d(w).to(DEV)
    if kind == "deconv":
        same = ops.deconv3d_s2(_ndhwc(x).to(DEV), Cw, bias.to(DEV), Cout, relu=True, addend=buf, out=buf)
    else:
        same = ops.conv3d(_ndhwc(x).to(DEV), Cw, bias.to(DEV), Cout, stride=1 if kind == "conv1" else 2, relu=True, addend=buf, out=buf)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(same, apart)


def test_packed_weights_follow_the_parameters():
    name = "batch"                                                       # twelve voxels at the bottom level: batch statistics exist
    x = U.case_input(name).to(DEV)
    net = mvs.DeviceCostRegNet.from_module(U.make_net(name).to(DEV))
    with torch.no_grad():
        first = net(x).clone()
        packed = net.packed()
        assert net.packed() is packed                                    # nothing changed: nothing is packed again
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    net.train()
    net.forward_torch(x).square().mean().backward()                      # the torch route: differentiable, batch statistics
    opt.step()                                                           # bumps the parameters' versions
    net.eval()
    with torch.no_grad():
        assert net.packed() is not packed
        second = net(x).clone()
        want = net.forward_torch(x)
        assert not torch.equal(first, second) and _err(second, want) <= 1e-4
        packed = net.packed()
        net.prob.weight.data.mul_(2.0)                                   # a .data write bumps no version
        net.invalidate()
        assert net.packed() is not packed
        assert _err(net(x), 2.0 * second) <= 1e-5
