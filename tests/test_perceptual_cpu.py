"""CPU: the perceptual network (perceptual.hip, diner_amd.perceptual) -- the entries are declared, exported and bound and refuse bad
arguments before any device work; the Python layers check their arguments without a device; the loader packs the same tensors from the
three forms the weights come in; and fixture G26 (tools/make_golden_perceptual.py) is what its generator says it is: the float64
restatement of the VGG loss agrees with src.losses.VGGLoss, and the seeded weights still have the recorded checksum.

Every test here but the last two fails without the feature (no diner_amd.perceptual, no symbols); the last two exercise the generator's
restatement and the fixture."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests.helpers import ROOT, load

ENTRIES = ("diner_conv3x3_pack_floats", "diner_conv3x3_f32", "diner_maxpool2_f32", "diner_maxpool2_bwd_f32", "diner_image_in_f32",
           "diner_image_in_bwd_f32", "diner_feature_l1_workspace_bytes", "diner_feature_l1_f32", "diner_lpips_layer_workspace_bytes",
           "diner_lpips_layer_f32")


from diner_amd.evaluate import evaluate_folder as evaluate_folder_real          # noqa: E402  (before any test patches it)


def generator():
    """tools/make_golden_perceptual.py as a module (tools/ is not a package)."""
    spec = importlib.util.spec_from_file_location("make_golden_perceptual", os.path.join(ROOT, "tools", "make_golden_perceptual.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entries_declared_exported_and_bound():
    from diner_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "perceptual.hip" in build.SOURCES
    assert lib.diner_conv3x3_pack_floats(3, 8) == 1 * 9 * 8 * 64 and lib.diner_conv3x3_pack_floats(64, 65) == 8 * 9 * 8 * 128
    assert lib.diner_conv3x3_pack_floats(0, 8) == 0 and lib.diner_conv3x3_pack_floats(8, 0) == 0
    assert lib.diner_feature_l1_workspace_bytes(0) == 0 and lib.diner_feature_l1_workspace_bytes(10 ** 9) == 1024 * 8
    assert lib.diner_lpips_layer_workspace_bytes(0, 5) == 0 and lib.diner_lpips_layer_workspace_bytes(3, 1) == 3 * 8


def test_entries_refuse_bad_arguments_without_gpu():
    import ctypes as C
    from diner_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)          # never dereferenced: every call below is refused before any device work
    f3 = (C.c_float * 3)(1.0, 1.0, 1.0)
    z3 = (C.c_float * 3)(1.0, 0.0, 1.0)

    def refused(rc, word):
        assert rc == _lib.E_INVALID and word in lib.diner_last_error(), (rc, lib.diner_last_error())

    refused(lib.diner_conv3x3_f32(p, p, None, None, None, p, 0, 4, 4, 3, 8, 0, None), b"N, H, W, C")
    refused(lib.diner_conv3x3_f32(p, p, None, None, None, p, 1, 4, 4, 0, 8, 0, None), b"N, H, W, C")
    refused(lib.diner_conv3x3_f32(p, p, None, None, None, p, 1, 4, 4, 3, -1, 0, None), b"N, H, W, C")
    refused(lib.diner_conv3x3_f32(p, p, None, None, None, p, 70000, 4, 4, 3, 8, 0, None), b"65535")
    refused(lib.diner_conv3x3_f32(None, p, None, None, None, p, 1, 4, 4, 3, 8, 0, None), b"null")
    refused(lib.diner_conv3x3_f32(p, None, None, None, None, p, 1, 4, 4, 3, 8, 0, None), b"null")
    refused(lib.diner_conv3x3_f32(p, C.c_void_p(p.value + 4), None, None, None, p, 1, 4, 4, 3, 8, 0, None), b"aligned")
    refused(lib.diner_maxpool2_f32(p, p, 1, 1, 4, 8, None), b"H, W")
    refused(lib.diner_maxpool2_f32(p, None, 1, 4, 4, 8, None), b"null")
    refused(lib.diner_maxpool2_bwd_f32(p, p, None, 0, p, 1, 4, 1, 8, None), b"H, W")
    refused(lib.diner_maxpool2_bwd_f32(p, None, None, 0, p, 1, 4, 4, 8, None), b"null")
    refused(lib.diner_image_in_f32(p, f3, f3, p, 1, 4, 4, 5, None), b"Cs")
    refused(lib.diner_image_in_f32(p, f3, z3, p, 1, 4, 4, 4, None), b"scale")
    refused(lib.diner_image_in_f32(p, None, f3, p, 1, 4, 4, 4, None), b"null")
    refused(lib.diner_image_in_bwd_f32(p, z3, p, 1, 4, 4, 3, None), b"scale")
    refused(lib.diner_image_in_bwd_f32(p, f3, p, 1, 4, 4, 2, None), b"Cs")
    refused(lib.diner_feature_l1_f32(p, p, 0, 1.0, 0, None, p, p, None), b"n =")
    refused(lib.diner_feature_l1_f32(p, p, 10, float("nan"), 0, None, p, p, None), b"weight")
    refused(lib.diner_feature_l1_f32(p, None, 10, 1.0, 0, None, p, p, None), b"null")
    refused(lib.diner_lpips_layer_f32(p, p, p, 0, 10, 8, 0, p, p, None), b"N =")
    refused(lib.diner_lpips_layer_f32(p, p, p, 1, 0, 8, 0, p, p, None), b"HW")
    refused(lib.diner_lpips_layer_f32(p, p, None, 1, 10, 8, 0, p, p, None), b"null")


def test_ops_check_their_arguments_without_a_device():
    from diner_amd import ops
    x = torch.zeros(2, 5, 7, 3)
    wp = ops.pack_conv3x3(torch.zeros(8, 3, 3, 3))
    b = torch.zeros(64)
    assert tuple(wp.shape) == (1, 9, 8, 64)
    assert ops._check_conv3x3_args(x, wp, b, 8, None, None) == (2, 5, 7, 3)
    assert ops._check_conv3x3_args(torch.zeros(2, 5, 7, 4), wp, b, 8, None, None) == (2, 5, 7, 4)          # the padded first layer
    for bad in (dict(x=x.double()), dict(x=x[0]), dict(x=x.permute(0, 3, 1, 2)), dict(x=x[:, :, ::2]), dict(x="x"),
                dict(wp=wp[:, :, :4]), dict(wp=wp.double()), dict(wp=ops.pack_conv3x3(torch.zeros(8, 9, 3, 3))), dict(Cout=65), dict(Cout=0),
                dict(b=torch.zeros(8)), dict(addend=torch.zeros(2, 5, 7, 9)), dict(mask=torch.zeros(2, 5, 8, 8)),
                dict(mask=torch.zeros(2, 5, 7, 8, dtype=torch.bool))):
        a = dict(x=x, wp=wp, b=b, Cout=8, addend=None, mask=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ops._check_conv3x3_args(a["x"], a["wp"], a["b"], a["Cout"], a["addend"], a["mask"])
    for w in (torch.zeros(8, 3, 3), torch.zeros(8, 3, 5, 5), torch.zeros(8, 3, 3, 3, dtype=torch.float64), torch.zeros(0, 3, 3, 3)):
        with pytest.raises(ValueError):
            ops.pack_conv3x3(w)
    with pytest.raises(ValueError):
        ops._check_nhwc("maxpool2", "x", torch.zeros(1, 1, 4, 8), min_hw=2)
    with pytest.raises(ValueError):
        ops.maxpool2_bwd(torch.zeros(1, 5, 7, 8), torch.zeros(1, 3, 3, 8))               # gy must be (1, 2, 3, 8)
    for bad in (dict(x=torch.zeros(1, 4, 5, 5)), dict(x=torch.zeros(3, 5, 5)), dict(x=torch.zeros(1, 3, 5, 5).double()),
                dict(scale=(1.0, 0.0, 1.0)), dict(shift=(0.0, 1.0)), dict(scale=(1.0, float("nan"), 1.0))):
        a = dict(x=torch.zeros(1, 3, 5, 5), shift=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0))
        a.update(bad)
        with pytest.raises(ValueError):
            ops._check_image_in_args(a["x"], a["shift"], a["scale"])
    with pytest.raises(ValueError):
        ops.image_in_bwd(torch.zeros(1, 5, 5, 2), (1.0, 1.0, 1.0))
    for fx, fy, w in ((torch.zeros(4), torch.zeros(5), 1.0), (torch.zeros(4).double(), torch.zeros(4).double(), 1.0),
                      (torch.zeros(4), torch.zeros(4), float("inf")), (torch.zeros(0), torch.zeros(0), 1.0)):
        with pytest.raises(ValueError):
            ops._check_feature_l1_args(fx, fy, w)
    f = torch.zeros(2, 4, 4, 8)
    assert ops._check_lpips_layer_args(f, f, torch.zeros(8), None) == (2, 16, 8)
    for fy, lin, out in ((torch.zeros(2, 4, 4, 9), torch.zeros(8), None), (f, torch.zeros(9), None), (f, torch.zeros(8).double(), None),
                         (f, torch.zeros(8), torch.zeros(2)), (f, torch.zeros(8), torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops._check_lpips_layer_args(f, fy, lin, out)
    # valid arguments on the CPU: refused, never computed some other way
    for call in (lambda: ops.conv3x3(x, wp, b, 8), lambda: ops.maxpool2(f), lambda: ops.maxpool2_bwd(f, torch.zeros(2, 2, 2, 8)),
                 lambda: ops.image_in(torch.zeros(1, 3, 5, 5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), lambda: ops.image_in_bwd(torch.zeros(1, 5, 5, 3), (1.0, 1.0, 1.0)),
                 lambda: ops.feature_l1(f, f), lambda: ops.lpips_layer(f, f, torch.zeros(8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_pack_conv3x3_layout():
    from diner_amd import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn(5, 11, 3, 3, generator=g)
    p = ops.pack_conv3x3(w)
    t = ops.pack_conv3x3(w, transpose=True)
    assert tuple(p.shape) == (2, 9, 8, 64) and tuple(t.shape) == (1, 9, 8, 64)
    for co, ci, ky, kx in ((0, 0, 0, 0), (4, 10, 2, 1), (3, 7, 1, 2), (2, 8, 0, 2)):
        assert p[ci // 8, ky * 3 + kx, ci % 8, co] == w[co, ci, ky, kx]
        assert t[co // 8, (2 - ky) * 3 + (2 - kx), co % 8, ci] == w[co, ci, ky, kx]          # taps flipped, Cin and Cout swapped
    assert float(p.abs().sum()) == float(w.abs().sum()) and float(t.abs().sum()) == float(w.abs().sum())      # the rest is zero
    assert p[1, :, 3:, :].abs().max() == 0 and p[:, :, :, 5:].abs().max() == 0


def test_perceptual_checks_without_a_device():
    from diner_amd import perceptual as P
    from diner_amd.synthetic import make_vgg_state_dict
    x = torch.zeros(2, 3, 16, 16)
    for who, lo in (("Lpips", 16), ("VggLoss", 8)):
        for a, b in ((x.double(), x.double()), (x[0], x[0]), (x[:, :2], x[:, :2]), (x, x[:1]), (x[:, :, :lo - 1], x[:, :, :lo - 1]),
                     (x[..., :lo - 1], x[..., :lo - 1]), (x, "y")):
            with pytest.raises(ValueError):
                P._check_pair(who, a, b, lo)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P._check_pair(who, x, x, lo)
    sd = make_vgg_state_dict("vgg16", 1, width_div=16, with_lins=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.VggFeatures(sd, "vgg16", device="cpu")
    with pytest.raises(ValueError, match="arch"):
        P.load_layers(sd, "vgg11")
    # a missing convolution, as a mapping and as a stack
    with pytest.raises(ValueError, match="14"):
        P.load_layers({k: v for k, v in sd.items() if not k.startswith("features.14.")}, "vgg16")
    with pytest.raises(ValueError, match="bias"):
        P.load_layers({k: v for k, v in sd.items() if k != "features.5.bias"}, "vgg16")
    G = generator()
    sd19 = make_vgg_state_dict("vgg19", 2, width_div=16)
    seq = G.sequential_from(sd19, "vgg19")
    with pytest.raises(ValueError, match="index 12"):
        P.load_layers(torch.nn.Sequential(*list(seq)[:12]), "vgg19")
    mods = list(seq)
    mods[7] = torch.nn.ReLU()
    with pytest.raises(ValueError, match="index 7"):
        P.load_layers(torch.nn.Sequential(*mods), "vgg19")
    mods = list(seq)
    mods[9] = torch.nn.AvgPool2d(2, 2)
    with pytest.raises(ValueError, match="MaxPool2d"):
        P.load_layers(torch.nn.Sequential(*mods), "vgg19")
    mods = list(seq)
    mods[5] = torch.nn.Conv2d(mods[5].in_channels, mods[5].out_channels, 3, padding=1, stride=2)
    with pytest.raises(ValueError, match="index 5"):
        P.load_layers(torch.nn.Sequential(*mods), "vgg19")
    bad = dict(sd19)
    bad["features.10.weight"] = torch.zeros(16, 9, 3, 3)          # does not continue the width of the convolution below
    with pytest.raises(ValueError, match="index 10"):
        P.load_layers(bad, "vgg19")
    with pytest.raises(ValueError):
        P.load_layers([1, 2, 3], "vgg19")
    # lin tensors
    layers = P.load_layers(sd, "vgg16")
    assert [tuple(t.shape) for t in P.load_lins(sd, layers)] == [(4,), (8,), (16,), (32,), (32,)]
    bad = dict(sd)
    bad["lin2.model.1.weight"] = torch.zeros(1, 17, 1, 1)
    with pytest.raises(ValueError, match="lin2"):
        P.load_lins(bad, layers)
    with pytest.raises(ValueError, match="lin4"):
        P.load_lins({k: v for k, v in sd.items() if not k.startswith("lin4.")}, layers)
    with pytest.raises(ValueError):
        P.load_lins(G.sequential_from(sd, "vgg16"), layers)


def test_loader_packs_the_same_tensors_from_three_forms():
    from diner_amd import perceptual as P
    from diner_amd.synthetic import make_vgg_state_dict
    G = generator()
    for arch in ("vgg16", "vgg19"):
        sd = make_vgg_state_dict(arch, 5, width_div=8, with_lins=arch == "vgg16")
        a = P.load_layers(G.sequential_from(sd, arch), arch)
        b = P.load_layers(sd, arch)
        # the lpips package's naming: net.slice<K>.<N>.*, beside its lin and scaling-layer entries
        bounds = (4, 9, 16, 23, 30)
        sliced = {(f"net.slice{1 + sum(int(k.split('.')[1]) >= e for e in bounds)}." + k.split(".", 1)[1]) if k.startswith("features.") else k: v
                  for k, v in sd.items()}
        sliced.update({"scaling_layer.shift": torch.zeros(1, 3, 1, 1), "scaling_layer.scale": torch.ones(1, 3, 1, 1)})
        if arch == "vgg16":
            sliced.update({f"lins.{k}.model.1.weight": sd[f"lin{k}.model.1.weight"] for k in range(5)})
        assert any(k.startswith("net.slice3.") for k in sliced) and not any(k.startswith("features.") for k in sliced)
        c = P.load_layers(sliced, arch)
        assert len(a) == len(b) == len(c) == len(P.ARCHS[arch]["convs"])
        for la, lb, lc in zip(a, b, c):
            assert la[:3] == lb[:3] == lc[:3] and la[6:] == lb[6:] == lc[6:]
            for f in ("w_fwd", "bias", "w_bwd"):
                ta, tb, tc = getattr(la, f), getattr(lb, f), getattr(lc, f)
                assert ta.dtype == torch.float32 and ta.device.type == "cpu" and torch.equal(ta, tb) and torch.equal(ta, tc), (arch, la.index, f)
        assert [L.index for L in a] == list(P.ARCHS[arch]["convs"]) and a[0].Cin == 3
        assert [L.index for L in a if L.tap] == list(P.ARCHS[arch]["taps"])
        assert [L.index for L in a if L.pool_before] == [min(i for i in P.ARCHS[arch]["convs"] if i > p) for p in P.ARCHS[arch]["pools"]]
        w = sd[f"features.{a[1].index}.weight"]
        assert torch.equal(a[1].w_fwd[0, 4, 3, :w.shape[0]], w[:, 3, 1, 1]) and torch.equal(a[1].bias[:w.shape[0]], sd[f"features.{a[1].index}.bias"])


def test_cli_and_drop_in_pass_the_weights_file_on(monkeypatch, tmp_path):
    import inspect
    from diner_amd import evaluate
    from src.evaluation import eval_suite as E
    assert inspect.signature(evaluate.evaluate_folder).parameters["lpips_weights"].default is None
    calls = []
    monkeypatch.setattr(evaluate, "evaluate_folder", lambda *a, **k: calls.append((a, k)) or {"psnr": 1.0})
    evaluate.main(["--eval_path", str(tmp_path), "--lpips_weights", str(tmp_path / "w.pth")])
    assert calls == [((tmp_path / "visualizations", tmp_path), dict(show_tqdm=True, lpips_weights=tmp_path / "w.pth"))]
    assert evaluate._parser().parse_args(["--eval_path", "x"]).lpips_weights is None
    calls.clear()
    assert E.LPIPS_WEIGHTS is None
    monkeypatch.setattr(E, "LPIPS_WEIGHTS", "w.pth")
    E.evaluate_folder("a", "b")
    assert calls[0][0] == ("a", "b") and calls[0][1]["lpips_weights"] == "w.pth"
    with pytest.raises(ValueError, match="not both"):
        evaluate_folder_real("a", "b", lpips_fn=lambda p, g: 0.0, lpips_weights="w.pth")


def test_g26_restated_vgg_loss_is_the_drop_in_in_float64():
    from src.losses import VGGLoss
    G = generator()
    g = load("g26_perceptual.npz")
    for c, (arch, div, N, H, W, seed) in enumerate(G.LOSS_CASES):
        if div == 1:
            continue
        sd = G.state_dict(arch, div)
        x, y = G.loss_inputs(N, H, W, seed)
        assert np.array_equal(x.numpy(), g[f"loss{c}_x"]) and np.array_equal(y.numpy(), g[f"loss{c}_y"])
        l64, g64 = G.vgg_loss_restated(sd, x, y)
        ref = VGGLoss(features=G.sequential_from(sd, arch).double())
        xr = x.double().requires_grad_(True)
        lr = ref(xr, y.double())
        lr.backward()
        assert abs(float(l64) - float(lr.detach())) <= 1e-12 * abs(float(lr.detach()))
        assert float((g64 - xr.grad).norm()) <= 1e-12 * float(xr.grad.norm())
        assert abs(float(l64) - float(g[f"loss{c}_loss64"])) <= 1e-12 * abs(float(l64))
        assert float((g64 - torch.from_numpy(g[f"loss{c}_grad64"])).norm()) <= 1e-12 * float(g64.norm())
    for c, (arch, div, N, H, W, seed) in enumerate(G.LPIPS_CASES):
        if div == 1:
            continue
        pred, gt = G.lpips_inputs(N, H, W, seed)
        assert np.array_equal(pred.numpy(), g[f"lpips{c}_pred"]) and np.array_equal(gt.numpy(), g[f"lpips{c}_gt"])
        s = G.lpips_restated(G.state_dict(arch, div), pred, gt)
        assert np.abs(s.numpy() - g[f"lpips{c}_score64"]).max() <= 1e-12 * np.abs(s.numpy()).max()
        assert float(G.lpips_restated(G.state_dict(arch, div), pred, pred).abs().max()) == 0.0          # identical images score 0


def test_g26_seeded_weights_keep_their_checksum():
    G = generator()
    g = load("g26_perceptual.npz")
    for arch in ("vgg16", "vgg19"):
        for div in (G.NARROW, 1):
            sd = G.state_dict(arch, div)
            got, want = G.weights_checksum(sd), g[f"checksum_{arch}_div{div}"]
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (arch, div, got, want)
            assert all(float(v.min()) >= 0 for k, v in sd.items() if k.startswith("lin"))
    full = G.state_dict("vgg16", 1)
    assert [full[f"features.{i}.weight"].shape[0] for i in (0, 5, 10, 17, 28)] == [64, 128, 256, 512, 512] and len(full) == 2 * 13 + 5
    assert G.state_dict("vgg19", 1)["features.19.weight"].shape == (512, 256, 3, 3)
