"""CPU: the image encoder's trunk on the device (encoder.hip, diner_amd.encoder) -- the entries are declared, exported and bound and
refuse bad arguments before any device work; the Python layers check their arguments without a device; BatchNorm folding is exact in
float64; and fixture G27 (tools/make_golden_encoder.py) is what its generator says it is: the float64 restatement of
SpatialEncoder.forward reproduces the recorded sub-sample, the seeded weights still have the recorded sha256 and, where the reference
tree is present, the reference's own forward agrees with the restatement.

Every test here imports diner_amd.encoder, the new symbols or the generator, so each fails without the feature."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ROOT, load

ENTRIES = ("diner_conv2d_s2_pack_floats", "diner_conv2d_s2_f32", "diner_maxpool3s2_f32", "diner_encoder_input_f32", "diner_pyramid_level_f32")


def generator():
    """tools/make_golden_encoder.py as a module (tools/ is not a package)."""
    spec = importlib.util.spec_from_file_location("make_golden_encoder", os.path.join(ROOT, "tools", "make_golden_encoder.py"))
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
    assert "encoder.hip" in build.SOURCES and "-Rpass-analysis=kernel-resource-usage" in build.EXTRA_FLAGS["encoder.hip"]
    # [ceil(Cin / 8)][R R][8][Cout rounded up to 64]
    assert lib.diner_conv2d_s2_pack_floats(21, 64, 7) == 3 * 49 * 8 * 64 and lib.diner_conv2d_s2_pack_floats(24, 64, 7) == 3 * 49 * 8 * 64
    assert lib.diner_conv2d_s2_pack_floats(64, 128, 1) == 8 * 1 * 8 * 128 and lib.diner_conv2d_s2_pack_floats(3, 65, 7) == 1 * 49 * 8 * 128
    assert lib.diner_conv2d_s2_pack_floats(64, 128, 3) == lib.diner_conv3x3_pack_floats(64, 128)          # the same layout for R = 3
    for bad in ((0, 8, 3), (8, 0, 3), (8, 8, 5), (8, 8, 0), (8, 8, 2)):
        assert lib.diner_conv2d_s2_pack_floats(*bad) == 0


def test_entries_refuse_bad_arguments_without_gpu():
    import ctypes as C
    from diner_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)          # never dereferenced: every call below is refused before any device work
    off = C.c_void_p(p.value + 4)

    def refused(rc, word, code=_lib.E_INVALID):
        assert rc == code and word in lib.diner_last_error(), (rc, lib.diner_last_error())

    conv = lib.diner_conv2d_s2_f32      # (x, wpack, bias, y, N, H, W, Cin, Cout, R, relu, ldy, coff, stream)
    refused(conv(p, p, None, p, 0, 4, 4, 3, 8, 3, 0, 8, 0, None), b"N, H, W, C")
    refused(conv(p, p, None, p, 1, 0, 4, 3, 8, 3, 0, 8, 0, None), b"N, H, W, C")
    refused(conv(p, p, None, p, 1, 4, 4, 0, 8, 3, 0, 8, 0, None), b"N, H, W, C")
    refused(conv(p, p, None, p, 1, 4, 4, 3, 0, 3, 0, 8, 0, None), b"N, H, W, C")
    for R in (0, 2, 5, 9, -1):
        refused(conv(p, p, None, p, 1, 4, 4, 3, 8, R, 0, 8, 0, None), b"R =", _lib.E_UNSUPPORTED)
    refused(conv(p, p, None, p, 70000, 4, 4, 3, 8, 3, 0, 8, 0, None), b"65535")
    refused(conv(p, p, None, p, 1, 4, 4, 3, 8, 3, 0, 8, 1, None), b"do not fit")          # channels 1 .. 8 of an 8-channel output
    refused(conv(p, p, None, p, 1, 4, 4, 3, 8, 3, 0, 512, -1, None), b"do not fit")
    refused(conv(p, p, None, p, 1, 4, 4, 3, 8, 3, 0, 0, 0, None), b"do not fit")
    refused(conv(None, p, None, p, 1, 4, 4, 3, 8, 3, 0, 8, 0, None), b"null")
    refused(conv(p, None, None, p, 1, 4, 4, 3, 8, 3, 0, 8, 0, None), b"null")
    refused(conv(p, p, None, None, 1, 4, 4, 3, 8, 3, 0, 8, 0, None), b"null")
    refused(conv(p, off, None, p, 1, 4, 4, 3, 8, 7, 0, 8, 0, None), b"aligned")
    pool = lib.diner_maxpool3s2_f32     # (x, y, N, H, W, C, ldx, stream)
    refused(pool(p, p, 1, 0, 4, 8, 8, None), b"N, H, W, C")
    refused(pool(p, p, 1, 4, 4, 8, 7, None), b"ldx")
    refused(pool(p, None, 1, 4, 4, 8, 8, None), b"null")
    inp = lib.diner_encoder_input_f32   # (x, ring, y, N, H, W, pad, Cring, C, stream)
    refused(inp(p, p, p, 1, 4, 4, -1, 18, 21, None), b"pad")
    refused(inp(p, p, p, 1, 4, 4, 2, 18, 20, None), b"ring channels")
    refused(inp(p, None, p, 1, 4, 4, 2, 0, 2, None), b"ring channels")
    refused(inp(p, p, p, 0, 4, 4, 2, 18, 21, None), b"N, H, W, C")
    refused(inp(p, p, p, 1, 0, 4, 2, 18, 21, None), b"N, H, W, C")
    refused(inp(p, None, p, 1, 4, 4, 2, 18, 24, None), b"null")
    refused(inp(None, None, p, 1, 4, 4, 0, 0, 3, None), b"null")
    lvl = lib.diner_pyramid_level_f32   # (x, y, N, h, w, c, Hf, Wf, Ctot, c0, stream)
    refused(lvl(p, p, 1, 0, 4, 8, 8, 8, 8, 0, None), b"N, H, W, C")
    refused(lvl(p, p, 1, 4, 4, 8, 0, 8, 8, 0, None), b"N, H, W, C")
    refused(lvl(p, p, 1, 4, 4, 8, 8, 8, 12, 5, None), b"do not fit")
    refused(lvl(p, p, 1, 4, 4, 8, 8, 8, 12, -1, None), b"do not fit")
    refused(lvl(None, p, 1, 4, 4, 8, 8, 8, 8, 0, None), b"null")
    refused(lvl(p, p, 70000, 4, 4, 8, 8, 8, 8, 0, None), b"65535")
    refused(lvl(p, p, 1, 4, 4, 8, 70000, 8, 8, 0, None), b"65535")


def test_ops_check_their_arguments_without_a_device():
    from diner_amd import ops
    g = torch.Generator().manual_seed(1)
    w = torch.randn(5, 11, 7, 7, generator=g)
    p = ops.pack_conv_s2(w)
    assert tuple(p.shape) == (2, 49, 8, 64)
    for co, ci, ky, kx in ((0, 0, 0, 0), (4, 10, 6, 1), (3, 7, 1, 5), (2, 8, 0, 2)):
        assert p[ci // 8, ky * 7 + kx, ci % 8, co] == w[co, ci, ky, kx]
    assert float(p.abs().sum()) == float(w.abs().sum()) and p[1, :, 3:, :].abs().max() == 0 and p[:, :, :, 5:].abs().max() == 0
    wide = ops.pack_conv_s2(torch.randn(64, 21, 7, 7, generator=g), Cin=24)
    assert tuple(wide.shape) == (3, 49, 8, 64) and wide[2, :, 5:, :].abs().max() == 0
    w3 = torch.randn(9, 12, 3, 3, generator=g)
    assert torch.equal(ops.pack_conv_s2(w3), ops.pack_conv3x3(w3))
    assert tuple(ops.pack_conv_s2(torch.zeros(128, 64, 1, 1)).shape) == (8, 1, 8, 128)
    for bad in (torch.zeros(8, 3, 5, 5), torch.zeros(8, 3, 3), torch.zeros(8, 3, 3, 7), torch.zeros(8, 3, 3, 3).double(), torch.zeros(0, 3, 3, 3)):
        with pytest.raises(ValueError):
            ops.pack_conv_s2(bad)
    with pytest.raises(ValueError):
        ops.pack_conv_s2(w, Cin=8)
    assert [ops.conv_s2_out_size(n, R) for n, R in ((45, 7), (58, 7), (12, 3), (15, 1), (1, 3), (2, 7), (928, 7))] == [23, 29, 6, 8, 1, 1, 464]
    x = torch.zeros(2, 45, 58, 11)
    b = torch.zeros(64)
    assert ops._check_conv_s2_args(x, p, b, 5, 7, None, 0) == (2, 45, 58, 11, 23, 29, 5)
    lat = torch.zeros(2, 23, 29, 512)
    assert ops._check_conv_s2_args(x, p, b[:5], 5, 7, lat, 64) == (2, 45, 58, 11, 23, 29, 512)
    with pytest.raises(NotImplementedError):
        ops._check_conv_s2_args(x, p, b, 5, 5, None, 0)
    for bad in (dict(x=x.double()), dict(x=x[0]), dict(x=x[:, :, ::2]), dict(p=p[:, :9]), dict(p=p.double()), dict(Cout=65), dict(Cout=0),
                dict(b=torch.zeros(4)), dict(b=b.double()), dict(out=torch.zeros(2, 23, 28, 512)), dict(out=lat, coff=508), dict(coff=1),
                dict(out=lat.double())):
        a = dict(x=x, p=p, b=b, Cout=5, out=None, coff=0)
        a.update(bad)
        with pytest.raises(ValueError):
            ops._check_conv_s2_args(a["x"], a["p"], a["b"], a["Cout"], 7, a["out"], a["coff"])
    assert ops._check_maxpool3s2_args(lat, 64, None) == (2, 23, 29, 64, 512, 12, 15)
    assert ops._check_maxpool3s2_args(torch.zeros(1, 1, 1, 3), None, None) == (1, 1, 1, 3, 3, 1, 1)
    for C, out in ((513, None), (0, None), (64, torch.zeros(2, 12, 15, 63))):
        with pytest.raises(ValueError):
            ops._check_maxpool3s2_args(lat, C, out)
    img = torch.zeros(2, 3, 5, 7)
    ring = torch.zeros(13, 15, 18)
    assert ops._check_encoder_input_args(img, ring, 4, None, None) == (2, 5, 7, 4, 18, 21)
    assert ops._check_encoder_input_args(img, ring, 4, 24, None) == (2, 5, 7, 4, 18, 24)
    assert ops._check_encoder_input_args(img, None, 0, None, None) == (2, 5, 7, 0, 0, 3)
    for bad in (dict(x=img.double()), dict(x=img[:, :2]), dict(x=img[0]), dict(ring=torch.zeros(13, 14, 18)), dict(ring=ring.double()), dict(pad=-1),
                dict(C=20), dict(out=torch.zeros(2, 13, 15, 22))):
        a = dict(x=img, ring=ring, pad=4, C=None, out=None)
        a.update(bad)
        with pytest.raises(ValueError):
            ops._check_encoder_input_args(a["x"], a["ring"], a["pad"], a["C"], a["out"])
    assert ops._check_pyramid_level_args(torch.zeros(2, 3, 4, 64), lat, 64) == (2, 3, 4, 64, 23, 29, 512)
    for lv, out, c0 in ((torch.zeros(2, 3, 4, 64), lat, 449), (torch.zeros(1, 3, 4, 64), lat, 0), (torch.zeros(2, 3, 4, 64), lat, -1),
                        (torch.zeros(2, 3, 4, 64).double(), lat, 0), (torch.zeros(2, 3, 4, 64), lat.permute(0, 3, 1, 2), 0)):
        with pytest.raises(ValueError):
            ops._check_pyramid_level_args(lv, out, c0)
    # valid arguments on the CPU: refused, never computed some other way
    for call in (lambda: ops.conv_s2(x, p, b, 5, 7), lambda: ops.maxpool3s2(lat, 64), lambda: ops.encoder_input(img, ring, 4),
                 lambda: ops.pyramid_level(torch.zeros(2, 3, 4, 64), lat, 64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_device_trunk_checks_without_a_device():
    from diner_amd import encoder as E
    from src.models.image_encoder import SpatialEncoder
    G = generator()
    sd = G.state_dict("A")
    t = E.DeviceTrunk(sd, image_padding=4)
    assert (t.backbone, t.num_layers, t.ring_channels, t.stem_cin, t.latent_size) == ("resnet34", 4, 18, 24, 512)
    assert len(t._names) == 1 + 2 * (3 + 4 + 6) + 2 == 29                      # the 29 convolutions up to layer3
    shapes, size = t.plan(2, 37, 50)
    assert size == (23, 29) and dict(shapes)["input"] == (2, 45, 58, 24) and dict(shapes)["pool"] == (2, 12, 15, 64)
    assert dict(shapes)["s1a"] == (2, 6, 8, 128) and dict(shapes)["s2d"] == (2, 3, 4, 256) and "level0" not in dict(shapes)
    c = E.DeviceTrunk(G.state_dict("C"), num_layers=3, use_first_pool=False, image_padding=0, padding_pe=-1)
    assert (c.ring_channels, c.stem_cin, c.latent_size) == (0, 4, 256) and dict(c.plan(1, 16, 20)[0])["level0"] == (1, 8, 10, 64)
    assert E.DeviceTrunk(G.state_dict("B"), backbone="resnet18", num_layers=5, image_padding=8).latent_size == 1024
    enc = SpatialEncoder(pretrained=False, image_padding=64, padding_pe=4)
    m = E.DeviceTrunk(enc, backbone="resnet18", num_layers=2, image_padding=0)          # a module's own configuration wins
    assert (m.backbone, m.num_layers, m.image_padding, m.ring_channels, m._prefix) == ("resnet34", 4, 64, 18, "model.")
    assert E.DeviceTrunk({k[len("model."):]: v for k, v in sd.items()}, image_padding=4)._prefix == ""
    with pytest.raises(NotImplementedError, match="upsample_interp"):
        E.DeviceTrunk(sd, upsample_interp="nearest")
    enc.upsample_interp = "nearest"
    with pytest.raises(NotImplementedError, match="upsample_interp"):
        E.DeviceTrunk(enc)
    with pytest.raises(NotImplementedError, match="backbone"):
        E.DeviceTrunk(sd, backbone="resnet50")
    for kw in (dict(num_layers=0), dict(num_layers=6), dict(image_padding=3), dict(image_padding=-2)):
        with pytest.raises(ValueError):
            E.DeviceTrunk(sd, **kw)
    with pytest.raises(ValueError):
        E.DeviceTrunk([1, 2])
    with pytest.raises(ValueError, match="conv1.weight"):
        E.DeviceTrunk({"features.0.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="layer2.0.downsample.1.running_var"):
        E.DeviceTrunk({k: v for k, v in sd.items() if k != "model.layer2.0.downsample.1.running_var"}, image_padding=4)._tensors()
    for bad in (torch.zeros(1, 2, 3, 8), torch.zeros(1, 2, 4, 8, 8), torch.zeros(1, 2, 3, 8, 8).double(), "x"):
        with pytest.raises(ValueError):
            t(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t(torch.zeros(1, 2, 3, 8, 8))
    assert SpatialEncoder.device_trunk is False


def test_switch_and_cli_flag(monkeypatch, tmp_path):
    import inspect
    from diner_amd import evaluate
    from src.models.image_encoder import SpatialEncoder
    assert inspect.signature(evaluate.write_prediction_folder).parameters["device_trunk"].default is False
    assert evaluate._parser().parse_args(["--eval_path", "x"]).device_trunk is False
    monkeypatch.setattr(evaluate, "evaluate_folder", lambda *a, **k: {"psnr": 1.0})
    monkeypatch.setattr(SpatialEncoder, "device_trunk", False)
    evaluate.main(["--eval_path", str(tmp_path)])
    assert SpatialEncoder.device_trunk is False
    evaluate.main(["--eval_path", str(tmp_path), "--device_trunk"])
    assert SpatialEncoder.device_trunk is True


def test_folding_is_batchnorm_in_float64():
    """conv with (w', b') equals BN(conv(w)) to 1e-12 on one convolution of each kind: stride 1, stride 2 with its downsample, the stem."""
    from diner_amd import encoder as E
    G = generator()
    sd = {k: v.double() for k, v in G.state_dict("A").items() if v.is_floating_point()}
    g = torch.Generator().manual_seed(7)
    for conv, bn, stride, pad in (("layer1.1.conv2", "layer1.1.bn2", 1, 1), ("layer2.0.conv1", "layer2.0.bn1", 2, 1),
                                  ("layer2.0.downsample.0", "layer2.0.downsample.1", 2, 0), ("conv1", "bn1", 2, 3)):
        w = sd[f"model.{conv}.weight"]
        p = [sd[f"model.{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")]
        x = torch.randn(2, w.shape[1], 13, 11, generator=g, dtype=torch.float64)
        want = F.batch_norm(F.conv2d(x, w, stride=stride, padding=pad), p[2], p[3], p[0], p[1], False, 0.0, 1e-5)
        wf, bf = E.fold_bn(w.float(), *[t.float() for t in p])
        assert wf.dtype == torch.float64 and bf.dtype == torch.float64
        got = F.conv2d(x, wf, bf, stride=stride, padding=pad)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), conv
        assert float((wf - w).abs().max()) > 0.05 * float(w.abs().max())          # the statistics are far from the identity


def test_g27_restatement_reproduces_the_fixture():
    G = generator()
    g = load("g27_encoder.npz")
    for case, c in G.CASES.items():
        sd, images = G.state_dict(case), G.images_of(case)
        assert G.sha256_of(sd) == str(g[f"{case}_sha256"]), case
        assert list(g[f"{case}_images"]) == list(c["images"]) and list(g[f"{case}_seeds"]) == [c["seed"], c["image_seed"]]
        with torch.no_grad():
            lat = G.trunk_restated(sd, images, torch.float64, **G.config(case))
        assert list(lat.shape) == list(g[f"{case}_shape"])
        sub, stride = G.subsample(lat)
        assert stride == int(g[f"{case}_stride"])
        assert np.abs(sub.numpy() - g[f"{case}_sub64"]).max() <= 1e-12 * float(g[f"{case}_absmax"]), case
        # the yardstick: torch's own float32 sits two orders of magnitude inside the 1e-4 bar of the GPU test
        assert len(g[f"{case}_yard"]) == c["num_layers"] and float(g[f"{case}_yard"].max()) < 1e-5 and float(g[f"{case}_ref_rel"]) <= 1e-12
    assert list(g["A_shape"]) == [1, 2, 512, 23, 29] and list(g["D_shape"]) == [1, 1, 512, 94, 104]


def test_g27_reference_pin():
    """The reference's own SpatialEncoder.forward, in float64 on the same seeded weights, against the restatement."""
    from oracle import ref_import
    if not ref_import.reference_available():
        pytest.skip("reference tree not present")
    G = generator()
    for case in ("A", "C"):
        sd, images, cfg = G.state_dict(case), G.images_of(case), G.config(case)
        ref = G.reference_latent(sd, images, cfg)
        with torch.no_grad():
            lat = G.trunk_restated(sd, images, torch.float64, **cfg)
        assert ref.shape == lat.shape and ref.dtype == torch.float64
        assert float((ref - lat).abs().max()) <= 1e-12 * float(lat.abs().max()), case
