"""Image metrics without a GPU: the host restatement against G24 (skimage 0.18.3 on seeded pairs), the drop-in
src.evaluation.eval_suite's public names against the reference's (G24), the PNG reader's row filters, and the refusals of the
diner_image_metrics_* entries."""
import ctypes as C
import hashlib
import inspect
import json
import struct
import zlib

import numpy as np
import pytest

from diner_amd.png import read_png, write_png
from diner_amd.synthetic import METRIC_CASES, metric_pair
from tests.helpers import load
from tests.metrics_host import host_metrics

COLS = ("ssim", "psnr", "mse", "l1", "l1_f64", "ssim_f32")


def g24_rows():
    g = load("g24_image_metrics.npz")
    assert list(g["columns"]) == list(COLS)
    assert [str(c) for c in g["cases"]] == [f"{k}:{h}:{w}:{s}" for k, h, w, s in METRIC_CASES]
    for case, sha, row in zip(METRIC_CASES, g["sha"], g["scores"]):
        p, gt = metric_pair(*case)
        assert hashlib.sha256(p.tobytes()).hexdigest() + hashlib.sha256(gt.tobytes()).hexdigest() == str(sha), case
        yield case, p, gt, dict(zip(COLS, row))


def test_host_restatement_matches_g24():
    kinds = set()
    for case, p, gt, ref in g24_rows():
        m = host_metrics(p, gt)
        assert abs(m["ssim"] - ref["ssim"]) <= 1e-12, (case, m["ssim"], ref["ssim"])
        if np.isinf(ref["psnr"]):
            assert m["psnr"] == ref["psnr"] and m["l2"] == 0.0
        else:
            assert abs(m["psnr"] - ref["psnr"]) <= 1e-12, case
        assert abs(m["l2"] - ref["mse"]) <= 1e-12 * ref["mse"], case
        assert abs(m["l1"] - ref["l1_f64"]) <= 1e-12 * max(ref["l1_f64"], 1e-300), case
        assert abs(m["l1"] - ref["l1"]) <= max(abs(ref["l1"] - ref["l1_f64"]), 1e-12 * ref["l1_f64"]), case
        kinds.add(case[0])
    assert kinds == {"uniform", "smooth", "object", "identical", "constant", "rgba", "near"}


def test_g24_yardsticks_are_reported():
    g = load("g24_image_metrics.npz")
    assert str(g["skimage_version"]) == "0.18.3"
    s = g["scores"]
    ident = [i for i, c in enumerate(METRIC_CASES) if c[0] == "identical"]
    assert all(np.isinf(s[i, 1]) and s[i, 0] == 1.0 for i in ident)
    gap = np.abs(s[:, 5] - s[:, 0])          # float32-SSIM vs 0.18's float64: reported, never asserted against
    print("ssim float32 / float64 gap: max", gap.max(), "l1 float32 accumulation error: max", np.abs(s[:, 3] - s[:, 4]).max())


def test_drop_in_names_match_reference():
    from src.evaluation import eval_suite as E
    g = load("g24_image_metrics.npz")
    consts = json.loads(str(g["ref_constants_json"]))
    for name, value in consts.items():
        mine = getattr(E, name)
        assert json.loads(json.dumps(mine)) == value, name
    params = list(inspect.signature(E.evaluate_folder).parameters)
    assert params == [str(p) for p in g["ref_evaluate_folder_params"]]
    with pytest.raises(NotImplementedError):
        E.compare_evaluations([], "unused")


def test_evaluate_folder_refuses_cpu_device(tmp_path):
    from src.evaluation import eval_suite as E
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.evaluate_folder(tmp_path, tmp_path, device="cpu")


# ---- PNG row filters ---------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def _filter_row(ft, cur, prev, bpp):
    out = []
    for j, x in enumerate(cur):
        a = cur[j - bpp] if j >= bpp else 0
        b = prev[j]
        c = prev[j - bpp] if j >= bpp else 0
        pred = (0, a, b, (a + b) // 2, _paeth(a, b, c))[ft]
        out.append((x - pred) & 0xff)
    return out


def _write_filtered_png(path, img, types):
    H, W = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    flat = img.reshape(H, W * ch).astype(int)
    raw = bytearray()
    prev = [0] * (W * ch)
    for i in range(H):
        ft = types[i % len(types)]
        raw.append(ft)
        raw.extend(_filter_row(ft, list(flat[i]), prev, ch))
        prev = list(flat[i])

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {1: 0, 3: 2, 4: 6}[ch], 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b""))


@pytest.mark.parametrize("shape", [(9, 13), (9, 13, 3), (11, 7, 4)])
def test_read_png_decodes_all_filter_types(tmp_path, shape):
    rs = np.random.RandomState(sum(shape))
    img = rs.randint(0, 256, shape).astype(np.uint8)
    img[::3] = 250                               # wrap-around of the modulo-256 sums
    for types in ([0], [1], [2], [3], [4], [0, 1, 2, 3, 4], [4, 3, 2, 1]):
        p = tmp_path / f"f{''.join(map(str, types))}.png"
        _write_filtered_png(p, img, types)
        np.testing.assert_array_equal(read_png(p), img, err_msg=str(types))


def test_read_png_pil_files(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:40, 0:57]
    for img in (rs.randint(0, 256, (40, 57, 3)).astype(np.uint8),
                np.stack([(xx * 4) % 256, (yy * 6) % 256, (xx + yy) % 256], -1).astype(np.uint8),
                np.concatenate([np.stack([(xx * 4) % 256] * 3, -1), rs.randint(0, 256, (40, 57, 1))], -1).astype(np.uint8)):
        p = tmp_path / "pil.png"
        PIL.fromarray(img).save(p)
        np.testing.assert_array_equal(read_png(p), img)


def test_read_png_type0_roundtrip(tmp_path):
    img = np.random.RandomState(5).randint(0, 256, (17, 23, 3)).astype(np.uint8)
    write_png(tmp_path / "a.png", img)
    np.testing.assert_array_equal(read_png(tmp_path / "a.png"), img)


# ---- C ABI refusals ----------------------------------------------------------------------------------------------------------
def test_metrics_argument_validation_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(8)
    ok = dict(N=2, H=16, W=16, pc=3, gc=3)
    for bad, word in ((dict(N=0), b"N = 0"), (dict(H=6), b"at least 7"), (dict(W=3), b"at least 7"), (dict(pc=4), b"pred has 4"),
                      (dict(gc=2), b"gt has 2"), (dict(gc=5), b"gt has 5")):
        a = dict(ok, **bad)
        rc = lib.diner_image_metrics_u8(p, p, a["N"], a["H"], a["W"], a["pc"], a["gc"], p, p, None)
        assert rc == _lib.E_INVALID and word in lib.diner_last_error(), (bad, lib.diner_last_error())
    rc = lib.diner_image_metrics_u8(None, p, 1, 16, 16, 3, 3, p, p, None)
    assert rc == _lib.E_INVALID and b"null" in lib.diner_last_error()
    rc = lib.diner_image_metrics_u8(p, p, 1, 16, 16, 3, 4, None, p, None)
    assert rc == _lib.E_INVALID and b"null" in lib.diner_last_error()
    rc = lib.diner_image_metrics_f32(p, p, 1, 16, 16, p, None, None)
    assert rc == _lib.E_INVALID and b"null" in lib.diner_last_error()
    rc = lib.diner_image_metrics_f32(p, p, 1, 16, 5, p, p, None)
    assert rc == _lib.E_INVALID and b"at least 7" in lib.diner_last_error()
    assert lib.diner_image_metrics_workspace_bytes(1, 6, 16) == 0
    assert lib.diner_image_metrics_workspace_bytes(2, 600, 800) > 0
