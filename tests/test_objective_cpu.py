"""The training objective without a GPU: the new C-ABI entries resolve and refuse bad arguments, fixture G25 (the reference's MSELoss /
AntibiasLoss / autograd gradient on seeded inputs, tools/make_golden_objective.py) regenerates its inputs and agrees with the numpy
restatement kept here, the patch rule restated here reproduces G25's index lists, and the drop-in src.losses classes keep the
reference's names."""
import ctypes as C
import hashlib
import inspect
import json

import numpy as np
import pytest
import torch

from diner_amd.synthetic import OBJECTIVE_CASES, PATCH_CASES, objective_case, patch_case
from tests.helpers import load


# ---- numpy restatements (the device tests import them) -----------------------------------------------------------------------------
def host_objective(pred, gt, s, n, w_antibias, w_mse=1.0):
    """float64: {rgb_fine, antibias, w_mse rgb_fine + w_antibias antibias} and the gradient of the third with respect to pred."""
    d = pred.astype(np.float64) - gt.astype(np.float64)
    SB, B, _ = d.shape
    mse = np.mean(d * d)
    grad = w_mse * 2.0 * d / d.size
    ab = 0.0
    if s > 0:
        c = 1 << n
        k = s // c
        D = d.reshape(SB, k, c, k, c, 3).mean(axis=(2, 4))                  # (SB, k, k, 3): cell means of p - g
        ab = np.mean(np.abs(D))
        g_cell = w_antibias * np.sign(D) / (c * c * D.size)
        grad = grad + np.broadcast_to(g_cell[:, :, None, :, None, :], (SB, k, c, k, c, 3)).reshape(SB, B, 3)
    return np.array([mse, ab, w_mse * mse + w_antibias * ab]), grad


def host_patch(fg, u, s):
    """The patch rule: border of pad = (s + 1) // 2 zeroed, centre = first pixel (row-major) whose inclusive float64 prefix sum
    exceeds u * total, image centre + flag for an all-zero padded mask; the patch is rows cy - pad .. of columns cx - pad .. ."""
    SB, H, W = fg.shape
    pad = (s + 1) // 2
    centres, lists, flags = [], [], []
    for o in range(SB):
        w = np.where(fg[o] > 0, fg[o], 0).astype(np.float64)
        keep = np.zeros((H, W), bool)
        keep[pad:H - pad, pad:W - pad] = True
        cs = np.cumsum(np.where(keep, w, 0.0).reshape(-1))
        hit = np.nonzero(cs > np.float64(u[o]) * cs[-1])[0]
        if cs[-1] > 0 and len(hit):
            cx, cy, flag = int(hit[0]) % W, int(hit[0]) // W, 0
        else:
            cx, cy, flag = W // 2, H // 2, 1
        rows = np.arange(s)[:, None] + (cy - pad)
        cols = np.arange(s)[None, :] + (cx - pad)
        lists.append((rows * W + cols).reshape(-1))
        centres.append((cx, cy))
        flags.append(flag)
    return np.array(centres, np.int32), np.array(lists, np.int32), np.array(flags, np.int32)


def g25_cases():
    """-> (case tuple, pred, gt, dict of the stored reference values) for every objective case, inputs checked against their sha256."""
    g = load("g25_objective.npz")
    assert [str(c) for c in g["cases"]] == [":".join(str(v) for v in c) for c in OBJECTIVE_CASES]
    for i, case in enumerate(OBJECTIVE_CASES):
        kind, SB, s, n, w, B, seed = case
        pred, gt = objective_case(kind, SB, s, n, B, seed)
        assert hashlib.sha256(pred.tobytes()).hexdigest() + hashlib.sha256(gt.tobytes()).hexdigest() == str(g[f"c{i}_sha"]), case
        step = 1 if pred.size <= int(g["grad_full_limit"]) else int(g["grad_stride"])
        yield case, pred, gt, dict(loss32=g[f"c{i}_loss32"], loss64=g[f"c{i}_loss64"], grad32=g[f"c{i}_grad32"], grad64=g[f"c{i}_grad64"],
                                   grad_spread=float(g[f"c{i}_grad_spread"]), grad64_sums=g[f"c{i}_grad64_sums"], step=step)


def g25_patches():
    g = load("g25_objective.npz")
    assert [str(c) for c in g["patch_cases"]] == [":".join(str(v) for v in c) for c in PATCH_CASES]
    for i, (H, W, s, seed) in enumerate(PATCH_CASES):
        fg, u = patch_case(H, W, s, seed)
        assert np.array_equal(fg, g[f"p{i}_fg"]) and np.array_equal(u, g[f"p{i}_u"])
        yield (H, W, s), fg, u, g[f"p{i}_centres"], g[f"p{i}_pix"], g[f"p{i}_flags"]


# ---- fixture against the restatements ------------------------------------------------------------------------------------------------
def test_host_restatement_matches_g25():
    kinds = set()
    for case, pred, gt, ref in g25_cases():
        kind, SB, s, n, w, B, seed = case
        losses, grad = host_objective(pred, gt, s, n, w)
        for k in range(3):
            assert abs(losses[k] - ref["loss64"][k]) <= 1e-12 * max(abs(ref["loss64"][k]), 1e-300), (case, k, losses[k], ref["loss64"][k])
        scale = np.abs(ref["grad64"]).max()
        assert np.abs(grad.reshape(-1)[::ref["step"]] - ref["grad64"]).max() <= 1e-12 * scale, case
        assert abs(grad.sum() - ref["grad64_sums"][0]) <= 1e-12 * ref["grad64_sums"][1], case
        assert abs(np.abs(grad).sum() - ref["grad64_sums"][1]) <= 1e-12 * ref["grad64_sums"][1], case
        # the reference's own float32 run sits where its float32-versus-float64 spread says it does
        assert np.abs(ref["grad32"].astype(np.float64) - ref["grad64"]).max() <= ref["grad_spread"]
        print(f"{case}: reference float32 - float64: losses {ref['loss32'] - ref['loss64']}, gradient {ref['grad_spread']:.2e} "
              f"(largest |gradient| {scale:.2e})")
        if kind == "zero_cells":
            assert (grad == 0).sum() == pred.size // 2 and (ref["grad64"] == 0).sum() == ref["grad64"].size // 2
        kinds.add((kind, SB, s, n, w))
    assert {("patch", 4, 64, 3, 1.0), ("patch", 4, 64, 3, 5.0), ("patch", 2, 32, 2, 1.0), ("patch", 1, 64, 0, 1.0),
            ("zero_cells", 2, 32, 3, 1.0), ("random", 4, 0, 0, 0.0)} <= kinds


def test_patch_rule_matches_g25():
    seen_flags, seen_u = set(), set()
    for (H, W, s), fg, u, centres, pix, flags in g25_patches():
        c, p, f = host_patch(fg, u, s)
        assert np.array_equal(c, centres) and np.array_equal(p, pix) and np.array_equal(f, flags), (H, W, s)
        assert pix.min() >= 0 and pix.max() < H * W
        pad = (s + 1) // 2
        for o in range(fg.shape[0]):
            cx, cy = centres[o]
            if not flags[o]:
                assert fg[o, cy, cx] > 0 and pad <= cx < W - pad and pad <= cy < H - pad
            assert pix[o, 0] == (cy - pad) * W + cx - pad and pix[o, 1] == pix[o, 0] + 1 and pix[o, s] == pix[o, 0] + W
        seen_flags |= set(flags.tolist())
        seen_u |= set(float(v) for v in u)
        assert (fg[0] * 65536 % 1 == 0).all() and ((fg[0] > 0) & (fg[0] < 1)).any()            # fractional weights, exact sums
    assert seen_flags == {0, 1} and 0.0 in seen_u and max(seen_u) == float(np.float32(1) - np.float32(2.0 ** -24))
    # the orientation of the patch: the reference's own index arithmetic, run by the generator for one centre
    g = load("g25_objective.npz")
    s, W = int(g["orient_s"]), int(g["orient_W"])
    cx, cy = (int(v) for v in g["orient_centre"])
    pad = (s + 1) // 2
    want = ((np.arange(s)[:, None] + cy - pad) * W + np.arange(s)[None, :] + cx - pad).reshape(-1)
    assert np.array_equal(g["orient_pix"], want)


# ---- drop-in names -------------------------------------------------------------------------------------------------------------------
def test_drop_in_loss_names_match_reference():
    import src.losses as L
    names = json.loads(str(load("g25_objective.npz")["ref_names_json"]))
    ref = names["antibiasloss.AntibiasLoss"]
    assert list(inspect.signature(L.AntibiasLoss.__init__).parameters) == ref["__init__"]
    assert list(inspect.signature(L.AntibiasLoss.forward).parameters) == ref["forward"]
    ref = names["vggloss.VGGLoss"]
    assert list(inspect.signature(L.VGGLoss.forward).parameters) == ref["forward"]
    # the reference's constructor takes nothing (it loads torchvision's pretrained VGG-19 itself); the drop-in adds one optional argument
    assert ref["__init__"] == ["self"]
    sig = inspect.signature(L.VGGLoss.__init__).parameters
    assert list(sig) == ["self", "features"] and sig["features"].default is None
    with pytest.raises(NotImplementedError):
        L.AntibiasLoss(3, metric=torch.nn.MSELoss())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.AntibiasLoss(2)(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def _vgg_like_features(seed, width=4):
    """21 modules laid out like torchvision's vgg19().features[:21] (conv / relu / pool positions), narrow and seeded."""
    torch.manual_seed(seed)
    mods, c_in = [], 3
    for kind in "CRCRPCRCRPCRCRCRCRPCR":
        if kind == "C":
            mods.append(torch.nn.Conv2d(c_in, width, 3, padding=1))
            c_in = width
        else:
            mods.append(torch.nn.MaxPool2d(2, 2) if kind == "P" else torch.nn.ReLU(inplace=False))
    return torch.nn.Sequential(*mods)


def test_vggloss_forward_spelt_out():
    from src.losses import VGGLoss
    feats = _vgg_like_features(5)
    assert [type(m).__name__ for m in feats][:7] == ["Conv2d", "ReLU", "Conv2d", "ReLU", "MaxPool2d", "Conv2d", "ReLU"]
    loss = VGGLoss(features=feats)
    g = torch.Generator().manual_seed(6)
    x = torch.rand(2, 3, 32, 32, generator=g).requires_grad_(True)
    y = torch.rand(2, 3, 32, 32, generator=g).requires_grad_(True)
    got = loss(x, y)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    xs, ys = (x - mean) / std, (y - mean) / std
    want = 0
    for (a, b), w in zip(((0, 2), (2, 7), (7, 12), (12, 21)), (1 / 16, 1 / 8, 1 / 4, 1.0)):
        for i in range(a, b):
            xs, ys = feats[i](xs), feats[i](ys)
        want = want + w * (xs - ys).abs().mean()
    assert abs(float(got) - float(want)) <= 1e-6 * abs(float(want)) and float(got) > 0
    got.backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0 and y.grad is None          # the target side is detached
    assert not any(p.requires_grad for p in loss.parameters())
    with pytest.raises(ValueError):
        VGGLoss(features=torch.nn.Sequential(*list(feats)[:12]))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_objective_symbols_and_argument_validation_without_gpu():
    from diner_amd import _lib
    lib = _lib.load()
    for sym in ("diner_sample_patch", "diner_gen_rays_at_f32", "diner_objective_workspace_bytes", "diner_objective_f32"):
        assert hasattr(lib, sym) and sym in _lib.SIGNATURES, sym
    p = C.c_void_p(8)
    inv = _lib.E_INVALID

    def err():
        return lib.diner_last_error()

    # the patch of the step
    assert lib.diner_sample_patch(None, 2, 48, 56, 16, None, 0, 0, p, p, p, None) == inv and b"null" in err()
    assert lib.diner_sample_patch(p, 2, 48, 56, 16, None, 0, 0, p, None, p, None) == inv and b"null" in err()
    assert lib.diner_sample_patch(p, 2, 48, 56, 16, None, 0, 0, p, p, None, None) == inv and b"null" in err()
    assert lib.diner_sample_patch(p, 2, 48, 56, 48, None, 0, 0, p, p, p, None) == inv and b"min(H, W)" in err()      # s + 1 > min(H, W)
    assert lib.diner_sample_patch(p, 2, 64, 64, 64, None, 0, 0, p, p, p, None) == inv and b"min(H, W)" in err()
    assert lib.diner_sample_patch(p, 2, 48, 56, 0, None, 0, 0, p, p, p, None) == inv
    assert lib.diner_sample_patch(p, 0, 48, 56, 16, None, 0, 0, p, p, p, None) == inv
    # rays at listed pixels
    cams = (C.c_float * (17 * 16))()
    cp = C.cast(cams, C.c_void_p)
    assert lib.diner_gen_rays_at_f32(cp, cp, cp, cp, 17, 40, 30, p, 10, p, None) == inv and b"at most 16" in err()
    assert lib.diner_gen_rays_at_f32(cp, cp, cp, cp, 2, 40, 30, None, 10, p, None) == inv and b"null" in err()
    assert lib.diner_gen_rays_at_f32(cp, cp, cp, cp, 2, 40, 30, p, 10, None, None) == inv and b"null" in err()
    assert lib.diner_gen_rays_at_f32(None, cp, cp, cp, 2, 40, 30, p, 10, p, None) == inv and b"null" in err()
    assert lib.diner_gen_rays_at_f32(cp, cp, cp, cp, 2, 0, 30, p, 10, p, None) == inv
    assert lib.diner_gen_rays_at_f32(cp, cp, cp, cp, 2, 40, 30, p, 0, p, None) == 0               # nothing to do is not an error
    # the objective
    ok = dict(pred=p, gt=p, images=None, pix=None, SB=4, B=4096, H=0, W=0, s=64, n=3, wm=1.0, wa=1.0, ws=p, losses=p, d=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.diner_objective_f32(a["pred"], a["gt"], a["images"], a["pix"], a["SB"], a["B"], a["H"], a["W"], a["s"], a["n"],
                                       a["wm"], a["wa"], a["ws"], a["losses"], a["d"], None)

    for bad, word in ((dict(pred=None), b"null"), (dict(ws=None), b"null"), (dict(losses=None), b"null"), (dict(d=None), b"null"),
                      (dict(gt=None), b"null"), (dict(gt=None, images=p), b"null"), (dict(gt=None, pix=p), b"null"),
                      (dict(s=60), b"not the s x s"), (dict(B=4095), b"not the s x s"), (dict(s=0, B=128), b"B != s * s"),
                      (dict(s=36, B=1296), b"not a multiple"), (dict(n=7), b"not a multiple"), (dict(n=-1), b"n_downsampling"),
                      (dict(SB=0), b"SB = 0"), (dict(wa=-1.0), b">= 0"), (dict(wa=float("nan")), b">= 0"),
                      (dict(gt=None, images=p, pix=p, H=0, W=40), b"image size")):
        assert call(**bad) == inv and word in err(), (bad, err())
    assert lib.diner_objective_workspace_bytes(4, 4096, 64, 3) == 4 * 8 * 2 * 8
    assert lib.diner_objective_workspace_bytes(4, 128, 0, 0) == 4 * 1 * 2 * 8
    assert lib.diner_objective_workspace_bytes(4, 4096, 60, 3) == 0 and lib.diner_objective_workspace_bytes(4, 4096, 64, 7) == 0
    with pytest.raises(RuntimeError, match="E_INVALID|code -1"):
        _lib.check(call(s=60))


def test_objective_wrappers_refuse_cpu_tensors():
    from diner_amd import objective, ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objective.sample_patch(torch.ones(1, 40, 40), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objective.objective(torch.zeros(1, 16, 3), torch.zeros(1, 16, 3), s=4, n_downsampling=1, w_antibias=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        objective.photometric(torch.zeros(1, 16, 3), torch.zeros(1, 16, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gen_rays_at(torch.eye(4)[None], torch.eye(3)[None], 8, 8, 0.5, 1.5, torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError):
        objective.calc_losses(None, None, dict(target_rgb=torch.zeros(1, 3, 80, 80)), znear=0.5, zfar=1.5, w_vgg=0.1)      # no vgg_fn
    with pytest.raises(ValueError):
        objective.calc_losses(None, None, dict(target_rgb=torch.zeros(1, 3, 80, 80)), znear=0.5, zfar=1.5, w_antibias=1.0)  # no patch
