"""Generate tests/golden/g25_objective.npz: the reference's training objective on seeded inputs, and the patch sampler's rule.

    python tools/make_golden_objective.py REFERENCE_DIR

REFERENCE_DIR/src/losses/antibiasloss.py is loaded by file path (the package __init__ pulls in torchvision).  For every case of
diner_amd.synthetic.OBJECTIVE_CASES the file stores what DINER.calc_losses computes from pred and gt (diner.py:267-288):
torch.nn.MSELoss, the reference's AntibiasLoss on the patch viewed as (SB,3,s,s), their weighted total and autograd's gradient of the
total with respect to pred -- once in float32, as the reference runs, and once with the same modules on float64 tensors.  The
float32-versus-float64 spread is the yardstick of the device tests.  Per case: loss32 / loss64 (3,), grad_spread = max |grad32 -
grad64|, the sums of grad64 and |grad64|, and the gradients themselves -- every element for cases of at most 16384 elements, every
8th element (grad_stride) above, which keeps the file under the size limit of a committed fixture; the numpy restatement in
tests/test_objective_cpu.py is held to the stored elements and sums and carries the comparison to the rest.  Inputs are regenerated
from seeds (sha256 of their bytes is stored).

The patch sampler has no reproducible counterpart in the reference (torch.multinomial cannot be replayed draw for draw), so its
expected centres and index lists come from a plain numpy statement of the documented rule, for the masks and u of
diner_amd.synthetic.PATCH_CASES.  To pin the patch orientation, the index arithmetic of REFERENCE_DIR/src/models/diner.py (the
statements that turn `patch_centers` into `pix_idcs`) is read from that file at generation time and executed through torch for one
centre; only its output is stored.

The class and parameter names of the reference's src/losses modules are parsed with ast (no code is run)."""
import ast
import hashlib
import importlib.util
import json
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diner_amd.synthetic import OBJECTIVE_CASES, PATCH_CASES, objective_case, patch_case   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g25_objective.npz")
FULL_LIMIT, STRIDE = 16384, 8


def load_antibias(ref_dir):
    spec = importlib.util.spec_from_file_location("ref_antibiasloss", os.path.join(ref_dir, "src", "losses", "antibiasloss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.AntibiasLoss


def reference_objective(AntibiasLoss, pred, gt, s, n, w, dtype):
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    g = torch.from_numpy(gt).to(dtype)
    SB = p.shape[0]
    mse = torch.nn.MSELoss(reduction="mean")(p, g)
    total = mse
    ab = torch.zeros((), dtype=dtype)
    if s > 0:
        ab = AntibiasLoss(n_downsampling=n)(p.view(SB, s, s, 3).permute(0, 3, 1, 2), g.view(SB, s, s, 3).permute(0, 3, 1, 2))
        total = total + w * ab
    total.backward()
    return np.array([mse.item(), ab.item(), total.item()], np.float64), p.grad.numpy()


def patch_rule(fg, u, s):
    """The documented rule in numpy: zero the border, first pixel whose inclusive float64 prefix sum exceeds u * total."""
    SB, H, W = fg.shape
    pad = (s + 1) // 2
    centres, lists, flags = [], [], []
    for o in range(SB):
        w = np.where(fg[o] > 0, fg[o], 0).astype(np.float64)
        w[:pad] = 0
        w[-pad:] = 0
        w[:, :pad] = 0
        w[:, -pad:] = 0
        cs = np.cumsum(w.reshape(-1))
        if cs[-1] > 0:
            c = int(np.argmax(cs > np.float64(u[o]) * cs[-1]))
            cx, cy, flag = c % W, c // W, 0
        else:
            cx, cy, flag = W // 2, H // 2, 1
        ii, jj = np.mgrid[0:s, 0:s]
        lists.append(((cy - pad + ii) * W + (cx - pad + jj)).reshape(-1))
        centres.append((cx, cy))
        flags.append(flag)
    return np.array(centres, np.int32), np.array(lists, np.int32), np.array(flags, np.int32)


def reference_patch_indices(ref_dir, centre, s, W):
    """Runs the reference's own statements between `patch_centers = torch.cat(...)` and `pix_idcs = pix_idcs.flatten(...)`."""
    lines = open(os.path.join(ref_dir, "src", "models", "diner.py")).read().split("\n")
    a = next(i for i, l in enumerate(lines) if l.strip().startswith("pix_coords = torch.stack("))
    b = next(i for i, l in enumerate(lines) if l.strip().startswith("pix_idcs = pix_idcs.flatten("))
    code = textwrap.dedent("\n".join(lines[a:b + 1]))
    ns = dict(torch=torch, self=types.SimpleNamespace(vgg_spatch=s, device="cpu"), pad=(s + 1) // 2, W=W,
              patch_centers=torch.tensor([list(centre)], dtype=torch.long))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exec(compile(code, "reference diner.py", "exec"), ns)
    return ns["pix_idcs"][0].numpy().astype(np.int32)


def reference_names(ref_dir):
    out = {}
    for mod in ("antibiasloss", "vggloss"):
        tree = ast.parse(open(os.path.join(ref_dir, "src", "losses", mod + ".py")).read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef):
                out[f"{mod}.{node.name}"] = {f.name: [a.arg for a in f.args.args] for f in node.body
                                             if isinstance(f, ast.FunctionDef) and f.name in ("__init__", "forward")}
    return out


def main():
    ref_dir = sys.argv[1]
    AntibiasLoss = load_antibias(ref_dir)
    out = dict(cases=np.array([":".join(str(v) for v in c) for c in OBJECTIVE_CASES]), grad_full_limit=np.array(FULL_LIMIT),
               grad_stride=np.array(STRIDE))
    for i, (kind, SB, s, n, w, B, seed) in enumerate(OBJECTIVE_CASES):
        pred, gt = objective_case(kind, SB, s, n, B, seed)
        l32, g32 = reference_objective(AntibiasLoss, pred, gt, s, n, w, torch.float32)
        l64, g64 = reference_objective(AntibiasLoss, pred, gt, s, n, w, torch.float64)
        step = 1 if g64.size <= FULL_LIMIT else STRIDE
        out[f"c{i}_sha"] = np.array(hashlib.sha256(pred.tobytes()).hexdigest() + hashlib.sha256(gt.tobytes()).hexdigest())
        out[f"c{i}_loss32"], out[f"c{i}_loss64"] = l32, l64
        out[f"c{i}_grad32"], out[f"c{i}_grad64"] = g32.reshape(-1)[::step].copy(), g64.reshape(-1)[::step].copy()
        out[f"c{i}_grad_spread"] = np.array(np.abs(g32.astype(np.float64) - g64).max())
        out[f"c{i}_grad64_sums"] = np.array([g64.sum(), np.abs(g64).sum()])
        print(f"{kind:10s} SB {SB} s {s:2d} n {n} w {w}: losses f64 {l64}, f32 - f64 {l32 - l64}, grad spread {out[f'c{i}_grad_spread']:.2e} "
              f"(max |grad| {np.abs(g64).max():.2e}), exact-zero gradients {int((g64 == 0).sum())}")
    out["patch_cases"] = np.array([":".join(str(v) for v in c) for c in PATCH_CASES])
    for i, (H, W, s, seed) in enumerate(PATCH_CASES):
        fg, u = patch_case(H, W, s, seed)
        centres, lists, flags = patch_rule(fg, u, s)
        out[f"p{i}_fg"], out[f"p{i}_u"] = fg, u
        out[f"p{i}_centres"], out[f"p{i}_pix"], out[f"p{i}_flags"] = centres, lists, flags
        print(f"patch {H}x{W} s {s}: centres {centres.tolist()} flags {flags.tolist()}")
    H, W, s, _ = PATCH_CASES[0]
    out["orient_centre"], out["orient_s"], out["orient_W"] = np.array([20, 17], np.int32), np.array(s), np.array(W)
    out["orient_pix"] = reference_patch_indices(ref_dir, (20, 17), s, W)
    out["ref_names_json"] = np.array(json.dumps(reference_names(ref_dir), sort_keys=True))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
