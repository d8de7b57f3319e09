"""Evaluation on the device: the counterparts of DINER.create_prediction_folder (diner.py:99-136) and of the reference's
evaluate_folder (eval_suite.py:44-118), with the per-image scores computed by the HIP kernels of diner_amd.metrics.

    python -m diner_amd.evaluate --eval_path DIR      # scores DIR/visualizations, writes the reports into DIR

write_prediction_folder renders the sample dicts of diner_amd.datasets and writes <stem>-pred.png, -depth.png, -ref.png and -gt.png
per sample (the reference's suffixes); evaluate_folder pairs the -gt / -pred files of a folder, scores them on the device and writes
average_scores.json, detailed_report.json and examples.png.  LPIPS needs network weights that are not part of this project: it is
computed by a caller-supplied `lpips_fn`, by diner_amd.perceptual.Lpips on the device from a weights file (`lpips_weights`,
--lpips_weights FILE), or by the `lpips` package when that is importable, and otherwise left out with a warning."""
import argparse
import json
import os
import warnings
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from .png import read_png, write_png

PRED_SUFFIX = "-pred.png"
GT_SUFFIX = "-gt.png"
REF_SUFFIX = "-ref.png"
DEPTH_SUFFIX = "-depth.png"
ALPHA_SUFFIX = "-alpha.png"
ZDEPTH_SUFFIX = "-zdepth.png"
NORMAL_SUFFIX = "-normal.png"
PLY_SUFFIX = ".ply"
MESH_SUFFIX = "-mesh.ply"
VDEPTH_SUFFIX = "-vdepth.png"
VNORMAL_SUFFIX = "-vnormal.png"
AVERAGE_SCORE_FILENAME = "average_scores.json"
REPORT_DETAIL_FILENAME = "detailed_report.json"
EXAMPLE_PLOT_FILENAME = "examples.png"
GT_PLY_SUFFIX = "-gt.ply"
GEOMETRY_SCORE_FILENAME = "geometry_scores.json"
GEOMETRY_REPORT_FILENAME = "geometry_report.json"
N_EXAMPLE_PLOTS = 5
BATCH = 16                       # same-sized pairs scored per kernel call


def _hip_device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("diner_amd.evaluate: no HIP device; the metrics run on the device and there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"diner_amd.evaluate: device {device} is not a HIP device; there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


@torch.no_grad()
def write_prediction_folder(nerf, renderer, batches, outdir, znear, zfar, ray_batch_size=8192, write_alpha=False, cull_empty=False,
                            write_geometry=False, write_mesh=False, write_volume_view=False, device_trunk=False):
    """Render every target view of `batches` (collated sample dicts of diner_amd.datasets) with `nerf` / `renderer` and write
    <sample_name>{-pred,-depth,-ref,-gt}.png into `outdir`: the render and its colour-mapped depth, the source views side by side and
    the target, each quantised as save_image does.  Returns {"sample_name": [...], "l1", "l2", "psnr", "ssim": float64 (N,)} -- the
    scores of the renders against their targets, computed on the device from the fp32 tensors (not from the files).  write_alpha: also
    <sample_name>-alpha.png, the render's opacity (the matte) as an 8-bit grey image, quantised like the others.
    cull_empty: passed to predict_image (render only the rays the depth maps put a surface on; an approximation, off by default).
    write_geometry (off by default): render with predict_geometry instead -- the same colour, depth and opacity bit for bit -- and also
    write <sample_name>-zdepth.png (the camera-z depth of the surface through the depth colour map), <sample_name>-normal.png (the
    camera-frame normals as n * 0.5 + 0.5, quantised like the others) and <sample_name>.ply (diner_amd.geometry.point_cloud at its
    defaults: points, colours and world-frame normals).  cull_empty does not combine with it and is ignored then.
    write_mesh (off by default): also <sample_name>-mesh.ply, the triangle mesh diner_amd.surface.mesh_from_sources fuses out of the
    sample's source depth maps and colours at its defaults (the prior's surface: no MLP involved, the renders are untouched).
    write_volume_view (off by default): also <sample_name>-vdepth.png and <sample_name>-vnormal.png, that volume ray-cast into the target
    camera (TsdfVolume.raycast): its z-depth through the depth colour map and its camera-frame normals encoded as -normal.png is --
    the prior's surface as the target camera sees it, no MLP involved.  With write_mesh the two share one volume.
    device_trunk (off by default): encode the source views with diner_amd.encoder.DeviceTrunk for this run (SpatialEncoder.device_trunk;
    it takes effect with `nerf` in eval mode) and put the switch back afterwards."""
    from .datasets import encode_args
    from .imageio import depth_to_uint8, gray_to_uint8, to_uint8
    from .metrics import KEYS, image_metrics
    from .render import predict_image
    os.makedirs(outdir, exist_ok=True)
    dev = next(nerf.parameters()).device
    names, scores = [], defaultdict(list)
    if device_trunk:
        before = nerf.encoder.device_trunk
        nerf.encoder.device_trunk = True
        try:
            return write_prediction_folder(nerf, renderer, batches, outdir, znear, zfar, ray_batch_size, write_alpha, cull_empty, write_geometry,
                                           write_mesh, write_volume_view)
        finally:
            nerf.encoder.device_trunk = before
    for batch in batches:
        nerf.encode(**encode_args(batch, dev))
        gt = batch["target_rgb"].to(dev)
        H, W = gt.shape[-2:]
        if write_geometry:
            from .geometry import point_cloud, write_ply
            from .render import predict_geometry
            geo = predict_geometry(nerf, renderer, batch["target_extrinsics"].to(dev), batch["target_intrinsics"].to(dev), W, H, znear,
                                   zfar, ray_batch_size=ray_batch_size)
            rgb, depth, alpha = geo["rgb"], geo["depth"], [geo["alpha"]]
        else:
            rgb, depth, *alpha = predict_image(nerf, renderer, batch["target_extrinsics"].to(dev), batch["target_intrinsics"].to(dev), W, H,
                                               znear, zfar, ray_batch_size=ray_batch_size, return_alpha=write_alpha, cull_empty=cull_empty)
        src = batch["src_rgbs"].to(dev)
        for i, stem in enumerate(batch["sample_name"]):
            write_png(os.path.join(outdir, stem + PRED_SUFFIX), to_uint8(rgb[i]))
            write_png(os.path.join(outdir, stem + DEPTH_SUFFIX), depth_to_uint8(depth[i]))
            write_png(os.path.join(outdir, stem + REF_SUFFIX), to_uint8(torch.cat(src[i].unbind(0), dim=-1)))
            write_png(os.path.join(outdir, stem + GT_SUFFIX), to_uint8(gt[i]))
            if write_alpha:
                write_png(os.path.join(outdir, stem + ALPHA_SUFFIX), gray_to_uint8(alpha[0][i]))
            if write_geometry:
                write_png(os.path.join(outdir, stem + ZDEPTH_SUFFIX), depth_to_uint8(geo["zdepth"][i]))
                write_png(os.path.join(outdir, stem + NORMAL_SUFFIX), to_uint8(geo["normals"][i] * 0.5 + 0.5))
                write_ply(os.path.join(outdir, stem + PLY_SUFFIX), *point_cloud({k: v[i:i + 1] for k, v in geo.items()}))
            if write_mesh or write_volume_view:
                from .surface import mesh_from_sources, write_mesh_ply
                mesh, vol = mesh_from_sources(batch, sb=i, device=dev)
                if write_mesh:
                    write_mesh_ply(os.path.join(outdir, stem + MESH_SUFFIX), *mesh)
                if write_volume_view:
                    view = vol.raycast(batch["target_extrinsics"][i:i + 1], batch["target_intrinsics"][i:i + 1], W, H)
                    write_png(os.path.join(outdir, stem + VDEPTH_SUFFIX), depth_to_uint8(view["zdepth"][0]))
                    write_png(os.path.join(outdir, stem + VNORMAL_SUFFIX), to_uint8(view["normal"][0] * 0.5 + 0.5))
            names.append(stem)
        s = image_metrics(rgb, gt)
        for k in KEYS:
            scores[k].append(s[k])
    out = {"sample_name": names}
    for k in KEYS:
        out[k] = torch.cat(scores[k]) if scores[k] else torch.empty(0, dtype=torch.float64)
    return out


def _lpips_from_package(device):
    try:
        import lpips
    except ImportError as e:
        return None, f"the lpips package is not importable ({e})"
    try:
        return lpips.LPIPS(net="vgg").to(device=device), None
    except Exception as e:        # the package fetches its VGG weights on first use
        return None, f"lpips.LPIPS(net='vgg') could not be built ({type(e).__name__}: {e})"


@torch.no_grad()
def evaluate_folder(source_dir, outdir, device=None, pred_suffix=PRED_SUFFIX, gt_suffix=GT_SUFFIX, ref_suffix=REF_SUFFIX,
                    depth_suffix=DEPTH_SUFFIX, show_tqdm=False, lpips_fn=None, lpips_weights=None):
    """Score every <x>{gt_suffix} / <x>{pred_suffix} pair of `source_dir` (sorted by file name) on the HIP device `device` (None:
    the current one) and write AVERAGE_SCORE_FILENAME, REPORT_DETAIL_FILENAME and EXAMPLE_PLOT_FILENAME into `outdir`.  Returns the
    averages {ssim, psnr, l2, l1[, lpips]}; an average over an infinite psnr stays inf.  `lpips_fn(pred, gt)` receives (1,3,H,W)
    float32 device tensors in [-1, 1], as the reference calls lpips_vgg; without it the lpips package is used when importable.
    `lpips_weights`: a torch.load-able file holding a mapping as diner_amd.perceptual.Lpips takes it (an lpips.LPIPS(net="vgg")
    state dict); LPIPS then runs on the device through Lpips, ahead of the lpips package."""
    from .metrics import image_metrics
    if lpips_fn is not None and lpips_weights is not None:
        raise ValueError("evaluate_folder: pass lpips_fn or lpips_weights, not both")
    device = _hip_device(device)
    if lpips_weights is not None:
        from .perceptual import Lpips
        lpips_fn = Lpips(torch.load(lpips_weights, map_location="cpu"), device=device)
    outdir = Path(outdir)
    os.makedirs(outdir, exist_ok=True)
    source_dir = Path(source_dir)
    gt_paths = [p for p in sorted(source_dir.iterdir()) if p.name.endswith(gt_suffix)]
    pred_paths = [p.parent / p.name.replace(gt_suffix, pred_suffix) for p in gt_paths]
    if not gt_paths:
        raise FileNotFoundError(f"evaluate_folder: no *{gt_suffix} files in {source_dir}")

    lpips_warn = None
    if lpips_fn is None:
        lpips_fn, lpips_warn = _lpips_from_package(device)
    if lpips_fn is None:
        warnings.warn(f"evaluate_folder: lpips is left out of the scores: {lpips_warn}; pass lpips_fn to include it")

    n = len(gt_paths)
    per = {k: [None] * n for k in ("ssim", "psnr", "l2", "l1")}
    lp = [None] * n
    groups = defaultdict(list)                  # (H, W, gt channels) -> indices, so that each kernel call holds one size
    imgs = []
    it = range(n)
    if show_tqdm:
        try:
            import tqdm
            it = tqdm.tqdm(it, total=n, mininterval=30.)
        except ImportError:
            pass
    for i in it:
        gt = read_png(gt_paths[i])
        pred = read_png(pred_paths[i])
        if gt.ndim == 2 or pred.ndim == 2 or pred.shape[2] != 3:
            raise ValueError(f"evaluate_folder: {pred_paths[i].name} / {gt_paths[i].name}: need an RGB pred and an RGB(A) gt")
        if pred.shape[:2] != gt.shape[:2]:
            raise ValueError(f"evaluate_folder: {pred_paths[i].name} {pred.shape} and {gt_paths[i].name} {gt.shape} differ in size")
        imgs.append((pred, gt))
        groups[gt.shape].append(i)
        if lpips_fn is not None:
            to = lambda a: (torch.from_numpy(a[..., :3].astype(np.float32) / 255.0).permute(2, 0, 1)[None] * 2.0 - 1.0).to(device)  # noqa: E731
            lp[i] = float(torch.as_tensor(lpips_fn(to(pred), to(gt))).flatten().cpu().item())
    with torch.cuda.device(device):
        for idx in groups.values():
            for b in range(0, len(idx), BATCH):
                chunk = idx[b:b + BATCH]
                pred = torch.from_numpy(np.stack([imgs[i][0] for i in chunk])).to(device)
                gt = torch.from_numpy(np.stack([imgs[i][1] for i in chunk])).to(device)
                s = {k: v.cpu().tolist() for k, v in image_metrics(pred, gt).items()}
                for j, i in enumerate(chunk):
                    for k in per:
                        per[k][i] = s[k][j]
    scores = dict(per)
    if lpips_fn is not None:
        scores["lpips"] = lp

    avg = {k: float(np.mean(v)) for k, v in scores.items()}
    with open(outdir / AVERAGE_SCORE_FILENAME, "w") as f:
        json.dump(avg, f, indent="\t")
    report = [dict(path=str(pred_paths[i]), **{k: float(v[i]) for k, v in scores.items()}) for i in range(n)]
    with open(outdir / REPORT_DETAIL_FILENAME, "w") as f:
        json.dump(report, f, indent="\t")

    rows = []
    for i in np.linspace(0, n - 1, N_EXAMPLE_PLOTS).astype(int):
        pp = pred_paths[i]
        pred = imgs[i][0]

        def side(suffix):
            p = pp.parent / pp.name.replace(pred_suffix, suffix)
            return read_png(p)[..., :3] if p.exists() else np.zeros_like(pred)

        ref, gt, depth = side(ref_suffix), imgs[i][1][..., :3], side(depth_suffix)
        nref = max(1, ref.shape[1] // pred.shape[1])
        rows.append(np.concatenate([*np.hsplit(ref, nref), gt, pred, depth], axis=1))
    write_png(outdir / EXAMPLE_PLOT_FILENAME, np.ascontiguousarray(np.concatenate(rows, axis=0)))
    return avg


def _check_geometry_args(max_dist, thresholds, thin):
    max_dist = float(max_dist)
    if not max_dist > 0.0:
        raise ValueError(f"evaluate_geometry_folder: max_dist {max_dist} must be > 0 (inf: no cap)")
    thresholds = tuple(float(t) for t in thresholds)
    if len(thresholds) > 8 or not all(t >= 0.0 for t in thresholds):
        raise ValueError(f"evaluate_geometry_folder: at most 8 thresholds, each >= 0, got {thresholds}")
    if thin is not None and not (float(thin) > 0.0 and np.isfinite(float(thin))):
        raise ValueError(f"evaluate_geometry_folder: thin {thin} must be > 0 and finite")
    return max_dist, thresholds


@torch.no_grad()
def evaluate_geometry_folder(source_dir, outdir, pred_suffix=PLY_SUFFIX, gt_suffix=GT_PLY_SUFFIX, max_dist=float("inf"), thresholds=(),
                             thin=None, device=None, mesh_suffix=MESH_SUFFIX):
    """Score every <x>{gt_suffix} / <x>{pred_suffix} pair of point clouds in `source_dir` (sorted by file name; geometry.read_ply) with
    diner_amd.cloudmetrics.cloud_scores on the HIP device `device` (None: the current one); where <x>{mesh_suffix} exists
    (surface.read_mesh_ply) it is scored by its vertices as well, under keys prefixed "mesh_".  Normals take part where both files carry
    them.  Writes GEOMETRY_SCORE_FILENAME (the averages over the pairs that have the key; nan scores are averaged as nan) and
    GEOMETRY_REPORT_FILENAME (per pair) into `outdir` and returns the averages."""
    max_dist, thresholds = _check_geometry_args(max_dist, thresholds, thin)
    source_dir, outdir = Path(source_dir), Path(outdir)
    gt_paths = [p for p in sorted(source_dir.iterdir()) if p.name.endswith(gt_suffix)]
    if not gt_paths:
        raise FileNotFoundError(f"evaluate_geometry_folder: no *{gt_suffix} files in {source_dir}")
    device = _hip_device(device)
    from .cloudmetrics import cloud_scores
    from .geometry import read_ply
    from .surface import read_mesh_ply
    os.makedirs(outdir, exist_ok=True)

    def up(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)

    def numbers(s, prefix=""):
        return {prefix + k: v for k, v in s.items() if isinstance(v, (int, float))}

    report = []
    for gp in gt_paths:
        stem = gp.name[:-len(gt_suffix)]
        pp = gp.parent / (stem + pred_suffix)
        gt_xyz, _, gt_n = read_ply(gp)
        xyz, _, nrm = read_ply(pp)
        kw = dict(max_dist=max_dist, thresholds=thresholds, thin=thin)
        both = gt_n is not None and nrm is not None
        row = dict(path=str(pp), **numbers(cloud_scores(up(xyz), up(gt_xyz), pred_normals=up(nrm) if both else None,
                                                        gt_normals=up(gt_n) if both else None, **kw)))
        mp = gp.parent / (stem + mesh_suffix)
        if mp.exists():
            mesh = read_mesh_ply(mp)
            both = gt_n is not None and mesh.normals is not None
            row.update(numbers(cloud_scores(up(mesh.vertices), up(gt_xyz), pred_normals=up(mesh.normals) if both else None,
                                            gt_normals=up(gt_n) if both else None, **kw), "mesh_"))
        report.append(row)
    keys = sorted({k for row in report for k in row if k != "path"})
    avg = {k: float(np.mean([row[k] for row in report if k in row])) for k in keys}
    with open(outdir / GEOMETRY_SCORE_FILENAME, "w") as f:
        json.dump(avg, f, indent="\t")
    with open(outdir / GEOMETRY_REPORT_FILENAME, "w") as f:
        json.dump(report, f, indent="\t")
    return avg


def _parser():
    ap = argparse.ArgumentParser(description="Score the predictions of DIR/visualizations on the device; reports go to DIR.")
    ap.add_argument("--eval_path", type=Path, required=True)
    ap.add_argument("--lpips_weights", type=Path, default=None,
                    help="a torch.load-able lpips.LPIPS(net='vgg') state dict: LPIPS is computed on the device from it")
    ap.add_argument("--geometry", action="store_true",
                    help="also score the <stem>.ply / <stem>-mesh.ply geometry against <stem>-gt.ply (instead, where there are no images)")
    ap.add_argument("--max_dist", type=float, default=float("inf"), help="--geometry: distances beyond it are outliers")
    ap.add_argument("--threshold", type=float, action="append", default=[], help="--geometry: a precision / recall / F-score distance")
    ap.add_argument("--thin", type=float, default=None, help="--geometry: keep one point per cell of this size")
    ap.add_argument("--device_trunk", action="store_true",
                    help="encoders of this process compute their latent on the device (SpatialEncoder.device_trunk = True for the run)")
    return ap


def main(argv=None):
    args = _parser().parse_args(argv)
    if args.device_trunk:
        from src.models.image_encoder import SpatialEncoder
        SpatialEncoder.device_trunk = True
    source = args.eval_path / "visualizations"
    lp = {} if args.lpips_weights is None else dict(lpips_weights=args.lpips_weights)
    if not args.geometry:
        avg = evaluate_folder(source, args.eval_path, show_tqdm=True, **lp)
    else:
        avg = {}
        if any(p.name.endswith(GT_SUFFIX) for p in source.iterdir()):
            avg.update(evaluate_folder(source, args.eval_path, show_tqdm=True, **lp))
        avg.update(evaluate_geometry_folder(source, args.eval_path, max_dist=args.max_dist, thresholds=args.threshold, thin=args.thin))
    print(json.dumps(avg, indent="\t"))


if __name__ == "__main__":
    main()
