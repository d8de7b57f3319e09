"""From rendered geometry maps to point clouds: the host side of diner_amd.render.predict_geometry.

    geo = predict_geometry(nerf, renderer, E, K, W, H, znear, zfar)          # maps of one or more target views
    xyz, rgb, normals = point_cloud(geo)                                       # the pixels that carry a surface
    xyz, rgb, normals, views = fuse_views(nerf, renderer, Es, Ks, W, H, znear, zfar)   # V views, cross-checked against each other
    write_ply("scene.ply", xyz, rgb, normals)

The per-ray reduction and the cross-view check are HIP kernels (ops.ray_geometry, ops.depth_consistency); selecting the surviving
pixels is torch boolean indexing on the device -- once per frame, not a hot path -- and the PLY writer is numpy on the host."""
import numpy as np
import torch

PLY_HEADER_MAX = 4096


def _quantize_u8(rgb):
    """save_image's quantisation, as diner_amd.imageio.to_uint8 applies it: uint8(clamp(v * 255 + 0.5, 0, 255)), NaN -> 0."""
    return torch.nan_to_num(rgb * 255.0 + 0.5, nan=0.0).clamp_(0.0, 255.0).to(torch.uint8)


def _rows(maps, mask):
    """maps (SB,C,H,W), mask (SB,1,H,W) bool -> (M,C): the masked pixels, view by view in row-major pixel order."""
    return maps.permute(0, 2, 3, 1)[mask[:, 0]]


def _world_normals(normals, extrinsics):
    """camera-frame normal maps (SB,3,H,W) -> world frame: n_w = R^T n_c per view, R the world->camera rotation."""
    R = extrinsics[:, :3, :3].to(normals.device, torch.float32)
    return torch.einsum("bki,bkhw->bihw", R, normals)


def point_cloud(geo, min_alpha=0.5, max_depth_std=None, keep=None):
    """The surface points of predict_geometry's maps `geo` -> xyz (M,3) float32, rgb (M,3) uint8, normals (M,3) float32 in the WORLD
    frame (geo["normals"] rotated by the transposed rotation of geo["extrinsics"]), view by view in row-major pixel order.  A pixel is
    kept iff it is valid, its opacity is at least min_alpha, its depth spread sqrt(depth_var) is at most max_depth_std (None: no such
    test) and `keep` (SB,1,H,W) bool (None: everything) is set."""
    mask = geo["valid"] & (geo["alpha"] >= float(min_alpha))
    if max_depth_std is not None:
        mask = mask & (geo["depth_var"].clamp(min=0).sqrt() <= float(max_depth_std))
    if keep is not None:
        if tuple(keep.shape) != tuple(mask.shape) or keep.dtype != torch.bool:
            raise ValueError(f"diner_amd: point_cloud keep must be a bool mask {tuple(mask.shape)}, got {keep.dtype} {tuple(keep.shape)}")
        mask = mask & keep.to(mask.device)
    nw = _world_normals(geo["normals"], geo["extrinsics"])
    return _rows(geo["points"], mask), _quantize_u8(_rows(geo["rgb"], mask)), _rows(nw, mask)


def backproject(zdepth, intrinsics, extrinsics):
    """z-depth maps (V,1,H,W) -> world points (V,3,H,W): pixel centres at +0.5, X_c = ((j + 0.5 - cx) / fx d, (i + 0.5 - cy) / fy d, d),
    X_w = R^T (X_c - t)."""
    V, _, H, W = zdepth.shape
    dev = zdepth.device
    Km, E = intrinsics.to(dev, torch.float32), extrinsics.to(dev, torch.float32)
    u = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5).view(1, 1, W)
    v = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5).view(1, H, 1)
    d = zdepth[:, 0]
    x = (u - Km[:, 0, 2].view(V, 1, 1)) / Km[:, 0, 0].view(V, 1, 1) * d
    y = (v - Km[:, 1, 2].view(V, 1, 1)) / Km[:, 1, 1].view(V, 1, 1) * d
    Xc = torch.stack((x, y, d), dim=1) - E[:, :3, 3].view(V, 3, 1, 1)
    return torch.einsum("bki,bkhw->bihw", E[:, :3, :3], Xc)


@torch.no_grad()
def fuse_views(nerf, renderer, extrinsics, intrinsics, W, H, znear, zfar, min_views=2, px_thr=1.0, rel_thr=0.01, **predict_kw):
    """Render V target views (extrinsics (V,4,4) world->camera, intrinsics (V,3,3) or one (3,3) for all; 2 <= V <= 16) of the encoded
    scene, one predict_geometry call each, cross-check their z-depth maps (ops.depth_consistency at px_thr / rel_thr), keep the pixels at
    least min_views OTHER views agree with, and back-project the agreeing views' average depth.  -> xyz (M,3), rgb (M,3) uint8, world
    normals (M,3) -- the concatenated cloud, view by view in row-major pixel order -- and the list of the V per-view map dicts, each with
    "count" (1,1,H,W) int32 and "depth_avg" (1,1,H,W) added.  predict_kw goes to predict_geometry (ray_batch_size, seed, quantile, ...)."""
    from diner_amd import ops
    from diner_amd.render import predict_geometry
    V = int(extrinsics.shape[0])
    if tuple(extrinsics.shape) != (V, 4, 4) or not 2 <= V <= 16:
        raise ValueError(f"diner_amd: fuse_views expects extrinsics (V,4,4) with 2 <= V <= 16, got {tuple(extrinsics.shape)}")
    if intrinsics.dim() == 2:
        intrinsics = intrinsics[None].expand(V, -1, -1)
    if tuple(intrinsics.shape) != (V, 3, 3):
        raise ValueError(f"diner_amd: fuse_views expects intrinsics ({V},3,3) or (3,3), got {tuple(intrinsics.shape)}")
    zn = torch.as_tensor(znear, dtype=torch.float32).reshape(-1).expand(V)            # one value for all views, or one per view
    zf = torch.as_tensor(zfar, dtype=torch.float32).reshape(-1).expand(V)
    views = [predict_geometry(nerf, renderer, extrinsics[v:v + 1], intrinsics[v:v + 1], W, H, zn[v:v + 1], zf[v:v + 1], **predict_kw)
             for v in range(V)]
    zdepth = torch.cat([g["zdepth"] for g in views], dim=0)
    count, avg = ops.depth_consistency(zdepth, intrinsics, extrinsics, px_thr, rel_thr)
    keep = (count >= int(min_views)).unsqueeze(1)
    pts = backproject(avg.unsqueeze(1), intrinsics, extrinsics)
    rgb = torch.cat([g["rgb"] for g in views], dim=0)
    nw = _world_normals(torch.cat([g["normals"] for g in views], dim=0), extrinsics)
    for v, g in enumerate(views):
        g["count"], g["depth_avg"] = count[v:v + 1, None], avg[v:v + 1, None]
    return _rows(pts, keep), _quantize_u8(_rows(rgb, keep)), _rows(nw, keep), views


def _host(a, dtype, cols=3):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    if a.ndim != 2 or a.shape[1] != cols or a.dtype != dtype:
        raise ValueError(f"diner_amd: PLY columns must be (M,{cols}) {np.dtype(dtype).name}, got {a.dtype.name} {a.shape}")
    return a


def _ply_dtype(has_normals, has_rgb):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if has_normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if has_rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields)


def write_ply(path, xyz, rgb=None, normals=None):
    """Binary little-endian PLY of M vertices: float x y z [, float nx ny nz] [, uchar red green blue].  xyz, normals (M,3) float32, rgb
    (M,3) uint8; tensors (any device) or numpy arrays.  M = 0 writes a header-only file."""
    xyz = _host(xyz, np.float32)
    M = xyz.shape[0]
    rgb = None if rgb is None else _host(rgb, np.uint8)
    normals = None if normals is None else _host(normals, np.float32)
    for name, a in (("rgb", rgb), ("normals", normals)):
        if a is not None and a.shape[0] != M:
            raise ValueError(f"diner_amd: write_ply {name} has {a.shape[0]} rows, xyz has {M}")
    dt = _ply_dtype(normals is not None, rgb is not None)
    rec = np.empty(M, dtype=dt)
    for cols, a in ((("x", "y", "z"), xyz), (("nx", "ny", "nz"), normals), (("red", "green", "blue"), rgb)):
        if a is not None:
            for c, name in enumerate(cols):
                rec[name] = a[:, c]
    kinds = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {M}"]
    header += [f"property {kinds[dt.fields[n][0].str]} {n}" for n in dt.names]
    header.append("end_header")
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def read_ply(path):
    """What write_ply wrote -> (xyz (M,3) float32, rgb (M,3) uint8 | None, normals (M,3) float32 | None) as numpy arrays.  Reads that
    subset of the format only: binary little-endian, one vertex element with float and uchar properties."""
    with open(path, "rb") as f:
        head = f.read(PLY_HEADER_MAX)
        end = head.find(b"end_header\n")
        if not head.startswith(b"ply\n") or end < 0:
            raise ValueError(f"diner_amd: {path} is not a PLY file with a header under {PLY_HEADER_MAX} bytes")
        lines = head[:end].decode("ascii").split("\n")
        f.seek(end + len(b"end_header\n"))
        body = f.read()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"diner_amd: {path}: only binary little-endian PLY is read")
    elements = [ln.split() for ln in lines if ln.startswith("element ")]
    if len(elements) != 1 or elements[0][1] != "vertex":
        raise ValueError(f"diner_amd: {path}: expected one vertex element, got {elements}")
    M = int(elements[0][2])
    kinds = {"float": "<f4", "uchar": "u1"}
    props = [ln.split() for ln in lines if ln.startswith("property ")]
    if any(len(p) != 3 or p[1] not in kinds for p in props):
        raise ValueError(f"diner_amd: {path}: only float and uchar properties are read")
    dt = np.dtype([(p[2], kinds[p[1]]) for p in props])
    if len(body) != M * dt.itemsize:
        raise ValueError(f"diner_amd: {path}: {len(body)} bytes of vertex data, expected {M * dt.itemsize}")
    rec = np.frombuffer(body, dtype=dt, count=M)

    def cols(names, dtype):
        if not all(n in dt.names for n in names):
            return None
        return np.stack([rec[n] for n in names], axis=1).astype(dtype, copy=False) if M else np.empty((0, 3), dtype=dtype)

    xyz = cols(("x", "y", "z"), np.float32)
    if xyz is None:
        raise ValueError(f"diner_amd: {path}: no x y z properties")
    return xyz, cols(("red", "green", "blue"), np.uint8), cols(("nx", "ny", "nz"), np.float32)
