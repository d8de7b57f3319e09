"""From depth maps to a triangle mesh: the volumetric half of the geometry chain (diner_amd.geometry stops at point clouds).

    vol = TsdfVolume(origin, voxel, dims, device="cuda")                      # a truncated signed distance volume on the device
    vol.integrate(zdepth, intrinsics, extrinsics, rgb=rgb, carve=True)        # fuse up to 16 z-depth maps per call, call again for more
    mesh = vol.extract()                                                      # Mesh(vertices, normals, rgb_u8, faces)
    write_mesh_ply("scene-mesh.ply", *mesh)

    mesh, vol, views = mesh_from_views(nerf, renderer, Es, Ks, W, H, znear, zfar)   # the model's surface: rendered z-depth of V views
    mesh, vol = mesh_from_sources(batch)                                             # the prior's surface: the source depth maps, no MLP

    maps = vol.raycast(Es, Ks, W, H)                                          # the volume seen by any cameras: zdepth, normal, rgb, ...
    src, vol = sources_through_volume(batch)                                  # view-consistent, hole-filled source depth maps

Fusing, meshing and ray-casting are HIP kernels (ops.tsdf_integrate, ops.surface_extract: surface.hip; ops.tsdf_raycast, ops.tsdf_bricks:
raycast.hip); choosing the box is torch on the device -- once per mesh, not a hot path -- and the PLY writer is numpy on the host."""
import collections

import numpy as np
import torch

from .geometry import PLY_HEADER_MAX, _host, _ply_dtype, _quantize_u8, backproject

Mesh = collections.namedtuple("Mesh", "vertices normals rgb faces")     # (nv,3) f32, (nv,3) f32, (nv,3) u8 | None, (nf,3) i32
TRUNC_VOXELS = 3.0
DEFAULT_CELLS = 256              # voxel=None: the longest side of the box / 256
MAX_VIEWS_PER_CALL = 16


class TsdfVolume:
    """A TSDF volume on a HIP device: sample (i,j,k) at origin + (i,j,k) voxel, dims = (Nx, Ny, Nz), planes (Nz,Ny,Nx).  trunc None:
    TRUNC_VOXELS voxels.  color: keep the four colour planes (sum w r, g, b and sum w) and give the mesh colours."""

    def __init__(self, origin, voxel, dims, trunc=None, color=True, device=None):
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3:
            raise ValueError(f"diner_amd: TsdfVolume dims must be (Nx, Ny, Nz), got {dims}")
        Nx, Ny, Nz = dims
        if not all(2 <= n <= 1024 for n in dims) or Nx * Ny * Nz >= 2 ** 31:
            raise ValueError(f"diner_amd: TsdfVolume takes 2 .. 1024 samples a side and fewer than 2^31 in all, got {dims}")
        self.origin = torch.as_tensor(origin, dtype=torch.float32).detach().to("cpu").reshape(-1).clone()
        if self.origin.numel() != 3:
            raise ValueError(f"diner_amd: TsdfVolume origin holds {self.origin.numel()} values, expected 3")
        self.voxel = float(voxel)
        self.trunc = TRUNC_VOXELS * self.voxel if trunc is None else float(trunc)
        if not (self.voxel > 0.0 and self.trunc > 0.0):
            raise ValueError(f"diner_amd: TsdfVolume voxel {voxel} and trunc {trunc} must be > 0")
        self.dims = dims
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise RuntimeError(f"diner_amd: a TsdfVolume lives on a HIP device, not on {device}; there is no CPU fallback")
        self.tsdf = torch.ones(Nz, Ny, Nx, dtype=torch.float32, device=device)
        self.wsum = torch.zeros(Nz, Ny, Nx, dtype=torch.float32, device=device)
        self.color4 = torch.zeros(4, Nz, Ny, Nx, dtype=torch.float32, device=device) if color else None

    @property
    def device(self):
        return self.tsdf.device

    def reset(self):
        self.tsdf.fill_(1.0)
        self.wsum.zero_()
        if self.color4 is not None:
            self.color4.zero_()

    def integrate(self, zdepth, intrinsics, extrinsics, rgb=None, weight=None, carve=False, max_weight=0.0):
        """Fuse zdepth (N,1,H,W) (camera z, 0 = no surface) seen through intrinsics (N,3,3) or one (3,3) and extrinsics (N,4,4)
        world->camera, in view order; any N (16 views per kernel call).  rgb (N,3,H,W) colours the volume (ignored by a volume without
        colour planes; a coloured volume given no rgb keeps its colour sums); weight (N,1,H,W) per pixel, None = 1; carve: a pixel
        without a surface votes free space along its whole ray; max_weight > 0 caps the accumulated weight."""
        from . import ops
        N = int(zdepth.shape[0])
        if intrinsics.dim() == 2:
            intrinsics = intrinsics[None].expand(N, -1, -1)
        dev = self.device
        zdepth = zdepth.to(dev)
        rgb = None if rgb is None or self.color4 is None else rgb.to(dev)
        weight = None if weight is None else weight.to(dev)
        color4 = None if rgb is None else self.color4
        for a in range(0, N, MAX_VIEWS_PER_CALL):
            b = min(N, a + MAX_VIEWS_PER_CALL)
            ops.tsdf_integrate(self.tsdf, self.wsum, color4, self.origin, self.voxel, self.trunc, zdepth[a:b], intrinsics[a:b],
                               extrinsics[a:b], weight=None if weight is None else weight[a:b], color=None if rgb is None else rgb[a:b],
                               carve=carve, max_weight=max_weight)
        return self

    def integrate_geometry(self, geo, intrinsics, min_alpha=0.5, carve=True):
        """Fuse predict_geometry's maps `geo` (any number of views): a pixel carries a surface iff it is valid and its opacity is at
        least min_alpha; it then weighs alpha.  Every other pixel is empty: depth 0, and weight 1 when carving (0 otherwise)."""
        solid = geo["valid"] & (geo["alpha"] >= float(min_alpha))
        zdepth = torch.where(solid, geo["zdepth"], torch.zeros_like(geo["zdepth"]))
        weight = torch.where(solid, geo["alpha"], torch.full_like(geo["alpha"], 1.0 if carve else 0.0))
        return self.integrate(zdepth, intrinsics, geo["extrinsics"], rgb=geo["rgb"], weight=weight, carve=carve)

    def extract(self, min_weight=0.0):
        """-> Mesh(vertices (nv,3), normals (nv,3) towards free space, rgb (nv,3) uint8 or None, faces (nf,3) int32) on the device."""
        from . import ops
        m = ops.surface_extract(self.tsdf, self.wsum, self.color4, self.origin, self.voxel, min_weight=min_weight)
        return Mesh(m.vertices, m.normals, None if m.rgb is None else _quantize_u8(m.rgb), m.faces)


    def raycast(self, extrinsics, intrinsics, W, H, znear=0.0, zfar=None, step=None, min_weight=0.0, accelerate=True):
        """The volume seen by V cameras (any V; 16 views per kernel call, in view order): extrinsics (V,4,4) world->camera, intrinsics
        (V,3,3) or one (3,3).  zfar None: each camera's distance to the farthest corner of the box; step None: voxel / 2; accelerate:
        build the brick mask once and let the march jump over the bricks no ray can end in (the same bits either way).
        -> dict in predict_geometry's names and layouts: zdepth (V,1,H,W) camera z with 0 = no surface, normal (V,3,H,W) camera frame
        and facing the camera (also under predict_geometry's key "normals"), rgb (V,3,H,W) or None for a volume without colour planes,
        weight (V,1,H,W) the interpolated wsum, valid (V,1,H,W) bool = zdepth > 0, points (V,3,H,W) = backproject(zdepth), extrinsics."""
        from . import ops
        if extrinsics.dim() != 3 or tuple(extrinsics.shape[1:]) != (4, 4) or extrinsics.shape[0] < 1:
            raise ValueError(f"diner_amd: TsdfVolume.raycast expects extrinsics (V,4,4) with V >= 1, got {tuple(extrinsics.shape)}")
        V = int(extrinsics.shape[0])
        if intrinsics.dim() == 2:
            intrinsics = intrinsics[None].expand(V, -1, -1)
        if tuple(intrinsics.shape) != (V, 3, 3):
            raise ValueError(f"diner_amd: TsdfVolume.raycast expects intrinsics ({V},3,3) or (3,3), got {tuple(intrinsics.shape)}")
        E = extrinsics.detach().to("cpu", torch.float32)
        Km = intrinsics.detach().to("cpu", torch.float32)
        step = 0.5 * self.voxel if step is None else float(step)
        if zfar is None:
            hi = self.origin + (torch.tensor(self.dims, dtype=torch.float32) - 1.0) * self.voxel
            box = torch.stack([torch.stack([(self.origin, hi)[(c >> a) & 1][a] for a in range(3)]) for c in range(8)])
            eye = -torch.einsum("vba,vb->va", E[:, :3, :3], E[:, :3, 3])
            zfars = (box[None] - eye[:, None]).norm(dim=-1).max(dim=1).values.tolist()
        else:
            zfars = [float(zfar)] * V
        bricks = ops.tsdf_bricks(self.tsdf, self.wsum, min_weight) if accelerate else None
        parts = []
        for a in range(0, V, MAX_VIEWS_PER_CALL):
            b = min(V, a + MAX_VIEWS_PER_CALL)
            # one zfar a launch: the farthest of its cameras (a longer march changes no hit)
            parts.append(ops.tsdf_raycast(self.tsdf, self.wsum, self.color4, self.origin, self.voxel, Km[a:b], E[a:b], W, H, znear,
                                          max(zfars[a:b]), step, min_weight=min_weight, bricks=bricks))
        zdepth = torch.cat([p.zdepth for p in parts])[:, None]
        normal = torch.cat([p.normal for p in parts])
        dev = self.device
        return {"zdepth": zdepth, "normal": normal, "normals": normal,
                "rgb": None if self.color4 is None else torch.cat([p.rgb for p in parts]),
                "weight": torch.cat([p.weight for p in parts])[:, None], "valid": zdepth > 0,
                "points": backproject(zdepth, Km.to(dev), E.to(dev)), "extrinsics": extrinsics}


def _volume_for(lo, hi, grow, voxel, trunc):
    """The volume that covers the box [lo, hi], grown by the truncation distance on every side if `grow`: -> (origin (3) tensor, voxel,
    dims).  voxel None: the longest side of the (grown) box / DEFAULT_CELLS; trunc None: TRUNC_VOXELS voxels."""
    lo = torch.as_tensor(lo, dtype=torch.float32).reshape(3).cpu().clone()
    hi = torch.as_tensor(hi, dtype=torch.float32).reshape(3).cpu().clone()
    side = float((hi - lo).max())
    if not side > 0.0:
        raise ValueError(f"diner_amd: the box {lo.tolist()} .. {hi.tolist()} is empty")
    if voxel is None:
        if not grow:
            voxel = side / DEFAULT_CELLS
        elif trunc is None:                   # side + 2 TRUNC_VOXELS voxel = DEFAULT_CELLS voxel
            voxel = side / (DEFAULT_CELLS - 2.0 * TRUNC_VOXELS)
        else:
            voxel = (side + 2.0 * float(trunc)) / DEFAULT_CELLS
    voxel = float(voxel)
    if grow:
        t = TRUNC_VOXELS * voxel if trunc is None else float(trunc)
        lo, hi = lo - t, hi + t
    dims = tuple(int(min(1024, max(2, np.ceil(float(s) / voxel) + 1))) for s in (hi - lo))
    return lo, voxel, dims


def _bounds_of(points, mask):
    """points (V,3,H,W), mask (V,1,H,W) bool -> (lo (3), hi (3)) over the masked pixels."""
    p = points.permute(0, 2, 3, 1)[mask[:, 0]]
    if p.shape[0] == 0:
        raise ValueError("diner_amd: the depth maps carry no surface to put a box around")
    return p.min(dim=0).values.cpu(), p.max(dim=0).values.cpu()


@torch.no_grad()
def mesh_from_views(nerf, renderer, extrinsics, intrinsics, W, H, znear, zfar, bounds=None, voxel=None, trunc=None, min_alpha=0.5,
                    carve=True, min_weight=0.0, **predict_kw):
    """fuse_views' sibling: render V target views (extrinsics (V,4,4) world->camera, intrinsics (V,3,3) or one (3,3)) of the encoded
    scene with predict_geometry, fuse their z-depth maps into a TsdfVolume and extract the mesh.  bounds ((3) lo, (3) hi) None: the box
    of the valid `points` grown by trunc; voxel None: the longest side / 256.  -> (Mesh, TsdfVolume, list of the V map dicts).
    predict_kw goes to predict_geometry (ray_batch_size, seed, quantile, ...)."""
    from .render import predict_geometry
    V = int(extrinsics.shape[0])
    if tuple(extrinsics.shape) != (V, 4, 4) or V < 1:
        raise ValueError(f"diner_amd: mesh_from_views expects extrinsics (V,4,4) with V >= 1, got {tuple(extrinsics.shape)}")
    if intrinsics.dim() == 2:
        intrinsics = intrinsics[None].expand(V, -1, -1)
    if tuple(intrinsics.shape) != (V, 3, 3):
        raise ValueError(f"diner_amd: mesh_from_views expects intrinsics ({V},3,3) or (3,3), got {tuple(intrinsics.shape)}")
    if extrinsics.device.type != "cuda":
        raise RuntimeError("diner_amd: mesh_from_views runs on a HIP device; there is no CPU fallback")
    zn = torch.as_tensor(znear, dtype=torch.float32).reshape(-1).expand(V)
    zf = torch.as_tensor(zfar, dtype=torch.float32).reshape(-1).expand(V)
    views = [predict_geometry(nerf, renderer, extrinsics[v:v + 1], intrinsics[v:v + 1], W, H, zn[v:v + 1], zf[v:v + 1], **predict_kw)
             for v in range(V)]
    geo = {k: torch.cat([g[k] for g in views], dim=0) for k in ("rgb", "alpha", "zdepth", "points", "valid", "extrinsics")}
    if bounds is None:
        lo, hi = _bounds_of(geo["points"], geo["valid"] & (geo["alpha"] >= float(min_alpha)))
    else:
        lo, hi = bounds
    origin, voxel, dims = _volume_for(lo, hi, bounds is None, voxel, trunc)
    vol = TsdfVolume(origin, voxel, dims, trunc=trunc, color=True, device=extrinsics.device)
    vol.integrate_geometry(geo, intrinsics, min_alpha=min_alpha, carve=carve)
    return vol.extract(min_weight=min_weight), vol, views


@torch.no_grad()
def mesh_from_sources(batch, sb=0, bounds=None, voxel=None, trunc=None, carve=True, min_weight=0.0, device=None):
    """The prior's surface, no MLP: fuse src_depths (SB,NV,1,H,W) / src_rgbs (SB,NV,3,H,W) / src_intrinsics (SB,NV,3,3) /
    src_extrinsics (SB,NV,4,4) of object `sb` of a collated sample (diner_amd.datasets.collate) and extract the mesh.  bounds None: the
    box of the back-projected depth maps grown by trunc; voxel None: the longest side / 256.  -> (Mesh, TsdfVolume)."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"diner_amd: mesh_from_sources runs on a HIP device, not on {device}; there is no CPU fallback")
    depth = batch["src_depths"][sb].to(device, torch.float32)
    rgb = batch["src_rgbs"][sb].to(device, torch.float32)
    Km, E = batch["src_intrinsics"][sb].to(torch.float32), batch["src_extrinsics"][sb].to(torch.float32)
    if depth.dim() != 4 or depth.shape[1] != 1 or tuple(rgb.shape) != (depth.shape[0], 3) + tuple(depth.shape[2:]):
        raise ValueError(f"diner_amd: mesh_from_sources expects src_depths (SB,NV,1,H,W) and src_rgbs (SB,NV,3,H,W), got "
                         f"{tuple(batch['src_depths'].shape)}, {tuple(batch['src_rgbs'].shape)}")
    if bounds is None:
        lo, hi = _bounds_of(backproject(depth, Km, E), depth > 0)
    else:
        lo, hi = bounds
    origin, voxel, dims = _volume_for(lo, hi, bounds is None, voxel, trunc)
    vol = TsdfVolume(origin, voxel, dims, trunc=trunc, color=True, device=device)
    vol.integrate(depth, Km, E, rgb=rgb, carve=carve)
    return vol.extract(min_weight=min_weight), vol


# ---------------------------------------------------------------------------------------------------------------------------- PLY
def write_mesh_ply(path, vertices, normals=None, rgb=None, faces=None):
    """Binary little-endian PLY of a triangle mesh: write_ply's vertex layout (float x y z [, float nx ny nz] [, uchar red green blue])
    followed by `element face` with `property list uchar int vertex_indices`.  vertices, normals (nv,3) float32, rgb (nv,3) uint8, faces
    (nf,3) int32; tensors (any device) or numpy arrays; the argument order is Mesh's.  0 vertices or 0 faces write empty elements."""
    xyz = _host(vertices, np.float32)
    M = xyz.shape[0]
    rgb = None if rgb is None else _host(rgb, np.uint8)
    normals = None if normals is None else _host(normals, np.float32)
    faces = np.empty((0, 3), np.int32) if faces is None else _host(faces, np.int32)
    for name, a in (("rgb", rgb), ("normals", normals)):
        if a is not None and a.shape[0] != M:
            raise ValueError(f"diner_amd: write_mesh_ply {name} has {a.shape[0]} rows, vertices has {M}")
    if faces.size and (faces.min() < 0 or faces.max() >= M):
        raise ValueError(f"diner_amd: write_mesh_ply faces index outside the {M} vertices")
    dt = _ply_dtype(normals is not None, rgb is not None)
    rec = np.empty(M, dtype=dt)
    for cols, a in ((("x", "y", "z"), xyz), (("nx", "ny", "nz"), normals), (("red", "green", "blue"), rgb)):
        if a is not None:
            for c, name in enumerate(cols):
                rec[name] = a[:, c]
    frec = np.empty(faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    frec["n"] = 3
    frec["v"] = faces
    kinds = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {M}"]
    header += [f"property {kinds[dt.fields[n][0].str]} {n}" for n in dt.names]
    header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())
        f.write(frec.tobytes())


def read_mesh_ply(path):
    """What write_mesh_ply wrote -> Mesh(vertices (nv,3) float32, normals (nv,3) float32 | None, rgb (nv,3) uint8 | None, faces (nf,3)
    int32) as numpy arrays.  Reads that subset of the format only: binary little-endian, a vertex element of float and uchar properties
    followed by a face element of triangles."""
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
    elements = [(n, ln.split()) for n, ln in enumerate(lines) if ln.startswith("element ")]
    if [e[1][1] for e in elements] != ["vertex", "face"]:
        raise ValueError(f"diner_amd: {path}: expected a vertex and a face element, got {[e[1] for e in elements]}")
    M, F = int(elements[0][1][2]), int(elements[1][1][2])
    kinds = {"float": "<f4", "uchar": "u1"}
    props = [ln.split() for ln in lines[elements[0][0] + 1:elements[1][0]] if ln.startswith("property ")]
    if any(len(p) != 3 or p[1] not in kinds for p in props):
        raise ValueError(f"diner_amd: {path}: only float and uchar vertex properties are read")
    if [ln for ln in lines[elements[1][0] + 1:] if ln] != ["property list uchar int vertex_indices"]:
        raise ValueError(f"diner_amd: {path}: the face element must be `property list uchar int vertex_indices`")
    dt = np.dtype([(p[2], kinds[p[1]]) for p in props])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    if len(body) != M * dt.itemsize + F * fdt.itemsize:
        raise ValueError(f"diner_amd: {path}: {len(body)} bytes of data, expected {M * dt.itemsize + F * fdt.itemsize}")
    rec = np.frombuffer(body, dtype=dt, count=M)
    frec = np.frombuffer(body, dtype=fdt, count=F, offset=M * dt.itemsize)
    if F and (frec["n"] != 3).any():
        raise ValueError(f"diner_amd: {path}: only triangles are read")

    def cols(names, dtype):
        if not all(n in dt.names for n in names):
            return None
        return np.stack([rec[n] for n in names], axis=1).astype(dtype, copy=False) if M else np.empty((0, 3), dtype=dtype)

    xyz = cols(("x", "y", "z"), np.float32)
    if xyz is None:
        raise ValueError(f"diner_amd: {path}: no x y z properties")
    return Mesh(xyz, cols(("nx", "ny", "nz"), np.float32), cols(("red", "green", "blue"), np.uint8),
                np.ascontiguousarray(frec["v"]).astype(np.int32, copy=False).reshape(F, 3))


@torch.no_grad()
def sources_through_volume(batch, sb=0, bounds=None, voxel=None, trunc=None, carve=False, min_weight=0.0, device=None):
    """View-consistent, hole-filled source depth maps in the encoder's unit: fuse src_depths / src_rgbs of object `sb` of a collated
    sample as mesh_from_sources does -- but carve=False by default: a hole must not vote free space -- and ray-cast the volume back
    into every source camera.  -> (dict, TsdfVolume); the dict holds src_depths (NV,1,H,W) the cast z-depth (0 = the volume shows no
    surface there), src_normals (NV,3,H,W) camera frame and facing the camera, filled (NV,1,H,W) bool: the original was 0 and the cast
    hit, agree (NV,1,H,W) bool: both are positive and |cast - original| <= trunc.  Feeding them to `encode` is the caller's choice."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"diner_amd: sources_through_volume runs on a HIP device, not on {device}; there is no CPU fallback")
    depth = batch["src_depths"][sb].to(device, torch.float32)
    rgb = batch["src_rgbs"][sb].to(device, torch.float32)
    Km, E = batch["src_intrinsics"][sb].to(torch.float32), batch["src_extrinsics"][sb].to(torch.float32)
    if depth.dim() != 4 or depth.shape[1] != 1 or tuple(rgb.shape) != (depth.shape[0], 3) + tuple(depth.shape[2:]):
        raise ValueError(f"diner_amd: sources_through_volume expects src_depths (SB,NV,1,H,W) and src_rgbs (SB,NV,3,H,W), got "
                         f"{tuple(batch['src_depths'].shape)}, {tuple(batch['src_rgbs'].shape)}")
    if bounds is None:
        lo, hi = _bounds_of(backproject(depth, Km, E), depth > 0)
    else:
        lo, hi = bounds
    origin, voxel, dims = _volume_for(lo, hi, bounds is None, voxel, trunc)
    vol = TsdfVolume(origin, voxel, dims, trunc=trunc, color=True, device=device)
    vol.integrate(depth, Km, E, rgb=rgb, carve=carve)
    H, W = (int(n) for n in depth.shape[-2:])
    cast = vol.raycast(E, Km, W, H, min_weight=min_weight)
    z = cast["zdepth"]
    return {"src_depths": z, "src_normals": cast["normal"], "filled": (depth == 0) & (z > 0),
            "agree": (depth > 0) & (z > 0) & ((z - depth).abs() <= vol.trunc)}, vol
