"""torch-facing wrappers around the C ABI of libdiner_hip.so.

PyTorch is plumbing here: it owns device memory (caching allocator), the stream and (for multi-GPU) the
process group.  Every function takes/returns torch tensors on a HIP device and enqueues kernels on the
current stream.  There is no CPU path and no eager-torch fallback: CPU tensors raise.
"""
import collections
import ctypes as C
import os
import threading

import numpy as np
import torch

from . import _lib

lib = _lib.load()          # ImportError when the extension is not built -- by design

# points per field launch: bounds the 2 KB/point hand-over workspace (2 GiB at the default) without costing throughput
# (a launch of 2^20 points is 64 tiles per CU).  The f16x3 kernels hand over a second plane of the same size, which the library keeps
# per stream (diner_field_release_buffers): + 2 GiB per stream at the default.
MAX_POINTS_PER_LAUNCH = int(os.environ.get("DINER_AMD_MAX_POINTS", 1 << 20))


def _require_hip(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("diner_amd: tensors must live on a HIP device (MI355X); there is no CPU fallback "
                               "for the rendering hot path")
        if t.dtype != torch.float32:
            raise TypeError(f"diner_amd: expected float32, got {t.dtype}")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32c(t):
    return t.detach().to(torch.float32).contiguous()


_const_cache = {}
_const_lock = threading.Lock()


def _t_base(n_cand, device):
    """torch.linspace(0, 1 - 1/n, n): the stratification offsets of sample_coarse (nerf_renderer.py:53-55),
    evaluated by the same torch op the reference uses, then uploaded once."""
    key = ("t_base", n_cand, str(device))
    with _const_lock:
        if key not in _const_cache:
            step = 1.0 / n_cand
            _const_cache[key] = torch.linspace(0, 1 - step, n_cand).to(device)
        return _const_cache[key]


def _std_pad_scale(device):
    """exp(e / 12 * ln 2) for e = 0..99, computed exactly like torch_helpers.py:120."""
    key = ("std_pad", str(device))
    with _const_lock:
        if key not in _const_cache:
            e = torch.arange(100, dtype=torch.float32)
            _const_cache[key] = torch.exp(e / 12 * np.log(2)).to(device)
        return _const_cache[key]


class HipScene:
    """Per-object scene state in the layout the kernels want (DinerScene of include/diner_hip.h).

    latent (NV,C,Hf,Wf) is re-laid-out to channels-last ONCE here (each bilinear tap then is one contiguous
    2 KB read instead of 512 strided 4-byte reads); depth/std/normal maps are used as they are; the three tiny
    camera arrays are kept on the host and travel inside the kernel arguments.
    """

    def __init__(self, latent, depths, depths_std, normals, poses, focal, c, image_shape, feature_padding):
        nv = int(poses.shape[0])
        if not 1 <= nv <= _lib.MAX_VIEWS:          # before any device work: the library takes 1 .. DINER_MAX_VIEWS source views
            raise ValueError(f"diner_amd: a scene has 1 to {_lib.MAX_VIEWS} source views (got {nv}); four run on the fused kernels, "
                             f"any other number on the same kernels in groups of four (or on the generic exact-fp32 path)")
        dev = None
        for t in (latent, depths, depths_std, normals):
            if t is not None:
                _require_hip(t)
                dev = t.device
        if dev is None:
            raise ValueError("HipScene needs at least one map on a HIP device")
        self.device = dev
        self.nv = nv
        self.latent_cl = None
        self.C = self.Hf = self.Wf = 0
        if latent is not None:
            assert latent.dim() == 4 and latent.shape[0] == self.nv
            self.latent_cl = _f32c(latent.permute(0, 2, 3, 1))          # (NV,Hf,Wf,C)
            self.C, self.Hf, self.Wf = int(latent.shape[1]), int(latent.shape[2]), int(latent.shape[3])
        self.depth = _f32c(depths).view(self.nv, *depths.shape[-2:]) if depths is not None else None
        self.depth_std = _f32c(depths_std).view(self.nv, *depths_std.shape[-2:]) if depths_std is not None else None
        self.normals = _f32c(normals) if normals is not None else None
        ref = self.depth if self.depth is not None else (self.depth_std if self.depth_std is not None else self.normals)
        self.Hs, self.Ws = (int(ref.shape[-2]), int(ref.shape[-1])) if ref is not None else (0, 0)
        # tiny camera arrays -> host (one sync per scene, at encode time; never inside a render call)
        self.poses_h = _f32c(poses).cpu().contiguous()
        if self.poses_h.shape[-2:] != (4, 4):
            p44 = torch.eye(4).repeat(self.nv, 1, 1)
            p44[:, :self.poses_h.shape[-2], :] = self.poses_h
            self.poses_h = p44.contiguous()
        self.focal_h = _f32c(focal).cpu().contiguous()
        self.c_h = _f32c(c).cpu().contiguous()
        ish = image_shape.detach().cpu().float()
        self.img_w, self.img_h = float(ish[0]), float(ish[1])
        self.feature_padding = float(feature_padding)
        self.std_pad_scale = _std_pad_scale(dev)
        s = _lib.DinerScene()
        s.latent_cl = self.latent_cl.data_ptr() if self.latent_cl is not None else None
        s.depth = self.depth.data_ptr() if self.depth is not None else None
        s.depth_std = self.depth_std.data_ptr() if self.depth_std is not None else None
        s.normals = self.normals.data_ptr() if self.normals is not None else None
        s.poses_host, s.focal_host, s.c_host = self.poses_h.data_ptr(), self.focal_h.data_ptr(), self.c_h.data_ptr()
        s.std_pad_scale = self.std_pad_scale.data_ptr()
        s.img_w, s.img_h, s.feature_padding = self.img_w, self.img_h, self.feature_padding
        s.nv, s.C, s.Hf, s.Wf, s.Hs, s.Ws = self.nv, self.C, self.Hf, self.Wf, self.Hs, self.Ws
        s.latent_proj = None
        s.latent_proj_f16 = None
        s.proj_stamp = 0
        s.proj_stamp_f16 = 0
        self.struct = s
        self.latent_proj = None
        self.latent_proj_f16 = None
        self._prepared_for = None
        self._f16_current = False

    def prepare(self, mlp, force=False, f16=False):
        """Hoist lin_z[0..2] out of the sample loop: project the channels-last latent once (k_hoist_linz).
        Re-run when the MLP handle changes (the handle itself is rebuilt whenever a parameter changes).  Any view count: a scene with
        other than four views goes through the *_views entries (the maps of all NV views, gathered from group by group).
        f16: also (re)build the fp16 copy of the projected maps that PRECISION_F16 gathers from (+50 % memory, made only when that mode
        is used; one conversion pass per preparation)."""
        if self.latent_cl is None:
            raise RuntimeError("diner_amd: scene has no latent map")
        fresh = force or self._prepared_for is not mlp or self.latent_proj is None
        if fresh:
            with torch.cuda.device(self.device):
                four = self.nv == 4
                if self.latent_proj is None:
                    nbytes = (lib.diner_scene_proj_bytes if four else lib.diner_scene_proj_views_bytes)(self.ref)
                    self.latent_proj = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
                _lib.check((lib.diner_scene_prepare_f32 if four else lib.diner_scene_prepare_views_f32)(
                    self.ref, mlp.handle, _ptr(self.latent_proj), _stream()))
            self.struct.latent_proj = self.latent_proj.data_ptr()
            self.struct.proj_stamp = lib.diner_mlp_stamp(mlp.handle)      # the library refuses these maps with any other handle
            self._prepared_for = mlp
            self._f16_current = False
        if f16 and not self._f16_current:
            with torch.cuda.device(self.device):
                if self.latent_proj_f16 is None:
                    self.latent_proj_f16 = torch.empty(lib.diner_scene_proj_f16_bytes(self.ref) // 2, dtype=torch.float16, device=self.device)
                _lib.check(lib.diner_scene_prepare_f16(self.ref, _ptr(self.latent_proj_f16), _stream()))
            self.struct.latent_proj_f16 = self.latent_proj_f16.data_ptr()
            self.struct.proj_stamp_f16 = self.struct.proj_stamp          # ABI v5: the fp16 copy belongs to the maps of this handle
            self._f16_current = True

    @property
    def ref(self):
        return C.byref(self.struct)


class HipMlp:
    """Packed ResnetFC weights (opaque DinerMlp handle).  Built from a state_dict-like mapping with the
    reference key names (resnetfc.py:72-127); tensors must be on the HIP device."""

    def __init__(self, sd, prefix="", combine_layer=3, d_latent=512, num_freqs=6, freq_factor=6.28, include_input=True):
        self._conf = dict(prefix=prefix, combine_layer=combine_layer, num_freqs=num_freqs, include_input=include_input)
        p = self._params(sd, freq_factor)
        self.device = self._keep["lin_in_w"].device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            # returns once the packing has completed on the stream (the sources may then be freed or updated in place)
            _lib.check(lib.diner_mlp_create(C.byref(p), _stream(), C.byref(h)))
        self.handle = h
        self._range = None

    def _params(self, sd, freq_factor):
        """DinerMlpParams over the tensors of a state_dict-like mapping (kept alive on self until the next call)."""
        prefix, combine_layer = self._conf["prefix"], self._conf["combine_layer"]
        g = lambda k: _f32c(sd[prefix + k])
        n_blocks = len([k for k in sd if k.startswith(prefix + "blocks.") and k.endswith("fc_0.weight")])
        n_z = len([k for k in sd if k.startswith(prefix + "lin_z.") and k.endswith(".weight")])
        keep = {"lin_in_w": g("lin_in.weight"), "lin_in_b": g("lin_in.bias"),
                "lin_out_w": g("lin_out.weight"), "lin_out_b": g("lin_out.bias")}
        lists = {"fc0_w": [g(f"blocks.{i}.fc_0.weight") for i in range(n_blocks)],
                 "fc0_b": [g(f"blocks.{i}.fc_0.bias") for i in range(n_blocks)],
                 "fc1_w": [g(f"blocks.{i}.fc_1.weight") for i in range(n_blocks)],
                 "fc1_b": [g(f"blocks.{i}.fc_1.bias") for i in range(n_blocks)],
                 "lin_z_w": [g(f"lin_z.{i}.weight") for i in range(n_z)],
                 "lin_z_b": [g(f"lin_z.{i}.bias") for i in range(n_z)]}
        for t in list(keep.values()) + [t for l in lists.values() for t in l]:
            _require_hip(t)
        p = _lib.DinerMlpParams()
        p.d_in = keep["lin_in_w"].shape[1]
        p.d_hidden = keep["lin_in_w"].shape[0]
        p.d_out = keep["lin_out_w"].shape[0]
        p.d_latent = lists["lin_z_w"][0].shape[1] if n_z else 0
        p.n_blocks, p.combine_layer = n_blocks, combine_layer
        # the positional encoding that produces the 55 inputs is evaluated inside the field kernels (pixelnerf.py:15-18)
        p.num_freqs, p.include_input, p.freq_factor = int(self._conf["num_freqs"]), int(bool(self._conf["include_input"])), float(freq_factor)
        p.lin_in_w, p.lin_in_b = keep["lin_in_w"].data_ptr(), keep["lin_in_b"].data_ptr()
        p.lin_out_w, p.lin_out_b = keep["lin_out_w"].data_ptr(), keep["lin_out_b"].data_ptr()
        self._arrays = {}
        for name, ts in lists.items():
            arr = (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
            self._arrays[name] = arr
            setattr(p, name, C.cast(arr, C.POINTER(C.c_void_p)))
        self._keep, self._lists = keep, lists
        return p

    def update(self, sd, freq_factor=6.28, train_only=False):
        """New parameter values into this handle (diner_mlp_update, ABI v6): packed on the current stream, no allocation, no host
        synchronisation.  train_only: only what the fused training forward reads -- the handle then serves diner_amd.train alone."""
        p = self._params(sd, freq_factor)
        with torch.cuda.device(self.device):
            _lib.check(lib.diner_mlp_update(self.handle, C.byref(p), _lib.MLP_UPDATE_TRAIN_ONLY if train_only else 0, _stream()))
        self._range = None

    def _weight_range(self):
        # the fp16-operand modes carry the weights x16 as fp16 hi/lo parts: |w| must stay below 1024.  The range was reduced on the
        # device while packing (read back by diner_mlp_create; after update(): here, one stream wait); the library itself falls back
        # to the exact kernels when it does not fit.
        if self._range is None:
            wmax = C.c_float()
            ok = lib.diner_mlp_weights_fit_f16x3(self.handle, C.byref(wmax))
            if ok < 0:
                _lib.check(ok)
            self._range = (ok == 1, float(wmax.value))
        return self._range

    @property
    def h3_ok(self):
        return self._weight_range()[0]

    @property
    def wmax(self):
        return self._weight_range()[1]

    def fallback_launches(self, reset=False):
        """Field launches with this handle that the fp16-operand kernels could not finish (an activation left the fp16 range or an
        input was not finite) and that the gated exact-fp32 kernels recomputed on the device: correct results, 2-3x the time.
        Synchronises the current stream (one 4-byte read back)."""
        n = C.c_longlong()
        with torch.cuda.device(self.device):
            _lib.check(lib.diner_mlp_fallback_count(self.handle, C.byref(n), int(bool(reset)), _stream()))
        return int(n.value)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib.diner_mlp_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def fused_shape(d_in, d_latent, d_hidden, d_out, n_blocks, combine_layer, nv=4, num_freqs=6, include_input=True, beta=0.0):
    """True for the one ResnetFC / PixelNeRF configuration the fused field kernels are built for (every shipped DINER config,
    configs/train_dtu.yaml:39-50); anything else takes the generic slow path (GenericMlp)."""
    return (d_in, d_latent, d_hidden, d_out, n_blocks, combine_layer, nv, int(num_freqs), bool(include_input)) == \
        (55, 512, 512, 4, 5, 3, 4, 6, True) and not beta > 0


def fused_shape_any_views(d_in, d_latent, d_hidden, d_out, n_blocks, combine_layer, nv=4, num_freqs=6, include_input=True, beta=0.0):
    """fused_shape without the view count: the shipped configuration with 1 <= nv <= 16 source views, which the field entries render on
    the fused kernels -- four views directly, any other number in groups of four (the *_views entries of the C ABI)."""
    return fused_shape(d_in, d_latent, d_hidden, d_out, n_blocks, combine_layer, 4, num_freqs, include_input, beta) and \
        1 <= int(nv) <= _lib.MAX_VIEWS


class GenericMlp:
    """ResnetFC parameters for the generic slow path (csrc/generic.hip; ABI v5): ANY configuration the reference's constructor
    accepts (resnetfc.py:72-127) -- d_hidden, n_blocks, combine_layer, d_in / d_latent / d_out, Softplus for beta > 0 -- chained by
    the library on the general exact-fp32 MFMA GEMM, one launch per layer.  No packing: the struct points at the parameter tensors
    (kept alive here)."""

    def __init__(self, sd, prefix="", combine_layer=1000, beta=0.0, num_freqs=6, freq_factor=6.28, include_input=True, d_latent=None):
        g = lambda k: _f32c(sd[prefix + k])
        n_blocks = len([k for k in sd if k.startswith(prefix + "blocks.") and k.endswith("fc_0.weight")])
        n_z = len([k for k in sd if k.startswith(prefix + "lin_z.") and k.endswith(".weight")])
        has_in = prefix + "lin_in.weight" in sd
        self._keep = {"lin_out_w": g("lin_out.weight"), "lin_out_b": g("lin_out.bias")}
        if has_in:
            self._keep.update({"lin_in_w": g("lin_in.weight"), "lin_in_b": g("lin_in.bias")})
        lists = {"fc0_w": [g(f"blocks.{i}.fc_0.weight") for i in range(n_blocks)],
                 "fc0_b": [g(f"blocks.{i}.fc_0.bias") for i in range(n_blocks)],
                 "fc1_w": [g(f"blocks.{i}.fc_1.weight") for i in range(n_blocks)],
                 "fc1_b": [g(f"blocks.{i}.fc_1.bias") for i in range(n_blocks)],
                 "lin_z_w": [g(f"lin_z.{i}.weight") for i in range(n_z)],
                 "lin_z_b": [g(f"lin_z.{i}.bias") for i in range(n_z)]}
        self._lists = lists
        for t in list(self._keep.values()) + [t for l in lists.values() for t in l]:
            _require_hip(t)
        if any(k.startswith(prefix + "blocks.") and ".shortcut." in k for k in sd):
            raise NotImplementedError("diner_amd: ResnetBlockFC shortcut layers (size_in != size_out) do not occur in ResnetFC (resnetfc.py:104)")
        p = _lib.DinerMlpParams()
        p.d_hidden, p.d_out = self._keep["lin_out_w"].shape[1], self._keep["lin_out_w"].shape[0]
        p.d_in = self._keep["lin_in_w"].shape[1] if has_in else 0
        # the latent width is the module's (resnetfc.py:140-142 slices zx by self.d_latent whether or not a lin_z layer exists: combine_layer = 0)
        p.d_latent = int(d_latent) if d_latent is not None else (lists["lin_z_w"][0].shape[1] if n_z else 0)
        p.n_blocks, p.combine_layer = n_blocks, int(min(combine_layer, 2 ** 30))
        p.num_freqs, p.include_input, p.freq_factor = int(num_freqs), int(bool(include_input)), float(freq_factor)
        if has_in:
            p.lin_in_w, p.lin_in_b = self._keep["lin_in_w"].data_ptr(), self._keep["lin_in_b"].data_ptr()
        p.lin_out_w, p.lin_out_b = self._keep["lin_out_w"].data_ptr(), self._keep["lin_out_b"].data_ptr()
        self._arrays = {}
        for name, ts in lists.items():
            arr = (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
            self._arrays[name] = arr
            setattr(p, name, C.cast(arr, C.POINTER(C.c_void_p)))
        self.params = p
        self.beta = float(beta)
        self.device = self._keep["lin_out_w"].device
        self.d_in, self.d_latent, self.d_out, self.d_hidden = p.d_in, p.d_latent, p.d_out, p.d_hidden
        self.combines = 0 <= p.combine_layer < p.n_blocks        # views averaged inside the network
        self.num_freqs, self.include_input, self.freq_factor = int(num_freqs), bool(include_input), float(freq_factor)

    def forward(self, zx):
        """zx (NV, B, d_latent + d_in) -> (B, d_out) when the views are combined inside the network, else (NV, B, d_out)."""
        _require_hip(zx)
        zx = _f32c(zx)
        NV, B, D = zx.shape
        if D != self.d_latent + self.d_in:
            raise ValueError(f"diner_amd: ResnetFC input width {D} != d_latent + d_in = {self.d_latent + self.d_in}")
        out = torch.empty((B, self.d_out) if self.combines else (NV, B, self.d_out), device=zx.device, dtype=torch.float32)
        if B == 0:
            return out
        with torch.cuda.device(zx.device):
            ws = _workspace(lib.diner_mlp_generic_workspace_bytes(C.byref(self.params), NV, B), zx.device)
            _lib.check(lib.diner_mlp_generic_forward_f32(C.byref(self.params), self.beta, _ptr(zx), NV, B, _ptr(out), _ptr(ws), _stream()))
        return out


GENERIC_POINTS_PER_LAUNCH = 1 << 18      # bounds the (NV, P, d_latent + d_in) matrix of the generic path (2.4 GB at NV 4 x 567 floats)


def generic_points_per_launch(nv):
    """Points per generic launch for a scene of nv views: GENERIC_POINTS_PER_LAUNCH up to four views, scaled by 4 / nv above, so that the
    (nv, P, d_row) matrix and the 3 nv P d_hidden floats of MLP workspace stay at the four-view size."""
    return max(1, GENERIC_POINTS_PER_LAUNCH * 4 // max(4, int(nv)))


def field_generic(scene: HipScene, mlp: GenericMlp, rays=None, z=None, xyz=None, viewdirs=None):
    """PixelNeRF.forward on the generic slow path: (rays (NR,8), z (NR,K)) or (xyz, viewdirs) (P,3) -> (P,4) [r, g, b, sigma]
    (sigmoid / relu applied, pixelnerf.py:139-143).  The network must combine its views (combine_layer < n_blocks), as PixelNeRF's does."""
    if not mlp.combines:
        raise NotImplementedError("diner_amd: PixelNeRF needs an MLP that combines its views (combine_layer < n_blocks)")
    per = 2 * mlp.num_freqs + (1 if mlp.include_input else 0)
    if mlp.d_in != 4 * per + 3 or mlp.d_latent != scene.C or mlp.d_out != 4:
        raise ValueError(f"diner_amd: MLP d_in {mlp.d_in} / d_latent {mlp.d_latent} / d_out {mlp.d_out} do not match the positional "
                         f"encoding ({4 * per + 3} inputs), the scene's latent width ({scene.C}) and 4 outputs")
    if rays is not None:
        _require_hip(rays, z)
        rays, z = _f32c(rays), _f32c(z)
        NR, K = z.shape
        P, dev = NR * K, rays.device
    else:
        _require_hip(xyz, viewdirs)
        xyz, viewdirs = _f32c(xyz), _f32c(viewdirs)
        P, K, dev = xyz.shape[0], 1, xyz.device
    out = torch.empty(P, 4, device=dev, dtype=torch.float32)
    if P == 0:
        return out
    D = mlp.d_latent + mlp.d_in
    per_launch = generic_points_per_launch(scene.nv)
    step = per_launch if rays is None else max(1, per_launch // K) * K
    with torch.cuda.device(dev):
        for p0 in range(0, P, step):
            p1 = min(P, p0 + step)
            n = p1 - p0
            zx = torch.empty(scene.nv, n, D, device=dev, dtype=torch.float32)
            if rays is not None:
                r0, r1 = p0 // K, p1 // K
                _lib.check(lib.diner_field_inputs_generic_f32(scene.ref, _ptr(rays[r0:r1]), _ptr(z[r0:r1]), K, None, None, n, mlp.num_freqs,
                                                              int(mlp.include_input), mlp.freq_factor, _ptr(zx), _stream()))
            else:
                _lib.check(lib.diner_field_inputs_generic_f32(scene.ref, None, None, 0, _ptr(xyz[p0:p1]), _ptr(viewdirs[p0:p1]), n,
                                                              mlp.num_freqs, int(mlp.include_input), mlp.freq_factor, _ptr(zx), _stream()))
            raw = mlp.forward(zx)
            _lib.check(lib.diner_field_act_f32(_ptr(raw), None, n, 4, _ptr(out[p0:p1]), _stream()))
    return out


# ---------------------------------------------------------------------------------------------------------
SamplerInfo = collections.namedtuple("SamplerInfo", "z_ordered slot_L slot_idx sum_L sum_O prior_depth prior_std")


def sample_depthguided(scene: HipScene, rays, n_samples, n_candidates, n_gaussian, depth_diff_max=0.05,
                       noise=None, seed=0, want_unfilled=False, ray_index0=0, want_info=False):
    """rays (NR,8) -> ascending z (NR,K) [, unfilled z with zeros].  noise = (coarse, gauss, fill) or None
    (in-kernel Philox keyed by (`seed`, ray_index0 + i): pass the index of rays[0] in the frame's ray list and one seed per
    frame, and the frame does not depend on how its rays are batched or sharded).  The bounded entry: K <= 256,
    n_candidates <= 1024 (sample_depthguided_long: K <= 1024, n_candidates <= 4096).
    want_unfilled: slot order within a ray unspecified.  want_info (instead): -> (z, SamplerInfo) through the info entry -- the same z
    bit for bit; z_ordered (NR,K) the unfilled z in the reference's slot order (picks by descending likelihood, then the gaussian
    samples), slot_L / slot_idx (NR,K-G) likelihood and candidate index of each pick slot (0 / -1: empty), and per ray sum_L, sum_O
    (the depth maps' probability that the ray meets a surface), prior_depth, prior_std (mean and sigma of the gaussian fit; 0 where
    sum_O is 0)."""
    return _sample_depthguided(lib.diner_sample_depthguided_info_f32 if want_info else lib.diner_sample_depthguided_f32, scene, rays,
                               n_samples, n_candidates, n_gaussian, depth_diff_max, noise, seed, want_unfilled, ray_index0, want_info)


def sample_depthguided_long(scene: HipScene, rays, n_samples, n_candidates, n_gaussian, depth_diff_max=0.05,
                            noise=None, seed=0, want_unfilled=False, ray_index0=0, want_info=False):
    """sample_depthguided for K <= 1024 samples and n_candidates <= 4096 (the reference's --nsamples): the same kernel as
    sample_depthguided where it fits (K <= 256, n_candidates <= 1024, bit-identical results), one workgroup per ray above."""
    return _sample_depthguided(lib.diner_sample_depthguided_info_long_f32 if want_info else lib.diner_sample_depthguided_long_f32, scene,
                               rays, n_samples, n_candidates, n_gaussian, depth_diff_max, noise, seed, want_unfilled, ray_index0, want_info)


def _sample_depthguided(entry, scene, rays, n_samples, n_candidates, n_gaussian, depth_diff_max, noise, seed, want_unfilled,
                        ray_index0, want_info=False):
    _require_hip(rays)
    rays = _f32c(rays)
    NR = rays.shape[0]
    K, G = int(n_samples), int(n_gaussian)
    z = torch.empty(NR, K, device=rays.device, dtype=torch.float32)
    zu = torch.empty(NR, K, device=rays.device, dtype=torch.float32) if want_unfilled else None
    if want_info:
        if want_unfilled:
            raise ValueError("diner_amd: want_info delivers z_ordered; want_unfilled belongs to the plain entry -- ask for one of them")
        zo = torch.empty(NR, K, device=rays.device, dtype=torch.float32)
        sl = torch.empty(NR, max(K - G, 0), device=rays.device, dtype=torch.float32)
        si = torch.empty(NR, max(K - G, 0), device=rays.device, dtype=torch.int32)
        st = torch.empty(NR, 4, device=rays.device, dtype=torch.float32)
        info = SamplerInfo(zo, sl, si, st[:, 0], st[:, 1], st[:, 2], st[:, 3])
        outs = (_ptr(z), _ptr(zo), _ptr(sl) if K > G else None, _ptr(si) if K > G else None, _ptr(st))
    else:
        outs = (_ptr(z), _ptr(zu))
    if NR == 0:                     # nothing to do (the C ABI rejects empty launches)
        return (z, info) if want_info else (z, zu) if want_unfilled else z
    nc = ng = nf = None
    if noise is not None:
        nc, ng, nf = (_f32c(t) if t is not None else None for t in noise)
        _require_hip(nc, ng, nf)
        assert nc is None or tuple(nc.shape) == (NR, n_candidates)
        assert ng is None or tuple(ng.shape) == (NR, G)
        assert nf is None or tuple(nf.shape) == (NR, K)
    with torch.cuda.device(rays.device):
        _lib.check(entry(
            scene.ref, _ptr(rays), NR, int(n_candidates), K, G, float(depth_diff_max),
            _ptr(_t_base(int(n_candidates), rays.device)), _ptr(nc), _ptr(ng), _ptr(nf),
            C.c_uint64(int(seed) & (2 ** 64 - 1)), int(ray_index0), *outs, _stream()))
    return (z, info) if want_info else (z, zu) if want_unfilled else z


def fill_uniform(z_in, rays, noise_fill=None, seed=0, ray_index0=0):
    """Stratified fill of the zero slots of z_in (NR,K), K <= 1024 -> ascending z (the bounded kernel for K <= 256)."""
    _require_hip(z_in, rays, noise_fill)
    z_in, rays = _f32c(z_in), _f32c(rays)
    NR, K = z_in.shape
    out = torch.empty_like(z_in)
    if NR == 0:
        return out
    nf = _f32c(noise_fill) if noise_fill is not None else None
    with torch.cuda.device(rays.device):
        _lib.check(lib.diner_fill_uniform_long_f32(_ptr(z_in), _ptr(rays), NR, K, _ptr(nf),
                                                   C.c_uint64(int(seed) & (2 ** 64 - 1)), int(ray_index0), _ptr(out), _stream()))
    return out


def _workspace(nbytes, device):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def field_from_rays(scene: HipScene, mlp: HipMlp, rays, z, precision=None):
    """PixelNeRF.forward at every (ray, sample): (NR,8),(NR,K) -> (NR,K,4) [sigmoid rgb, relu sigma].
    precision: PRECISION_* for this call (default: get_precision())."""
    _require_hip(rays, z)
    rays, z = _f32c(rays), _f32c(z)
    NR, K = z.shape
    prec = _precision_for(scene, precision)
    four = scene.nv == 4              # any other view count: the same kernels over groups of four views
    scene.prepare(mlp, f16=four and prec == PRECISION_F16)
    out = torch.empty(NR, K, 4, device=rays.device, dtype=torch.float32)
    if NR == 0:
        return out
    rays_per = max(1, MAX_POINTS_PER_LAUNCH // K)
    entry = lib.diner_field_from_rays_f32 if four else lib.diner_field_from_rays_views_f32
    with torch.cuda.device(rays.device):
        ws = _workspace((lib.diner_field_workspace_bytes if four else lib.diner_field_views_workspace_bytes)(min(NR, rays_per) * K), rays.device)
        for r0 in range(0, NR, rays_per):
            r1 = min(NR, r0 + rays_per)
            _lib.check(entry(scene.ref, mlp.handle, _ptr(rays[r0:r1]), _ptr(z[r0:r1]),
                             r1 - r0, K, prec, _ptr(out[r0:r1]), _ptr(ws), _stream()))
    return out


def field_from_points(scene: HipScene, mlp: HipMlp, xyz, viewdirs, precision=None):
    """PixelNeRF.forward(xyz, viewdirs): (P,3),(P,3) -> (P,4)."""
    _require_hip(xyz, viewdirs)
    xyz, viewdirs = _f32c(xyz), _f32c(viewdirs)
    P = xyz.shape[0]
    prec = _precision_for(scene, precision)
    four = scene.nv == 4
    scene.prepare(mlp, f16=four and prec == PRECISION_F16)
    out = torch.empty(P, 4, device=xyz.device, dtype=torch.float32)
    if P == 0:
        return out
    step = MAX_POINTS_PER_LAUNCH
    entry = lib.diner_field_from_points_f32 if four else lib.diner_field_from_points_views_f32
    with torch.cuda.device(xyz.device):
        ws = _workspace((lib.diner_field_workspace_bytes if four else lib.diner_field_views_workspace_bytes)(min(P, step)), xyz.device)
        for p0 in range(0, P, step):
            p1 = min(P, p0 + step)
            _lib.check(entry(scene.ref, mlp.handle, _ptr(xyz[p0:p1]), _ptr(viewdirs[p0:p1]),
                             p1 - p0, prec, _ptr(out[p0:p1]), _ptr(ws), _stream()))
    return out


def mlp_forward(mlp: HipMlp, zx):
    """ResnetFC.forward on an explicit (NV,B,567) matrix -> raw (B,4)."""
    _require_hip(zx)
    zx = _f32c(zx)
    NV, B, D = zx.shape
    if NV != 4 or D != 567:
        raise ValueError(f"diner_amd: fused ResnetFC is built for (4, B, 567) inputs, got {tuple(zx.shape)}")
    out = torch.empty(B, 4, device=zx.device, dtype=torch.float32)
    if B == 0:
        return out
    with torch.cuda.device(zx.device):
        ws = _workspace(lib.diner_mlp_forward_workspace_bytes(B), zx.device)
        _lib.check(lib.diner_mlp_forward_f32(mlp.handle, _ptr(zx), B, _ptr(out), _ptr(ws), _stream()))
    return out


def composite(field, z, rays, white_bkgd, want_weights=True, want_aux=False):
    """(NR,K,4),(NR,K),(NR,8) -> weights (NR,K) | None, rgb (NR,3), depth (NR); K <= 1024 (the bounded kernel for K <= 256).
    want_aux: -> weights | None, rgb, depth, alpha (NR), depth_var (NR): the ray's opacity sum_k w_k (pix_alpha of
    nerf_renderer.py:359) and the spread sum_k w_k (z_k - depth)^2 of its samples around `depth`, from the same launch
    (diner_composite_aux_f32); weights, rgb and depth are those of the default call bit for bit."""
    _require_hip(field, z, rays)
    field, z, rays = _f32c(field), _f32c(z), _f32c(rays)
    NR, K = z.shape
    rgb = torch.empty(NR, 3, device=z.device, dtype=torch.float32)
    depth = torch.empty(NR, device=z.device, dtype=torch.float32)
    w = torch.empty(NR, K, device=z.device, dtype=torch.float32) if want_weights else None
    alpha = torch.empty(NR, device=z.device, dtype=torch.float32) if want_aux else None
    var = torch.empty(NR, device=z.device, dtype=torch.float32) if want_aux else None
    if NR > 0:
        with torch.cuda.device(z.device):
            if want_aux:
                _lib.check(lib.diner_composite_aux_f32(_ptr(field), _ptr(z), _ptr(rays), NR, K, int(bool(white_bkgd)),
                                                       _ptr(rgb), _ptr(depth), _ptr(w), _ptr(alpha), _ptr(var), _stream()))
            else:
                _lib.check(lib.diner_composite_long_f32(_ptr(field), _ptr(z), _ptr(rays), NR, K, int(bool(white_bkgd)),
                                                        _ptr(rgb), _ptr(depth), _ptr(w), _stream()))
    return (w, rgb, depth, alpha, var) if want_aux else (w, rgb, depth)


def render(scene: HipScene, mlp: HipMlp, rays, z, white_bkgd, want_weights=False, precision=None, want_aux=False):
    """field + composite (NeRFRendererDGS.composite): -> weights | None, rgb, depth [, alpha, depth_var with want_aux, see composite].
    A HipMlp takes a scene of any view count (four on the fused kernels directly, any other number in groups of four); a GenericMlp
    renders on the generic exact-fp32 path."""
    if isinstance(mlp, GenericMlp):        # a configuration outside the fused kernels: exact fp32, one GEMM launch per layer
        NR, K = z.shape
        field = field_generic(scene, mlp, rays=rays, z=z).view(NR, K, 4)
    else:
        field = field_from_rays(scene, mlp, rays, z, precision=precision)
    return composite(field, z, rays, white_bkgd, want_weights, want_aux)


def sampler_stats(info):
    """The (NR,4) tensor [sum_L, sum_O, prior_depth, prior_std] a SamplerInfo's four per-ray fields are columns of."""
    st = info.sum_O._base
    if st is not None and st.dim() == 2 and st.shape[1] == 4 and st.is_contiguous() and st.data_ptr() == info.sum_L.data_ptr():
        return st
    return torch.stack((info.sum_L, info.sum_O, info.prior_depth, info.prior_std), dim=-1).contiguous()


def compact_live(stats, threshold, rays, z, ray_index0, rays_out, z_out, live_idx, n_live):
    """Empty-ray culling, first half (diner_compact_live_f32): append the LIVE rays of one sampler batch, in ray order, to a frame-level
    list.  stats (NR,4) as the info sampler writes it (sampler_stats(info)) or a SamplerInfo; ray i is live iff
    not (sum_O[i] <= threshold) -- a NaN is live.  rays (NR,8), z (NR,K); rays_out (capacity,8), z_out (capacity,K), live_idx (capacity)
    int32 and the device counter n_live (1) int32 are the caller's frame-level buffers: rows n_live .. n_live + live - 1 are written
    (live_idx: ray_index0 + i), rows at or beyond the capacity are not, and n_live advances by the true live count.
    -> (slot (NR) int32: the row each ray went to, -1 for a dead ray and for one beyond the capacity; n_live, the same device tensor,
    NOT read here).  Enqueue-only; the result is a function of the inputs alone (integer arithmetic, no atomics)."""
    if isinstance(stats, SamplerInfo):
        stats = sampler_stats(stats)
    _require_hip(stats, rays, z, rays_out, z_out)
    stats, rays, z = _f32c(stats), _f32c(rays), _f32c(z)
    NR, K = z.shape
    cap = int(rays_out.shape[0])
    if tuple(stats.shape) != (NR, 4) or tuple(rays.shape) != (NR, 8):
        raise ValueError(f"diner_amd: compact_live expects stats (NR,4), rays (NR,8), z (NR,K), got {tuple(stats.shape)}, {tuple(rays.shape)}, "
                         f"{tuple(z.shape)}")
    if tuple(rays_out.shape) != (cap, 8) or tuple(z_out.shape) != (cap, K) or tuple(live_idx.shape) != (cap,) or n_live.numel() != 1:
        raise ValueError(f"diner_amd: compact_live expects rays_out (capacity,8), z_out (capacity,{K}), live_idx (capacity), n_live (1), got "
                         f"{tuple(rays_out.shape)}, {tuple(z_out.shape)}, {tuple(live_idx.shape)}, {tuple(n_live.shape)}")
    for t in (live_idx, n_live):
        if not t.is_cuda or t.dtype != torch.int32:
            raise TypeError("diner_amd: compact_live expects int32 live_idx and n_live on the HIP device")
    for t in (rays_out, z_out, live_idx, n_live):
        if not t.is_contiguous():
            raise ValueError("diner_amd: compact_live writes into contiguous buffers")
    slot = torch.empty(NR, device=z.device, dtype=torch.int32)
    if NR == 0:
        return slot, n_live
    with torch.cuda.device(z.device):
        ws = _workspace(lib.diner_compact_live_workspace_bytes(NR), z.device)
        _lib.check(lib.diner_compact_live_f32(_ptr(stats), float(threshold), _ptr(rays), _ptr(z), NR, K, int(ray_index0), cap,
                                              _ptr(rays_out), _ptr(z_out), _ptr(live_idx), _ptr(slot), _ptr(n_live), _ptr(ws), _stream()))
    return slot, n_live


def expand_live(tiles, slot, bg, n_tiles=None):
    """Empty-ray culling, second half (diner_expand_live_f32): tiles (n,C) of the live rays, slot (N) int32 as compact_live wrote it,
    bg (C) -> out (N,C) with out[i] = tiles[slot[i]] where 0 <= slot[i] < n_tiles (default: n), else bg.  1 <= C <= 8."""
    _require_hip(tiles, bg)
    tiles, bg = _f32c(tiles), _f32c(bg)
    if not slot.is_cuda or slot.dtype != torch.int32:
        raise TypeError("diner_amd: expand_live expects an int32 slot tensor on the HIP device")
    slot = slot.contiguous()
    N, C_ = int(slot.shape[0]), int(bg.shape[0])
    n = int(tiles.shape[0]) if n_tiles is None else int(n_tiles)
    if tiles.dim() != 2 or tiles.shape[1] != C_ or slot.dim() != 1 or not 0 <= n <= tiles.shape[0]:
        raise ValueError(f"diner_amd: expand_live expects tiles (n,C), slot (N), bg (C), got {tuple(tiles.shape)}, {tuple(slot.shape)}, "
                         f"{tuple(bg.shape)} with n_tiles {n}")
    out = torch.empty(N, C_, device=slot.device, dtype=torch.float32)
    if N == 0:
        return out
    with torch.cuda.device(slot.device):
        _lib.check(lib.diner_expand_live_f32(_ptr(tiles) if n > 0 else None, n, _ptr(slot), _ptr(bg), N, C_, _ptr(out), _stream()))
    return out


def background_row(white_bkgd, n_aux, device):
    """What the compositor returns for a ray of zero density (nerf_renderer.py:349-360 at sigma = 0): rgb 1 with white_bkgd else 0,
    depth 0, then n_aux zeros (alpha, depth_var).  A cached device tensor (uploaded once per configuration)."""
    key = ("bg_row", bool(white_bkgd), int(n_aux), str(device))
    with _const_lock:
        if key not in _const_cache:
            c = 1.0 if white_bkgd else 0.0
            _const_cache[key] = torch.tensor([c, c, c, 0.0] + [0.0] * int(n_aux), dtype=torch.float32).to(device)
        return _const_cache[key]


def posenc(x, num_freqs, freq_factor, include_input=True):
    _require_hip(x)
    shp = x.shape
    xf = _f32c(x).reshape(-1, shp[-1])
    d_out = shp[-1] * (2 * num_freqs + (1 if include_input else 0))
    out = torch.empty(xf.shape[0], d_out, device=x.device, dtype=torch.float32)
    if xf.shape[0] == 0:
        return out.reshape(*shp[:-1], d_out)
    with torch.cuda.device(x.device):
        _lib.check(lib.diner_posenc_f32(_ptr(xf), xf.shape[0], shp[-1], int(num_freqs), float(freq_factor),
                                        int(bool(include_input)), _ptr(out), _stream()))
    return out.reshape(*shp[:-1], d_out)


INDEX_LATENT, INDEX_DEPTH, INDEX_DEPTH_STD, INDEX_NORMAL = 0, 1, 2, 3


def index(scene: HipScene, mode, uv):
    """uv (NV,N,2) -> (NV,Cout,N)."""
    _require_hip(uv)
    uv = _f32c(uv)
    NV, N, _ = uv.shape
    cout = {0: scene.C, 1: 1, 2: 1, 3: 3}[mode]
    out = torch.empty(NV, cout, N, device=uv.device, dtype=torch.float32)
    if N == 0:
        return out
    with torch.cuda.device(uv.device):
        _lib.check(lib.diner_index_f32(scene.ref, int(mode), _ptr(uv), N, _ptr(out), _stream()))
    return out


def depth2normal(dmap, K):
    """Reference src/util/depth2normal.py:7-87 on the device: dmap (N,1,H,W), K (N,3,3) -> normals (N,3,H,W)."""
    _require_hip(dmap, K)
    dmap, K = _f32c(dmap), _f32c(K)
    N, one, H, W = dmap.shape
    if one != 1 or tuple(K.shape) != (N, 3, 3):
        raise ValueError(f"diner_amd: depth2normal expects dmap (N,1,H,W) and K (N,3,3), got {tuple(dmap.shape)}, {tuple(K.shape)}")
    out = torch.empty(N, 3, H, W, device=dmap.device, dtype=torch.float32)
    with torch.cuda.device(dmap.device):
        _lib.check(lib.diner_depth2normal_f32(_ptr(dmap), _ptr(K), N, H, W, _ptr(out), _stream()))
    return out


RayGeometry = collections.namedtuple("RayGeometry", "depth_median median_idx depth_mean zdepth points")
POINT_DEPTH = {"median": 0, "mean": 1}


def _check_ray_geometry_args(weights, z, rays, cam_fwd, quantile, alpha_min, point_depth):
    """The argument checks of ray_geometry that need no device: -> (NR, K, cam_fwd as three host floats or None)."""
    if point_depth not in POINT_DEPTH:
        raise ValueError(f"diner_amd: ray_geometry point_depth must be 'median' or 'mean', got {point_depth!r}")
    if not 0.0 < float(quantile) <= 1.0:
        raise ValueError(f"diner_amd: ray_geometry quantile {quantile} outside (0, 1]")
    if not float(alpha_min) >= 0.0:
        raise ValueError(f"diner_amd: ray_geometry alpha_min {alpha_min} must be >= 0")
    if z.dim() != 2 or tuple(weights.shape) != tuple(z.shape) or tuple(rays.shape) != (z.shape[0], 8):
        raise ValueError(f"diner_amd: ray_geometry expects weights (NR,K), z (NR,K), rays (NR,8), got {tuple(weights.shape)}, "
                         f"{tuple(z.shape)}, {tuple(rays.shape)}")
    NR, K = int(z.shape[0]), int(z.shape[1])
    if not 1 <= K <= 1024:
        raise ValueError(f"diner_amd: ray_geometry K = {K} outside [1, 1024]")
    fwd = None
    if cam_fwd is not None:
        fwd = torch.as_tensor(cam_fwd).detach().to("cpu", torch.float32).reshape(-1)
        if fwd.numel() != 3:
            raise ValueError(f"diner_amd: ray_geometry cam_fwd holds {fwd.numel()} values, expected 3 (row 2 of the world->camera rotation)")
        fwd = (C.c_float * 3)(*fwd.tolist())
    return NR, K, fwd


def ray_geometry(weights, z, rays, cam_fwd=None, quantile=0.5, alpha_min=1e-3, point_depth="median"):
    """Geometry of rendered rays (diner_ray_geometry_f32): weights (NR,K) as composite / render return them with want_weights, the z
    (NR,K) and rays (NR,8) they were given -> RayGeometry(depth_median (NR), median_idx (NR) int32, depth_mean (NR), zdepth (NR) | None,
    points (NR,3)).  With c_k the running sum of the weights in sample order and A = c_{K-1}: a ray is valid iff A > alpha_min;
    median_idx is the first k with c_k >= quantile A, depth_median = z[median_idx], depth_mean = sum_k w_k z_k / A; points = o + t d with
    t the median (point_depth "median") or the mean ("mean"); zdepth = t (d . cam_fwd), the camera-z depth of the point, needs cam_fwd
    (3 values, host or device: row 2 of the target's world->camera rotation) and is None without it.  An invalid ray gets 0 in every
    float output and -1 in median_idx.  No gradient flows through any output."""
    NR, K, fwd = _check_ray_geometry_args(weights, z, rays, cam_fwd, quantile, alpha_min, point_depth)
    _require_hip(weights, z, rays)
    weights, z, rays = _f32c(weights), _f32c(z), _f32c(rays)
    dev = z.device
    d_med = torch.empty(NR, device=dev, dtype=torch.float32)
    idx = torch.empty(NR, device=dev, dtype=torch.int32)
    d_mean = torch.empty(NR, device=dev, dtype=torch.float32)
    zd = torch.empty(NR, device=dev, dtype=torch.float32) if fwd is not None else None
    pts = torch.empty(NR, 3, device=dev, dtype=torch.float32)
    if NR > 0:
        with torch.cuda.device(dev):
            _lib.check(lib.diner_ray_geometry_f32(_ptr(weights), _ptr(z), _ptr(rays), NR, K, float(quantile), float(alpha_min), fwd,
                                                  POINT_DEPTH[point_depth], _ptr(d_med), _ptr(idx), _ptr(d_mean), _ptr(zd), _ptr(pts),
                                                  _stream()))
    return RayGeometry(d_med, idx, d_mean, zd, pts)


def _check_depth_consistency_args(depth, intrinsics, extrinsics, px_thr, rel_thr):
    """The argument checks of depth_consistency that need no device: -> (N, H, W, host intrinsics, host extrinsics)."""
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"diner_amd: depth_consistency expects depth (N,H,W) or (N,1,H,W), got {tuple(depth.shape)}")
    N, H, W = (int(v) for v in depth.shape)
    if not 2 <= N <= _lib.MAX_VIEWS:
        raise ValueError(f"diner_amd: depth_consistency takes 2 .. {_lib.MAX_VIEWS} views, got {N}")
    if tuple(intrinsics.shape) != (N, 3, 3) or tuple(extrinsics.shape) != (N, 4, 4):
        raise ValueError(f"diner_amd: depth_consistency expects intrinsics ({N},3,3) and extrinsics ({N},4,4), got "
                         f"{tuple(intrinsics.shape)}, {tuple(extrinsics.shape)}")
    if not (float(px_thr) >= 0.0 and float(rel_thr) >= 0.0):
        raise ValueError(f"diner_amd: depth_consistency thresholds must be >= 0, got {px_thr}, {rel_thr}")
    Km = intrinsics.detach().to("cpu", torch.float32).contiguous()
    E = extrinsics.detach().to("cpu", torch.float32).contiguous()
    return N, H, W, Km, E


def depth_consistency(depth, intrinsics, extrinsics, px_thr=1.0, rel_thr=0.01):
    """Cross-view consistency of N z-depth maps (diner_depth_consistency_f32): depth (N,H,W) or (N,1,H,W) with 0 = no surface,
    intrinsics (N,3,3), extrinsics (N,4,4) world->camera (read on the host), 2 <= N <= 16 -> count (N,H,W) int32, depth_avg (N,H,W).
    Every pixel of every view is carried into each other view at its depth, that view's depth is sampled there (bilinear; all four
    taps inside and non-zero) and carried back: the pair agrees iff the pixel returns within px_thr pixels and its depth within rel_thr
    relative.  count = the agreeing views, depth_avg = the mean of the pixel's depth and the agreeing views' returned depths; both 0
    where the pixel has no surface.  Pixel centres at +0.5, as gen_rays and depth2normal."""
    N, H, W, Km, E = _check_depth_consistency_args(depth, intrinsics, extrinsics, px_thr, rel_thr)
    _require_hip(depth)
    depth = _f32c(depth).reshape(N, H, W)
    count = torch.empty(N, H, W, device=depth.device, dtype=torch.int32)
    avg = torch.empty(N, H, W, device=depth.device, dtype=torch.float32)
    if H * W > 0:
        with torch.cuda.device(depth.device):
            _lib.check(lib.diner_depth_consistency_f32(_ptr(depth), Km.data_ptr(), E.data_ptr(), N, H, W, float(px_thr), float(rel_thr),
                                                       _ptr(count), _ptr(avg), _stream()))
    return count, avg


SURFACE_MAX_DIM = 1024


def _check_volume(who, tsdf, wsum, color4, origin, voxel):
    """The volume checks of tsdf_integrate / surface_extract that need no device: -> (Nx, Ny, Nz, origin as three host floats)."""
    if tsdf.dim() != 3 or tuple(wsum.shape) != tuple(tsdf.shape):
        raise ValueError(f"diner_amd: {who} expects tsdf and wsum (Nz,Ny,Nx), got {tuple(tsdf.shape)}, {tuple(wsum.shape)}")
    Nz, Ny, Nx = (int(v) for v in tsdf.shape)
    if not all(2 <= n <= SURFACE_MAX_DIM for n in (Nx, Ny, Nz)) or Nx * Ny * Nz >= 2 ** 31:
        raise ValueError(f"diner_amd: {who} takes volumes of 2 .. {SURFACE_MAX_DIM} samples a side and fewer than 2^31 in all, got "
                         f"{(Nz, Ny, Nx)}")
    if color4 is not None and tuple(color4.shape) != (4, Nz, Ny, Nx):
        raise ValueError(f"diner_amd: {who} expects color4 (4,{Nz},{Ny},{Nx}), got {tuple(color4.shape)}")
    o = torch.as_tensor(origin, dtype=torch.float32).detach().to("cpu").reshape(-1)
    if o.numel() != 3:
        raise ValueError(f"diner_amd: {who} origin holds {o.numel()} values, expected 3")
    if not float(voxel) > 0.0:
        raise ValueError(f"diner_amd: {who} voxel size {voxel} must be > 0")
    return Nx, Ny, Nz, (C.c_float * 3)(*o.tolist())


def _require_volume(who, *planes):
    _require_hip(*planes)
    for t in planes:
        if t is not None and not t.is_contiguous():
            raise ValueError(f"diner_amd: {who} works on contiguous volume planes")


def _check_tsdf_integrate_args(tsdf, wsum, color4, origin, voxel, trunc, depth, intrinsics, extrinsics, weight, color):
    """The argument checks of tsdf_integrate that need no device: -> (Nx, Ny, Nz, origin, N, H, W, host intrinsics, host extrinsics)."""
    Nx, Ny, Nz, o = _check_volume("tsdf_integrate", tsdf, wsum, color4, origin, voxel)
    if not float(trunc) > 0.0:
        raise ValueError(f"diner_amd: tsdf_integrate truncation distance {trunc} must be > 0")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"diner_amd: tsdf_integrate expects depth (N,H,W) or (N,1,H,W), got {tuple(depth.shape)}")
    N, H, W = (int(v) for v in depth.shape)
    if not 1 <= N <= _lib.MAX_VIEWS:
        raise ValueError(f"diner_amd: tsdf_integrate takes 1 .. {_lib.MAX_VIEWS} views, got {N}")
    if H < 1 or W < 1:
        raise ValueError(f"diner_amd: tsdf_integrate got empty depth maps {tuple(depth.shape)}")
    if tuple(intrinsics.shape) != (N, 3, 3) or tuple(extrinsics.shape) != (N, 4, 4):
        raise ValueError(f"diner_amd: tsdf_integrate expects intrinsics ({N},3,3) and extrinsics ({N},4,4), got "
                         f"{tuple(intrinsics.shape)}, {tuple(extrinsics.shape)}")
    if weight is not None and weight.numel() != N * H * W:
        raise ValueError(f"diner_amd: tsdf_integrate expects weight ({N},{H},{W}) or ({N},1,{H},{W}), got {tuple(weight.shape)}")
    if color is not None and tuple(color.shape) != (N, 3, H, W):
        raise ValueError(f"diner_amd: tsdf_integrate expects color ({N},3,{H},{W}), got {tuple(color.shape)}")
    if (color is None) != (color4 is None):
        raise ValueError("diner_amd: tsdf_integrate takes color maps and the color4 planes together or not at all")
    Km = intrinsics.detach().to("cpu", torch.float32).contiguous()
    E = extrinsics.detach().to("cpu", torch.float32).contiguous()
    return Nx, Ny, Nz, o, N, H, W, Km, E


def tsdf_integrate(tsdf, wsum, color4, origin, voxel, trunc, depth, intrinsics, extrinsics, weight=None, color=None, carve=False,
                   max_weight=0.0):
    """Fuse N z-depth maps into a TSDF volume IN PLACE (diner_tsdf_integrate_f32, one launch): tsdf, wsum (Nz,Ny,Nx) and color4
    (4,Nz,Ny,Nx) or None, contiguous on the HIP device (fresh: 1, 0, 0); sample (i,j,k) lies at origin + (i,j,k) voxel.  depth (N,H,W)
    or (N,1,H,W) camera-z maps with 0 = no surface, weight the same shape or None (1), color (N,3,H,W) or None -- given iff color4 is;
    intrinsics (N,3,3), extrinsics (N,4,4) world->camera (read on the host), 1 <= N <= 16.  Each voxel is projected into every view in
    order (nearest pixel, centres at +0.5) and takes the running weighted mean of min(1, (D - z) / trunc) where D > 0 and D - z >= -trunc;
    carve: a pixel with D == 0 votes free space (1) along its whole ray.  max_weight > 0 caps wsum.  Returns None."""
    Nx, Ny, Nz, o, N, H, W, Km, E = _check_tsdf_integrate_args(tsdf, wsum, color4, origin, voxel, trunc, depth, intrinsics, extrinsics,
                                                               weight, color)
    _require_volume("tsdf_integrate", tsdf, wsum, color4)
    _require_hip(depth, weight, color)
    depth = _f32c(depth).reshape(N, H, W)
    weight = None if weight is None else _f32c(weight).reshape(N, H, W)
    color = None if color is None else _f32c(color)
    with torch.cuda.device(tsdf.device):
        _lib.check(lib.diner_tsdf_integrate_f32(_ptr(tsdf), _ptr(wsum), _ptr(color4), Nx, Ny, Nz, o, float(voxel), float(trunc), _ptr(depth),
                                                _ptr(weight), _ptr(color), Km.data_ptr(), E.data_ptr(), N, H, W, int(bool(carve)),
                                                float(max_weight), _stream()))


SurfaceMesh = collections.namedtuple("SurfaceMesh", "vertices normals rgb faces")


def surface_extract(tsdf, wsum, color4, origin, voxel, min_weight=0.0):
    """The naive surface nets mesh of a TSDF volume (diner_surface_count + diner_surface_extract_f32): tsdf, wsum (Nz,Ny,Nx), color4
    (4,Nz,Ny,Nx) or None as tsdf_integrate leaves them -> SurfaceMesh(vertices (nv,3), normals (nv,3), rgb (nv,3) float32 in [0, 1] or
    None without color4, faces (2 nq,3) int32).  One vertex per cell whose 8 corners are observed (wsum > min_weight) and of both
    signs, in linear cell order; one quad -- two triangles, wound so that the normal points out of the negative side -- per
    sign-changing grid edge whose four cells are active.  The counts are read back once (8 bytes) to size the outputs: not a hot path."""
    Nx, Ny, Nz, o = _check_volume("surface_extract", tsdf, wsum, color4, origin, voxel)
    _require_volume("surface_extract", tsdf, wsum, color4)
    dev = tsdf.device
    with torch.cuda.device(dev):
        ws = _workspace(lib.diner_surface_workspace_bytes(Nx, Ny, Nz), dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        _lib.check(lib.diner_surface_count(_ptr(tsdf), _ptr(wsum), Nx, Ny, Nz, float(min_weight), _ptr(ws), _ptr(counts), _stream()))
        nv, nq = (int(c) for c in counts.tolist())
        vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        normals = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        rgb = None if color4 is None else torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(2 * nq, 3, dtype=torch.int32, device=dev)
        _lib.check(lib.diner_surface_extract_f32(_ptr(tsdf), _ptr(wsum), _ptr(color4), Nx, Ny, Nz, o, float(voxel), float(min_weight), _ptr(ws),
                                                 nv, nq, _ptr(vertices), _ptr(normals), _ptr(rgb), _ptr(faces), _stream()))
    return SurfaceMesh(vertices, normals, rgb, faces)


RAYCAST_MAX_SAMPLES = 1 << 20
TsdfRaycast = collections.namedtuple("TsdfRaycast", "zdepth normal rgb weight")


def tsdf_bricks(tsdf, wsum, min_weight=0.0):
    """The brick mask of a TSDF volume (diner_tsdf_bricks, one launch): tsdf, wsum (Nz,Ny,Nx) contiguous on the HIP device -> uint8
    (ceil((Nz-1)/8), ceil((Ny-1)/8), ceil((Nx-1)/8)): 1 iff some cell of the brick of 8^3 cells has all 8 corners observed
    (wsum > min_weight) and at least one negative -- the only cells a ray-cast can end in.  For tsdf_raycast(bricks=...) on the same
    planes with the same min_weight."""
    if tsdf.dim() != 3 or tuple(wsum.shape) != tuple(tsdf.shape):
        raise ValueError(f"diner_amd: tsdf_bricks expects tsdf and wsum (Nz,Ny,Nx), got {tuple(tsdf.shape)}, {tuple(wsum.shape)}")
    Nz, Ny, Nx = (int(v) for v in tsdf.shape)
    if not all(2 <= n <= SURFACE_MAX_DIM for n in (Nx, Ny, Nz)) or Nx * Ny * Nz >= 2 ** 31:
        raise ValueError(f"diner_amd: tsdf_bricks takes volumes of 2 .. {SURFACE_MAX_DIM} samples a side and fewer than 2^31 in all, got "
                         f"{(Nz, Ny, Nx)}")
    _require_volume("tsdf_bricks", tsdf, wsum)
    dev = tsdf.device
    with torch.cuda.device(dev):
        bricks = torch.empty((Nz + 6) // 8, (Ny + 6) // 8, (Nx + 6) // 8, dtype=torch.uint8, device=dev)
        assert bricks.numel() == lib.diner_tsdf_bricks_bytes(Nx, Ny, Nz)
        _lib.check(lib.diner_tsdf_bricks(_ptr(tsdf), _ptr(wsum), Nx, Ny, Nz, float(min_weight), _ptr(bricks), _stream()))
    return bricks


def _check_tsdf_raycast_args(tsdf, wsum, color4, origin, voxel, intrinsics, extrinsics, W, H, znear, zfar, step, bricks):
    """The argument checks of tsdf_raycast that need no device: -> (Nx, Ny, Nz, origin, V, host intrinsics, host extrinsics)."""
    Nx, Ny, Nz, o = _check_volume("tsdf_raycast", tsdf, wsum, color4, origin, voxel)
    V = int(extrinsics.shape[0]) if extrinsics.dim() == 3 else -1
    if tuple(extrinsics.shape) != (V, 4, 4) or tuple(intrinsics.shape) != (V, 3, 3):
        raise ValueError(f"diner_amd: tsdf_raycast expects extrinsics (V,4,4) and intrinsics (V,3,3), got {tuple(extrinsics.shape)}, "
                         f"{tuple(intrinsics.shape)}")
    if not 1 <= V <= _lib.MAX_VIEWS:
        raise ValueError(f"diner_amd: tsdf_raycast takes 1 .. {_lib.MAX_VIEWS} views a call, got {V}")
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"diner_amd: tsdf_raycast got an empty image {H} x {W}")
    znear, zfar, step = float(znear), float(zfar), float(step)
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError(f"diner_amd: tsdf_raycast step {step} must be > 0 and finite")
    if not znear >= 0.0:
        raise ValueError(f"diner_amd: tsdf_raycast znear {znear} must be >= 0")
    if not (np.isfinite(zfar) and zfar > znear):
        raise ValueError(f"diner_amd: tsdf_raycast zfar {zfar} must be finite and > znear {znear}")
    if bricks is not None and (bricks.dtype != torch.uint8 or tuple(bricks.shape) != ((Nz + 6) // 8, (Ny + 6) // 8, (Nx + 6) // 8)):
        raise ValueError(f"diner_amd: tsdf_raycast expects bricks uint8 {((Nz + 6) // 8, (Ny + 6) // 8, (Nx + 6) // 8)} (tsdf_bricks), got "
                         f"{bricks.dtype} {tuple(bricks.shape)}")
    Km = intrinsics.detach().to("cpu", torch.float32).contiguous()
    E = extrinsics.detach().to("cpu", torch.float32).contiguous()
    return Nx, Ny, Nz, o, V, Km, E


def tsdf_raycast(tsdf, wsum, color4, origin, voxel, intrinsics, extrinsics, W, H, znear, zfar, step, min_weight=0.0, bricks=None,
                 want_normal=True, want_rgb=True, want_weight=True):
    """Ray-cast a TSDF volume into V cameras (diner_tsdf_raycast_f32, one launch): tsdf, wsum (Nz,Ny,Nx), color4 (4,Nz,Ny,Nx) or None as
    tsdf_integrate leaves them; intrinsics (V,3,3), extrinsics (V,4,4) world->camera (read on the host), 1 <= V <= 16.  Every pixel's ray
    is sampled at camera depths z_n = n step / |d_c| (d_c the pixel's direction with z = 1), znear <= z_n <= zfar, with the trilinear
    interpolant of tsdf; the first observed negative sample ends the march, a hit iff the sample before it was observed too.
    -> TsdfRaycast(zdepth (V,H,W) camera z, 0 = miss; normal (V,3,H,W) camera frame, facing the camera; rgb (V,3,H,W), None without
    color4; weight (V,H,W) the interpolated wsum), each None when not wanted.  bricks: tsdf_bricks of the same planes and min_weight --
    the march jumps over bricks no ray can end in; the outputs are the same bits with and without it."""
    Nx, Ny, Nz, o, V, Km, E = _check_tsdf_raycast_args(tsdf, wsum, color4, origin, voxel, intrinsics, extrinsics, W, H, znear, zfar, step,
                                                       bricks)
    _require_volume("tsdf_raycast", tsdf, wsum, color4)
    if bricks is not None and not (bricks.is_cuda and bricks.is_contiguous()):
        raise RuntimeError("diner_amd: tsdf_raycast expects the brick mask contiguous on the HIP device; there is no CPU fallback")
    dev = tsdf.device
    H, W = int(H), int(W)
    with torch.cuda.device(dev):
        zdepth = torch.empty(V, H, W, dtype=torch.float32, device=dev)
        normal = torch.empty(V, 3, H, W, dtype=torch.float32, device=dev) if want_normal else None
        rgb = torch.empty(V, 3, H, W, dtype=torch.float32, device=dev) if want_rgb and color4 is not None else None
        weight = torch.empty(V, H, W, dtype=torch.float32, device=dev) if want_weight else None
        _lib.check(lib.diner_tsdf_raycast_f32(_ptr(tsdf), _ptr(wsum), _ptr(color4), Nx, Ny, Nz, o, float(voxel), _ptr(bricks), Km.data_ptr(),
                                              E.data_ptr(), V, H, W, float(znear), float(zfar), float(step), float(min_weight),
                                              _ptr(zdepth), _ptr(normal), _ptr(rgb), _ptr(weight), _stream()))
    return TsdfRaycast(zdepth, normal, rgb, weight)


CLOUD_MAX_DIM = 1024
CLOUD_MAX_CELLS = 1 << 26
CLOUD_MAX_THRESHOLDS = 8
CLOUD_REDUCE_OUT = 3 + CLOUD_MAX_THRESHOLDS
# xyz: the target cloud the grid was built over; ws: its workspace; lo: the box corner (3 host floats); order: the target's indices in cell order
CloudGridData = collections.namedtuple("CloudGridData", "xyz ws lo cell dims order")


def _check_cloud(who, name, xyz):
    if not torch.is_tensor(xyz) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"diner_amd: {who} expects {name} (N,3), got {tuple(xyz.shape) if torch.is_tensor(xyz) else type(xyz).__name__}")
    if not 1 <= xyz.shape[0] < 2 ** 31:
        raise ValueError(f"diner_amd: {who} takes 1 .. 2^31 - 1 points, {name} has {xyz.shape[0]}")
    if xyz.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects {name} float32, got {xyz.dtype}")
    return int(xyz.shape[0])


def _check_max_dist(who, max_dist):
    max_dist = float(max_dist)
    if not max_dist > 0.0:
        raise ValueError(f"diner_amd: {who} max_dist {max_dist} must be > 0 (inf: no cap)")
    return max_dist


def _check_cloud_grid_args(xyz_b, lo, cell, dims):
    """The argument checks of cloud_grid that need no device: -> (NB, lo as three host floats, cell, (Gx, Gy, Gz))."""
    NB = _check_cloud("cloud_grid", "xyz_b", xyz_b)
    o = torch.as_tensor(lo, dtype=torch.float32).detach().to("cpu").reshape(-1)
    if o.numel() != 3 or not bool(torch.isfinite(o).all()):
        raise ValueError(f"diner_amd: cloud_grid lo must be three finite values, got {o.tolist()}")
    cell = float(cell)
    if not (cell > 0.0 and np.isfinite(cell)):
        raise ValueError(f"diner_amd: cloud_grid cell size {cell} must be > 0 and finite")
    dims = tuple(int(g) for g in dims)
    if len(dims) != 3 or not all(1 <= g <= CLOUD_MAX_DIM for g in dims) or dims[0] * dims[1] * dims[2] > CLOUD_MAX_CELLS:
        raise ValueError(f"diner_amd: cloud_grid dims (Gx,Gy,Gz) must be 1 .. {CLOUD_MAX_DIM} a side and at most 2^26 cells, got {dims}")
    return NB, (C.c_float * 3)(*o.tolist()), cell, dims


def cloud_grid(xyz_b, lo, cell, dims):
    """A uniform grid over the target cloud xyz_b (NB,3) float32 on the HIP device (diner_cloud_grid_build_f32): a box at `lo` of
    dims = (Gx,Gy,Gz) cubic cells of side `cell`; points outside fall into the outermost cells, points with a non-finite coordinate into
    none.  -> CloudGridData for cloud_nearest; .order (NB,) int32 are the target's indices sorted by cell (a permutation)."""
    NB, o, cell, dims = _check_cloud_grid_args(xyz_b, lo, cell, dims)
    _require_hip(xyz_b)
    xyz_b = xyz_b.detach().contiguous()
    dev = xyz_b.device
    with torch.cuda.device(dev):
        ws = _workspace(lib.diner_cloud_grid_bytes(NB, *dims), dev)
        _lib.check(lib.diner_cloud_grid_build_f32(_ptr(xyz_b), NB, o, cell, *dims, _ptr(ws), _stream()))
    at = lib.diner_cloud_grid_order_offset(NB, *dims)
    return CloudGridData(xyz_b, ws, o, cell, dims, ws[at:at + 4 * NB].view(torch.int32))


def _check_cloud_nearest_args(grid, xyz_a, max_dist, order):
    if not isinstance(grid, CloudGridData):
        raise ValueError(f"diner_amd: cloud_nearest expects the CloudGridData of cloud_grid, got {type(grid).__name__}")
    NA = _check_cloud("cloud_nearest", "xyz_a", xyz_a)
    if order is not None and (not torch.is_tensor(order) or order.dtype != torch.int32 or tuple(order.shape) != (NA,)):
        raise ValueError(f"diner_amd: cloud_nearest expects order int32 ({NA},), a permutation of the queries")
    return NA, _check_max_dist("cloud_nearest", max_dist)


def cloud_nearest(grid, xyz_a, max_dist=float("inf"), order=None):
    """The nearest target point of every query (diner_cloud_nearest_f32, one launch): xyz_a (NA,3) float32 on the grid's device ->
    (d2 (NA,) float32, idx (NA,) int32).  d2 = (dx dx + dy dy) + dz dz in fp32; only targets with d2 <= max_dist^2 (fp32) count; the smaller
    d2 wins, equal d2 the smaller index; nothing within max_dist, or a non-finite query: idx -1, d2 inf.  The result equals exhaustive
    search bit for bit.  order (NA,) int32, a permutation: the order in which the threads take the queries (the .order of a grid over
    xyz_a makes neighbouring threads walk the same cells); it changes no output."""
    NA, max_dist = _check_cloud_nearest_args(grid, xyz_a, max_dist, order)
    _require_hip(xyz_a)
    if xyz_a.device != grid.xyz.device or (order is not None and order.device != grid.xyz.device):
        raise RuntimeError("diner_amd: cloud_nearest expects the queries and their order on the grid's device")
    xyz_a = xyz_a.detach().contiguous()
    order = None if order is None else order.contiguous()
    dev = xyz_a.device
    with torch.cuda.device(dev):
        d2 = torch.empty(NA, dtype=torch.float32, device=dev)
        idx = torch.empty(NA, dtype=torch.int32, device=dev)
        _lib.check(lib.diner_cloud_nearest_f32(_ptr(grid.xyz), grid.xyz.shape[0], grid.lo, grid.cell, *grid.dims, _ptr(grid.ws), _ptr(xyz_a),
                                               NA, _ptr(order), max_dist, _ptr(d2), _ptr(idx), _stream()))
    return d2, idx


def _check_cloud_reduce_args(d2, idx, max_dist, thresholds, normals_a, normals_b):
    if not (torch.is_tensor(d2) and torch.is_tensor(idx)) or d2.dim() != 1 or d2.shape[0] < 1 or tuple(idx.shape) != tuple(d2.shape):
        raise ValueError("diner_amd: cloud_reduce expects d2 (n,) and idx (n,) with n >= 1, as cloud_nearest returns them")
    if d2.dtype != torch.float32 or idx.dtype != torch.int32:
        raise ValueError(f"diner_amd: cloud_reduce expects d2 float32 and idx int32, got {d2.dtype}, {idx.dtype}")
    taus = [float(t) for t in thresholds]
    if len(taus) > CLOUD_MAX_THRESHOLDS or not all(t >= 0.0 for t in taus):
        raise ValueError(f"diner_amd: cloud_reduce takes at most {CLOUD_MAX_THRESHOLDS} thresholds, each >= 0, got {taus}")
    if (normals_a is None) != (normals_b is None):
        raise ValueError("diner_amd: cloud_reduce takes the normals of both clouds or of neither")
    if normals_a is not None:
        if tuple(normals_a.shape) != (d2.shape[0], 3) or normals_b.dim() != 2 or normals_b.shape[1] != 3 or normals_b.shape[0] < 1:
            raise ValueError(f"diner_amd: cloud_reduce expects normals_a ({d2.shape[0]},3) and normals_b (NB,3), got "
                             f"{tuple(normals_a.shape)}, {tuple(normals_b.shape)}")
        if normals_a.dtype != torch.float32 or normals_b.dtype != torch.float32:
            raise ValueError("diner_amd: cloud_reduce expects float32 normals")
    return int(d2.shape[0]), _check_max_dist("cloud_reduce", max_dist), taus


def cloud_reduce(d2, idx, max_dist=float("inf"), thresholds=(), normals_a=None, normals_b=None):
    """The sums of the distance scores over one direction (diner_cloud_reduce_f32): d2, idx (n,) of cloud_nearest -> a (11,) float64
    device tensor {matched, sum of sqrt(d2) in double, sum of |n_a . n_b[idx]|, count with d2 <= tau^2 per threshold}.  An entry is matched
    iff idx >= 0 and d2 <= max_dist^2.  Fixed summation order: two calls give the same bits."""
    n, max_dist, taus = _check_cloud_reduce_args(d2, idx, max_dist, thresholds, normals_a, normals_b)
    _require_hip(d2, normals_a, normals_b)
    if not idx.is_cuda:
        raise RuntimeError("diner_amd: cloud_reduce expects idx on the HIP device; there is no CPU fallback")
    dev = d2.device
    d2, idx = d2.contiguous(), idx.contiguous()
    normals_a = None if normals_a is None else normals_a.detach().contiguous()
    normals_b = None if normals_b is None else normals_b.detach().contiguous()
    t = (C.c_float * CLOUD_MAX_THRESHOLDS)(*taus)
    with torch.cuda.device(dev):
        ws = _workspace(lib.diner_cloud_reduce_workspace_bytes(n), dev)
        out = torch.empty(CLOUD_REDUCE_OUT, dtype=torch.float64, device=dev)
        _lib.check(lib.diner_cloud_reduce_f32(_ptr(d2), _ptr(idx), n, max_dist, t, len(taus), _ptr(normals_a), _ptr(normals_b),
                                              0 if normals_b is None else normals_b.shape[0], _ptr(ws), _ptr(out), _stream()))
    return out


# ---- the 2-D convolution (conv2d.hip): conv3x3 (stride 1) and conv_s2 (stride 2) ----------------------------------------------------------
CONV3X3_CIN_CHUNK = 8            # DINER_CONV3X3_CIN_CHUNK
CONV3X3_COUT_TILE = 64           # DINER_CONV3X3_COUT_TILE
CONV_S2_KERNELS = (1, 3, 7)      # the kernel sizes diner_conv2d_s2_f32 is built for


def _pad_to(n, m):
    return -(-int(n) // m) * m


def _pack_conv2d(who, weight, kernels, Cin=None, transpose=False):
    """A torch Conv2d weight (Cout,Cw,R,R), R in `kernels`, as [ceil(Cin / 8)][ky R + kx][8][Cout rounded up to 64], zeros beyond Cw and
    Cout; transpose: taps flipped, Cin and Cout swapped first."""
    if not torch.is_tensor(weight) or weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in kernels \
            or weight.shape[0] < 1 or weight.shape[1] < 1:
        want = "(Cout,Cin,3,3) weight" if kernels == (3,) else f"(Cout,Cin,R,R) weight with R in {kernels}"
        raise ValueError(f"diner_amd: {who} expects a {want}, got {tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    if weight.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects float32, got {weight.dtype}")
    w = weight.detach()
    if transpose:
        w = w.flip(2, 3).transpose(0, 1)
    Cout, Cw, R = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
    Cin = Cw if Cin is None else int(Cin)
    if Cin < Cw:
        raise ValueError(f"diner_amd: {who}: Cin = {Cin} is less than the weight's {Cw} input channels")
    cp, op = _pad_to(Cin, CONV3X3_CIN_CHUNK), _pad_to(Cout, CONV3X3_COUT_TILE)
    p = w.new_zeros(cp, R * R, op)
    p[:Cw, :, :Cout] = w.reshape(Cout, Cw, R * R).permute(1, 2, 0)
    return p.view(cp // CONV3X3_CIN_CHUNK, CONV3X3_CIN_CHUNK, R * R, op).permute(0, 2, 1, 3).contiguous()


def pack_conv3x3(weight, transpose=False, Cin=None):
    """A torch Conv2d weight (Cout,Cin,3,3) in the layout diner_conv3x3_f32 reads: [ceil(Cin / 8)][tap][8][Cout rounded up to 64], zeros
    beyond Cin and Cout.  transpose: the weight set of the data gradient instead (taps flipped, Cin and Cout swapped).  Cin: pack for that
    many input channels (>= the weight's; the added ones are zero), for an input that encoder_input widened.  Plain torch on the weight's
    own device (done once at load), so it needs no HIP device."""
    return _pack_conv2d("pack_conv3x3", weight, (3,), Cin=Cin, transpose=transpose)


def _check_nhwc(who, name, t, shape=None, min_hw=1):
    """A channels-last activation (N,H,W,C): float32, 4-D, contiguous -> its shape."""
    if not torch.is_tensor(t) or t.dim() != 4:
        raise ValueError(f"diner_amd: {who} expects {name} channels-last (N,H,W,C), got "
                         f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects {name} float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"diner_amd: {who} expects {name} contiguous in (N,H,W,C) order, got strides {t.stride()}")
    if min(t.shape) < 1 or t.shape[1] < min_hw or t.shape[2] < min_hw:
        raise ValueError(f"diner_amd: {who} expects {name} with N, C >= 1 and H, W >= {min_hw}, got {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"diner_amd: {who} expects {name} {tuple(shape)}, got {tuple(t.shape)}")
    return tuple(int(s) for s in t.shape)


def _check_conv2d_args(who, x, wpack, bias, Cout, R, kernels, padded_bias):
    """What conv3x3 and conv_s2 check alike: x, the kernel size, the packed weights for (Cin, Cout, R), the bias (of the packed width, or
    of at least Cout elements) and the image count -> (N, H, W, Cin)."""
    N, H, W, Cin = _check_nhwc(who, "x", x)
    if R not in kernels:
        raise NotImplementedError(f"diner_amd: {who} is built for kernel sizes {kernels}, got {R}")
    want = (_pad_to(Cin, CONV3X3_CIN_CHUNK) // CONV3X3_CIN_CHUNK, R * R, CONV3X3_CIN_CHUNK, _pad_to(max(Cout, 1), CONV3X3_COUT_TILE))
    if Cout < 1 or not torch.is_tensor(wpack) or wpack.dtype != torch.float32 or tuple(wpack.shape) != want or not wpack.is_contiguous():
        raise ValueError(f"diner_amd: {who} expects wpack float32 {want} (pack_{who}) for Cin {Cin}, Cout {Cout}"
                         f"{'' if who == 'conv3x3' else f', R {R}'}, got {tuple(wpack.shape) if torch.is_tensor(wpack) else type(wpack).__name__}")
    if bias is not None:
        ok = torch.is_tensor(bias) and bias.dtype == torch.float32 and bias.dim() == 1 and bias.is_contiguous()
        if padded_bias:
            if not (ok and bias.shape[0] == want[3]):
                raise ValueError(f"diner_amd: {who} expects bias float32 ({want[3]},) (zero-padded to the packed width)")
        elif not (ok and bias.shape[0] >= Cout):
            raise ValueError(f"diner_amd: {who} expects bias float32 with at least Cout = {Cout} elements")
    if N > 65535:
        raise ValueError(f"diner_amd: {who} takes at most 65535 images a call, got {N}")
    return N, H, W, Cin


def _check_conv3x3_args(x, wpack, bias, Cout, addend, mask):
    """The argument checks of conv3x3 that need no device -> (N, H, W, Cin)."""
    Cout = int(Cout)
    N, H, W, Cin = _check_conv2d_args("conv3x3", x, wpack, bias, Cout, 3, (3,), True)
    for name, t in (("addend", addend), ("mask", mask)):
        if t is not None:
            _check_nhwc("conv3x3", name, t, (N, H, W, Cout))
    return N, H, W, Cin


def conv3x3(x, wpack, bias, Cout, relu=False, addend=None, mask=None, out=None):
    """3 x 3 convolution, stride 1, zero padding 1 (diner_conv3x3_f32): x (N,H,W,Cin) channels-last -> (N,H,W,Cout), = conv + bias, then
    + addend, ReLU, and zero where !(mask > 0), each if given.  wpack / bias: pack_conv3x3's layout and the bias zero-padded to its
    width.  With the transposed weight set this is the data gradient; addend and mask are then the loss gradient entering below and the
    saved activation.  out (N,H,W,Cout): write there instead of a new tensor (it may be the addend, not x)."""
    N, H, W, Cin = _check_conv3x3_args(x, wpack, bias, Cout, addend, mask)
    if out is not None:
        _check_nhwc("conv3x3", "out", out, (N, H, W, int(Cout)))
    _require_hip(x, wpack, bias, addend, mask, out)
    dev = x.device
    with torch.cuda.device(dev):
        y = out if out is not None else torch.empty(N, H, W, int(Cout), dtype=torch.float32, device=dev)
        _lib.check(lib.diner_conv3x3_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(addend), _ptr(mask), _ptr(y), N, H, W, Cin, int(Cout),
                                         int(bool(relu)), _stream()))
    return y


def maxpool2(x):
    """torch's MaxPool2d(2, 2) on a channels-last activation (diner_maxpool2_f32): (N,H,W,C) -> (N, H // 2, W // 2, C)."""
    N, H, W, Cc = _check_nhwc("maxpool2", "x", x, min_hw=2)
    _require_hip(x)
    with torch.cuda.device(x.device):
        y = torch.empty(N, H // 2, W // 2, Cc, dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_maxpool2_f32(_ptr(x), _ptr(y), N, H, W, Cc, _stream()))
    return y


def maxpool2_bwd(x, gy, addend=None, relu_mask=False):
    """The adjoint of maxpool2 (diner_maxpool2_bwd_f32): the saved input x (N,H,W,C) and gy (N, H // 2, W // 2, C) -> gx (N,H,W,C); the
    gradient goes to each window's first maximum in row-major order.  Then + addend (N,H,W,C) and zero where !(x > 0) (relu_mask)."""
    N, H, W, Cc = _check_nhwc("maxpool2_bwd", "x", x, min_hw=2)
    _check_nhwc("maxpool2_bwd", "gy", gy, (N, H // 2, W // 2, Cc))
    if addend is not None:
        _check_nhwc("maxpool2_bwd", "addend", addend, (N, H, W, Cc))
    _require_hip(x, gy, addend)
    with torch.cuda.device(x.device):
        gx = torch.empty_like(x)
        _lib.check(lib.diner_maxpool2_bwd_f32(_ptr(x), _ptr(gy), _ptr(addend), int(bool(relu_mask)), _ptr(gx), N, H, W, Cc, _stream()))
    return gx


# ---- the image encoder's trunk (encoder.hip) ---------------------------------------------------------------------------------------------
def pack_conv_s2(weight, Cin=None):
    """A torch Conv2d weight (Cout,Cin,R,R), R in {1, 3, 7}, in the layout diner_conv2d_s2_f32 reads: [ceil(Cin / 8)][ky R + kx][8][Cout
    rounded up to 64], zeros beyond Cin and Cout.  Cin: pack for that many input channels (>= the weight's; the added ones are zero), for
    an input that encoder_input widened.  Plain torch on the weight's own device (done once at load), so it needs no HIP device."""
    return _pack_conv2d("pack_conv_s2", weight, CONV_S2_KERNELS, Cin=Cin)


def conv_s2_out_size(n, R):
    """Output size of a stride-2 convolution with kernel R and zero padding R // 2 along an axis of n pixels."""
    return (int(n) + 2 * (R // 2) - R) // 2 + 1


def _check_conv_s2_args(x, wpack, bias, Cout, R, out, coff):
    """The argument checks of conv_s2 that need no device -> (N, H, W, Cin, Ho, Wo, ldy)."""
    Cout, R, coff = int(Cout), int(R), int(coff)
    N, H, W, Cin = _check_conv2d_args("conv_s2", x, wpack, bias, Cout, R, CONV_S2_KERNELS, False)
    Ho, Wo = conv_s2_out_size(H, R), conv_s2_out_size(W, R)
    ldy = Cout
    if out is not None:
        No, Hy, Wy, ldy = _check_nhwc("conv_s2", "out", out)
        if (No, Hy, Wy) != (N, Ho, Wo) or coff < 0 or coff + Cout > ldy:
            raise ValueError(f"diner_amd: conv_s2 expects out ({N},{Ho},{Wo},>= {coff + Cout}) for channels {coff} .. {coff + Cout - 1}, got "
                             f"{tuple(out.shape)}")
    elif coff != 0:
        raise ValueError("diner_amd: conv_s2: a channel offset needs the output buffer it refers to (out=)")
    return N, H, W, Cin, Ho, Wo, ldy


def conv_s2(x, wpack, bias, Cout, R, relu=False, out=None, coff=0):
    """R x R convolution, stride 2, zero padding R // 2 (diner_conv2d_s2_f32): x (N,H,W,Cin) channels-last -> (N,Ho,Wo,Cout), = conv +
    bias, then ReLU if asked.  out (N,Ho,Wo,C >= coff + Cout): write channels coff .. coff + Cout - 1 of it instead (the rest of it is
    not touched) and return it."""
    N, H, W, Cin, Ho, Wo, ldy = _check_conv_s2_args(x, wpack, bias, Cout, R, out, coff)
    _require_hip(x, wpack, bias, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, Ho, Wo, int(Cout), dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_conv2d_s2_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(y), N, H, W, Cin, int(Cout), int(R), int(bool(relu)), ldy,
                                           int(coff), _stream()))
    return y


def _check_maxpool3s2_args(x, C, out):
    """-> (N, H, W, C, ldx, Ho, Wo); x (N,H,W,ldx) of which channels 0 .. C - 1 are pooled (C None: all)."""
    N, H, W, ldx = _check_nhwc("maxpool3s2", "x", x)
    C = ldx if C is None else int(C)
    if not 1 <= C <= ldx:
        raise ValueError(f"diner_amd: maxpool3s2: C = {C} channels of an input with {ldx}")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is not None:
        _check_nhwc("maxpool3s2", "out", out, (N, Ho, Wo, C))
    return N, H, W, C, ldx, Ho, Wo


def maxpool3s2(x, C=None, out=None):
    """torch's MaxPool2d(3, 2, 1) on a channels-last activation (diner_maxpool3s2_f32): channels 0 .. C - 1 of x (N,H,W,ldx) ->
    (N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)."""
    N, H, W, C, ldx, Ho, Wo = _check_maxpool3s2_args(x, C, out)
    _require_hip(x, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, Ho, Wo, C, dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_maxpool3s2_f32(_ptr(x), _ptr(y), N, H, W, C, ldx, _stream()))
    return y


def _check_encoder_input_args(x, ring, pad, C, out):
    """-> (N, H, W, pad, Cring, C)."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or min(x.shape) < 1:
        raise ValueError(f"diner_amd: encoder_input expects x (N,3,H,W), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"diner_amd: encoder_input expects x float32 and contiguous, got {x.dtype}, strides {x.stride()}")
    N, _, H, W = (int(s) for s in x.shape)
    pad = int(pad)
    if pad < 0:
        raise ValueError(f"diner_amd: encoder_input: pad = {pad}")
    Cring = 0
    if ring is not None:
        if not torch.is_tensor(ring) or ring.dtype != torch.float32 or ring.dim() != 3 or tuple(ring.shape[:2]) != (H + 2 * pad, W + 2 * pad) \
                or ring.shape[2] < 1 or not ring.is_contiguous():
            raise ValueError(f"diner_amd: encoder_input expects ring float32 ({H + 2 * pad},{W + 2 * pad},Cring), got "
                             f"{tuple(ring.shape) if torch.is_tensor(ring) else type(ring).__name__}")
        Cring = int(ring.shape[2])
    C = 3 + Cring if C is None else int(C)
    if C < 3 + Cring:
        raise ValueError(f"diner_amd: encoder_input: C = {C} output channels do not hold 3 + {Cring}")
    if out is not None:
        _check_nhwc("encoder_input", "out", out, (N, H + 2 * pad, W + 2 * pad, C))
    return N, H, W, pad, Cring, C


def encoder_input(x, ring=None, pad=0, C=None, out=None):
    """(N,3,H,W) -> channels-last (N, H + 2 pad, W + 2 pad, C) (diner_encoder_input_f32): the image replication-padded by pad, then the
    channels of ring (H + 2 pad, W + 2 pad, Cring) -- the positional encoding of the padding ring --, then zeros up to C (default
    3 + Cring)."""
    N, H, W, pad, Cring, C = _check_encoder_input_args(x, ring, pad, C, out)
    _require_hip(x, ring, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, H + 2 * pad, W + 2 * pad, C, dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_encoder_input_f32(_ptr(x), _ptr(ring), _ptr(y), N, H, W, pad, Cring, C, _stream()))
    return y


def _check_pyramid_level_args(x, out, c0):
    """-> (N, h, w, c, Hf, Wf, Ctot)."""
    N, h, w, c = _check_nhwc("pyramid_level", "x", x)
    No, Hf, Wf, Ctot = _check_nhwc("pyramid_level", "out", out)
    c0 = int(c0)
    if No != N or c0 < 0 or c0 + c > Ctot:
        raise ValueError(f"diner_amd: pyramid_level expects out ({N},Hf,Wf,>= {c0 + c}) for channels {c0} .. {c0 + c - 1}, got {tuple(out.shape)}")
    return N, h, w, c, Hf, Wf, Ctot


def pyramid_level(x, out, c0):
    """Bilinear align_corners=True resampling of the level x (N,h,w,c) to out's size, written into channels c0 .. c0 + c - 1 of out
    (N,Hf,Wf,Ctot) (diner_pyramid_level_f32); the other channels of out are not touched.  -> out."""
    N, h, w, c, Hf, Wf, Ctot = _check_pyramid_level_args(x, out, c0)
    _require_hip(x, out)
    with torch.cuda.device(x.device):
        _lib.check(lib.diner_pyramid_level_f32(_ptr(x), _ptr(out), N, h, w, c, Hf, Wf, Ctot, int(c0), _stream()))
    return out


def _check_mvs_limits(B, NS, Cf, D, H, W):
    """The limits of diner_mvs_cost_volume_f32: refused, never truncated."""
    if not 1 <= NS <= _lib.MAX_VIEWS - 1:
        raise ValueError(f"diner_amd: mvs_cost_volume takes 1 .. {_lib.MAX_VIEWS - 1} source views, got {NS}")
    if Cf % 4 or not 4 <= Cf <= _lib.MVS_MAX_CHANNELS:
        raise ValueError(f"diner_amd: mvs_cost_volume takes a multiple of 4 channels in [4, {_lib.MVS_MAX_CHANNELS}], got {Cf}")
    if not 1 <= D <= _lib.MVS_MAX_DEPTHS:
        raise ValueError(f"diner_amd: mvs_cost_volume takes 1 .. {_lib.MVS_MAX_DEPTHS} depth hypotheses, got {D}")
    if min(B, H, W) < 1 or B * D * H * W >= 2 ** 31:
        raise ValueError(f"diner_amd: mvs_cost_volume needs B, H, W >= 1 and B D H W < 2^31, got {B} x {D} x {H} x {W}")


def _check_mvs_cost_volume_args(ref_cl, src_cl, proj, depth, pixelwise, view_weights):
    """The argument checks of mvs_cost_volume that need no device (the limits of diner_mvs_cost_volume_f32) -> (B, NS, C, D, H, W)."""
    if ref_cl.dim() != 4 or src_cl.dim() != 5 or depth.dim() != 4:
        raise ValueError(f"diner_amd: mvs_cost_volume expects ref (B,H,W,C), src (NS,B,H,W,C), depth (B,D,H,W), got {tuple(ref_cl.shape)}, "
                         f"{tuple(src_cl.shape)}, {tuple(depth.shape)}")
    B, H, W, Cf = (int(v) for v in ref_cl.shape)
    NS, D = int(src_cl.shape[0]), int(depth.shape[1])
    if tuple(src_cl.shape[1:]) != (B, H, W, Cf) or tuple(depth.shape) != (B, D, H, W) or tuple(proj.shape) != (B, NS + 1, 2, 4, 4):
        raise ValueError(f"diner_amd: mvs_cost_volume shapes disagree: ref {tuple(ref_cl.shape)}, src {tuple(src_cl.shape)}, depth "
                         f"{tuple(depth.shape)}, proj {tuple(proj.shape)}")
    _check_mvs_limits(B, NS, Cf, D, H, W)
    if (pixelwise is None) == (view_weights is None):
        raise ValueError("diner_amd: mvs_cost_volume takes either the folded pixelwise net or the view weights")
    if pixelwise is not None and pixelwise.numel() != _lib.MVS_PIXELWISE_FLOATS:
        raise ValueError(f"diner_amd: the folded pixelwise net has {_lib.MVS_PIXELWISE_FLOATS} floats, got {pixelwise.numel()}")
    if view_weights is not None and tuple(view_weights.shape) != (B, NS, H, W):
        raise ValueError(f"diner_amd: mvs_cost_volume expects view weights ({B},{NS},{H},{W}), got {tuple(view_weights.shape)}")
    return B, NS, Cf, D, H, W


def mvs_cost_volume(ref_cl, src_cl, proj, depth, pixelwise=None, view_weights=None, return_homography=False):
    """diner_mvs_cost_volume_f32: channels-last features ref (B,H,W,C) and src (NS,B,H,W,C), camera pairs proj (B,NS+1,2,4,4), hypotheses
    depth (B,D,H,W) and either the folded pixelwise net (177 floats) or view weights (B,NS,H,W) -> (similarity (B,D,H,W), view weights
    (B,NS,H,W): the computed ones, or the given ones[, the homography (B,NS,12) that mvs_similarity_grad takes])."""
    B, NS, Cf, D, H, W = _check_mvs_cost_volume_args(ref_cl, src_cl, proj, depth, pixelwise, view_weights)
    _require_hip(ref_cl, src_cl, proj, depth, pixelwise, view_weights)
    ref_cl, src_cl, proj, depth = ref_cl.contiguous(), src_cl.contiguous(), proj.contiguous(), depth.contiguous()
    dev = ref_cl.device
    sim = torch.empty(B, D, H, W, device=dev, dtype=torch.float32)
    hom = torch.empty(B, NS, 12, device=dev, dtype=torch.float32)
    if pixelwise is not None:
        pixelwise, vw_in = pixelwise.contiguous(), None
        vw_out = torch.empty(B, NS, H, W, device=dev, dtype=torch.float32)
    else:
        vw_in, vw_out = view_weights.contiguous(), None
    with torch.cuda.device(dev):
        _lib.check(lib.diner_mvs_cost_volume_f32(_ptr(ref_cl), _ptr(src_cl), _ptr(proj), _ptr(depth), _ptr(pixelwise), _ptr(vw_in), _ptr(sim),
                                                 _ptr(vw_out), _ptr(hom), B, NS, Cf, D, H, W, _stream()))
    if return_homography:
        return sim, (vw_out if vw_out is not None else view_weights), hom
    return sim, (vw_out if vw_out is not None else view_weights)


def _check_mvs_similarity_args(ref_cl, src_cl, depth, who="mvs_similarity"):
    """The shape and limit checks the similarity entries share (no device needed) -> (B, NS, C, D, H, W)."""
    if ref_cl.dim() != 4 or src_cl.dim() != 5 or depth.dim() != 4:
        raise ValueError(f"diner_amd: {who} expects ref (B,H,W,C), src (NS,B,H,W,C), depth (B,D,H,W), got {tuple(ref_cl.shape)}, "
                         f"{tuple(src_cl.shape)}, {tuple(depth.shape)}")
    B, H, W, Cf = (int(v) for v in ref_cl.shape)
    NS, D = int(src_cl.shape[0]), int(depth.shape[1])
    if tuple(src_cl.shape[1:]) != (B, H, W, Cf) or tuple(depth.shape) != (B, D, H, W):
        raise ValueError(f"diner_amd: {who} shapes disagree: ref {tuple(ref_cl.shape)}, src {tuple(src_cl.shape)}, depth {tuple(depth.shape)}")
    _check_mvs_limits(B, NS, Cf, D, H, W)
    return B, NS, Cf, D, H, W


def mvs_similarity(ref_cl, src_cl, proj, depth):
    """diner_mvs_similarity_f32: channels-last features ref (B,H,W,C) and src (NS,B,H,W,C), camera pairs proj (B,NS+1,2,4,4), hypotheses
    depth (B,D,H,W) -> (per-view similarity (B,NS,D,H,W), homography (B,NS,12) for mvs_similarity_grad)."""
    B, NS, Cf, D, H, W = _check_mvs_similarity_args(ref_cl, src_cl, depth)
    if tuple(proj.shape) != (B, NS + 1, 2, 4, 4):
        raise ValueError(f"diner_amd: mvs_similarity expects proj ({B},{NS + 1},2,4,4), got {tuple(proj.shape)}")
    _require_hip(ref_cl, src_cl, proj, depth)
    ref_cl, src_cl, proj, depth = ref_cl.contiguous(), src_cl.contiguous(), proj.contiguous(), depth.contiguous()
    dev = ref_cl.device
    sim = torch.empty(B, NS, D, H, W, device=dev, dtype=torch.float32)
    hom = torch.empty(B, NS, 12, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.diner_mvs_similarity_f32(_ptr(ref_cl), _ptr(src_cl), _ptr(proj), _ptr(depth), _ptr(sim), _ptr(hom), B, NS, Cf, D, H, W,
                                                _stream()))
    return sim, hom


def mvs_similarity_grad(ref_cl, src_cl, homography, depth, grad_views=None, grad_aggregated=None, view_weights=None):
    """diner_mvs_similarity_grad_f32: the feature maps and the homography of the forward, and the upstream gradient either per view,
    grad_views (B,NS,D,H,W), or aggregated, grad_aggregated (B,D,H,W) with view_weights (B,NS,H,W)
    -> (d_ref (B,H,W,C), d_src (NS,B,H,W,C)).  d_ref is the same bits on every run; d_src is summed by float atomics."""
    who = "mvs_similarity_grad"
    B, NS, Cf, D, H, W = _check_mvs_similarity_args(ref_cl, src_cl, depth, who)
    if tuple(homography.shape) != (B, NS, 12):
        raise ValueError(f"diner_amd: {who} expects the homography ({B},{NS},12) of the forward, got {tuple(homography.shape)}")
    if (grad_views is None) == (grad_aggregated is None):
        raise ValueError(f"diner_amd: {who} takes either grad_views or grad_aggregated with view_weights")
    if (grad_aggregated is None) != (view_weights is None):
        raise ValueError(f"diner_amd: {who}: view_weights belong to grad_aggregated, and it needs them")
    if grad_views is not None and tuple(grad_views.shape) != (B, NS, D, H, W):
        raise ValueError(f"diner_amd: {who} expects grad_views ({B},{NS},{D},{H},{W}), got {tuple(grad_views.shape)}")
    if grad_aggregated is not None and (tuple(grad_aggregated.shape) != (B, D, H, W) or tuple(view_weights.shape) != (B, NS, H, W)):
        raise ValueError(f"diner_amd: {who} expects grad_aggregated ({B},{D},{H},{W}) and view_weights ({B},{NS},{H},{W}), got "
                         f"{tuple(grad_aggregated.shape)}, {tuple(view_weights.shape)}")
    _require_hip(ref_cl, src_cl, homography, depth, grad_views, grad_aggregated, view_weights)
    c = lambda t: None if t is None else t.contiguous()
    ref_cl, src_cl, homography, depth = c(ref_cl), c(src_cl), c(homography), c(depth)
    grad_views, grad_aggregated, view_weights = c(grad_views), c(grad_aggregated), c(view_weights)
    d_ref, d_src = torch.empty_like(ref_cl), torch.empty_like(src_cl)
    with torch.cuda.device(ref_cl.device):
        _lib.check(lib.diner_mvs_similarity_grad_f32(_ptr(ref_cl), _ptr(src_cl), _ptr(homography), _ptr(depth), _ptr(grad_views),
                                                     _ptr(grad_aggregated), _ptr(view_weights), _ptr(d_ref), _ptr(d_src), B, NS, Cf, D, H, W,
                                                     _stream()))
    return d_ref, d_src


def mvs_select_depth(cost, hypotheses, prob_init=None, return_prob=True):
    """diner_mvs_select_depth_f32: cost (B,D,H,W) [+ prob_init], hypotheses (B,D,H,W) -> (depth (B,H,W), confidence (B,H,W), prob volume
    (B,D,H,W) or None)."""
    if cost.dim() != 4 or tuple(hypotheses.shape) != tuple(cost.shape) or (prob_init is not None and tuple(prob_init.shape) != tuple(cost.shape)):
        raise ValueError(f"diner_amd: mvs_select_depth expects cost, hypotheses [and prob_init] of one shape (B,D,H,W), got {tuple(cost.shape)}, "
                         f"{tuple(hypotheses.shape)}" + ("" if prob_init is None else f", {tuple(prob_init.shape)}"))
    B, D, H, W = (int(v) for v in cost.shape)
    if min(B, D, H, W) < 1 or B * D * H * W >= 2 ** 31:
        raise ValueError(f"diner_amd: mvs_select_depth needs B, D, H, W >= 1 and B D H W < 2^31, got {B} x {D} x {H} x {W}")
    _require_hip(cost, hypotheses, prob_init)
    cost, hypotheses = cost.contiguous(), hypotheses.contiguous()
    prob_init = prob_init.contiguous() if prob_init is not None else None
    depth = torch.empty(B, H, W, device=cost.device, dtype=torch.float32)
    conf = torch.empty_like(depth)
    prob = torch.empty_like(cost) if return_prob else None
    with torch.cuda.device(cost.device):
        _lib.check(lib.diner_mvs_select_depth_f32(_ptr(cost), _ptr(prob_init), _ptr(hypotheses), _ptr(depth), _ptr(conf), _ptr(prob), B, D, H, W,
                                                  _stream()))
    return depth, conf, prob


def _check_mvs_hypotheses_args(cur_depth, ndepth, image_hw, stage_scale):
    """The argument checks of mvs_hypotheses that need no device -> (B, h, w, H, W, scale, D)."""
    if cur_depth.dim() != 3:
        raise ValueError(f"diner_amd: mvs_hypotheses expects the previous stage's depth (B,h,w), got {tuple(cur_depth.shape)}")
    B, h, w = (int(v) for v in cur_depth.shape)
    H, W = (int(v) for v in image_hw)
    s, D = int(stage_scale), int(ndepth)
    if s != stage_scale or s not in (1, 2, 4):
        raise ValueError(f"diner_amd: mvs_hypotheses stage scale must be 1, 2 or 4, got {stage_scale}")
    if not 2 <= D <= _lib.MVS_MAX_DEPTHS:
        raise ValueError(f"diner_amd: mvs_hypotheses takes 2 .. {_lib.MVS_MAX_DEPTHS} depth hypotheses, got {D}")
    if min(B, h, w) < 1 or H < s or W < s or B * D * (H // s) * (W // s) >= 2 ** 31:
        raise ValueError(f"diner_amd: mvs_hypotheses needs B, h, w >= 1, an image of at least {s} x {s} and B D (H / s) (W / s) < 2^31, got "
                         f"depth {B} x {h} x {w}, image {H} x {W}, D {D}")
    return B, h, w, H, W, s, D


def mvs_hypotheses(cur_depth, ndepth, half_range, image_hw, stage_scale):
    """diner_mvs_hypotheses_f32: the previous stage's depth (B,h,w) -> this stage's hypotheses (B, ndepth, H // s, W // s)."""
    B, h, w, H, W, s, D = _check_mvs_hypotheses_args(cur_depth, ndepth, image_hw, stage_scale)
    _require_hip(cur_depth)
    cur_depth = cur_depth.contiguous()
    out = torch.empty(B, D, H // s, W // s, device=cur_depth.device, dtype=torch.float32)
    with torch.cuda.device(cur_depth.device):
        _lib.check(lib.diner_mvs_hypotheses_f32(_ptr(cur_depth), _ptr(out), B, h, w, H, W, s, D, float(half_range), _stream()))
    return out


CONV3D_CIN_CHUNK = 8             # DINER_CONV3D_CIN_CHUNK
CONV3D_COUT_TILE = 16            # DINER_CONV3D_COUT_TILE


def conv3d_cout_pad(Cout):
    """The packed width of diner_conv3d_f32 / diner_deconv3d_s2_f32: one, two or four 16-wide column tiles a workgroup."""
    Cout = int(Cout)
    return 16 if Cout <= 16 else 32 if Cout <= 32 else _pad_to(Cout, 64)


def _pack3d(who, weight, transposed):
    if not torch.is_tensor(weight) or weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or weight.shape[0] < 1 or weight.shape[1] < 1:
        raise ValueError(f"diner_amd: {who} expects a ({'Cin,Cout' if transposed else 'Cout,Cin'},3,3,3) weight, got "
                         f"{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    if weight.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects float32, got {weight.dtype}")
    w = weight.detach()
    if transposed:
        w = w.transpose(0, 1)                    # the gather reads tap k = o + 1 - 2 i as stored: no flip
    Cout, Cin = w.shape[:2]
    cp, op = _pad_to(Cin, CONV3D_CIN_CHUNK), conv3d_cout_pad(Cout)
    p = w.new_zeros(cp, 27, op)
    p[:Cin, :, :Cout] = w.reshape(Cout, Cin, 27).permute(1, 2, 0)
    return p.view(cp // CONV3D_CIN_CHUNK, CONV3D_CIN_CHUNK, 27, op).permute(0, 2, 1, 3).contiguous()


def pack_conv3d(weight):
    """A torch Conv3d weight (Cout,Cin,3,3,3) in the layout diner_conv3d_f32 reads: [ceil(Cin / 8)][tap (kd 3 + kh) 3 + kw][8][CoutPad],
    zeros beyond Cin and Cout, CoutPad = conv3d_cout_pad(Cout).  Plain torch on the weight's own device, so it needs no HIP device."""
    return _pack3d("pack_conv3d", weight, False)


def pack_deconv3d(weight):
    """A torch ConvTranspose3d weight (Cin,Cout,3,3,3) in the layout diner_deconv3d_s2_f32 reads: pack_conv3d's, element
    w[cin][cout][kd][kh][kw] (taps not flipped)."""
    return _pack3d("pack_deconv3d", weight, True)


def _check_ndhwc(who, name, t, shape=None):
    """A channels-last volume (N,D,H,W,C): float32, 5-D, contiguous -> its shape."""
    if not torch.is_tensor(t) or t.dim() != 5:
        raise ValueError(f"diner_amd: {who} expects {name} channels-last (N,D,H,W,C), got "
                         f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects {name} float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"diner_amd: {who} expects {name} contiguous in (N,D,H,W,C) order, got strides {t.stride()}")
    if min(t.shape) < 1:
        raise ValueError(f"diner_amd: {who} expects {name} with every size >= 1, got {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"diner_amd: {who} expects {name} {tuple(shape)}, got {tuple(t.shape)}")
    return tuple(int(s) for s in t.shape)


def _check_conv3d_args(who, x, wpack, bias, Cout, stride, addend, out):
    """The argument checks of conv3d (stride 1 | 2) and deconv3d_s2 (stride None) that need no device -> (N, D, H, W, Cin, output shape)."""
    N, D, H, W, Cin = _check_ndhwc(who, "x", x)
    Cout = int(Cout)
    if stride not in (None, 1, 2):
        raise ValueError(f"diner_amd: {who} stride must be 1 or 2, got {stride}")
    want = (_pad_to(Cin, CONV3D_CIN_CHUNK) // CONV3D_CIN_CHUNK, 27, CONV3D_CIN_CHUNK, conv3d_cout_pad(max(Cout, 1)))
    if Cout < 1 or not torch.is_tensor(wpack) or wpack.dtype != torch.float32 or tuple(wpack.shape) != want or not wpack.is_contiguous():
        raise ValueError(f"diner_amd: {who} expects wpack float32 {want} (pack_{'deconv3d' if stride is None else 'conv3d'}) for Cin {Cin}, "
                         f"Cout {Cout}, got {tuple(wpack.shape) if torch.is_tensor(wpack) else type(wpack).__name__}")
    if bias is not None and (not torch.is_tensor(bias) or bias.dtype != torch.float32 or tuple(bias.shape) != (Cout,) or not bias.is_contiguous()):
        raise ValueError(f"diner_amd: {who} expects bias float32 ({Cout},)")
    if N > 65535:
        raise ValueError(f"diner_amd: {who} takes at most 65535 samples a call, got {N}")
    oshape = (N, 2 * D, 2 * H, 2 * W, Cout) if stride is None else (N,) + tuple((n - 1) // stride + 1 for n in (D, H, W)) + (Cout,)
    for name, t in (("addend", addend), ("out", out)):
        if t is not None:
            _check_ndhwc(who, name, t, oshape)
    return N, D, H, W, Cin, oshape


def conv3d(x, wpack, bias, Cout, stride=1, relu=False, addend=None, out=None):
    """3 x 3 x 3 convolution, stride 1 or 2, zero padding 1 (diner_conv3d_f32): x (N,D,H,W,Cin) channels-last -> (N,Do,Ho,Wo,Cout) with
    (n - 1) // stride + 1 voxels per axis, = conv + bias, then ReLU, then + addend, each if given -- the skip tensor is added AFTER the
    activation, unlike conv3x3.  wpack: pack_conv3d's layout; bias (Cout,) or None.  out: write there instead of a new tensor (it may be
    the addend, not x)."""
    N, D, H, W, Cin, oshape = _check_conv3d_args("conv3d", x, wpack, bias, Cout, stride, addend, out)
    _require_hip(x, wpack, bias, addend, out)
    dev = x.device
    with torch.cuda.device(dev):
        y = out if out is not None else torch.empty(oshape, dtype=torch.float32, device=dev)
        _lib.check(lib.diner_conv3d_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(addend), _ptr(y), N, D, H, W, Cin, int(Cout), int(stride),
                                        int(bool(relu)), _stream()))
    return y


def deconv3d_s2(x, wpack, bias, Cout, relu=False, addend=None, out=None):
    """torch's ConvTranspose3d(3, stride 2, padding 1, output_padding 1) as a gather (diner_deconv3d_s2_f32): x (N,D,H,W,Cin)
    channels-last -> (N, 2 D, 2 H, 2 W, Cout), = deconv + bias, then ReLU, then + addend, each if given.  wpack: pack_deconv3d's layout;
    bias (Cout,) or None.  out: write there instead of a new tensor (it may be the addend, not x)."""
    N, D, H, W, Cin, oshape = _check_conv3d_args("deconv3d_s2", x, wpack, bias, Cout, None, addend, out)
    _require_hip(x, wpack, bias, addend, out)
    dev = x.device
    with torch.cuda.device(dev):
        y = out if out is not None else torch.empty(oshape, dtype=torch.float32, device=dev)
        _lib.check(lib.diner_deconv3d_s2_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(addend), _ptr(y), N, D, H, W, Cin, int(Cout),
                                             int(bool(relu)), _stream()))
    return y


# ---- the depth estimator's feature transformer (fmt.hip) ------------------------------------------------------------------------------
FMT_D_MODEL, FMT_NHEAD, FMT_D_FF, FMT_MAX_HW = 32, 8, 64, 600      # DINER_FMT_*
FMT_STATE_FLOATS, FMT_KV_TOKENS, FMT_PACK_FLOATS = 160, 512, 8544
FPN_MAX_CHANNELS = 64                                              # DINER_FPN_MAX_CHANNELS
# the sixteen tensors of one encoder layer in the pack's order, under the reference's state-dict keys: six matrices, then ten vectors
FMT_LAYER_KEYS = ("attention.query_projection.weight", "attention.key_projection.weight", "attention.value_projection.weight",
                  "attention.out_projection.weight", "linear1.weight", "linear2.weight",
                  "attention.query_projection.bias", "attention.key_projection.bias", "attention.value_projection.bias",
                  "attention.out_projection.bias", "norm1.weight", "norm1.bias", "linear1.bias", "linear2.bias", "norm2.weight", "norm2.bias")
_FMT_LAYER_SHAPES = ((32, 32), (32, 32), (32, 32), (32, 32), (64, 32), (32, 64), (32,), (32,), (32,), (32,), (32,), (32,), (64,), (32,),
                     (32,), (32,))


def fmt_kv_blocks(L):
    """Workgroups (partial sums) an image of L tokens takes in diner_fmt_kv_f32."""
    return -(-int(L) // FMT_KV_TOKENS)


def pack_fmt_layer(state_dict, prefix=""):
    """One encoder layer's sixteen tensors (FMT_LAYER_KEYS under `prefix`) in the layout the kernels read: the six matrices transposed to
    [in][out] -- query, key, value, out projection, linear1, linear2 -- then the ten vectors; FMT_PACK_FLOATS float32.  Plain torch on the
    tensors' own device, so it needs no HIP device."""
    parts = []
    for key, shape in zip(FMT_LAYER_KEYS, _FMT_LAYER_SHAPES):
        if prefix + key not in state_dict:
            raise KeyError(f"diner_amd: pack_fmt_layer misses {prefix + key}")
        t = state_dict[prefix + key]
        if not torch.is_tensor(t) or tuple(t.shape) != shape:
            raise ValueError(f"diner_amd: pack_fmt_layer expects {prefix + key} of shape {shape} (d_model 32, 8 heads, d_ff 64), got "
                             f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"diner_amd: pack_fmt_layer expects float32, got {t.dtype} for {prefix + key}")
        t = t.detach()
        parts.append((t.t() if t.dim() == 2 else t).reshape(-1))
    return torch.cat(parts).contiguous()


def _check_tokens(who, name, t, shape=None):
    """Channels-last tokens (N,L,32): float32, contiguous -> (N, L)."""
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != FMT_D_MODEL:
        raise ValueError(f"diner_amd: {who} expects {name} tokens (N,L,{FMT_D_MODEL}), got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"diner_amd: {who} expects {name} float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"diner_amd: {who} expects {name} contiguous, got strides {t.stride()}")
    N, L = int(t.shape[0]), int(t.shape[1])
    if not (1 <= N <= 65535 and 1 <= L <= FMT_MAX_HW * FMT_MAX_HW):
        raise ValueError(f"diner_amd: {who} expects 1 <= N <= 65535 images of 1 <= L <= {FMT_MAX_HW * FMT_MAX_HW} tokens, got {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"diner_amd: {who} expects {name} {tuple(shape)}, got {tuple(t.shape)}")
    return N, L


def _check_fmt_pack(who, pack):
    if not torch.is_tensor(pack) or pack.dtype != torch.float32 or tuple(pack.shape) != (FMT_PACK_FLOATS,) or not pack.is_contiguous():
        raise ValueError(f"diner_amd: {who} expects pack float32 ({FMT_PACK_FLOATS},) (pack_fmt_layer), got "
                         f"{tuple(pack.shape) if torch.is_tensor(pack) else type(pack).__name__}")


def _check_fmt_tokenise_args(x, pe, out=None):
    """-> (N, H, W)."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != FMT_D_MODEL:
        raise ValueError(f"diner_amd: fmt_tokenise expects x (N,{FMT_D_MODEL},H,W), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if not torch.is_tensor(pe) or pe.dim() != 3 or pe.shape[0] != FMT_D_MODEL or max(pe.shape[1:]) > FMT_MAX_HW:
        raise ValueError(f"diner_amd: fmt_tokenise expects pe ({FMT_D_MODEL},h,w) with h, w <= {FMT_MAX_HW}, got "
                         f"{tuple(pe.shape) if torch.is_tensor(pe) else type(pe).__name__}")
    for name, t in (("x", x), ("pe", pe)):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"diner_amd: fmt_tokenise expects {name} float32 and contiguous, got {t.dtype}, strides {t.stride()}")
    N, _, H, W = (int(s) for s in x.shape)
    if not (1 <= N <= 65535 and 1 <= H <= pe.shape[1] and 1 <= W <= pe.shape[2]):
        raise ValueError(f"diner_amd: fmt_tokenise expects 1 <= N <= 65535 and a map within the positional encoding's {tuple(pe.shape[1:])} "
                         f"(at most {FMT_MAX_HW} a side), got {tuple(x.shape)}")
    if out is not None:
        _check_tokens("fmt_tokenise", "out", out, (N, H * W, FMT_D_MODEL))
    return N, H, W


def fmt_tokenise(x, pe, out=None):
    """(N,32,H,W) NCHW + the top-left H x W of the positional encoding pe (32,h,w) -> tokens (N, H W, 32) (diner_fmt_tokenise_f32)."""
    N, H, W = _check_fmt_tokenise_args(x, pe, out)
    _require_hip(x, pe, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, H * W, FMT_D_MODEL, dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_fmt_tokenise_f32(_ptr(x), _ptr(pe), _ptr(y), N, FMT_D_MODEL, H, W, int(pe.shape[1]), int(pe.shape[2]), _stream()))
    return y


def _check_fmt_kv_args(src, pack, partials=None, out=None):
    """-> (N, L, partial blocks)."""
    N, L = _check_tokens("fmt_kv", "src", src)
    _check_fmt_pack("fmt_kv", pack)
    nblk = fmt_kv_blocks(L)
    if partials is not None and (not torch.is_tensor(partials) or partials.dtype != torch.float64 or not partials.is_contiguous()
                                 or partials.numel() < N * nblk * FMT_STATE_FLOATS):
        raise ValueError(f"diner_amd: fmt_kv expects partials float64, contiguous, of at least {N * nblk * FMT_STATE_FLOATS} elements")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (N, FMT_STATE_FLOATS)
                            or not out.is_contiguous()):
        raise ValueError(f"diner_amd: fmt_kv expects out float32 ({N},{FMT_STATE_FLOATS}), contiguous")
    return N, L, nblk


def fmt_kv(src, pack, partials=None, out=None):
    """The attention state of the source tokens src (N,L,32) under a layer pack's key and value projections -> (N,160): per head
    KV[m][d] (128 floats as [h][m][d]), then Ksum[h][d] (diner_fmt_kv_f32).  partials: float64 workspace of N x fmt_kv_blocks(L) x 160."""
    N, L, nblk = _check_fmt_kv_args(src, pack, partials, out)
    _require_hip(src, pack, out)
    if partials is not None and not partials.is_cuda:
        raise RuntimeError("diner_amd: tensors must live on a HIP device (MI355X); there is no CPU fallback")
    with torch.cuda.device(src.device):
        if partials is None:
            partials = torch.empty(N * nblk * FMT_STATE_FLOATS, dtype=torch.float64, device=src.device)
        state = out if out is not None else torch.empty(N, FMT_STATE_FLOATS, dtype=torch.float32, device=src.device)
        _lib.check(lib.diner_fmt_kv_f32(_ptr(src), _ptr(pack), _ptr(partials), _ptr(state), N, L, _stream()))
    return state


def _check_fmt_layer_args(x, pack, state, out=None):
    """-> (N, L, rows of state)."""
    N, L = _check_tokens("fmt_layer", "x", x)
    _check_fmt_pack("fmt_layer", pack)
    if not torch.is_tensor(state) or state.dtype != torch.float32 or state.dim() != 2 or state.shape[1] != FMT_STATE_FLOATS \
            or not state.is_contiguous() or state.shape[0] < 1 or N % state.shape[0] != 0:
        raise ValueError(f"diner_amd: fmt_layer expects state float32 (R,{FMT_STATE_FLOATS}), contiguous, R a divisor of N = {N}, got "
                         f"{tuple(state.shape) if torch.is_tensor(state) else type(state).__name__}")
    if out is not None:
        _check_tokens("fmt_layer", "out", out, (N, L, FMT_D_MODEL))
    return N, L, int(state.shape[0])


def fmt_layer(x, pack, state, out=None):
    """One encoder layer on the tokens x (N,L,32) with the attention state (R,160) of fmt_kv: image n reads row n mod R -- R = N for a
    self layer, R = the batch size for a cross layer on view-major images (diner_fmt_layer_f32).  out may be x."""
    N, L, R = _check_fmt_layer_args(x, pack, state, out)
    _require_hip(x, pack, state, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty_like(x)
        _lib.check(lib.diner_fmt_layer_f32(_ptr(x), _ptr(pack), _ptr(state), _ptr(y), N, L, R, _stream()))
    return y


FMT_GRAD_TOKENS, FMT_GRAD_QUERY_SLAB_FLOATS, FMT_GRAD_SOURCE_SLAB_FLOATS, FMT_GRAD_MAX_SLABS = 128, 6432, 2112, 1024      # DINER_FMT_GRAD_*


def fmt_grad_slabs(N, L, R, S, slabs=0):
    """(query side, source side): the per-workgroup slabs the parameter gradients are added from -- a function of the shape alone, or the
    caller's `slabs`; a tile is FMT_GRAD_TOKENS tokens of one image."""
    want = int(slabs) if slabs else 128
    return min(int(N) * -(-int(L) // FMT_GRAD_TOKENS), want), min(int(R) * -(-int(S) // FMT_GRAD_TOKENS), want)


def fmt_grad_workspace_floats(N, L, R, S, slabs=0):
    """diner_fmt_layer_grad_workspace_floats on the host: the tiles' shares of d_state as doubles, d_state, then per side the slabs and
    their carries."""
    sq, ss = fmt_grad_slabs(N, L, R, S, slabs)
    return (2 * int(N) * -(-int(L) // FMT_GRAD_TOKENS) * FMT_STATE_FLOATS + int(R) * FMT_STATE_FLOATS
            + 2 * (sq * FMT_GRAD_QUERY_SLAB_FLOATS + ss * FMT_GRAD_SOURCE_SLAB_FLOATS))


def _check_fmt_layer_grad_args(x, source, pack, state, dy, want=(True, True, True), slabs=0):
    """The argument checks of fmt_layer_grad that need no device -> (N, L, R, S, self layer)."""
    N, L = _check_tokens("fmt_layer_grad", "x", x)
    R, S = _check_tokens("fmt_layer_grad", "source", source)
    _check_tokens("fmt_layer_grad", "dy", dy, (N, L, FMT_D_MODEL))
    _check_fmt_pack("fmt_layer_grad", pack)
    if N % R:
        raise ValueError(f"diner_amd: fmt_layer_grad expects the source's {R} images to divide x's {N} (image n reads row n mod R)")
    if not torch.is_tensor(state) or state.dtype != torch.float32 or tuple(state.shape) != (R, FMT_STATE_FLOATS) or not state.is_contiguous():
        raise ValueError(f"diner_amd: fmt_layer_grad expects state float32 ({R},{FMT_STATE_FLOATS}), contiguous (fmt_kv of the source), got "
                         f"{tuple(state.shape) if torch.is_tensor(state) else type(state).__name__}")
    if len(tuple(want)) != 3:
        raise ValueError("diner_amd: fmt_layer_grad expects want = (d_x, d_source, parameters) as three flags")
    if isinstance(slabs, bool) or not isinstance(slabs, int) or not 0 <= slabs <= FMT_GRAD_MAX_SLABS:
        raise ValueError(f"diner_amd: fmt_layer_grad expects slabs an int in [0, {FMT_GRAD_MAX_SLABS}] (0: the default), got {slabs!r}")
    return N, L, R, S, source is x


def fmt_layer_grad(x, source, pack, state, dy, want=(True, True, True), slabs=0):
    """The backward pass of fmt_layer(x, pack, fmt_kv(source, pack)) (diner_fmt_layer_grad_f32): x (N,L,32), source (R,S,32) with R a
    divisor of N, state (R,160) the forward's, dy (N,L,32) -> (d_x (N,L,32), d_source (R,S,32), d_params (8544,) in the pack's order with
    the matrices as torch keeps them, (out, in)); an output whose `want` flag is False is None and its work is skipped.  When `source is
    x` it is the self layer: the two paths add into d_x and d_source is None.  No atomics: the same bits on every run.  slabs: 0, or the
    number of partial sums the parameter gradients are added from."""
    N, L, R, S, self_layer = _check_fmt_layer_grad_args(x, source, pack, state, dy, want, slabs)
    _require_hip(x, source, pack, state, dy)
    wx, ws, wp = (bool(f) for f in want)
    if self_layer:
        wx, ws = wx or ws, False
    with torch.cuda.device(x.device):
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
        d_x = new(N, L, FMT_D_MODEL) if wx else None
        d_src = new(R, S, FMT_D_MODEL) if ws else None
        d_par = new(FMT_PACK_FLOATS) if wp else None
        work = None
        if ws or wp or (self_layer and wx):
            floats = int(lib.diner_fmt_layer_grad_workspace_floats(N, L, R, S, int(slabs)))
            if floats != fmt_grad_workspace_floats(N, L, R, S, slabs):
                raise RuntimeError("diner_amd: fmt_layer_grad: the library and the host disagree on the workspace")
            work = new(floats)
        _lib.check(lib.diner_fmt_layer_grad_f32(_ptr(x), _ptr(source), _ptr(pack), _ptr(state), _ptr(dy), N, L, R, S, _ptr(d_x), _ptr(d_src),
                                                _ptr(d_par), _ptr(work), int(self_layer), int(slabs), _stream()))
    return d_x, d_src, d_par


def unpack_fmt_layer_grad(d_params):
    """d_params (8544,) of fmt_layer_grad -> the sixteen gradients in FMT_LAYER_KEYS' order, as views in the parameters' own shapes."""
    out, at = [], 0
    for shape in _FMT_LAYER_SHAPES:
        n = int(np.prod(shape))
        out.append(d_params[at:at + n].view(shape))
        at += n
    return out


def _check_fpn_merge_args(top, weight, lateral, out=None):
    """-> (N, H, W, Ctop, Clat)."""
    N, H, W, Ctop = _check_nhwc("fpn_merge", "top", top)
    if not torch.is_tensor(weight) or weight.dtype != torch.float32 or not weight.is_contiguous() or weight.dim() not in (2, 4) \
            or weight.shape[1] != Ctop or weight.numel() != weight.shape[0] * Ctop:
        raise ValueError(f"diner_amd: fpn_merge expects the 1 x 1 weight float32 (Clat,{Ctop}) or (Clat,{Ctop},1,1), contiguous, got "
                         f"{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    Clat = int(weight.shape[0])
    if Ctop > FPN_MAX_CHANNELS or Clat > FPN_MAX_CHANNELS or Clat < 4 or Clat % 4:
        raise ValueError(f"diner_amd: fpn_merge expects Ctop <= {FPN_MAX_CHANNELS} and Clat a multiple of 4 up to it, got {Ctop} -> {Clat}")
    if max(H, W) > 1 << 14:
        raise ValueError(f"diner_amd: fpn_merge expects H, W <= 2^14, got {H}, {W}")
    _check_nhwc("fpn_merge", "lateral", lateral, (N, 2 * H, 2 * W, Clat))
    if out is not None:
        _check_nhwc("fpn_merge", "out", out, (N, 2 * H, 2 * W, Clat))
    return N, H, W, Ctop, Clat


def fpn_merge(top, weight, lateral, out=None):
    """The pathway's merge on channels-last maps (diner_fpn_merge_f32): top (N,H,W,Ctop), weight the bias-free 1 x 1 convolution
    (Clat,Ctop[,1,1]), lateral (N,2H,2W,Clat) -> bilinear2x(conv1x1(top)) + lateral, the upsampling as
    F.interpolate(mode="bilinear", align_corners=False).  out may be lateral."""
    N, H, W, Ctop, Clat = _check_fpn_merge_args(top, weight, lateral, out)
    _require_hip(top, weight, lateral, out)
    with torch.cuda.device(top.device):
        reduced = torch.empty(N, H, W, Clat, dtype=torch.float32, device=top.device)
        y = out if out is not None else torch.empty_like(lateral)
        _lib.check(lib.diner_fpn_merge_f32(_ptr(top), _ptr(weight), _ptr(lateral), _ptr(reduced), _ptr(y), N, H, W, Ctop, Clat, _stream()))
    return y


# ---- the depth estimator's FeatureNet (deform.hip, conv2d.hip) ----------------------------------------------------------------------------
DEFORM_MAX_CIN = 64              # DINER_DEFORM_MAX_CIN
DEFORM_TAPS = 9


def deform_col_tile(Cout):
    """The column tile diner_deform_conv3x3_f32 pads Cout to: 16 up to 16 output channels, else 32."""
    return 16 if int(Cout) <= 16 else 32


def pack_deform_conv3x3(weight):
    """A DCN weight (Cout,Cin,3,3) in the layout diner_deform_conv3x3_f32 reads: [ceil(Cout / BN)][tap ky 3 + kx][Cin][BN] with BN =
    deform_col_tile(Cout), zeros beyond Cout.  Plain torch on the weight's own device, so it needs no HIP device."""
    if not torch.is_tensor(weight) or weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[0] < 1:
        raise ValueError(f"diner_amd: pack_deform_conv3x3 expects a (Cout,Cin,3,3) weight, got "
                         f"{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    if weight.dtype != torch.float32:
        raise ValueError(f"diner_amd: pack_deform_conv3x3 expects float32, got {weight.dtype}")
    Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
    if Cin < 8 or Cin > DEFORM_MAX_CIN or Cin % 8:
        raise ValueError(f"diner_amd: pack_deform_conv3x3 expects Cin a multiple of 8 in [8, {DEFORM_MAX_CIN}], got {Cin}")
    bn = deform_col_tile(Cout)
    tiles = -(-Cout // bn)
    p = weight.new_zeros(tiles * bn, Cin, DEFORM_TAPS)
    p[:Cout] = weight.detach().reshape(Cout, Cin, DEFORM_TAPS)
    return p.view(tiles, bn, Cin, DEFORM_TAPS).permute(0, 3, 2, 1).contiguous()


def _check_bias(who, bias, Cout):
    if bias is not None and not (torch.is_tensor(bias) and bias.dtype == torch.float32 and bias.dim() == 1 and bias.is_contiguous()
                                 and bias.shape[0] >= Cout):
        raise ValueError(f"diner_amd: {who} expects bias float32 with at least Cout = {Cout} elements")


def _check_deform_conv3x3_args(x, offmask, wpack, bias, Cout, out=None):
    """The argument checks of deform_conv3x3 that need no device -> (N, H, W, Cin)."""
    Cout = int(Cout)
    N, H, W, Cin = _check_nhwc("deform_conv3x3", "x", x)
    if Cin < 8 or Cin > DEFORM_MAX_CIN or Cin % 8:
        raise ValueError(f"diner_amd: deform_conv3x3 expects Cin a multiple of 8 in [8, {DEFORM_MAX_CIN}], got {Cin}")
    if Cout < 1:
        raise ValueError(f"diner_amd: deform_conv3x3 expects Cout >= 1, got {Cout}")
    if max(H, W) > 1 << 14 or N > 65535:
        raise ValueError(f"diner_amd: deform_conv3x3 expects H, W <= 2^14 and at most 65535 images, got {N} x {H} x {W}")
    _check_nhwc("deform_conv3x3", "offmask", offmask, (N, H, W, 3 * DEFORM_TAPS))
    bn = deform_col_tile(Cout)
    want = (-(-Cout // bn), DEFORM_TAPS, Cin, bn)
    if not torch.is_tensor(wpack) or wpack.dtype != torch.float32 or tuple(wpack.shape) != want or not wpack.is_contiguous():
        raise ValueError(f"diner_amd: deform_conv3x3 expects wpack float32 {want} (pack_deform_conv3x3) for Cin {Cin}, Cout {Cout}, got "
                         f"{tuple(wpack.shape) if torch.is_tensor(wpack) else type(wpack).__name__}")
    _check_bias("deform_conv3x3", bias, Cout)
    if out is not None:
        _check_nhwc("deform_conv3x3", "out", out, (N, H, W, Cout))
        if out.data_ptr() in (x.data_ptr(), offmask.data_ptr()):
            raise ValueError("diner_amd: deform_conv3x3: out must not be x or offmask")
    return N, H, W, Cin


def deform_conv3x3(x, offmask, wpack, bias, Cout, relu=False, out=None):
    """torchvision's modulated deform_conv2d, 3 x 3, stride 1, padding 1, one offset group (diner_deform_conv3x3_f32): x (N,H,W,Cin) and
    offmask (N,H,W,27) channels-last -- the raw output of the layer's conv_offset_mask: channels 2 k, 2 k + 1 the row and column offset
    of tap k, channel 18 + k the logit of its modulation -> (N,H,W,Cout) = bias + sum over taps and channels, then ReLU if asked.
    wpack: pack_deform_conv3x3's layout; bias (>= Cout,) or None."""
    N, H, W, Cin = _check_deform_conv3x3_args(x, offmask, wpack, bias, Cout, out)
    _require_hip(x, offmask, wpack, bias, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, H, W, int(Cout), dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_deform_conv3x3_f32(_ptr(x), _ptr(offmask), _ptr(wpack), _ptr(bias), _ptr(y), N, H, W, Cin, int(Cout),
                                                int(bool(relu)), _stream()))
    return y


DEFORM_GRAD_MAX_COUT = 64        # the backward pass keeps a tap's Cout x Cin accumulators in registers
DEFORM_GRAD_MAX_SLABS = 1024


def deform_grad_supported(Cin, Cout):
    """Whether diner_deform_conv3x3_grad_f32 takes these channel counts."""
    Cin, Cout = int(Cin), int(Cout)
    return 8 <= Cin <= DEFORM_MAX_CIN and Cin % 8 == 0 and 1 <= Cout <= DEFORM_GRAD_MAX_COUT


def deform_grad_slabs(N, H, W, slabs=0):
    """The number of per-workgroup slabs d_weight and d_bias are added from: a function of the shape alone, or the caller's `slabs`."""
    tiles = int(N) * (-(-int(H) * int(W) // 64))
    return min(tiles, min(int(slabs), DEFORM_GRAD_MAX_SLABS) if slabs else 128)


def _check_deform_conv3x3_grad_args(x, offmask, weight, dy, want=(True, True, True, True), slabs=0):
    """The argument checks of deform_conv3x3_grad that need no device -> (N, H, W, Cin, Cout)."""
    N, H, W, Cin = _check_nhwc("deform_conv3x3_grad", "x", x)
    if Cin < 8 or Cin > DEFORM_MAX_CIN or Cin % 8:
        raise ValueError(f"diner_amd: deform_conv3x3_grad expects Cin a multiple of 8 in [8, {DEFORM_MAX_CIN}], got {Cin}")
    if (not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.dim() != 4 or tuple(weight.shape[1:]) != (Cin, 3, 3)
            or not weight.is_contiguous()):
        raise ValueError(f"diner_amd: deform_conv3x3_grad expects weight float32 contiguous (Cout, {Cin}, 3, 3), got "
                         f"{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    Cout = int(weight.shape[0])
    if Cout < 1 or Cout > DEFORM_GRAD_MAX_COUT:
        raise ValueError(f"diner_amd: deform_conv3x3_grad expects Cout in [1, {DEFORM_GRAD_MAX_COUT}], got {Cout}")
    if max(H, W) > 1 << 14 or N > 65535 or N * (-(-H * W // 64)) >= 1 << 30:
        raise ValueError(f"diner_amd: deform_conv3x3_grad expects H, W <= 2^14, at most 65535 images and fewer than 2^30 tiles, got "
                         f"{N} x {H} x {W}")
    _check_nhwc("deform_conv3x3_grad", "offmask", offmask, (N, H, W, 3 * DEFORM_TAPS))
    _check_nhwc("deform_conv3x3_grad", "dy", dy, (N, H, W, Cout))
    if len(tuple(want)) != 4:
        raise ValueError("diner_amd: deform_conv3x3_grad expects want = (d_x, d_offmask, d_weight, d_bias) as four flags")
    if isinstance(slabs, bool) or not isinstance(slabs, int) or slabs < 0:
        raise ValueError(f"diner_amd: deform_conv3x3_grad expects slabs an int >= 0 (0: the default), got {slabs!r}")
    return N, H, W, Cin, Cout


def deform_conv3x3_grad(x, offmask, weight, dy, want=(True, True, True, True), slabs=0):
    """The backward pass of deform_conv3x3 with relu=False (diner_deform_conv3x3_grad_f32): x (N,H,W,Cin), the raw offmask (N,H,W,27) and
    the upstream gradient dy (N,H,W,Cout) channels-last, weight the plain (Cout,Cin,3,3) tensor -> (d_x (N,H,W,Cin), d_offmask (N,H,W,27)
    in the forward's channel order with the sigmoid's derivative included, d_weight (Cout,Cin,3,3), d_bias (Cout,)); an output whose `want`
    flag is False is None and its work is skipped.  d_offmask, d_weight and d_bias have the same bits on every run; d_x is added with
    float atomics and is NOT bit-reproducible.  slabs: 0, or the number of partial sums d_weight and d_bias are added from."""
    N, H, W, Cin, Cout = _check_deform_conv3x3_grad_args(x, offmask, weight, dy, want, slabs)
    _require_hip(x, offmask, weight, dy)
    wx, wo, ww, wb = (bool(f) for f in want)
    with torch.cuda.device(x.device):
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=x.device)
        d_x = new(N, H, W, Cin) if wx else None
        d_om = new(N, H, W, 3 * DEFORM_TAPS) if wo else None
        d_w = new(Cout, Cin, 3, 3) if ww else None
        d_b = new(Cout) if wb else None
        work = None
        if ww or wb:
            floats = int(lib.diner_deform_conv3x3_grad_workspace_floats(N, H, W, Cin, Cout, int(slabs)))
            if floats != deform_grad_slabs(N, H, W, slabs) * (DEFORM_TAPS * Cout * Cin + Cout):
                raise RuntimeError("diner_amd: deform_conv3x3_grad: the library and the host disagree on the workspace")
            work = new(floats)
        _lib.check(lib.diner_deform_conv3x3_grad_f32(_ptr(x), _ptr(offmask), _ptr(weight), _ptr(dy), _ptr(d_x), _ptr(d_om), _ptr(d_w),
                                                     _ptr(d_b), _ptr(work), N, H, W, Cin, Cout, int(slabs), _stream()))
    return d_x, d_om, d_w, d_b


def pack_conv5x5(weight):
    """A torch Conv2d weight (Cout,Cin,5,5) in the layout diner_conv5x5_s2_f32 reads: [ceil(Cin / 8)][ky 5 + kx][8][Cout rounded up to 64]."""
    return _pack_conv2d("pack_conv5x5", weight, (5,))


def pack_conv1x1(weight):
    """A torch Conv2d weight (Cout,Cin,1,1) in the layout diner_conv1x1_f32 reads: [ceil(Cin / 8)][1][8][Cout rounded up to 64]."""
    return _pack_conv2d("pack_conv1x1", weight, (1,))


def _check_conv_fixed_args(who, x, wpack, bias, Cout, R, stride, out=None):
    """conv5x5_s2 and conv1x1 -> (N, H, W, Cin, Ho, Wo)."""
    Cout = int(Cout)
    N, H, W, Cin = _check_conv2d_args(who, x, wpack, bias, Cout, R, (R,), False)
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else (H, W)
    if out is not None:
        _check_nhwc(who, "out", out, (N, Ho, Wo, Cout))
    return N, H, W, Cin, Ho, Wo


def conv5x5_s2(x, wpack, bias, Cout, relu=False, out=None):
    """5 x 5 convolution, stride 2, zero padding 2 (diner_conv5x5_s2_f32): x (N,H,W,Cin) channels-last -> (N, (H - 1) // 2 + 1,
    (W - 1) // 2 + 1, Cout) = conv + bias, then ReLU if asked.  wpack: pack_conv5x5's layout; bias (>= Cout,) or None."""
    N, H, W, Cin, Ho, Wo = _check_conv_fixed_args("conv5x5", x, wpack, bias, Cout, 5, 2, out)
    _require_hip(x, wpack, bias, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, Ho, Wo, int(Cout), dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_conv5x5_s2_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(y), N, H, W, Cin, int(Cout), int(bool(relu)), _stream()))
    return y


def conv1x1(x, wpack, bias, Cout, relu=False, out=None):
    """1 x 1 convolution (diner_conv1x1_f32): x (N,H,W,Cin) channels-last -> (N,H,W,Cout) = conv + bias, then ReLU if asked.  wpack:
    pack_conv1x1's layout; bias (>= Cout,) or None.  out must not be x."""
    N, H, W, Cin, Ho, Wo = _check_conv_fixed_args("conv1x1", x, wpack, bias, Cout, 1, 1, out)
    if out is not None and out.data_ptr() == x.data_ptr():
        raise ValueError("diner_amd: conv1x1: out must not be x")
    _require_hip(x, wpack, bias, out)
    with torch.cuda.device(x.device):
        y = out if out is not None else torch.empty(N, H, W, int(Cout), dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_conv1x1_f32(_ptr(x), _ptr(wpack), _ptr(bias), _ptr(y), N, H, W, Cin, int(Cout), int(bool(relu)), _stream()))
    return y


def _check_fpn_lateral_args(top, lateral, weight, bias, out=None):
    """-> (N, H, W, Ctop, Clat) with H, W the fine size."""
    N, H, W, Clat = _check_nhwc("fpn_lateral", "lateral", lateral)
    if H % 2 or W % 2 or max(H, W) > 1 << 15:
        raise ValueError(f"diner_amd: fpn_lateral expects a lateral of even H, W <= 2^15, got {H}, {W}")
    if not torch.is_tensor(weight) or weight.dtype != torch.float32 or not weight.is_contiguous() or weight.dim() not in (2, 4) \
            or weight.shape[1] != Clat or weight.numel() != weight.shape[0] * Clat:
        raise ValueError(f"diner_amd: fpn_lateral expects the 1 x 1 weight float32 (Ctop,{Clat}) or (Ctop,{Clat},1,1), contiguous, got "
                         f"{tuple(weight.shape) if torch.is_tensor(weight) else type(weight).__name__}")
    Ctop = int(weight.shape[0])
    if Ctop > FPN_MAX_CHANNELS or Clat > FPN_MAX_CHANNELS or Ctop < 4 or Ctop % 4:
        raise ValueError(f"diner_amd: fpn_lateral expects Clat <= {FPN_MAX_CHANNELS} and Ctop a multiple of 4 up to it, got {Clat} -> {Ctop}")
    _check_nhwc("fpn_lateral", "top", top, (N, H // 2, W // 2, Ctop))
    _check_bias("fpn_lateral", bias, Ctop)
    if out is not None:
        _check_nhwc("fpn_lateral", "out", out, (N, H, W, Ctop))
        if out.data_ptr() in (top.data_ptr(), lateral.data_ptr()):
            raise ValueError("diner_amd: fpn_lateral: out must not be top or lateral")
    return N, H, W, Ctop, Clat


def fpn_lateral(top, lateral, weight, bias=None, out=None):
    """FeatureNet's merge on channels-last maps (diner_fpn_lateral_f32): top (N,H/2,W/2,Ctop), lateral (N,H,W,Clat), weight the 1 x 1
    convolution (Ctop,Clat[,1,1]) with bias (Ctop,) -> (N,H,W,Ctop) = nearest2x(top) + conv1x1(lateral), one launch."""
    N, H, W, Ctop, Clat = _check_fpn_lateral_args(top, lateral, weight, bias, out)
    _require_hip(top, lateral, weight, bias, out)
    with torch.cuda.device(top.device):
        y = out if out is not None else torch.empty(N, H, W, Ctop, dtype=torch.float32, device=top.device)
        _lib.check(lib.diner_fpn_lateral_f32(_ptr(top), _ptr(lateral), _ptr(weight), _ptr(bias), _ptr(y), N, H, W, Ctop, Clat, _stream()))
    return y


def _check_affine(who, shift, scale):
    out = []
    for name, v in (("shift", shift), ("scale", scale)):
        v = [float(a) for a in v]
        if len(v) != 3 or not all(np.isfinite(a) for a in v) or (name == "scale" and not all(a != 0.0 for a in v)):
            raise ValueError(f"diner_amd: {who} expects three finite {name} values (scale != 0), got {v}")
        out.append((C.c_float * 3)(*v))
    return out


def _check_image_in_args(x, shift, scale, min_hw=1):
    """The argument checks of image_in that need no device -> (N, H, W, shift, scale as host floats)."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"diner_amd: image_in expects x (N,3,H,W), got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"diner_amd: image_in expects x float32, got {x.dtype}")
    N, _, H, W = (int(s) for s in x.shape)
    if N < 1 or H < min_hw or W < min_hw:
        raise ValueError(f"diner_amd: image_in expects N >= 1 and H, W >= {min_hw}, got {tuple(x.shape)}")
    return (N, H, W, *_check_affine("image_in", shift, scale))


def image_in(x, shift, scale, pad=True):
    """(N,3,H,W) -> channels-last (N,H,W,4 or 3) with y = (x - shift[c]) / scale[c] (diner_image_in_f32); pad: a zero fourth channel, so
    that the first convolution reads whole 16-byte pixels."""
    N, H, W, sh, sc = _check_image_in_args(x, shift, scale)
    _require_hip(x)
    x = x.detach().contiguous()
    Cs = 4 if pad else 3
    with torch.cuda.device(x.device):
        y = torch.empty(N, H, W, Cs, dtype=torch.float32, device=x.device)
        _lib.check(lib.diner_image_in_f32(_ptr(x), sh, sc, _ptr(y), N, H, W, Cs, _stream()))
    return y


def image_in_bwd(g, scale):
    """The adjoint of image_in (diner_image_in_bwd_f32): g (N,H,W,3 or 4) -> (N,3,H,W), = g[..., c] / scale[c]."""
    N, H, W, Cs = _check_nhwc("image_in_bwd", "g", g)
    if Cs not in (3, 4):
        raise ValueError(f"diner_amd: image_in_bwd expects g with 3 or 4 channels, got {Cs}")
    _, sc = _check_affine("image_in_bwd", (0.0, 0.0, 0.0), scale)
    _require_hip(g)
    with torch.cuda.device(g.device):
        gx = torch.empty(N, 3, H, W, dtype=torch.float32, device=g.device)
        _lib.check(lib.diner_image_in_bwd_f32(_ptr(g), sc, _ptr(gx), N, H, W, Cs, _stream()))
    return gx


def _check_feature_l1_args(fx, fy, weight):
    if not (torch.is_tensor(fx) and torch.is_tensor(fy)) or fx.shape != fy.shape or fx.numel() < 1:
        raise ValueError("diner_amd: feature_l1 expects fx and fy of one shape with at least one element")
    if fx.dtype != torch.float32 or fy.dtype != torch.float32:
        raise ValueError(f"diner_amd: feature_l1 expects float32, got {fx.dtype}, {fy.dtype}")
    if not (fx.is_contiguous() and fy.is_contiguous()):
        raise ValueError("diner_amd: feature_l1 expects contiguous tensors")
    weight = float(weight)
    if not np.isfinite(weight):
        raise ValueError(f"diner_amd: feature_l1 weight {weight} must be finite")
    return int(fx.numel()), weight


def feature_l1(fx, fy, weight=1.0, want_grad=True, mask_by_fx=False):
    """mean |fx - fy| of one tap layer (diner_feature_l1_f32) -> ((1,) float64 device tensor, the gradient plane for the x side
    weight * sign(fx - fy) / numel, or None).  mask_by_fx: the plane is zero where !(fx > 0).  The sum runs in double in a fixed order."""
    n, weight = _check_feature_l1_args(fx, fy, weight)
    _require_hip(fx, fy)
    dev = fx.device
    with torch.cuda.device(dev):
        ws = _workspace(lib.diner_feature_l1_workspace_bytes(n), dev)
        out = torch.empty(1, dtype=torch.float64, device=dev)
        grad = torch.empty_like(fx) if want_grad else None
        _lib.check(lib.diner_feature_l1_f32(_ptr(fx), _ptr(fy), n, weight, int(bool(mask_by_fx)), _ptr(grad), _ptr(ws), _ptr(out), _stream()))
    return out, grad


def _check_lpips_layer_args(fx, fy, lin, out):
    N, H, W, Cc = _check_nhwc("lpips_layer", "fx", fx)
    _check_nhwc("lpips_layer", "fy", fy, (N, H, W, Cc))
    if not torch.is_tensor(lin) or lin.dtype != torch.float32 or lin.numel() != Cc or not lin.is_contiguous():
        raise ValueError(f"diner_amd: lpips_layer expects lin float32 with {Cc} values (the layer's width), got "
                         f"{tuple(lin.shape) if torch.is_tensor(lin) else type(lin).__name__}")
    if N > 65535:
        raise ValueError(f"diner_amd: lpips_layer takes at most 65535 images a call, got {N}")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (N,) or not out.is_contiguous()):
        raise ValueError(f"diner_amd: lpips_layer expects out float64 ({N},)")
    return N, H * W, Cc


def lpips_layer(fx, fy, lin, out=None):
    """One layer's LPIPS term per image (diner_lpips_layer_f32): fx, fy (N,H,W,C), lin (C) -> (N,) float64 device tensor: the spatial mean
    of sum_c lin[c] (fx_c / (|fx| + 1e-10) - fy_c / (|fy| + 1e-10))^2.  out: accumulate into it instead (the sum over the layers)."""
    N, HW, Cc = _check_lpips_layer_args(fx, fy, lin, out)
    _require_hip(fx, fy, lin)
    dev = fx.device
    if out is not None and out.device != dev:
        raise RuntimeError("diner_amd: lpips_layer expects out on the features' device; there is no CPU fallback")
    with torch.cuda.device(dev):
        ws = _workspace(lib.diner_lpips_layer_workspace_bytes(N, HW), dev)
        acc = out is not None
        if not acc:
            out = torch.empty(N, dtype=torch.float64, device=dev)
        _lib.check(lib.diner_lpips_layer_f32(_ptr(fx), _ptr(fy), _ptr(lin), N, HW, Cc, int(acc), _ptr(ws), _ptr(out), _stream()))
    return out


def gen_rays(extrinsics, intrinsics, W, H, z_near, z_far, device, ray0=0, n_rays=None):
    """Reference src/util/cam_geometry.py:5-48 on the device: rays [ray0, ray0+n_rays) of each camera's row-major
    (H, W) list -> (B, n_rays, 8).  Camera tensors may live anywhere (they are read on the host: B x 27 floats)."""
    E = extrinsics.detach().to("cpu", torch.float32).contiguous()
    Km = intrinsics.detach().to("cpu", torch.float32).contiguous()
    B = E.shape[0]
    zn = torch.as_tensor(z_near, dtype=torch.float32).detach().to("cpu").reshape(-1).expand(B).contiguous()
    zf = torch.as_tensor(z_far, dtype=torch.float32).detach().to("cpu").reshape(-1).expand(B).contiguous()
    if tuple(E.shape) != (B, 4, 4) or tuple(Km.shape) != (B, 3, 3):
        raise ValueError(f"diner_amd: gen_rays expects (B,4,4) extrinsics and (B,3,3) intrinsics, got {tuple(E.shape)}, {tuple(Km.shape)}")
    n = int(W) * int(H) - int(ray0) if n_rays is None else int(n_rays)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("diner_amd: gen_rays generates on a HIP device; there is no CPU fallback")
    out = torch.empty(B, n, 8, device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        for b0 in range(0, B, 16):
            b1 = min(B, b0 + 16)
            _lib.check(lib.diner_gen_rays_f32(E[b0:b1].data_ptr(), Km[b0:b1].data_ptr(), zn[b0:b1].data_ptr(),
                                              zf[b0:b1].data_ptr(), b1 - b0, int(W), int(H), int(ray0), n,
                                              _ptr(out[b0:b1]), _stream()))
    return out


def gen_rays_at(extrinsics, intrinsics, W, H, z_near, z_far, pix):
    """gen_rays at listed pixels: pix (B, n) int32 on a HIP device (row-major pixel indices y * W + x of each camera's image)
    -> (B, n, 8); a row is bit-identical to the row gen_rays writes for that pixel.  Indices outside [0, W H) are clamped.  Camera
    tensors may live anywhere (they are read on the host; host tensors keep the call free of synchronisation)."""
    if not pix.is_cuda:
        raise RuntimeError("diner_amd: gen_rays_at generates on a HIP device; there is no CPU fallback")
    if pix.dtype != torch.int32:
        raise TypeError(f"diner_amd: gen_rays_at expects int32 pixel indices, got {pix.dtype}")
    E = extrinsics.detach().to("cpu", torch.float32).contiguous()
    Km = intrinsics.detach().to("cpu", torch.float32).contiguous()
    B = E.shape[0]
    zn = torch.as_tensor(z_near, dtype=torch.float32).detach().to("cpu").reshape(-1).expand(B).contiguous()
    zf = torch.as_tensor(z_far, dtype=torch.float32).detach().to("cpu").reshape(-1).expand(B).contiguous()
    if tuple(E.shape) != (B, 4, 4) or tuple(Km.shape) != (B, 3, 3) or pix.dim() != 2 or pix.shape[0] != B:
        raise ValueError(f"diner_amd: gen_rays_at expects (B,4,4) extrinsics, (B,3,3) intrinsics and (B,n) pixels, got {tuple(E.shape)}, "
                         f"{tuple(Km.shape)}, {tuple(pix.shape)}")
    pix = pix.contiguous()
    n = int(pix.shape[1])
    out = torch.empty(B, n, 8, device=pix.device, dtype=torch.float32)
    with torch.cuda.device(pix.device):
        for b0 in range(0, B, 16):
            b1 = min(B, b0 + 16)
            _lib.check(lib.diner_gen_rays_at_f32(E[b0:b1].data_ptr(), Km[b0:b1].data_ptr(), zn[b0:b1].data_ptr(), zf[b0:b1].data_ptr(),
                                                 b1 - b0, int(W), int(H), _ptr(pix[b0:b1]), n, _ptr(out[b0:b1]), _stream()))
    return out


# FLOPs of the two field kernels per sample point: NV views x (lin_in + 3 x (lin_z, fc_0, fc_1))
# before the view mean, 2 x (fc_0, fc_1) + lin_out after it.  Executed (the default f16x3 kernels): lin_z once per pixel, and fc_1 of the
# last per-view block once per point, in the post kernel, on the view means -- 5 per-view layers and 5 post layers.
FLOP_PRE_PER_POINT_REFERENCE = 2 * 4 * (55 * 512 + 9 * 512 * 512)     # as the reference computes it
FLOP_PRE_PER_POINT = 2 * 4 * (55 * 512 + 5 * 512 * 512)               # executed: lin_z hoisted, block 2's fc_1 moved behind the view mean
FLOP_HOIST_PER_PIXEL = 2 * 3 * 512 * 512
FLOP_POST_PER_POINT = 2 * (5 * 512 * 512 + 4 * 512)


def profile_enable(flag=True):
    _lib.check(lib.diner_profile_enable(int(bool(flag))))


def profile_collect():
    """-> dict(pre_ms, post_ms, launches, points): summed HIP-event durations of k_field_pre / k_field_post."""
    a, b, n, p = C.c_double(), C.c_double(), C.c_longlong(), C.c_longlong()
    _lib.check(lib.diner_profile_collect(C.byref(a), C.byref(b), C.byref(n), C.byref(p)))
    return dict(pre_ms=a.value, post_ms=b.value, launches=n.value, points=p.value)


# ---- arithmetic of the MLP GEMMs: a per-call argument of the C ABI (DINER_PRECISION_* of include/diner_hip.h) --------
PRECISION_FP32, PRECISION_F16X3, PRECISION_F16 = 0, 1, 3      # DINER_PRECISION_* (2 is retired and rejected)
PRECISION_NAMES = {"fp32": PRECISION_FP32, "f32": PRECISION_FP32, "exact": PRECISION_FP32,
                   "f16x3": PRECISION_F16X3, "f16x3n": PRECISION_F16X3, "split": PRECISION_F16X3,
                   "f16": PRECISION_F16, "fp16": PRECISION_F16, "half": PRECISION_F16}
_default_precision = [PRECISION_F16X3]
_warned_big_map = False


def set_precision(mode):
    """Default `precision` of the field calls of THIS Python host (the library has no global switch; every C call carries
    its mode).  PRECISION_FP32: exact fp32 MFMA.  PRECISION_F16X3 (default): split products on the fp16 MFMA with fp32
    accumulation, fp32-class accuracy (3e-6 end to end against the reference; every parity test holds it to the fp32
    bar).  PRECISION_F16: plain fp16 operands (BASELINE configs[4], "fp16 MLP on MFMA"): ~1e-3 relative, NOT inside the
    1e-4 parity bar.  Env: DINER_AMD_PRECISION = fp32 | f16x3 | f16."""
    if isinstance(mode, str):
        mode = PRECISION_NAMES[mode.lower()]
    if isinstance(mode, bool) or int(mode) not in (PRECISION_FP32, PRECISION_F16X3, PRECISION_F16):
        raise ValueError(f"diner_amd: unknown precision {mode!r} (use the names 'fp32' / 'f16x3' / 'f16' or the PRECISION_* "
                         f"constants; the integer 2 of ABI v1 is retired)")
    _default_precision[0] = int(mode)


def get_precision():
    return _default_precision[0]


def _precision_for(scene, precision):
    """Mode passed to the library for one call.  A scene whose projected maps exceed the 32-bit addressing of the
    fp16-operand kernels (>= 4 GiB per map of one group of up to four views: images beyond ~2700 x 2700, for any number of views) is
    rendered by the exact kernels."""
    prec = get_precision() if precision is None else (PRECISION_NAMES[precision.lower()] if isinstance(precision, str)
                                                      else int(precision))
    if prec not in (PRECISION_FP32, PRECISION_F16X3, PRECISION_F16):
        raise ValueError(f"diner_amd: unknown precision {precision!r}")
    group_bytes = min(scene.nv, 4) * scene.Hf * scene.Wf * 2048
    if prec != PRECISION_FP32 and group_bytes >= (1 << 32):
        global _warned_big_map
        if not _warned_big_map:       # not silent: the exact kernels are ~3x slower than the f16x3 ones
            import warnings
            warnings.warn(f"diner_amd: one projected feature map of this scene is {group_bytes / 2 ** 30:.1f} GiB per group of four views; the "
                          f"fp16-operand kernels address it with 32-bit offsets (< 4 GiB), so this scene is rendered by the exact-fp32 "
                          f"kernels (~3x slower)", RuntimeWarning, stacklevel=3)
            _warned_big_map = True
        return PRECISION_FP32
    return prec


_want = os.environ.get("DINER_AMD_PRECISION", "f16x3").lower()
if _want not in PRECISION_NAMES:
    raise ValueError(f"DINER_AMD_PRECISION={_want!r}: expected one of {sorted(PRECISION_NAMES)}")
set_precision(_want)


# ---- the depth estimator's fine-tuning objective and depth scores (csrc/mvsloss.hip) -------------------------------------------------------
def _check_mvs_loss_args(vol, hypotheses, gt, mask, init=None):
    """The argument checks of the stage loss that need no device -> (B, D, H, W)."""
    if vol.dim() != 4 or tuple(hypotheses.shape) != tuple(vol.shape) or (init is not None and tuple(init.shape) != tuple(vol.shape)):
        raise ValueError(f"diner_amd: mvs_stage_loss expects the volume, hypotheses [and init] of one shape (B,D,H,W), got {tuple(vol.shape)}, "
                         f"{tuple(hypotheses.shape)}" + ("" if init is None else f", {tuple(init.shape)}"))
    B, D, H, W = (int(v) for v in vol.shape)
    if tuple(gt.shape) != (B, H, W) or tuple(mask.shape) != (B, H, W):
        raise ValueError(f"diner_amd: mvs_stage_loss expects gt and mask ({B},{H},{W}), got {tuple(gt.shape)}, {tuple(mask.shape)}")
    if min(B, D, H, W) < 1 or B * D * H * W >= 2 ** 31:
        raise ValueError(f"diner_amd: mvs_stage_loss needs B, D, H, W >= 1 and B D H W < 2^31, got {B} x {D} x {H} x {W}")
    return B, D, H, W


def _thresholds(thresholds):
    t = [float(v) for v in thresholds]
    if len(t) > _lib.MVS_LOSS_MAX_THRESHOLDS:
        raise ValueError(f"diner_amd: at most {_lib.MVS_LOSS_MAX_THRESHOLDS} thresholds, got {len(t)}")
    return (C.c_double * max(len(t), 1))(*t), len(t)


def mvs_stage_loss(vol, hypotheses, gt, mask, init=None, from_prob=False, unit=None, thresholds=(), weight=1.0, record=True):
    """diner_mvs_stage_loss_f32 + diner_mvs_loss_finish_f32: one stage of the estimator's loss.  vol (B,D,H,W): the regularised cost
    [+ init], or with from_prob a probability volume; hypotheses (B,D,H,W); gt, mask (B,H,W) float32, valid where mask > 0.5; unit: (B,)
    float64 error unit of the scores or None; thresholds: host numbers.
    -> dict: scalars (13 float32: weight 2 entropy, 2 entropy, depth_loss, mean |err|, mean |err| / unit, shares under the thresholds),
    depth, confidence (B,H,W), record (B,H,W,4) or None, factors (B,) float64, sums (B,16) float64."""
    B, D, H, W = _check_mvs_loss_args(vol, hypotheses, gt, mask, init)
    if from_prob and init is not None:
        raise ValueError("diner_amd: mvs_stage_loss: init belongs to the cost, not to a probability volume")
    _require_hip(vol, hypotheses, gt, mask, init)
    if unit is not None and (not unit.is_cuda or unit.dtype != torch.float64 or tuple(unit.shape) != (B,)):
        raise ValueError(f"diner_amd: mvs_stage_loss expects unit as a ({B},) float64 HIP tensor")
    vol, hypotheses, gt, mask = vol.contiguous(), hypotheses.contiguous(), gt.contiguous(), mask.contiguous()
    init = init.contiguous() if init is not None else None
    unit = unit.contiguous() if unit is not None else None
    thr, n_thr = _thresholds(thresholds if unit is not None else ())
    dev = vol.device
    depth = torch.empty(B, H, W, device=dev, dtype=torch.float32)
    conf = torch.empty_like(depth)
    rec = torch.empty(B, H, W, 4, device=dev, dtype=torch.float32) if record else None
    part = torch.empty(int(lib.diner_mvs_loss_partial_doubles(B, H, W)), device=dev, dtype=torch.float64)
    scalars = torch.empty(_lib.MVS_LOSS_SCALARS, device=dev, dtype=torch.float32)
    factors = torch.empty(B, device=dev, dtype=torch.float64)
    sums = torch.empty(B, _lib.MVS_LOSS_SLOTS, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.diner_mvs_stage_loss_f32(_ptr(None if from_prob else vol), _ptr(init), _ptr(vol if from_prob else None), _ptr(hypotheses),
                                                _ptr(gt), _ptr(mask), _ptr(unit), thr, n_thr, _ptr(depth), _ptr(conf), _ptr(rec), _ptr(part),
                                                B, D, H, W, _stream()))
        _lib.check(lib.diner_mvs_loss_finish_f32(_ptr(part), B, H, W, n_thr, float(weight), _ptr(scalars), _ptr(factors), _ptr(sums), _stream()))
    return dict(scalars=scalars, depth=depth, confidence=conf, record=rec, factors=factors, sums=sums)


def mvs_stage_loss_grad(vol, init, from_prob, mask, record, factors, upstream, weight=1.0):
    """diner_mvs_stage_loss_grad_f32: d(upstream weight 2 entropy) / d(vol) as a dense (B,D,H,W) volume, one launch.  vol, init, mask, record
    and factors as mvs_stage_loss took and returned them; upstream: a 0-dim float32 HIP tensor, never read back."""
    B, D, H, W = (int(v) for v in vol.shape)
    if min(B, D, H, W) < 1 or B * D * H * W >= 2 ** 31:
        raise ValueError(f"diner_amd: mvs_stage_loss_grad needs B, D, H, W >= 1 and B D H W < 2^31, got {B} x {D} x {H} x {W}")
    if tuple(mask.shape) != (B, H, W) or tuple(record.shape) != (B, H, W, 4) or tuple(factors.shape) != (B,) or upstream.numel() != 1:
        raise ValueError("diner_amd: mvs_stage_loss_grad: mask, record, factors or upstream do not belong to this volume")
    _require_hip(vol, init, mask, record, upstream)
    if not factors.is_cuda or factors.dtype != torch.float64:
        raise TypeError("diner_amd: mvs_stage_loss_grad expects the factors mvs_stage_loss returned (float64, on the device)")
    vol, mask, record, factors, upstream = vol.contiguous(), mask.contiguous(), record.contiguous(), factors.contiguous(), upstream.contiguous()
    init = init.contiguous() if init is not None else None
    grad = torch.empty(B, D, H, W, device=vol.device, dtype=torch.float32)
    with torch.cuda.device(vol.device):
        _lib.check(lib.diner_mvs_stage_loss_grad_f32(_ptr(vol), _ptr(init), 1 if from_prob else 0, _ptr(mask), _ptr(record), _ptr(factors),
                                                     _ptr(upstream), float(weight), _ptr(grad), B, D, H, W, _stream()))
    return grad


def _check_depth_scores_args(est, gt, mask, thresholds):
    if est.dim() != 3 or tuple(gt.shape) != tuple(est.shape) or tuple(mask.shape) != tuple(est.shape):
        raise ValueError(f"diner_amd: depth_scores expects est, gt and mask of one shape (B,H,W), got {tuple(est.shape)}, {tuple(gt.shape)}, "
                         f"{tuple(mask.shape)}")
    B, H, W = (int(v) for v in est.shape)
    if min(B, H, W) < 1 or B * H * W >= 2 ** 31:
        raise ValueError(f"diner_amd: depth_scores needs B, H, W >= 1 and B H W < 2^31, got {B} x {H} x {W}")
    if len(thresholds) > _lib.MVS_LOSS_MAX_THRESHOLDS:
        raise ValueError(f"diner_amd: at most {_lib.MVS_LOSS_MAX_THRESHOLDS} thresholds, got {len(thresholds)}")
    return B, H, W


def depth_scores(est, gt, mask, thresholds=(), band=None):
    """diner_depth_scores_f32: est, gt, mask (B,H,W) float32 (valid where mask > 0.5) -> (per_image (B,10), batch (10,)) float32:
    [0] mean |est - gt|, [1] the same restricted to the errors inside band = (lo, hi) (0 when none is; 0 without a band), [2 + t] the share
    of errors above thresholds[t]; batch is the mean of the per-image values."""
    B, H, W = _check_depth_scores_args(est, gt, mask, thresholds)
    _require_hip(est, gt, mask)
    est, gt, mask = est.contiguous(), gt.contiguous(), mask.contiguous()
    thr, n_thr = _thresholds(thresholds)
    dev = est.device
    part = torch.empty(int(lib.diner_mvs_loss_partial_doubles(B, H, W)), device=dev, dtype=torch.float64)
    per_image = torch.empty(B, _lib.DEPTH_SCORES, device=dev, dtype=torch.float32)
    batch = torch.empty(_lib.DEPTH_SCORES, device=dev, dtype=torch.float32)
    lo, hi = (float(band[0]), float(band[1])) if band is not None else (0.0, 0.0)
    with torch.cuda.device(dev):
        _lib.check(lib.diner_depth_scores_f32(_ptr(est), _ptr(gt), _ptr(mask), B, H, W, thr, n_thr, 0 if band is None else 1, lo, hi, _ptr(part),
                                              _ptr(per_image), _ptr(batch), _stream()))
    return per_image, batch
