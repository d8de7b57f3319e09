"""NeRFRendererDGS -- drop-in for reference src/models/nerf_renderer.py (:12-430): same constructor, mutable
attributes (`n_samples`, `n_gaussian`, `n_depth_candidates`, `eval_batch_size`, `white_bkgd`; read at call time, as
create_prediction_folder.py:44-47 relies on), public methods and return types.

Everything runs in hand-written HIP kernels behind the C ABI of include/diner_hip.h:
  sample_depthguided / fill_up_uniform_samples  -> diner_sample_depthguided_long_f32 / diner_fill_uniform_long_f32 (sampler.hip)
  composite                                     -> diner_field_from_rays_f32 (mlp.hip) + diner_composite_long_f32
  forward                                       -> the three above, per object of the batch
The long entries take n_samples <= 1024 and n_depth_candidates <= 4096 (the reference's --nsamples); up to 256 samples and
1024 candidates they run the bounded kernels, so results there are those of the bounded entries bit for bit.
`model` must be the MI355X PixelNeRF of this package (it carries the channels-last scene and the packed weights).

Noise: the reference draws rand/randn from torch's global generator; here the kernels draw the same three noise
fields from an in-kernel Philox generator keyed by a seed taken from torch's global CPU generator, unless explicit
noise is injected with diner_amd.noise.inject (parity tests)."""
import torch

from diner_amd import noise as _noise
from diner_amd import ops
from src.util.general import DotMap


def _seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def _key(sb=0):
    """(seed, ray_index0) of this call's in-kernel noise: the frame key set by the image harness (one seed per frame + the
    position of this ray batch in the frame, diner_amd.noise.keyed), else a fresh seed from torch's global generator."""
    k = _noise.frame_key()
    return (k[0] + 0x9E3779B97F4A7C15 * sb, k[1]) if k is not None else (_seed(), 0)


class NeRFRendererDGS(torch.nn.Module):
    # Empty-ray culling (not in the reference; off by default).  Plain attributes read at call time, like white_bkgd.  With cull_empty
    # a no-grad forward renders only the rays whose sum_O -- the depth maps' probability that the ray meets a surface, the reference's
    # ray_mask of :182 -- is not <= cull_below; every other ray gets the compositor's values at zero density (rgb 1 with white_bkgd else
    # 0, depth 0, alpha 0, depth_var 0) WITHOUT running the MLP, where the reference evaluates it on K stratified samples: an
    # approximation (diner_amd.render.render_live_rays).  One host read-back per call and object.  Ignored in grad mode (training renders
    # every ray) and with want_weights (the per-sample weights are not culled).
    cull_empty = False
    cull_below = 0.0

    def __init__(self, n_samples=40, n_depth_candidates=1000, n_gaussian=15, eval_batch_size=100000, white_bkgd=True):
        super().__init__()
        self.n_samples = n_samples
        self.n_depth_candidates = n_depth_candidates
        self.n_gaussian = n_gaussian
        self.eval_batch_size = eval_batch_size      # kept for API compatibility: chunking never changes results
        self.white_bkgd = white_bkgd

    @staticmethod
    def _check_model(model):
        if not (hasattr(model, "hip_scene") and hasattr(model, "hip_mlp")):
            raise TypeError("diner_amd: `model` must be src.models.pixelnerf.PixelNeRF of this package")

    def _render_train_batch(self, model, rays, z, want_weights, want_alpha=False):
        """The SB objects of a training step at once (ABI v6): rays (SB,NR,8), z (SB,NR,K) -> weights | None, rgb (SB,NR,3), depth (SB,NR)
        [, alpha (SB,NR) with want_alpha: the opacity, a third output of the compositor node].
        One field node for all objects (diner_amd.train.field_train_batch: the layer products of the backward run once over SB x NR x K x NV
        rows), one compositor node over the SB x NR rays."""
        from diner_amd import train
        SB, NR, K = z.shape
        r = rays.detach()
        z = z.detach()
        xyz = (r[:, :, None, :3] + z[..., None] * r[:, :, None, 3:6]).reshape(SB, NR * K, 3)
        dirs = r[:, :, None, 3:6].expand(-1, -1, K, -1).reshape(SB, NR * K, 3)
        if model.is_generic():          # a configuration outside the fused kernels: the generic differentiable path, object by object
            field = model.forward(xyz, dirs).view(SB * NR, K, 4)
        else:
            scenes = [model.hip_scene(sb) for sb in range(SB)]
            field = train.field_train_batch(scenes, xyz, dirs, model.encoder.latent, train.mlp_params(model.mlp_fine),
                                            model.poscode.freq_factor).view(SB * NR, K, 4)
        zf, rf = z.reshape(SB * NR, K), r.reshape(SB * NR, 8)
        alpha = None
        if want_alpha:
            rgb, depth, alpha = train.composite_train(field, zf, rf, self.white_bkgd, want_alpha=True)
        else:
            rgb, depth = train.composite_train(field, zf, rf, self.white_bkgd)
        w = ops.composite(field.detach(), zf, rf, self.white_bkgd, want_weights=True)[0].view(SB, NR, K) if want_weights else None
        if want_alpha:
            return w, rgb.view(SB, NR, 3), depth.view(SB, NR), alpha.view(SB, NR)
        return w, rgb.view(SB, NR, 3), depth.view(SB, NR)

    def sample_coarse(self, rays, n_coarse=None):
        """Stratified candidates (:39-63) as a stand-alone helper (torch ops on the rays' device).  The depth-guided
        sampler generates its candidates inside the kernel and does not call this."""
        n_coarse = n_coarse if n_coarse else self.n_depth_candidates
        shp = rays.shape
        r = rays.reshape(-1, 8)
        near, far = r[:, -2:-1], r[:, -1:]
        step = 1.0 / n_coarse
        t = torch.linspace(0, 1 - step, n_coarse, device=rays.device).unsqueeze(0).repeat(r.shape[0], 1)
        t = t + torch.rand_like(t) * step
        return (near * (1 - t) + far * t).view(*shp[:-1], n_coarse)

    @torch.no_grad()
    def sample_depthguided(self, rays, model, n_samples, n_candidates, depth_diff_max=0.05, n_gaussian=None, return_info=False):
        """rays (SB,NR,8) -> z (SB,NR,n_samples) in the reference's slot order (:172-190): the top (n_samples - n_gaussian)
        candidates by descending surface likelihood (equal likelihoods: lower candidate index first), zeros marking empty slots,
        then n_gaussian samples of the likelihood-weighted gaussian (zeros where the ray sees no surface).
        return_info (not in the reference, which computes these and drops them): -> (z, DotMap(slot_L, slot_idx (SB,NR,K-G): likelihood
        and candidate index of each pick slot; sum_L, sum_O, prior_depth, prior_std (SB,NR): the ray's summed likelihood, the depth
        maps' probability that it meets a surface, mean and sigma of the gaussian fit)), see ops.sample_depthguided."""
        self._check_model(model)
        n_gaussian = n_gaussian if n_gaussian is not None else self.n_gaussian
        assert n_samples >= n_gaussian
        SB = rays.shape[0]
        inj = _noise.current()
        infos = []
        for sb in range(SB):
            nz = None if inj is None else tuple(None if t is None else t[sb] for t in inj)
            seed, r0 = _key(sb)
            infos.append(ops.sample_depthguided_long(model.hip_scene(sb), rays[sb], n_samples, n_candidates, n_gaussian,
                                                     depth_diff_max, noise=nz, seed=seed, ray_index0=r0, want_info=True)[1])
        z = torch.stack([i.z_ordered for i in infos])
        if not return_info:
            return z
        return z, DotMap(**{f: torch.stack([getattr(i, f) for i in infos]) for f in ops.SamplerInfo._fields[1:]})

    def fill_up_uniform_samples(self, z_samples, rays):
        """zeros in z (SB,NR,K) -> stratified samples of [near, far]; returns ascending z (:367-397)."""
        SB = rays.shape[0]
        inj = _noise.current()
        out = []
        for sb in range(SB):
            seed, r0 = _key(sb)
            out.append(ops.fill_uniform(z_samples[sb], rays[sb], None if inj is None or inj[2] is None else inj[2][sb],
                                        seed=seed, ray_index0=r0))
        return torch.stack(out)

    def composite(self, model, rays, z_samp):
        """-> weights (SB,B,K), rgb (SB,B,3), depth (SB,B)   (:286-365)."""
        self._check_model(model)
        model._check_poscode()
        SB = rays.shape[0]
        if model.needs_grad():
            return self._render_train_batch(model, rays, z_samp, True)
        else:
            mlp = model.hip_mlp()
            res = [ops.render(model.hip_scene(sb), mlp, rays[sb], z_samp[sb], self.white_bkgd, want_weights=True)
                   for sb in range(SB)]
        return tuple(torch.stack([r[i] for r in res]) for i in range(3))

    def forward(self, model, rays, want_weights=False, want_alpha=False):
        """rays (SB,B,8) -> DotMap(fine=DotMap(rgb (SB,B,3), depth (SB,B) [, weights (SB,B,K)]))   (:399-430).
        want_alpha (not in the reference, which computes the opacity at :359 and drops it): fine gains alpha (SB,B) = sum_k w_k -- in grad
        mode an output of the compositor's autograd node -- and, without grad, depth_var (SB,B), the spread of the ray's samples around
        its depth (a diagnostic without a gradient)."""
        assert len(rays.shape) == 3
        self._check_model(model)
        model._check_poscode()
        assert self.n_samples >= self.n_gaussian
        SB = rays.shape[0]
        training = model.needs_grad()
        mlp = None if training else model.hip_mlp()
        inj = _noise.current()
        rgbs, depths, wts = [], [], []
        if training:
            # the sampler per object (each has its own maps), then field + compositor for the SB objects as ONE autograd node each
            zs = []
            for sb in range(SB):
                nz = None if inj is None else tuple(None if t is None else t[sb] for t in inj)
                seed, r0 = _key(sb)
                zs.append(ops.sample_depthguided_long(model.hip_scene(sb), rays[sb], self.n_samples, self.n_depth_candidates,
                                                      self.n_gaussian, 0.05, noise=nz, seed=seed, ray_index0=r0))
            w, rgb, depth, *aux = self._render_train_batch(model, rays, torch.stack(zs), want_weights, want_alpha)
            out = self._format_outputs(w, rgb, depth, want_weights=want_weights)
            if want_alpha:
                out.alpha = aux[0]
            return DotMap(fine=out)
        alphas, dvars = [], []
        cull = bool(self.cull_empty) and not want_weights and rays.shape[1] > 0
        for sb in range(SB):
            scene = model.hip_scene(sb)
            nz = None if inj is None else tuple(None if t is None else t[sb] for t in inj)
            seed, r0 = _key(sb)
            if cull:
                t = self._forward_culled(scene, mlp, rays[sb], nz, seed, r0, want_alpha)
                rgbs.append(t[:, :3].contiguous())
                depths.append(t[:, 3].contiguous())
                if want_alpha:
                    alphas.append(t[:, 4].contiguous())
                    dvars.append(t[:, 5].contiguous())
                continue
            z = ops.sample_depthguided_long(scene, rays[sb], self.n_samples, self.n_depth_candidates, self.n_gaussian,
                                            0.05, noise=nz, seed=seed, ray_index0=r0)
            w, rgb, depth, *aux = ops.render(scene, mlp, rays[sb], z, self.white_bkgd, want_weights=want_weights, want_aux=want_alpha)
            rgbs.append(rgb)
            depths.append(depth)
            wts.append(w)
            if want_alpha:
                alphas.append(aux[0])
                dvars.append(aux[1])
        out = self._format_outputs(torch.stack(wts) if want_weights else None, torch.stack(rgbs), torch.stack(depths),
                                   want_weights=want_weights)
        if want_alpha:
            out.alpha, out.depth_var = torch.stack(alphas), torch.stack(dvars)
        return DotMap(fine=out)

    def forward_geometry(self, model, rays, cam_fwd=None, want_weights=False, quantile=0.5, alpha_min=1e-3, point_depth="median"):
        """forward with the geometry of the rendered rays (not in the reference; a method of its own, so that forward keeps its signature
        and its code).  No-grad mode only, ValueError in grad mode.  rays (SB,B,8) -> DotMap(fine=...) as forward(want_alpha=True)
        returns it -- rgb, depth, alpha, depth_var [, weights] are that call's, from the same sampler and compositor launches -- plus the
        outputs of ops.ray_geometry on the rendered weights and the same z: depth_median, median_idx (int32), depth_mean (SB,B), points
        (SB,B,3) and, with cam_fwd (SB,3), row 2 of each target's world->camera rotation, zdepth (SB,B); quantile, alpha_min and
        point_depth are ops.ray_geometry's.  cull_empty is ignored, as it is with want_weights."""
        assert len(rays.shape) == 3
        self._check_model(model)
        model._check_poscode()
        assert self.n_samples >= self.n_gaussian
        if model.needs_grad():
            raise ValueError("diner_amd: forward_geometry has no gradient; call it under torch.no_grad()")
        SB = rays.shape[0]
        if cam_fwd is not None:
            cam_fwd = torch.as_tensor(cam_fwd).detach().to("cpu", torch.float32)
            if tuple(cam_fwd.shape) != (SB, 3):
                raise ValueError(f"diner_amd: cam_fwd must be ({SB},3), got {tuple(cam_fwd.shape)}")
        mlp = model.hip_mlp()
        inj = _noise.current()
        cols = {k: [] for k in ("weights", "rgb", "depth", "alpha", "depth_var") + ops.RayGeometry._fields}
        for sb in range(SB):
            scene = model.hip_scene(sb)
            nz = None if inj is None else tuple(None if t is None else t[sb] for t in inj)
            seed, r0 = _key(sb)
            z = ops.sample_depthguided_long(scene, rays[sb], self.n_samples, self.n_depth_candidates, self.n_gaussian,
                                            0.05, noise=nz, seed=seed, ray_index0=r0)
            res = ops.render(scene, mlp, rays[sb], z, self.white_bkgd, want_weights=True, want_aux=True)
            geo = ops.ray_geometry(res[0], z, rays[sb], None if cam_fwd is None else cam_fwd[sb], quantile, alpha_min, point_depth)
            for k, v in zip(("weights", "rgb", "depth", "alpha", "depth_var"), res):
                cols[k].append(v)
            for k, v in zip(ops.RayGeometry._fields, geo):
                cols[k].append(v)
        out = self._format_outputs(torch.stack(cols["weights"]) if want_weights else None, torch.stack(cols["rgb"]),
                                   torch.stack(cols["depth"]), want_weights=want_weights)
        for k in ("alpha", "depth_var") + ops.RayGeometry._fields:
            if cols[k][0] is not None:
                out[k] = torch.stack(cols[k])
        return DotMap(fine=out)

    def _forward_culled(self, scene, mlp, rays, nz, seed, r0, want_alpha):
        """One object of a no-grad forward with cull_empty: (B,8) -> (B, 4 or 6) rows [rgb, depth (, alpha, depth_var)]."""
        from diner_amd.render import render_live_rays
        rays = ops._f32c(rays)

        def sample(a, b):
            part = None if nz is None else tuple(None if t is None else t[a:b] for t in nz)
            return ops.sample_depthguided_long(scene, rays[a:b], self.n_samples, self.n_depth_candidates, self.n_gaussian, 0.05,
                                               noise=part, seed=seed, ray_index0=r0 + a, want_info=True)

        return render_live_rays(scene, mlp, rays, sample, self.n_samples, self.white_bkgd, n_aux=2 if want_alpha else 0,
                                cull_below=float(self.cull_below), ray_batch_size=rays.shape[0])

    def _format_outputs(self, weights, rgb, depth, want_weights):
        out = DotMap(rgb=rgb, depth=depth)
        if want_weights:
            out.weights = weights
        return out
