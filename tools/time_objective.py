"""A/B timing of the objective side of a training step at the step the shipped configs run (SB 4 x 4096 rays x 40 samples, 400 x 300,
w_antibias 1; reference DINER.calc_losses, src/models/diner.py:217-290):

    python tools/time_objective.py [--objects 4] [--size 400x300] [--samples 40] [--steps 5] [--reps 3] [--no-launch-count]

  hip    diner_amd.objective.calc_losses: patch from the foreground mask, rays at its pixels, gather + MSE + anti-bias in HIP kernels
  torch  the same step with the torch expression of the objective: the same patch indices, full-frame ops.gen_rays + index, torch gather,
         mse_loss, AvgPool2d + L1Loss
Both variants encode the same source views (PixelNeRF.encode, ResNet trunk included), run ONE renderer.forward on (SB, 4096, 8) rays and
call backward on the total.  The patch mode is tied to w_vgg != 0 as in the reference; the VGG-19 weights are not available, so both
variants carry a constant-zero perceptual term with a negligible weight (two scalar ops each).  The variants alternate --reps times;
printed per run: ms per step and host enqueue ms per step (time until the step's last launch is queued), then the medians, then the
device-kernel launch count of the objective side alone (everything but encode, renderer.forward and the backward below fine.rgb), taken
with the torch profiler on a fixed fine.rgb."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from diner_amd import objective, ops                                          # noqa: E402
from diner_amd.synthetic import _Conf, make_mlp_state_dict, make_scene        # noqa: E402
from src.util.import_helper import import_obj                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=4)
ap.add_argument("--size", default="400x300")
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--patch", type=int, default=64)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-launch-count", action="store_true")
args = ap.parse_args()
W, H = (int(v) for v in args.size.split("x"))
SB, K, s, n_down, w_ab, w_vgg = args.objects, args.samples, args.patch, 3, 1.0, 1e-30
dev = torch.device("cuda", 0)
torch.manual_seed(0)
nerf = import_obj("src.models.pixelnerf.PixelNeRF")(
    poscode_conf=_Conf(kwargs=dict(num_freqs=6, freq_factor=6.28, include_input=True)),
    encoder_conf=_Conf("src.models.image_encoder.SpatialEncoder", dict(image_padding=64, padding_pe=4, pretrained=False)),
    mlp_fine_conf=_Conf("src.models.resnetfc.ResnetFC", dict(n_blocks=5, d_hidden=512, combine_layer=3, combine_type="average")))
nerf.mlp_fine.load_state_dict(make_mlp_state_dict())
nerf = nerf.to(dev).train()
ren = import_obj("src.models.nerf_renderer.NeRFRendererDGS")(n_samples=K, n_depth_candidates=1000, n_gaussian=int(15 * K / 40), white_bkgd=True)
scs = [make_scene(W, H, seed=i, latent=False) for i in range(SB)]
gen = torch.Generator().manual_seed(1)
st = lambda k: torch.stack([sc[k] for sc in scs]).to(dev)
yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
alpha = (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.4 * min(H, W)) ** 2).float()[None, None].repeat(SB, 1, 1, 1)
batch = dict(src_rgbs=torch.rand(SB, 4, 3, H, W, generator=gen).to(dev), src_depths=st("depths"), src_depth_stds=st("depths_std"),
             src_extrinsics=st("src_extrinsics"), src_intrinsics=st("src_intrinsics"), target_rgb=torch.rand(SB, 3, H, W, generator=gen).to(dev),
             target_alpha=alpha.to(dev), target_extrinsics=torch.stack([sc["target_extrinsics"] for sc in scs]),
             target_intrinsics=torch.stack([sc["target_intrinsics"] for sc in scs]))
znear, zfar = scs[0]["znear"], scs[0]["zfar"]
zero_vgg = lambda a, b: a.new_zeros(())
pool, l1 = torch.nn.AvgPool2d(2 ** n_down, 2 ** n_down), torch.nn.L1Loss()
params = list(nerf.parameters())
step_no = [0]


def torch_objective(pred, pix):
    """MSE + w_antibias * AntibiasLoss as the reference spells it (diner.py:265-288) on the rays of `pix`."""
    idx = pix.long()
    gt = batch["target_rgb"].view(SB, 3, -1).permute(0, 2, 1).gather(1, idx[..., None].expand(-1, -1, 3))
    total = torch.nn.functional.mse_loss(pred, gt)
    pn, gn = (t.view(SB, s, s, 3).permute(0, 3, 1, 2) for t in (pred, gt))
    total = total + w_ab * l1(pool(pn), pool(gn))
    return total + w_vgg * zero_vgg(pn, gn)


def step_hip():
    objective.calc_losses(nerf, ren, batch, znear=znear, zfar=zfar, w_vgg=w_vgg, vgg_spatch=s, w_antibias=w_ab, antibias_downsampling=n_down,
                          vgg_fn=zero_vgg, seed=11, step=step_no[0])["total"].backward()


def step_torch():
    nerf.encode(images=batch["src_rgbs"], depths=batch["src_depths"], depths_std=batch["src_depth_stds"],
                extrinsics=batch["src_extrinsics"], intrinsics=batch["src_intrinsics"])
    pix, _, _ = objective.sample_patch(batch["target_alpha"][:, 0], s, seed=11, step=step_no[0])      # the same patches as the other variant
    rays_all = ops.gen_rays(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, dev)
    rays = rays_all.gather(1, pix.long()[..., None].expand(-1, -1, 8))
    torch_objective(ren.forward(nerf, rays).fine.rgb, pix).backward()


def timed(fn):
    def one():
        for p in params:
            p.grad = None
        with torch.no_grad():                      # an optimiser step's in-place write: the parameters are new every step
            torch._foreach_add_(params, 0.0)
        fn()
        step_no[0] += 1
    one()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(args.steps):
        one()
    host = (time.perf_counter() - t) / args.steps
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / args.steps * 1e3, host * 1e3


res = {"hip": [], "torch": []}
for rep in range(args.reps):
    for name, fn in (("hip", step_hip), ("torch", step_torch)):
        step_no[0] = 100 * rep
        ms, host = timed(fn)
        res[name].append((ms, host))
        print(f"rep {rep} {name:5s}: {ms:8.2f} ms per step, host enqueue {host:6.2f} ms per step", flush=True)
for name, v in res.items():
    print(f"median {name:5s}: {statistics.median(x[0] for x in v):8.2f} ms per step, host enqueue {statistics.median(x[1] for x in v):6.2f} ms per step "
          f"({SB} objects x {s * s} rays x {K} samples, {W}x{H}, {args.reps} runs of {args.steps} steps)", flush=True)

if not args.no_launch_count:
    from torch.profiler import ProfilerActivity, profile
    pred0 = torch.rand(SB, s * s, 3, device=dev)

    def side_hip():
        pix, _, _ = objective.sample_patch(batch["target_alpha"][:, 0], s, seed=11, step=0)
        ops.gen_rays_at(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, pix)
        p = pred0.clone().requires_grad_(True)
        objective.photometric(p, (batch["target_rgb"], pix), s, n_down, w_ab).total.backward()

    def side_torch():
        pix, _, _ = objective.sample_patch(batch["target_alpha"][:, 0], s, seed=11, step=0)
        rays_all = ops.gen_rays(batch["target_extrinsics"], batch["target_intrinsics"], W, H, znear, zfar, dev)
        rays_all.gather(1, pix.long()[..., None].expand(-1, -1, 8))
        p = pred0.clone().requires_grad_(True)
        torch_objective(p, pix).backward()

    for name, fn in (("hip", side_hip), ("torch", side_torch)):
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kern = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        print(f"objective side alone, {name:5s}: {len(kern)} device kernels (the clone of fine.rgb and the patch kernel included in both)", flush=True)
