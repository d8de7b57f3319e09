"""A/B timing of the optimiser step on the shipped model's parameter set (PixelNeRF with the SpatialEncoder and the 5-block 512-wide ResnetFC,
built as in tools/time_objective.py; random gradients):

    python tools/time_optim.py [--windows 5] [--steps 200] [--loop] [--loop-windows 5] [--loop-steps 20]

  device         diner_amd.optim.DeviceAdam.step()                        one launch over the chunk table
  device+zero    ... step(zero_grads=True)                                the gradients zeroed in the same pass
  device+clip    ... max_grad_norm + skip_nonfinite, zero_grads=True      + the statistics pass (two more launches)
  torch          torch.optim.Adam (its default route on a HIP device)
  torch-fused    torch.optim.Adam(fused=True)                             the yardstick
All variants run in ONE process on the same parameters, alternating window by window after a warm-up; per window: stream time per step
(HIP events around the window: the device time unless the host is the slower side, which the second figure shows) and host enqueue time
per step (until the window's last launch is queued).  Printed: the median over the windows and the spread (min .. max), the bytes a step
must move by the table (28 B per element, +4 with zeroing, +4 for the statistics pass) and their share of 6.3 TB/s.
--loop: the whole step of diner_amd.fit.fit (objective, backward, DeviceAdam.step(zero_grads=True)) against the same loop on
torch.optim.Adam, at the step tools/time_objective.py times (SB 4 x 64 x 64 rays x 40 samples, 400 x 300), alternating windows."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from diner_amd.optim import DeviceAdam                                        # noqa: E402
from diner_amd.synthetic import _Conf, make_mlp_state_dict, make_scene        # noqa: E402
from src.util.import_helper import import_obj                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--loop", action="store_true")
ap.add_argument("--loop-windows", type=int, default=5)
ap.add_argument("--loop-steps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda", 0)
HBM = 6.3e12


def build_nerf():
    torch.manual_seed(0)
    nerf = import_obj("src.models.pixelnerf.PixelNeRF")(
        poscode_conf=_Conf(kwargs=dict(num_freqs=6, freq_factor=6.28, include_input=True)),
        encoder_conf=_Conf("src.models.image_encoder.SpatialEncoder", dict(image_padding=64, padding_pe=4, pretrained=False)),
        mlp_fine_conf=_Conf("src.models.resnetfc.ResnetFC", dict(n_blocks=5, d_hidden=512, combine_layer=3, combine_type="average")))
    nerf.mlp_fine.load_state_dict(make_mlp_state_dict())
    return nerf.to(dev).train()


def spread(v):
    return f"{statistics.median(v):8.4f} ({min(v):.4f} .. {max(v):.4f})"


def window(fn, steps):
    """-> (stream ms per step, host enqueue ms per step)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    host = (time.perf_counter() - t) / steps * 1e3
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, host


nerf = build_nerf()
sd0 = {k: v.clone() for k, v in nerf.state_dict().items()}
params = [p for p in nerf.parameters() if p.requires_grad]
opt = DeviceAdam(params, lr=1e-4)
n_elem = sum(opt.numels)
opt.grads.normal_().mul_(1e-3)
opt.step()                                                    # builds the table
torch.cuda.synchronize()
print(f"{len(params)} parameter tensors, {n_elem} elements ({n_elem * 4 / 2 ** 20:.1f} MiB), {opt._n_chunks} chunks of <= 4096 elements, "
      f"{sum(1 for p in params if p.data_ptr() % 16)} tensors off 16-byte alignment, smallest {min(opt.numels)}, largest {max(opt.numels)}", flush=True)
t_def, t_fused = torch.optim.Adam(params, lr=1e-4), torch.optim.Adam(params, lr=1e-4, fused=True)


def dev_variant(zero, clip):
    def fn():
        opt.max_grad_norm, opt.skip_nonfinite = (1.0, True) if clip else (None, False)
        opt.step(zero_grads=zero)
    return fn


variants = [("device", dev_variant(False, False), 28), ("device+zero", dev_variant(True, False), 32), ("device+clip", dev_variant(True, True), 36),
            ("torch", t_def.step, 28), ("torch-fused", t_fused.step, 28)]
for _, fn, _ in variants:                                     # warm-up: allocations, torch's state, code objects
    for _ in range(20):
        fn()
res = {name: [] for name, _, _ in variants}
for w in range(args.windows):
    for name, fn, _ in variants:
        opt.grads.normal_().mul_(1e-3)
        res[name].append(window(fn, args.steps))
        print(f"window {w} {name:12s}: stream {res[name][-1][0]:8.4f} ms per step, host enqueue {res[name][-1][1]:8.4f} ms per step", flush=True)
print(f"median (min .. max) of {args.windows} windows of {args.steps} steps:")
for name, _, bpe in variants:
    s, h = [x[0] for x in res[name]], [x[1] for x in res[name]]
    nbytes = n_elem * bpe
    print(f"  {name:12s}: stream {spread(s)} ms, host enqueue {spread(h)} ms; {nbytes / 1e6:7.1f} MB per step by the table ({bpe} B per element) = "
          f"{nbytes / (statistics.median(s) * 1e-3) / HBM * 100:5.1f} % of 6.3 TB/s", flush=True)

if args.loop:
    import copy
    from diner_amd import objective
    from diner_amd.fit import fit
    W, H, SB, K, s = 400, 300, 4, 40, 64
    nerf.load_state_dict(sd0)                                  # the timing above let the weights drift
    opt = DeviceAdam(params, lr=1e-4)
    nerf_t = copy.deepcopy(nerf)
    for p in nerf_t.parameters():
        p.grad = None
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
    kw = dict(znear=scs[0]["znear"], zfar=scs[0]["zfar"], w_vgg=1e-30, vgg_spatch=s, w_antibias=1.0, antibias_downsampling=3,
              vgg_fn=lambda a, b: a.new_zeros(()))
    t_opt = torch.optim.Adam([p for p in nerf_t.parameters() if p.requires_grad], lr=1e-4)
    n = args.loop_steps

    def loop_fit(k0):
        fit(nerf, ren, [batch], steps=n, optimizer=opt, seed=11, start_step=k0, log_every=n, **kw)

    def loop_torch(k0):
        terms = []
        for k in range(k0, k0 + n):
            t_opt.zero_grad()
            losses = objective.calc_losses(nerf_t, ren, batch, seed=11, step=k, **kw)
            losses["total"].backward()
            t_opt.step()
            terms.append(losses["total"].detach())
        torch.stack(terms).cpu()                                # the loop's one read-back, as fit's

    loops = (("fit (DeviceAdam)", loop_fit), ("loop on torch.optim.Adam", loop_torch))
    for _, fn in loops:
        fn(0)
    out = {name: [] for name, _ in loops}
    for w in range(args.loop_windows):
        for name, fn in loops:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn(100 * (w + 1))
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t) / n * 1e3)
            print(f"loop window {w} {name:26s}: {out[name][-1]:8.2f} ms per step", flush=True)
    for name, _ in loops:
        print(f"  whole step, {name:26s}: {spread(out[name])} ms ({args.loop_windows} windows of {n} steps; {SB} objects x {s * s} rays x {K} samples, {W}x{H})", flush=True)
