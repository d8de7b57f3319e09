"""Generate tests/golden/g23_many_views.npz from the IMPORTED reference (build container only; read-only use of the reference).

    python tools/make_golden_many_views.py

The reference's PixelNeRF takes any number of source views (pixelnerf.py:67, :91-128; resnetfc.py:150-152 averages them; the
depth-guided sampler takes the maximum likelihood over them, nerf_renderer.py:95-135).  Here it runs on seeded 48 x 48 scenes of
diner_amd.synthetic.make_scene(nv=NV) at NV = 6, 8 and 16 with the shipped MLP shape and injected noise (oracle/make_golden.py's
inject_noise):
  - NeRFRendererDGS.sample_depthguided (unfilled) and fill_up_uniform_samples on 64 rays at K = 64 / n_cand = 1000 / G = 24, and at
    NV = 8 once more at K = 320 / G = 96 (the wide sampler's range);
  - renderer.forward's rgb and depth on the same rays at K = 64;
  - at NV = 6 one grad-mode step with non-init weights (synthetic.realistic_mlp_state_dict, as G20): renderer.forward on 32 rays x 16
    samples with the latent requiring grad, MSE of the colours against seeded targets, .backward(); stored: the loss, the samples, the
    lin_out and blocks.0.fc_0 gradients (fc_0's weight every 8th row) and the latent gradient at 128 seeded texels it reaches.
The oracle restatement is compared against the reference on the same inputs.  Inputs are regenerated from seeds (their sha256 is
stored)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import diner_oracle as O                                   # noqa: E402
from oracle.make_golden import inject_noise, report, sha               # noqa: E402
from oracle.ref_import import import_reference, build_reference_nerf   # noqa: E402
from diner_amd.synthetic import make_scene, make_mlp_state_dict, realistic_mlp_state_dict   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g23_many_views.npz")
W = H = 48
NVS = (6, 8, 16)
NR, K, N_CAND, G = 64, 64, 1000, 24
K_WIDE, G_WIDE, NV_WIDE = 320, 96, 8
NR_T, K_T, G_T, NV_T = 32, 16, 6, 6
SCENE_SEED, RAY_SEED, NOISE_SEED, MLP_SEED, TRAIN_SEED = 23, 230, 231, 4321, 232
N_TEXELS = 128


def reference_model(ns, sc, normals, msd):
    nerf = build_reference_nerf(ns)
    nerf.mlp_fine.load_state_dict(msd, strict=True)
    enc = nerf.encoder
    nv = sc["src_extrinsics"].shape[0]
    enc.depths, enc.depths_std, enc.normals = sc["depths"][None], sc["depths_std"][None], normals[None]
    enc.latent = sc["latent"][None]
    enc.nviews, enc.nobjects = nv, 1
    nerf.poses = sc["src_extrinsics"][None]
    nerf.c = sc["src_intrinsics"][None, :, :2, -1]
    nerf.focal = sc["src_intrinsics"][None][:, :, [0, 1], [0, 1]]
    nerf.image_shape = sc["image_shape"].clone()
    return nerf


def oracle_scene(sc, normals, nerf):
    return O.Scene(latent=sc["latent"], depths=sc["depths"], depths_std=sc["depths_std"], normals=normals, poses=sc["src_extrinsics"],
                   focal=nerf.focal[0], c=nerf.c[0], image_shape=sc["image_shape"], feature_padding=float(nerf.encoder.feature_padding))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ns = import_reference()
    R = ns.nerf_renderer.NeRFRendererDGS
    msd = make_mlp_state_dict()
    gold = dict(W=W, H=H, nvs=np.array(NVS), NR=NR, K=K, n_cand=N_CAND, G=G, K_wide=K_WIDE, G_wide=G_WIDE, nv_wide=NV_WIDE,
                scene_seed=SCENE_SEED, ray_seed=RAY_SEED, noise_seed=NOISE_SEED, mlp_seed=MLP_SEED, train_seed=TRAIN_SEED,
                NR_t=NR_T, K_t=K_T, G_t=G_T, nv_t=NV_T)
    g = torch.Generator().manual_seed(RAY_SEED)
    sel = torch.randperm(W * H, generator=g)[:NR].sort().values
    gold["ray_idx"] = sel.numpy()
    for nv in NVS:
        print(f"NV={nv}")
        sc = make_scene(W, H, nv=nv, seed=SCENE_SEED)
        normals = ns.depth2normal.depth2normal(sc["depths"], sc["src_intrinsics"])
        nerf = reference_model(ns, sc, normals, msd)
        scene = oracle_scene(sc, normals, nerf)
        w = O.MLPWeights.from_state_dict(msd)
        rays = ns.cam_geometry.gen_rays(sc["target_extrinsics"][None], sc["target_intrinsics"][None], W, H,
                                        torch.tensor([sc["znear"]]), torch.tensor([sc["zfar"]])).view(H * W, 8)
        rs = rays[sel].contiguous()
        gn = torch.Generator().manual_seed(NOISE_SEED + nv)
        cfgs = [(K, G)] + ([(K_WIDE, G_WIDE)] if nv == NV_WIDE else [])
        for (k, gg) in cfgs:
            nc, ng, nf = torch.rand(NR, N_CAND, generator=gn), torch.randn(NR, gg, generator=gn), torch.rand(NR, k, generator=gn)
            ren = R(n_samples=k, n_depth_candidates=N_CAND, n_gaussian=gg, white_bkgd=False)
            with torch.no_grad(), inject_noise(nc, ng, nf):
                z0_ref = ren.sample_depthguided(rs[None], nerf, n_samples=k, n_candidates=N_CAND, n_gaussian=gg)[0]
                z_ref = ren.fill_up_uniform_samples(z0_ref[None].clone(), rs[None])[0]
            z0, aux = O.sample_depthguided(scene, rs, k, N_CAND, gg, nc, ng, return_aux=True)
            report(f"nv{nv} K{k} z unfilled", z0_ref, z0, exact=True)
            report(f"nv{nv} K{k} z filled", z_ref, O.fill_up_uniform_samples(z0, rs, nf), exact=True)
            tag = f"{nv}_{k}"
            gold.update({f"in_sha_{tag}": sha(nc, ng, nf), f"z_unfilled_{tag}": z0_ref.numpy(), f"z_{tag}": z_ref.numpy(),
                         f"L_sum_{tag}": aux["L"].sum(-1).numpy()})
            print(f"  K={k}: rays with surface {(aux['O'] != 0).any(-1).sum().item()}/{NR}, zeros before the fill {(z0 == 0).sum().item()}")
            if k == K:
                ren = R(n_samples=k, n_depth_candidates=N_CAND, n_gaussian=gg, white_bkgd=False)
                with torch.no_grad(), inject_noise(nc, ng, nf):
                    o = ren.forward(nerf, rs[None])
                oo = O.render(scene, w, rs, k, N_CAND, gg, False, nc, ng, nf)
                report(f"nv{nv} rgb", o.fine.rgb[0], oo["rgb"])
                report(f"nv{nv} depth", o.fine.depth[0], oo["depth"])
                gold.update({f"rgb_{nv}": o.fine.rgb[0].numpy(), f"depth_{nv}": o.fine.depth[0].numpy()})
        gold[f"rays_{nv}"] = rs.numpy()
        gold[f"latent_sha_{nv}"] = sha(sc["latent"][:, :4, :8, :8], sc["latent"][:, -4:, -8:, -8:])

    # ---- one grad-mode step at NV_T with non-init weights
    print(f"grad step NV={NV_T}")
    sc = make_scene(W, H, nv=NV_T, seed=SCENE_SEED)
    normals = ns.depth2normal.depth2normal(sc["depths"], sc["src_intrinsics"])
    rsd = realistic_mlp_state_dict(MLP_SEED)
    nerf = reference_model(ns, sc, normals, rsd)
    lat = sc["latent"][None].clone().requires_grad_()
    nerf.encoder.latent = lat
    rays = ns.cam_geometry.gen_rays(sc["target_extrinsics"][None], sc["target_intrinsics"][None], W, H,
                                    torch.tensor([sc["znear"]]), torch.tensor([sc["zfar"]])).view(H * W, 8)
    gt = torch.Generator().manual_seed(TRAIN_SEED)
    idx = torch.randperm(W * H, generator=gt)[:NR_T].sort().values
    rs = rays[idx].contiguous()
    nc, ng, nf = torch.rand(NR_T, N_CAND, generator=gt), torch.randn(NR_T, G_T, generator=gt), torch.rand(NR_T, K_T, generator=gt)
    target = torch.rand(NR_T, 3, generator=gt)
    ren = R(n_samples=K_T, n_depth_candidates=N_CAND, n_gaussian=G_T, white_bkgd=False)
    with inject_noise(nc, ng, nf):
        o = ren.forward(nerf, rs[None])
    with torch.no_grad(), inject_noise(nc, ng, nf):
        z_t = ren.fill_up_uniform_samples(ren.sample_depthguided(rs[None], nerf, n_samples=K_T, n_candidates=N_CAND, n_gaussian=G_T),
                                          rs[None])[0]
    loss = torch.nn.functional.mse_loss(o.fine.rgb[0], target)
    loss.backward()
    pg = {n: p.grad for n, p in nerf.mlp_fine.named_parameters()}
    # the oracle's autograd on the reference's samples
    scene = oracle_scene(sc, normals, nerf)
    scene.latent = sc["latent"].clone().requires_grad_()
    w = O.MLPWeights.from_state_dict(rsd)
    w.lin_out_w.requires_grad_()
    xyz = (rs[:, None, :3] + z_t[..., None] * rs[:, None, 3:6]).reshape(-1, 3)
    dirs = rs[:, None, 3:6].expand(-1, K_T, -1).reshape(-1, 3)
    f = O.pixelnerf_forward(scene, w, xyz, dirs).view(NR_T, K_T, 4)
    _, rgb_o, _ = O.composite_from_field(f, rs, z_t, False)
    loss_o = torch.nn.functional.mse_loss(rgb_o, target)
    loss_o.backward()
    report("train loss", loss.detach()[None], loss_o.detach()[None])
    report("train d lin_out.weight", pg["lin_out.weight"], w.lin_out_w.grad)
    report("train d latent", lat.grad[0], scene.latent.grad)
    # the latent gradient at N_TEXELS seeded texels among those it reaches (view, y, x), all channels
    gl = lat.grad[0]                                                   # (NV, C, Hf, Wf)
    hit = (gl.abs().sum(1) != 0).nonzero()                             # (n, 3): v, y, x
    pick = hit[torch.randperm(hit.shape[0], generator=gt)[:N_TEXELS].sort().values]
    gold.update({"t_ray_idx": idx.numpy(), "t_rays": rs.numpy(), "t_in_sha": sha(nc, ng, nf, target), "t_target": target.numpy(),
                 "t_z": z_t.numpy(), "t_loss": loss.detach().numpy(), "t_rgb": o.fine.rgb[0].detach().numpy(),
                 "t_mlp_sha": sha(*[rsd[k] for k in sorted(rsd)]),
                 "t_g_lin_out_w": pg["lin_out.weight"].numpy(), "t_g_lin_out_b": pg["lin_out.bias"].numpy(),
                 "t_g_fc0_w_rows8": pg["blocks.0.fc_0.weight"][::8].numpy(), "t_g_fc0_b": pg["blocks.0.fc_0.bias"].numpy(),
                 "t_g_fc0_w_absmax": float(pg["blocks.0.fc_0.weight"].abs().max()),
                 "t_g_lat_texels": pick.numpy(), "t_g_lat": gl[pick[:, 0], :, pick[:, 1], pick[:, 2]].numpy(),
                 "t_g_lat_absmax": float(gl.abs().max()), "t_g_lat_nonzero_texels": int(hit.shape[0])})
    np.savez_compressed(OUT, **gold)
    print("wrote", OUT, f"{os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
