"""Generate tests/golden/g22_long_rays.npz from the IMPORTED reference (build container only; read-only use of the reference).

    python tools/make_golden_long_rays.py

The reference's NeRFRendererDGS.sample_depthguided (unfilled), fill_up_uniform_samples and composite run with injected noise
(oracle/make_golden.py's inject_noise) on 64 rays of the seeded 64x64 scene at the long-ray sizes (K, n_cand, G) =
(512, 1000, 192) and (1024, 4096, 384): what create_prediction_folder.py --nsamples 512 / 1024 asks for.  The oracle
restatement is compared against it on the same inputs, and the reference's outputs are stored.  Inputs are regenerated from
seeds (their sha256 is stored)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import diner_oracle as O                                   # noqa: E402
from oracle.make_golden import inject_noise, setup, report, sha        # noqa: E402
from oracle.ref_import import import_reference                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g22_long_rays.npz")
CONFIGS = ((512, 1000, 192, False), (1024, 4096, 384, True))          # (K, n_cand, G, white_bkgd of the composite)
NR, W, H, SEED, NOISE_SEED = 64, 64, 64, 0, 122


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    ns = import_reference()
    R = ns.nerf_renderer.NeRFRendererDGS
    sc, nerf, scene, w, rays = setup(ns, W, H, seed=SEED)
    g = torch.Generator().manual_seed(NOISE_SEED)
    sel = torch.randperm(W * H, generator=g)[:NR].sort().values
    rs = rays[sel].contiguous()
    gold = dict(W=W, H=H, seed=SEED, noise_seed=NOISE_SEED, ray_idx=sel.numpy(), rays=rs.numpy(),
                configs=np.array([c[:3] for c in CONFIGS]), white=np.array([int(c[3]) for c in CONFIGS]))
    with torch.no_grad():
        for (K, n_cand, G, white) in CONFIGS:
            print(f"K={K} n_cand={n_cand} G={G} white={white}")
            nc, ng, nf = torch.rand(NR, n_cand, generator=g), torch.randn(NR, G, generator=g), torch.rand(NR, K, generator=g)
            ren = R(n_samples=K, n_depth_candidates=n_cand, n_gaussian=G, white_bkgd=white)
            with inject_noise(nc, ng, nf):
                z0_ref = ren.sample_depthguided(rs[None], nerf, n_samples=K, n_candidates=n_cand, n_gaussian=G)[0]
                z_ref = ren.fill_up_uniform_samples(z0_ref[None].clone(), rs[None])[0]
            w_ref, rgb_ref, d_ref = (t[0] for t in ren.composite(nerf, rs[None], z_ref[None]))
            z0, aux = O.sample_depthguided(scene, rs, K, n_cand, G, nc, ng, return_aux=True)
            report("z unfilled", z0_ref, z0, exact=True)
            report("z filled", z_ref, O.fill_up_uniform_samples(z0, rs, nf), exact=True)
            wo, rgbo, do, _ = O.composite(scene, w, rs, z_ref, white)
            report("composite rgb", rgb_ref, rgbo)
            report("composite depth", d_ref, do)
            report("composite weights", w_ref, wo)
            Ls = aux["L"].sort(dim=-1, descending=True).values
            ties = ((Ls[:, K - G - 1] == Ls[:, K - G]) & (Ls[:, K - G] > 0)).nonzero().flatten()
            print(f"  rays with surface {(aux['O'] != 0).any(-1).sum().item()}/{NR}, ties at the cut-off {ties.tolist()}, "
                  f"zeros before the fill {(z0 == 0).sum().item()}")
            gold.update({f"in_sha_{K}": sha(nc, ng, nf), f"tie_rays_{K}": ties.numpy(), f"L_sum_{K}": aux["L"].sum(-1).numpy(),
                         f"z_unfilled_{K}": z0_ref.numpy(), f"z_{K}": z_ref.numpy(), f"weights_{K}": w_ref.numpy(),
                         f"rgb_{K}": rgb_ref.numpy(), f"depth_{K}": d_ref.numpy()})
    np.savez_compressed(OUT, **gold)
    print("wrote", OUT, f"{os.path.getsize(OUT) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
