"""Fixture G27 (tests/golden/g27_encoder.npz): the image encoder's trunk on seeded weights, restated in float64 torch.

    python tools/make_golden_encoder.py            # rewrites the fixture

SpatialEncoder.forward (image_encoder.py:225-291 of the reference) is written out here as plain functional torch -- replication padding,
the positional-encoding ring, the ResNet stem, pool and basic blocks with BatchNorm on its running statistics, the align-corners
upsampling and the concatenation -- so that tests/test_encoder_gpu.py can evaluate it in float64 on the CPU at run time (the drop-in's
PositionalEncoding.forward is HIP-only, so the module itself cannot run there).  Where the reference tree is present the generator also
runs the reference's own SpatialEncoder.forward in float64 on the same weights and records that the two agree to 1e-12.

The seeded state dicts are full width (resnet34: 33 MB) and are not committed: the fixture holds, per case, the seeds and shapes, a strided
sub-sample of the float64 latent, a sha256 of the state dict's bytes and `yard` -- torch's own CPU float32 distance from float64 per
pyramid level, relative to the level's maximum, the yardstick DESIGN.md 8l quotes."""
import hashlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}          # written out again (diner_amd.encoder.LAYERS is the code under test)
WIDTHS = (64, 128, 256, 512)
EPS = 1e-5
SAMPLES = 4096                       # latent elements kept per case
# name: backbone, num_layers, use_first_pool, image_padding, padding_pe, (SB, NV, H, W), weight seed, image seed
CASES = {
    "A": dict(backbone="resnet34", num_layers=4, use_first_pool=True, image_padding=4, padding_pe=4, images=(1, 2, 37, 50), seed=2701, image_seed=2711),
    "B": dict(backbone="resnet18", num_layers=5, use_first_pool=True, image_padding=8, padding_pe=4, images=(2, 2, 21, 30), seed=2702, image_seed=2712),
    "C": dict(backbone="resnet34", num_layers=3, use_first_pool=False, image_padding=0, padding_pe=-1, images=(1, 1, 16, 20), seed=2703, image_seed=2713),
    "D": dict(backbone="resnet34", num_layers=4, use_first_pool=True, image_padding=64, padding_pe=4, images=(1, 1, 60, 80), seed=2704, image_seed=2714),
}
GPU_CASES = ("A", "B", "C")          # D (the shipped padding) is the CPU-only yardstick
CONFIG_KEYS = ("backbone", "num_layers", "use_first_pool", "image_padding", "padding_pe")


def config(case):
    return {k: CASES[case][k] for k in CONFIG_KEYS}


def ring_channels(image_padding, padding_pe):
    return 0 if (padding_pe < 0 or image_padding == 0) else 2 * (2 * padding_pe + 1)


def seeded_state_dict(backbone, seed, image_padding=64, padding_pe=4):
    """A full-width `model.*` state dict of the trunk (all four stages) from torch.Generator draws on the CPU.  Convolutions: normal with
    He's standard deviation (half of it inside the blocks: the running statistics do not normalise anything here, and sixteen residual
    blocks at full gain would grow the activations by orders of magnitude); BatchNorm: gamma in [0.5, 1.5], beta and the running mean
    0.2 normal, the running variance in [0.25, 1.75] -- nothing a folding mistake could cancel against."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, cout, cin, r, gain=0.5):
        sd[name + ".weight"] = torch.randn(cout, cin, r, r, generator=g) * float(gain * np.sqrt(2.0 / (cin * r * r)))

    def bn(name, c):
        sd[name + ".weight"] = 0.5 + torch.rand(c, generator=g)
        sd[name + ".bias"] = 0.2 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.2 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 0.25 + 1.5 * torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(100)

    conv("model.conv1", 64, 3 + ring_channels(image_padding, padding_pe), 7, gain=1.0)
    bn("model.bn1", 64)
    cin = 64
    for i, n in enumerate(BLOCKS[backbone]):
        c = WIDTHS[i]
        for j in range(n):
            p = f"model.layer{i + 1}.{j}."
            conv(p + "conv1", c, cin, 3)
            bn(p + "bn1", c)
            conv(p + "conv2", c, c, 3)
            bn(p + "bn2", c)
            if j == 0 and i > 0:
                conv(p + "downsample.0", c, cin, 1)
                bn(p + "downsample.1", c)
            cin = c
    return sd


def state_dict(case):
    c = CASES[case]
    return seeded_state_dict(c["backbone"], c["seed"], c["image_padding"], c["padding_pe"])


def sha256_of(sd):
    """sha256 over the keys (sorted) and the bytes of their tensors."""
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def images_of(case):
    SB, NV, H, W = CASES[case]["images"]
    g = torch.Generator().manual_seed(CASES[case]["image_seed"])
    return torch.rand(SB, NV, 3, H, W, generator=g) * 2 - 1            # normalised images: (rgb - 0.5) / 0.5


def ring_plane(H, W, p, num_freqs, dtype):
    """(H + 2 p, W + 2 p, 2 (2 num_freqs + 1)): [x, y, sin(f0 x), sin(f0 y), cos(f0 x), cos(f0 y), sin(f1 x), ...] of the pixel grid in
    [-1, 1]^2 with f_k = pi 2^k, zero inside the image.  As the reference evaluates it: the grid and the frequencies are float32 values, the
    cosine is sin(. + float32(pi / 2)), the arithmetic runs in `dtype`."""
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H + 2 * p), torch.linspace(-1, 1, W + 2 * p), indexing="ij")
    xy = torch.stack((xs, ys), dim=-1).to(dtype)                                     # x first
    freqs = (np.pi * 2.0 ** torch.arange(0, num_freqs)).to(torch.float32).to(dtype)
    half_pi = torch.tensor(np.pi * 0.5, dtype=torch.float32).to(dtype)
    parts = [xy]
    for f in freqs:
        parts += [torch.sin(xy * f), torch.sin(half_pi + xy * f)]
    pe = torch.cat(parts, dim=-1)
    pe[p:-p, p:-p] = 0
    return pe


def levels_restated(sd, images, dtype=torch.float64, backbone="resnet34", num_layers=4, use_first_pool=True, image_padding=64, padding_pe=4):
    """The pyramid levels of SpatialEncoder.forward in eval mode, before the upsampling: [(N,C_l,h_l,w_l)] in `dtype`."""
    SB, NV, _, H, W = images.shape
    p = image_padding
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}

    def bn(x, name):
        return F.batch_norm(x, w[name + ".running_mean"], w[name + ".running_var"], w[name + ".weight"], w[name + ".bias"], False, 0.0, EPS)

    x = images.reshape(SB * NV, 3, H, W).to(dtype)
    if p > 0:
        x = F.pad(x, (p, p, p, p), mode="replicate")
    if ring_channels(p, padding_pe):
        pe = ring_plane(H, W, p, padding_pe, dtype)
        x = torch.cat((x, pe.permute(2, 0, 1).unsqueeze(0).expand(SB * NV, -1, -1, -1)), dim=1)
    x = F.relu(bn(F.conv2d(x, w["model.conv1.weight"], stride=2, padding=3), "model.bn1"))
    levels = [x]
    for i in range(num_layers - 1):
        if i == 0 and use_first_pool:
            x = F.max_pool2d(x, 3, 2, 1)
        for j in range(BLOCKS[backbone][i]):
            q = f"model.layer{i + 1}.{j}."
            stride = 2 if (j == 0 and i > 0) else 1
            idt = x
            if q + "downsample.0.weight" in w:
                idt = bn(F.conv2d(x, w[q + "downsample.0.weight"], stride=stride), q + "downsample.1")
            y = F.relu(bn(F.conv2d(x, w[q + "conv1.weight"], stride=stride, padding=1), q + "bn1"))
            y = bn(F.conv2d(y, w[q + "conv2.weight"], padding=1), q + "bn2")
            x = F.relu(y + idt)
        levels.append(x)
    return levels


def trunk_restated(sd, images, dtype=torch.float64, **cfg):
    """SpatialEncoder.forward's latent (SB,NV,L,Hf,Wf) in `dtype` (cfg: backbone, num_layers, use_first_pool, image_padding, padding_pe)."""
    levels = levels_restated(sd, images, dtype, **cfg)
    size = levels[0].shape[-2:]
    lat = torch.cat([F.interpolate(l, size, mode="bilinear", align_corners=True) for l in levels], dim=1)
    return lat.view(images.shape[0], images.shape[1], -1, *size)


def level_slices(num_layers):
    """The channel range of each pyramid level in the latent."""
    out, c0 = [], 0
    for c in ((64,) + WIDTHS)[:num_layers]:
        out.append(slice(c0, c0 + c))
        c0 += c
    return out


def subsample(lat):
    """A strided sub-sample of the latent (float64, 1-D) and its stride."""
    flat = lat.reshape(-1)
    stride = max(1, flat.numel() // SAMPLES) | 1
    return flat[::stride].clone(), stride


def reference_latent(sd, images, cfg):
    """The reference's own SpatialEncoder.forward in float64 on the CPU, or None where the reference tree is absent.  torchvision is not
    installed: the reference gets a trunk with torchvision's module names (the drop-in's _ResNetTrunk) in its place."""
    from oracle import ref_import
    if not ref_import.reference_available():
        return None
    from src.models.image_encoder import _ResNetTrunk
    ns = ref_import.import_reference()
    models = ns.image_encoder.torchvision.models
    for name, blocks in BLOCKS.items():
        setattr(models, name, lambda pretrained=False, norm_layer=None, _b=blocks: _ResNetTrunk(list(_b), norm_layer))
    enc = ns.image_encoder.SpatialEncoder(backbone=cfg["backbone"], pretrained=False, num_layers=cfg["num_layers"],
                                          use_first_pool=cfg["use_first_pool"], image_padding=cfg["image_padding"], padding_pe=cfg["padding_pe"])
    missing = enc.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("positional_encoding.") for k in missing.missing_keys), missing
    enc = enc.double().eval()
    with torch.no_grad():
        enc(images.double(), None, None, None)
    return enc.latent


def yard_of(sd, images, cfg):
    """torch's CPU float32 evaluation against float64, per level: max |difference| / max |level| -> (float64 latent, [yard])."""
    with torch.no_grad():
        l64 = trunk_restated(sd, images, torch.float64, **cfg)
        l32 = trunk_restated(sd, images, torch.float32, **cfg).double()
    yard = [float((l32[:, :, s] - l64[:, :, s]).abs().max() / l64[:, :, s].abs().max()) for s in level_slices(cfg["num_layers"])]
    return l64, yard


def main():
    out = {}
    for case, c in CASES.items():
        cfg, sd, images = config(case), state_dict(case), images_of(case)
        l64, yard = yard_of(sd, images, cfg)
        ref = reference_latent(sd, images, cfg)
        ref_rel = float("nan") if ref is None else float((ref - l64).abs().max() / l64.abs().max())
        assert ref is None or (ref.shape == l64.shape and ref_rel <= 1e-12), (case, ref_rel)
        sub, stride = subsample(l64)
        out[f"{case}_shape"] = np.array(l64.shape, dtype=np.int64)
        out[f"{case}_images"] = np.array(c["images"], dtype=np.int64)
        out[f"{case}_seeds"] = np.array([c["seed"], c["image_seed"]], dtype=np.int64)
        out[f"{case}_sub64"], out[f"{case}_stride"] = sub.numpy(), np.int64(stride)
        out[f"{case}_sha256"] = np.array(sha256_of(sd))
        out[f"{case}_yard"] = np.array(yard, dtype=np.float64)
        out[f"{case}_ref_rel"] = np.float64(ref_rel)
        out[f"{case}_absmax"] = np.float64(l64.abs().max())
        print(f"case {case} {cfg} images {c['images']} -> latent {tuple(l64.shape)}, |latent| <= {float(l64.abs().max()):.3f}, yard "
              f"{[f'{y:.2e}' for y in yard]}, reference rel {ref_rel:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "g27_encoder.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
