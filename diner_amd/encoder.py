"""The image encoder's trunk on the device: SpatialEncoder.forward's ResNet feature pyramid (image_encoder.py:225-291 of the reference)
in this library's own kernels (csrc/encoder.hip + the convolutions of csrc/conv2d.hip), for inference.

    trunk = DeviceTrunk(nerf.encoder)                      # or a state dict with torchvision's key names (`model.*`)
    latent = trunk(images)                                 # (SB,NV,3,H,W) normalised, on the HIP device -> (SB,NV,L,Hf,Wf)

Eval mode only: BatchNorm uses its running statistics and is folded into the convolutions.  Everything is fp32, activations
channels-last; the latent comes back with NCHW shape and channels-last strides, the format HipScene aliases without a copy.  There is no
gradient, no CPU path and no host synchronisation inside a call.  SpatialEncoder.device_trunk = True routes forward() through this."""
import collections

import numpy as np
import torch

LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
PLANES = (64, 128, 256, 512)
BN_EPS = 1e-5                    # torchvision's BatchNorm2d default; a module's own eps is read from it

# one folded convolution on the device: w packed for the kernel that runs it, b zero-padded to the packed width
Conv = collections.namedtuple("Conv", "w b Cin Cout R stride")
Block = collections.namedtuple("Block", "conv1 conv2 down")


def fold_bn(w, gamma, beta, mean, var, eps=BN_EPS):
    """BatchNorm in eval mode folded into the convolution before it: s = gamma / sqrt(var + eps), w' = w s, b' = beta - mean s, computed in
    float64 -> (w', b') float64 (the caller rounds once to fp32)."""
    s = gamma.detach().double() / torch.sqrt(var.detach().double() + eps)
    return w.detach().double() * s.view(-1, 1, 1, 1), beta.detach().double() - mean.detach().double() * s


def conv_names(backbone, num_layers):
    """[(conv key, bn key prefix)] of every convolution the trunk runs for `num_layers` pyramid levels, in execution order, without the
    `model.` prefix."""
    names = [("conv1", "bn1")]
    for i in range(max(0, num_layers - 1)):
        for j in range(LAYERS[backbone][i]):
            p = f"layer{i + 1}.{j}."
            names += [(p + "conv1", p + "bn1"), (p + "conv2", p + "bn2")]
            if i > 0 and j == 0:
                names.append((p + "downsample.0", p + "downsample.1"))
    return names


def _hip_device(t):
    if not t.is_cuda:
        raise RuntimeError("diner_amd.encoder: the trunk runs on the HIP device; there is no CPU fallback")
    return t.device


class DeviceTrunk:
    """The trunk of `source` -- a SpatialEncoder (its configuration is read from the module and the keyword arguments are ignored) or a
    state-dict-like mapping with torchvision's key names, with or without the `model.` prefix -- for resnet18 / resnet34, 1 .. 5 pyramid
    levels, with or without the first pool, and with or without the padding ring (padding_pe < 0 or image_padding = 0: the stem has 3
    input channels).

    The weights are folded, packed and uploaded at the first call and again whenever the (data_ptr, _version) of any tensor read changes:
    load_state_dict, optimiser steps and every other in-place operation on the parameters and buffers are seen.  A write through `.data`
    bumps no version counter: call invalidate() after one."""

    def __init__(self, source, backbone="resnet34", num_layers=4, use_first_pool=True, image_padding=64, padding_pe=4,
                 upsample_interp="bilinear"):
        self._module = None
        self._eps = {}
        if isinstance(source, torch.nn.Module):
            self._module = source
            num_layers, use_first_pool = source.num_layers, source.use_first_pool
            image_padding, padding_pe, upsample_interp = source.image_padding, source.padding_pe, source.upsample_interp
            if getattr(source, "index_interp", "bilinear") == "nearest ":
                raise NotImplementedError("diner_amd.encoder: index_interp 'nearest ' (align_corners=None upsampling) is not built")
            keys = source.state_dict().keys()
            self._eps = {n: m.eps for n, m in source.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
        elif hasattr(source, "keys"):
            self._mapping = source
            keys = source.keys()
        else:
            raise ValueError(f"diner_amd.encoder: expected a SpatialEncoder or a state-dict-like mapping, got {type(source).__name__}")
        if upsample_interp != "bilinear":
            raise NotImplementedError(f"diner_amd.encoder: upsample_interp {upsample_interp!r} (only 'bilinear' is built)")
        self._prefix = "model." if "model.conv1.weight" in keys else ""
        if self._prefix + "conv1.weight" not in keys:
            raise ValueError("diner_amd.encoder: no 'model.conv1.weight' / 'conv1.weight' among the keys: not a ResNet trunk's state dict")
        counts = tuple(len({k[len(self._prefix):].split(".")[1] for k in keys if k.startswith(f"{self._prefix}layer{i}.")}) for i in range(1, 5))
        if self._module is not None:
            found = [b for b, c in LAYERS.items() if c == counts]
            if not found:
                raise NotImplementedError(f"diner_amd.encoder: blocks per stage {counts}: only {sorted(LAYERS)} are built")
            backbone = found[0]
        if backbone not in LAYERS:
            raise NotImplementedError(f"diner_amd.encoder: backbone {backbone!r}: only {sorted(LAYERS)} are built")
        if not 1 <= int(num_layers) <= 5:
            raise ValueError(f"diner_amd.encoder: num_layers = {num_layers} (need 1 .. 5)")
        self.backbone, self.num_layers, self.use_first_pool = backbone, int(num_layers), bool(use_first_pool)
        self.image_padding, self.padding_pe = int(image_padding), int(padding_pe)
        if self.image_padding < 0 or self.image_padding % 2:
            raise ValueError(f"diner_amd.encoder: image_padding = {image_padding} (need an even number >= 0: the stem halves it)")
        self.ring_channels = 0 if (self.padding_pe < 0 or self.image_padding == 0) else 2 * (2 * self.padding_pe + 1)
        self.stem_cin = -(-(3 + self.ring_channels) // 4) * 4         # the input kernel writes zero channels up to a multiple of 4: float4 loads
        self.latent_size = [0, 64, 128, 256, 512, 1024][self.num_layers]
        self._names = conv_names(backbone, self.num_layers)
        self._key = None
        self._stem, self._stages = None, None
        self._ring = (None, None)
        self._workspace = None
        self.packs = 0                 # times the weights were folded and packed (tests, diagnostics)

    # ---- weights --------------------------------------------------------------------------------------------------------------------------
    def _tensors(self):
        sd = self._module.state_dict(keep_vars=True) if self._module is not None else self._mapping
        out = {}
        for conv, bn in self._names:
            for k in (conv + ".weight", bn + ".weight", bn + ".bias", bn + ".running_mean", bn + ".running_var"):
                if self._prefix + k not in sd:
                    raise ValueError(f"diner_amd.encoder: the {self.backbone} trunk with {self.num_layers} levels needs the key "
                                     f"'{self._prefix + k}'")
                out[k] = sd[self._prefix + k]
        return out

    def invalidate(self):
        """Forget the packed weights: the next call folds and packs again (needed after a write through `.data`)."""
        self._key = None

    def _ensure_packed(self, device):
        from . import ops
        t = self._tensors()
        key = (str(device),) + tuple((k, v.data_ptr(), v._version) for k, v in t.items())
        if key == self._key:
            return
        convs = {}
        for conv, bn in self._names:
            w = t[conv + ".weight"]
            stem, down = conv == "conv1", "downsample" in conv
            R = 7 if stem else 1 if down else 3
            # torchvision's strides: the stem, and the first block of layer2 .. layer4 (its conv1 and its downsample)
            stride = 2 if (stem or down or (conv.endswith(".0.conv1") and not conv.startswith("layer1."))) else 1
            if w.dim() != 4 or tuple(w.shape[2:]) != (R, R):
                raise ValueError(f"diner_amd.encoder: '{conv}.weight' has shape {tuple(w.shape)}, expected (Cout,Cin,{R},{R})")
            Cout, Cin = int(w.shape[0]), int(w.shape[1])
            eps = self._eps.get(self._prefix + bn, BN_EPS)
            w64, b64 = fold_bn(w, t[bn + ".weight"], t[bn + ".bias"], t[bn + ".running_mean"], t[bn + ".running_var"], eps)
            wf = w64.to(torch.float32).to(device)
            if stem:
                if Cin != 3 + self.ring_channels:
                    raise ValueError(f"diner_amd.encoder: the stem has {Cin} input channels, the configuration (image_padding {self.image_padding}, "
                                     f"padding_pe {self.padding_pe}) needs {3 + self.ring_channels}")
                Cin = self.stem_cin
            pack = ops.pack_conv_s2(wf, Cin) if stride == 2 else ops.pack_conv3x3(wf)
            b = torch.zeros(pack.shape[3], dtype=torch.float32, device=device)
            b[:Cout] = b64.to(torch.float32).to(device)
            convs[conv] = Conv(pack, b, Cin, Cout, R, stride)
        self._stem = convs["conv1"]
        self._stages = []
        for i in range(self.num_layers - 1):
            blocks = []
            for j in range(LAYERS[self.backbone][i]):
                p = f"layer{i + 1}.{j}."
                blocks.append(Block(convs[p + "conv1"], convs[p + "conv2"], convs.get(p + "downsample.0")))
            self._stages.append(blocks)
        self._key = key
        self.packs += 1

    # ---- shapes and buffers ---------------------------------------------------------------------------------------------------------------
    def plan(self, N, H, W):
        """-> ([(name, shape)] of the workspace buffers of a call on N images of H x W, (Hf, Wf) of the latent)."""
        from .ops import conv_s2_out_size
        p = self.image_padding
        Hp, Wp = H + 2 * p, W + 2 * p
        h, w = conv_s2_out_size(Hp, 7), conv_s2_out_size(Wp, 7)
        Hf, Wf = h, w
        shapes = [("input", (N, Hp, Wp, self.stem_cin))]
        if not self._stem_direct:
            shapes.append(("level0", (N, h, w, 64)))
        if self.num_layers > 1:
            if self.use_first_pool:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
                shapes.append(("pool", (N, h, w, 64)))
            for i in range(self.num_layers - 1):
                if i > 0:
                    h, w = conv_s2_out_size(h, 3), conv_s2_out_size(w, 3)
                shapes += [(f"s{i}{k}", (N, h, w, PLANES[i])) for k in ("a", "b", "t") + (("d",) if i > 0 else ())]
        return shapes, (Hf, Wf)

    @property
    def _stem_direct(self):
        # the stem writes channels 0 .. 63 of the latent itself unless a stride-1 convolution (dense input) reads its output next
        return self.num_layers == 1 or self.use_first_pool

    def _buffers(self, shapes, device):
        sizes = [-(-int(np.prod(s)) // 4) * 4 for _, s in shapes]              # every buffer starts 16-byte aligned
        total = sum(sizes)
        ws = self._workspace
        if ws is None or ws.device != device or ws.numel() < total:
            self._workspace = ws = torch.empty(total, dtype=torch.float32, device=device)
        out, at = {}, 0
        for (name, s), n in zip(shapes, sizes):
            out[name] = ws[at:at + int(np.prod(s))].view(s)
            at += n
        return out

    def _ring_plane(self, H, W, device):
        """The (H + 2 p, W + 2 p, 18) positional encoding of the padding ring, zero inside the image (image_encoder.py:245-251 of the
        reference), computed once per (H, W, p, device) with the ops the torch route uses."""
        from . import ops
        if self.ring_channels == 0:
            return None
        key = (H, W, self.image_padding, str(device))
        if self._ring[0] != key:
            p = self.image_padding
            ys, xs = torch.meshgrid(torch.linspace(-1, 1, H + 2 * p, device=device), torch.linspace(-1, 1, W + 2 * p, device=device), indexing="ij")
            pe = ops.posenc(torch.stack((xs, ys), dim=-1), self.padding_pe, float(np.pi), True).clone()
            pe[p:-p, p:-p] = 0
            self._ring = (key, pe.contiguous())
        return self._ring[1]

    # ---- the call -------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, images):
        from . import ops
        if not torch.is_tensor(images) or images.dim() != 5 or images.shape[2] != 3 or min(images.shape) < 1:
            raise ValueError(f"diner_amd.encoder: expected images (SB,NV,3,H,W), got "
                             f"{tuple(images.shape) if torch.is_tensor(images) else type(images).__name__}")
        if images.dtype != torch.float32:
            raise ValueError(f"diner_amd.encoder: expected float32 images, got {images.dtype}")
        device = _hip_device(images)
        SB, NV, _, H, W = (int(s) for s in images.shape)
        N = SB * NV
        with torch.cuda.device(device):
            self._ensure_packed(device)
            shapes, (Hf, Wf) = self.plan(N, H, W)
            B = self._buffers(shapes, device)
            L = self.latent_size
            x = ops.encoder_input(images.detach().reshape(N, 3, H, W).contiguous(), self._ring_plane(H, W, device), self.image_padding,
                                  C=self.stem_cin, out=B["input"])
            lat = torch.empty(N, Hf, Wf, L, dtype=torch.float32, device=device)
            st = self._stem
            if self._stem_direct:
                ops.conv_s2(x, st.w, st.b, 64, 7, relu=True, out=lat, coff=0)
                cur = None
            else:
                cur = ops.conv_s2(x, st.w, st.b, 64, 7, relu=True, out=B["level0"])
                ops.pyramid_level(cur, lat, 0)
            c0 = 64
            if self.num_layers > 1:
                if self.use_first_pool:
                    cur = ops.maxpool3s2(lat, C=64, out=B["pool"])
                for i, blocks in enumerate(self._stages):
                    a, b, t, c = B[f"s{i}a"], B[f"s{i}b"], B[f"s{i}t"], PLANES[i]
                    for blk in blocks:
                        y = b if cur is a else a
                        if blk.down is not None:
                            # conv1 and the downsample read the same input
                            ops.conv_s2(cur, blk.conv1.w, blk.conv1.b, c, 3, relu=True, out=t)
                            idt = ops.conv_s2(cur, blk.down.w, blk.down.b, c, 1, relu=False, out=B[f"s{i}d"])
                        else:
                            ops.conv3x3(cur, blk.conv1.w, blk.conv1.b, c, relu=True, out=t)
                            idt = cur
                        cur = ops.conv3x3(t, blk.conv2.w, blk.conv2.b, c, relu=True, addend=idt, out=y)
                    ops.pyramid_level(cur, lat, c0)
                    c0 += c
        return lat.permute(0, 3, 1, 2).view(SB, NV, L, Hf, Wf)
