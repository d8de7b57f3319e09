"""Bit-level A/B of two checkouts (GPU box): sha256 of seeded outputs of the 2-D convolution's four instances and of everything built on
them or on the shared double-precision workgroup sum.
usage: python tools/conv2d_hash.py   -> one JSON line {name: digest}; identical lines from two checkouts = bit-identical kernels."""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import make_golden_encoder as GE
import make_golden_perceptual as GP
from diner_amd import encoder as E, metrics, objective, ops, optim, perceptual as P

out = {}


def put(name, *tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    out[name] = h.hexdigest()[:16]


def rand(g, *shape):
    return torch.randn(*shape, generator=g)


# the four instances: odd sizes with tails in both tilings, two images, float4 (ragged last chunk) and element-wise loads, two Cout tiles
Cout = 70
for (H, W), Cin in (((11, 19), 12), ((17, 35), 3)):
    g = torch.Generator().manual_seed(4000 + Cin)
    x = rand(g, 2, H, W, Cin).cuda()
    b = torch.zeros(128)
    b[:Cout] = rand(g, Cout) * 0.1
    b = b.cuda()
    for R in (3, 1, 7):
        w = rand(g, Cout, Cin, R, R) * (2.0 / (R * R * Cin)) ** 0.5
        wp = ops.pack_conv_s2(w).cuda()
        for relu in (False, True):
            put(f"conv_s2_R{R}_{H}x{W}x{Cin}_relu{int(relu)}", ops.conv_s2(x, wp, b, Cout, R, relu=relu))
            if R == 3:
                put(f"conv3x3_{H}x{W}x{Cin}_relu{int(relu)}", ops.conv3x3(x, wp, b, Cout, relu=relu))
        if R == 7:          # a channel slice of a wider buffer
            buf = torch.full((2, (H + 1) // 2, (W + 1) // 2, 200), -7.25, device="cuda")
            put(f"conv_s2_R7_{H}x{W}x{Cin}_coff", ops.conv_s2(x, wp, b, Cout, 7, relu=True, out=buf, coff=64))
        if R == 3:          # the data gradient: transposed weight set, addend and mask
            gy, addend, act = rand(g, 2, H, W, Cout).cuda(), rand(g, 2, H, W, Cin).cuda(), rand(g, 2, H, W, Cin).clamp(min=0).cuda()
            put(f"conv3x3_bwd_{H}x{W}x{Cin}", ops.conv3x3(gy, ops.pack_conv3x3(w, transpose=True).cuda(), None, Cin, addend=addend, mask=act))

# the perceptual network and the encoder's trunk at their tests' small sizes
for k, (arch, div, N, H, W, seed) in enumerate(GP.LPIPS_CASES):
    pred, gt = GP.lpips_inputs(N, H, W, seed)
    put(f"lpips{k}", P.Lpips(GP.state_dict(arch, div))(pred.cuda(), gt.cuda()))
for k, (arch, div, N, H, W, seed) in enumerate(GP.LOSS_CASES):
    x, y = GP.loss_inputs(N, H, W, seed)
    xd = x.cuda().requires_grad_(True)
    loss = P.VggLoss(GP.state_dict(arch, div))(xd, y.cuda())
    loss.backward()
    put(f"vgg_loss{k}", loss, xd.grad)
for case in ("A", "B", "C"):
    put(f"trunk{case}", E.DeviceTrunk(GE.state_dict(case), **GE.config(case))(GE.images_of(case).cuda()))

# one call each of what sums over a workgroup in double
g = torch.Generator().manual_seed(77)
fx, fy = rand(g, 2, 13, 17, 24).cuda(), rand(g, 2, 13, 17, 24).cuda()
put("feature_l1", *ops.feature_l1(fx, fy, weight=0.5, mask_by_fx=True))
put("lpips_layer", ops.lpips_layer(fx, fy, torch.rand(24, generator=g).cuda()))
m = metrics.image_metrics(torch.rand(2, 3, 37, 45, generator=g).cuda(), torch.rand(2, 3, 37, 45, generator=g).cuda())
put("image_metrics", *(m[k] for k in ("l1", "l2", "psnr", "ssim")))
n = 5000
d2, idx = torch.rand(n, generator=g).cuda(), torch.randint(-1, n, (n,), generator=g, dtype=torch.int32).cuda()
na, nb = torch.nn.functional.normalize(rand(g, n, 3), dim=1).cuda(), torch.nn.functional.normalize(rand(g, n, 3), dim=1).cuda()
put("cloud_reduce", ops.cloud_reduce(d2, idx, max_dist=0.9, thresholds=(0.1, 0.5), normals_a=na, normals_b=nb))
pred, gt = torch.rand(2, 32 * 32, 3, generator=g).cuda(), torch.rand(2, 32 * 32, 3, generator=g).cuda()
put("objective_patch", *objective.objective(pred, gt, s=32, n_downsampling=3, w_antibias=0.1))
put("objective_loose", *objective.objective(pred[:, :1000], gt[:, :1000]))
params = [rand(g, *s).cuda().requires_grad_(True) for s in ((300, 41), (4099,), (7, 5, 3))]
opt = optim.DeviceAdam(params, max_grad_norm=1.0)
for p in params:
    p.grad.copy_(rand(g, *p.shape))
opt.step(grad_norm=True)
put("adam_grad_norm", opt.grad_norm_tensor(), *params)
torch.cuda.synchronize()
print(json.dumps(out))
