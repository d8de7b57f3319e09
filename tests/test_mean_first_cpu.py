"""CPU: block 2's fc_1 moved behind the view mean (the f16x3 field kernels, csrc/mlp_h3n.hip).

Block 2 is the last per-view block and ends in a linear layer, so
    mean_v(x_v + fc_1(relu(h_v)) + b) = mean_v(x_v) + fc_1(mean_v relu(h_v)) + b            (resnetfc.py:147-159, combine_layer 3)
and the 512 x 512 product is needed once per point instead of once per point and view.  Here, without a device: the reordered evaluation
restated with torch on the oracle's inputs is as close to a float64 evaluation as the reference order is; the FLOP constants of the bench
line count the executed work; the entry that frees the library-owned second hand-over plane resolves and is a no-op before any launch."""
import torch
import torch.nn.functional as F

from oracle import diner_oracle as O
from tests.helpers import load, oracle_setup, max_norm_rel


def T(a):
    import numpy as np
    return torch.from_numpy(np.asarray(a))


def field(w, zx, dtype, moved):
    """PixelNeRF's field (sigmoid rgb, relu sigma) of the oracle's network in `dtype`; moved: block 2's fc_1 on the view means."""
    c = lambda t: t.to(dtype)
    lin = lambda x, W, b: F.linear(x, c(W), c(b))
    zx = c(zx)
    z = zx[..., :w.d_latent]
    x = lin(zx[..., w.d_latent:], w.lin_in_w, w.lin_in_b)
    for b in range(5):
        if b < 3:
            x = x + lin(z, w.lin_z_w[b], w.lin_z_b[b])
        if b == 3 and not moved:
            x = x.mean(0)
        net = lin(torch.relu(x), w.fc0_w[b], w.fc0_b[b])
        if b == 2 and moved:
            x = x.mean(0) + lin(torch.relu(net).mean(0), w.fc1_w[b], w.fc1_b[b])
        else:
            x = x + lin(torch.relu(net), w.fc1_w[b], w.fc1_b[b])
    out = lin(torch.relu(x), w.lin_out_w, w.lin_out_b)
    return torch.cat([torch.sigmoid(out[..., :3]), torch.relu(out[..., 3:4])], -1)


def test_reordered_evaluation_is_as_close_to_float64_as_the_reference_order():
    """G6 (512 points): the distance of the reference order (fp32) from a float64 evaluation of the same inputs is the yardstick; the
    reordered fp32 evaluation may be at most twice as far (measured: 5.5e-7 against 4.5e-7, max-norm-relative)."""
    g = load("g6_pixelnerf.npz")
    sc, scene, w, msd, rays = oracle_setup(int(g["W"]), int(g["H"]), int(g["seed"]))
    zx = O.mlp_input(scene, T(g["pts"]), T(g["dirs"]))
    ref32 = field(w, zx, torch.float32, False)
    assert max_norm_rel(ref32, g["out"]) < 1e-6, "this restatement is not the oracle's network"
    f64 = field(w, zx, torch.float64, False)
    assert max_norm_rel(field(w, zx, torch.float64, True).float(), f64.float()) < 1e-6      # the identity itself
    d_ref = max_norm_rel(ref32, f64.float())
    d_moved = max_norm_rel(field(w, zx, torch.float32, True), f64.float())
    print(f"G6: reference order {d_ref:.2e}, fc_1 behind the mean {d_moved:.2e} from float64 (max-norm-rel); "
          f"the two fp32 orders differ by {max_norm_rel(field(w, zx, torch.float32, True), ref32):.2e}")
    assert d_ref > 0
    assert d_moved <= 2.0 * d_ref


def test_reordered_colours_stay_inside_the_fixtures_yardstick_g20a():
    """G20 variant a (realistic magnitudes), the first 32 rays of the fixture's field: the reordered fp32 evaluation's colours against the
    reference's stay below the fixture's own fp32-vs-float64 distance yard_col_a (7.7e-5; measured 2.7e-5)."""
    from tests.test_hip_parity import _g20_inputs
    g, sc, msd = _g20_inputs("a")
    K, n = int(g["K"]), 32
    Kc = sc["src_intrinsics"]
    scene = O.Scene(latent=sc["latent"], depths=sc["depths"], depths_std=sc["depths_std"], normals=sc["normals"], poses=sc["src_extrinsics"],
                    focal=Kc[:, [0, 1], [0, 1]], c=Kc[:, :2, -1], image_shape=sc["image_shape"], feature_padding=sc["feature_padding"])
    w = O.MLPWeights.from_state_dict(msd)
    rays, z = T(g["rays"])[::4][:n], T(g["z"])[::4][:n]                         # (the fixture keeps the field of every fourth ray)
    xyz = (rays[:, None, :3] + z[..., None] * rays[:, None, 3:6]).reshape(-1, 3)
    dirs = rays[:, None, 3:6].expand(-1, K, -1).reshape(-1, 3)
    got = field(w, O.mlp_input(scene, xyz, dirs), torch.float32, True)
    ref = T(g["field_a"])[: n * K]
    e_col = (got[:, :3] - ref[:, :3]).abs().max().item()
    e_sig = ((got[:, 3] - ref[:, 3]).abs().max() / ref[:, 3].abs().max()).item()
    print(f"G20 a, {n} rays: colours {e_col:.2e} (abs; yard_col_a {float(g['yard_col_a']):.2e}), sigma {e_sig:.2e} (max-norm-rel)")
    assert e_col < float(g["yard_col_a"])


def test_flop_constants_count_the_executed_work():
    from diner_amd import ops
    assert ops.FLOP_PRE_PER_POINT == 2 * 4 * (55 * 512 + 5 * 512 * 512)
    assert ops.FLOP_POST_PER_POINT == 2 * (5 * 512 * 512 + 4 * 512)


def test_release_entry_without_a_device():
    from diner_amd import _lib
    lib = _lib.load()
    assert "diner_field_release_buffers" in _lib.SIGNATURES
    assert lib.diner_field_release_buffers() == 0
    assert lib.diner_field_release_buffers() == 0
