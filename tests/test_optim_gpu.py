"""GPU: diner_amd.optim.DeviceAdam (csrc/optim.hip) against the float64 restatement of torch.optim.Adam (tests/optim_util.py), with
torch.optim.Adam in float32 on the same device and inputs as the yardstick of what float32 can deliver."""
import math

import pytest
import torch

from tests import optim_util as U

pytestmark = pytest.mark.gpu
ODD = 6          # index of the parameter that starts 4 bytes past a 16-byte boundary (55 x 512 elements: several chunks on the scalar route)


@pytest.fixture(scope="module")
def inputs():
    params, grads = U.make_inputs(3, steps=4)
    return [p.cuda() for p in params], [[g.cuda() for g in gs] for gs in grads]


def make_params(params):
    out = []
    for k, p in enumerate(params):
        if k == ODD:
            buf = torch.empty(p.numel() + 1, device="cuda")
            buf[1:].copy_(p)
            q = torch.nn.Parameter(buf[1:])
            assert q.data_ptr() % 16 == 4
        else:
            q = torch.nn.Parameter(p.clone())
        out.append(q)
    return out


def set_grads(opt_or_params, grads):
    ps = opt_or_params.params if hasattr(opt_or_params, "params") else opt_or_params
    for p, g in zip(ps, grads):
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def moments(opt):
    m = [opt.exp_avg[o:o + n] for o, n in zip(opt.offsets, opt.numels)]
    v = [opt.exp_avg_sq[o:o + n] for o, n in zip(opt.offsets, opt.numels)]
    return m, v


def torch_moments(opt, ps):
    z = lambda p: torch.zeros_like(p)
    return [opt.state[p].get("exp_avg", z(p)) if p in opt.state else z(p) for p in ps], \
           [opt.state[p].get("exp_avg_sq", z(p)) if p in opt.state else z(p) for p in ps]


def snap(ps, m, v):
    return [x.detach().clone() for x in ps], [x.clone() for x in m], [x.clone() for x in v]


def check_step(label, before, after, grads, t, hyper, **kw):
    """The restated step from `before` (float32 values as stored) against `after`; returns the three errors."""
    p64, m64, v64, info = U.adam64(*before[:1], grads, *before[1:], t, **hyper, **kw)
    e = U.errors(*after, p64, m64, v64, hyper["lr"])
    print(f"{label} t={t}: e_p {e[0]:.3e} e_m {e[1]:.3e} e_v {e[2]:.3e}")
    return e, U.floors(p64, hyper["lr"]), info


def within_bar(e_dev, e_torch, floor):
    return all(d <= max(2.0 * t, f) for d, t, f in zip(e_dev, e_torch, floor))


def random_state(ps, step, seed=17):
    """A torch.optim.Adam state dict with plausible moments at `step`."""
    gen = torch.Generator().manual_seed(seed)
    state = {}
    for k, p in enumerate(ps):
        m = (torch.randn(p.shape, generator=gen) * 1e-2).cuda()
        v = (torch.rand(p.shape, generator=gen) * 1e-3 + m.cpu() ** 2).cuda()
        state[k] = dict(step=torch.tensor(float(step)), exp_avg=m, exp_avg_sq=v)
    return state


@pytest.mark.parametrize("case", range(len(U.HYPERS)))
def test_step_accuracy_against_float64_with_torch_float32_as_the_yardstick(inputs, case):
    """Measured on an MI355X (e_p, e_m, e_v; DeviceAdam | torch float32), worst over t = 1, 2, 3, 1000: see DESIGN.md section 8k."""
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    hyper = U.HYPERS[case]
    th = {k: v for k, v in hyper.items() if k != "decoupled"}
    cls = torch.optim.AdamW if hyper["decoupled"] else torch.optim.Adam
    ps_d, ps_t = make_params(params), make_params(params)
    dev, ref = DeviceAdam(ps_d, **hyper), cls(ps_t, foreach=False, **th)
    for t in (1, 2, 3, 1000):
        if t == 1000:
            sd = dict(state=random_state(ps_d, 999), param_groups=dev.state_dict()["param_groups"])
            dev.load_state_dict(sd)
            sd_t = ref.state_dict()
            sd_t["state"] = {k: {n: x.clone() for n, x in s.items()} for k, s in sd["state"].items()}
            ref.load_state_dict(sd_t)
            assert dev.stats()["step"] == 999
        g = grads[min(t, 4) - 1]
        set_grads(dev, g)
        set_grads(ps_t, g)
        before_d, before_t = snap(ps_d, *moments(dev)), snap(ps_t, *torch_moments(ref, ps_t))
        dev.step()
        ref.step()
        e_d, floor, _ = check_step(f"case {case} DeviceAdam", before_d, (ps_d, *moments(dev)), g, t, hyper)
        e_t, _, _ = check_step(f"case {case} torch f32 ", before_t, (ps_t, *torch_moments(ref, ps_t)), g, t, hyper)
        assert within_bar(e_d, e_t, floor), (t, e_d, e_t, floor)
        assert dev.stats()["step"] == t
        if t == 1 and hyper["weight_decay"] == 0:              # g = 0 and v = 0: the parameter stays finite and unchanged
            for p, p0, gk in zip(ps_d, before_d[0], g):
                z = gk == 0
                assert torch.isfinite(p).all() and torch.equal(p.detach()[z], p0[z])
            assert sum(int((gk == 0).sum()) for gk in g) > 100


def test_gradient_norm_is_exact_to_float64_and_reproducible(inputs):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    ps = make_params(params)
    opt = DeviceAdam(ps, lr=0.0)
    set_grads(opt, grads[0])
    want = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads[0]))
    N = sum(g.numel() for g in grads[0])
    opt.step(grad_norm=True)
    a = opt.grad_norm_tensor().clone()
    assert abs(float(a) - want) <= 1e-12 * math.sqrt(N) * want and opt.stats()["nonfinite"] == 0
    assert abs(opt.stats()["grad_norm"] - float(a)) == 0.0
    opt.step(grad_norm=True)
    b = opt.grad_norm_tensor().clone()
    opt._key = None                                            # the table built again over the same tensors in the same order
    opt.step(grad_norm=True)
    c = opt.grad_norm_tensor().clone()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))
    print(f"gradient norm {float(a):.17g} (float64 {want:.17g}, relative difference {abs(float(a) - want) / want:.2e}, N {N})")


def test_clipped_step_matches_the_restatement(inputs):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    hyper = U.HYPERS[0]
    th = {k: v for k, v in hyper.items() if k != "decoupled"}
    ps_d, ps_t = make_params(params), make_params(params)
    dev, ref = DeviceAdam(ps_d, max_grad_norm=5.0, **hyper), torch.optim.Adam(ps_t, foreach=False, **th)
    for t in (1, 2):
        g = grads[t - 1]
        set_grads(dev, g)
        set_grads(ps_t, g)
        before_d, before_t = snap(ps_d, *moments(dev)), snap(ps_t, *torch_moments(ref, ps_t))
        dev.step()
        torch.nn.utils.clip_grad_norm_(ps_t, 5.0)
        ref.step()
        e_d, floor, info = check_step("clip DeviceAdam", before_d, (ps_d, *moments(dev)), g, t, hyper, max_grad_norm=5.0)
        e_t, _, _ = check_step("clip torch f32 ", before_t, (ps_t, *torch_moments(ref, ps_t)), g, t, hyper, max_grad_norm=5.0)
        assert within_bar(e_d, e_t, floor), (t, e_d, e_t, floor)
        st = dev.stats()
        assert info["clip"] < 1e-2 and abs(st["clip"] - info["clip"]) <= 1e-12 * info["clip"]
        assert abs(st["grad_norm"] - info["grad_norm"]) <= 1e-9 * info["grad_norm"]


@pytest.mark.parametrize("poison", [float("inf"), float("nan")])
@pytest.mark.parametrize("zero_grads", [False, True])
def test_nonfinite_step_is_skipped(inputs, poison, zero_grads):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    hyper = U.HYPERS[1]
    ps = make_params(params)
    opt = DeviceAdam(ps, skip_nonfinite=True, **hyper)
    set_grads(opt, grads[0])
    opt.step()
    assert opt.stats() == dict(step=1, skipped=0, grad_norm=opt.stats()["grad_norm"], nonfinite=0, clip=1.0)
    set_grads(opt, grads[1])
    ps[4].grad.view(-1)[77] = poison
    before = snap(ps, *moments(opt))
    opt.step(zero_grads=zero_grads)
    after = (ps, *moments(opt))
    assert all(torch.equal(a.detach().view(torch.int32), b.view(torch.int32)) for xs, ys in zip(after, before) for a, b in zip(xs, ys))
    st = opt.stats()
    assert (st["step"], st["skipped"], st["nonfinite"], st["clip"]) == (1, 1, 1, 0.0)
    if zero_grads:
        assert all(float(p.grad.abs().max()) == 0.0 for p in ps if p.numel())
    else:
        assert not math.isfinite(float(ps[4].grad.view(-1)[77]))
    # the next finite step is step 2 of the restatement
    set_grads(opt, grads[2])
    opt.step()
    e, floor, _ = check_step("after a skip", before, (ps, *moments(opt)), grads[2], 2, hyper)
    assert within_bar(e, (0.0, 0.0, 0.0), floor), (e, floor)         # the floors alone: float32 rounding of the stored values
    st = opt.stats()
    assert (st["step"], st["skipped"], st["nonfinite"]) == (2, 1, 0)


def test_zero_grads_is_the_same_step_and_leaves_zeros(inputs):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    hyper = U.HYPERS[2]
    ps_a, ps_b = make_params(params), make_params(params)
    a, b = DeviceAdam(ps_a, **hyper), DeviceAdam(ps_b, **hyper)
    for t in (1, 2):
        set_grads(a, grads[t - 1])
        set_grads(b, grads[t - 1])
        a.step()
        b.step(zero_grads=True)
        assert all(float(p.grad.abs().max()) == 0.0 for p in ps_b if p.numel())
        assert all(torch.equal(p.grad, g) for p, g in zip(ps_a, grads[t - 1]))
    for xs, ys in zip((ps_a, *moments(a)), (ps_b, *moments(b))):
        assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(xs, ys))


def test_table_follows_replaced_and_removed_gradients(inputs):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    hyper = U.HYPERS[0]
    ps = make_params(params)
    opt = DeviceAdam(ps, **hyper)
    set_grads(opt, grads[0])
    opt.step()
    ps[5].grad = grads[1][5].clone()                           # a new tensor outside the flat buffer
    ps[7].grad = None                                          # left out, as torch does
    for k in (0, 1, 2, 3, 4, 6, 8):
        ps[k].grad.copy_(grads[1][k])
    before = snap(ps, *moments(opt))
    opt.step()
    m, v = moments(opt)
    assert torch.equal(ps[7].detach(), before[0][7]) and torch.equal(m[7], before[1][7]) and torch.equal(v[7], before[2][7])
    keep = [k for k in range(len(ps)) if k != 7]
    sub = lambda xs: [xs[k] for k in keep]
    e, floor, _ = check_step("rebound", tuple(sub(x) for x in before), (sub(ps), sub(m), sub(v)), sub(grads[1]), 2, hyper)
    assert within_bar(e, (0.0, 0.0, 0.0), floor), (e, floor)
    assert not torch.equal(ps[5].detach(), before[0][5])
    opt.zero_grad()                                            # puts the views back
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in ps if p.numel())
    assert ps[5].grad.data_ptr() == opt.grads.data_ptr() + 4 * opt.offsets[5]


def test_step_does_not_synchronise_and_bumps_versions(inputs):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    ps = make_params(params)
    opt = DeviceAdam(ps, max_grad_norm=1.0, skip_nonfinite=True)
    set_grads(opt, grads[0])
    versions = [p._version for p in ps]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()                                             # builds and uploads the table as well
        opt.step(zero_grads=True)
        norm = opt.grad_norm_tensor()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(norm) > 0 and opt.stats()["step"] == 2
    assert all(p._version > v for p, v in zip(ps, versions) if p.numel())


def test_state_dict_round_trips_with_torch_adam(inputs):
    from diner_amd.optim import DeviceAdam
    params, grads = inputs
    hyper = U.HYPERS[1]
    th = {k: v for k, v in hyper.items() if k != "decoupled"}
    # torch -> DeviceAdam: two torch steps, its state into DeviceAdam, one step there against torch's third
    ps_t = make_params(params)
    ref = torch.optim.Adam(ps_t, foreach=False, **th)
    for t in (1, 2):
        set_grads(ps_t, grads[t - 1])
        ref.step()
    ps_d = make_params([p.detach() for p in ps_t])
    dev = DeviceAdam(ps_d, lr=123.0)                           # the hyper-parameters come with the state
    dev.load_state_dict(ref.state_dict())
    assert dev.stats()["step"] == 2 and dev.group["lr"] == hyper["lr"] and dev.group["weight_decay"] == hyper["weight_decay"]
    before = snap(ps_t, *torch_moments(ref, ps_t))
    set_grads(ps_t, grads[2])
    set_grads(dev, grads[2])
    ref.step()
    dev.step()
    e_d, floor, _ = check_step("torch -> DeviceAdam", before, (ps_d, *moments(dev)), grads[2], 3, hyper)
    e_t, _, _ = check_step("torch's own third  ", before, (ps_t, *torch_moments(ref, ps_t)), grads[2], 3, hyper)
    assert within_bar(e_d, e_t, floor), (e_d, e_t, floor)
    # DeviceAdam -> torch: its state after those three steps into a fresh torch.optim.Adam, one step there against DeviceAdam's fourth
    ps_u = make_params([p.detach() for p in ps_d])
    back = torch.optim.Adam(ps_u, foreach=False, lr=55.0)
    back.load_state_dict(dev.state_dict())
    assert back.param_groups[0]["lr"] == hyper["lr"] and all(float(back.state[p]["step"]) == 3.0 for p in ps_u)
    before = snap(ps_d, *moments(dev))
    set_grads(ps_u, grads[3])
    set_grads(dev, grads[3])
    back.step()
    dev.step()
    e_d, floor, _ = check_step("DeviceAdam's fourth", before, (ps_d, *moments(dev)), grads[3], 4, hyper)
    e_t, _, _ = check_step("DeviceAdam -> torch", before, (ps_u, *torch_moments(back, ps_u)), grads[3], 4, hyper)
    assert within_bar(e_d, e_t, floor), (e_d, e_t, floor)
    assert all(x <= max(2 * y, f) for x, y, f in zip(e_t, e_d, floor)), (e_t, e_d, floor)
    uneven = dev.state_dict()
    uneven["state"][2]["step"] = torch.tensor(9.0)
    with pytest.raises(ValueError, match="step counts differ"):
        dev.load_state_dict(uneven)
    with pytest.raises(RuntimeError, match="HIP device"):
        DeviceAdam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(ValueError, match="contiguous float32"):
        DeviceAdam([torch.nn.Parameter(torch.zeros(4, 4, device="cuda").t())])
