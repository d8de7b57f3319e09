"""CPU: the host side of the device optimiser -- the C ABI entries, the chunk table (host arithmetic on fake addresses), the
torch.optim.Adam state-dict mapping and the checkpoint keys on CPU tensors, and the float64 restatement the GPU tests measure against."""
import copy
import ctypes as C
import os

import pytest
import torch

from tests import optim_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("diner_optim_table_bytes", "diner_optim_table_build", "diner_optim_grad_stats", "diner_adam_step_f32")


def test_entries_are_declared_exported_and_bound():
    from diner_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "diner_hip.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define DINER_ABI_VERSION 6" in header and lib.diner_abi_version() == 6 and _lib.ABI_VERSION == 6
    assert "optim.hip" in build.SOURCES
    assert f"#define DINER_OPTIM_CHUNK {_lib.OPTIM_CHUNK}" in header and _lib.OPTIM_CHUNK == U.CHUNK and U.CHUNK % 4 == 0
    assert C.sizeof(_lib.DinerOptimChunk) == 48 and C.sizeof(_lib.DinerOptimState) == 64
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in ENTRIES)


def _records():
    """Fake device addresses (the build never dereferences them); tensor 2's parameter lies 4 bytes past a 16-byte boundary."""
    recs, base = [], 0x7f0000000000
    for k, n in enumerate(U.SIZES):
        a = base + k * 0x10000000
        recs.append((a + (4 if k == 2 else 0), a + 0x2000000, a + 0x4000000, a + 0x6000000, n))
    return recs


def test_table_tiles_every_tensor_once_in_order():
    from diner_amd import _lib, optim
    lib = _lib.load()
    recs = _records()
    buf, n_chunks, nbytes = optim.build_table(recs)
    arr = (_lib.DinerOptimTensor * len(recs))(*[_lib.DinerOptimTensor(*r) for r in recs])
    assert nbytes == lib.diner_optim_table_bytes(arr, len(recs)) == n_chunks * (48 + 16)
    assert n_chunks == sum((n + U.CHUNK - 1) // U.CHUNK for n in U.SIZES)
    chunks = (_lib.DinerOptimChunk * n_chunks).from_buffer(buf)
    c = 0
    for k, (p, g, m, v, n) in enumerate(recs):
        off = 0
        while off < n:
            ch = chunks[c]
            assert ch.tensor == k and ch.offset == off
            assert (ch.param, ch.grad, ch.exp_avg, ch.exp_avg_sq) == (p + 4 * off, g + 4 * off, m + 4 * off, v + 4 * off)
            assert 1 <= ch.numel <= U.CHUNK and off % 4 == 0
            assert ch.numel == U.CHUNK or off + ch.numel == n          # only a tensor's last chunk is short
            off += ch.numel
            c += 1
        assert off == n
    assert c == n_chunks                                               # the empty tensor contributed none
    assert bytes(buf)[n_chunks * 48:] == bytes(n_chunks * 16)          # the partial slots are zeroed


def test_table_refuses_bad_arguments():
    from diner_amd import _lib
    lib = _lib.load()
    recs = _records()
    arr = (_lib.DinerOptimTensor * len(recs))(*[_lib.DinerOptimTensor(*r) for r in recs])
    nbytes = lib.diner_optim_table_bytes(arr, len(recs))
    out = (C.c_uint8 * nbytes)()
    nc = C.c_int(0)
    assert lib.diner_optim_table_bytes(arr, 0) == 0 and b"n >= 1" in lib.diner_last_error()
    assert lib.diner_optim_table_build(arr, 0, out, nbytes, C.byref(nc)) == _lib.E_INVALID
    assert lib.diner_optim_table_build(arr, -3, out, nbytes, C.byref(nc)) == _lib.E_INVALID
    assert lib.diner_optim_table_build(None, 2, out, nbytes, C.byref(nc)) == _lib.E_INVALID
    assert lib.diner_optim_table_build(arr, len(recs), out, nbytes - 1, C.byref(nc)) == _lib.E_INVALID and b"needs" in lib.diner_last_error()
    assert lib.diner_optim_table_build(arr, len(recs), None, nbytes, C.byref(nc)) == _lib.E_INVALID
    assert lib.diner_optim_table_build(arr, len(recs), out, nbytes, None) == _lib.E_INVALID
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        bad = (_lib.DinerOptimTensor * len(recs))(*[_lib.DinerOptimTensor(*r) for r in recs])
        setattr(bad[4], field, None)
        assert lib.diner_optim_table_bytes(bad, len(recs)) == 0
        assert lib.diner_optim_table_build(bad, len(recs), out, nbytes, C.byref(nc)) == _lib.E_INVALID
        assert b"null pointer" in lib.diner_last_error() and b"record 4" in lib.diner_last_error()
    empty_null = (_lib.DinerOptimTensor * 2)(_lib.DinerOptimTensor(*recs[0]), _lib.DinerOptimTensor(None, None, None, None, 0))
    assert lib.diner_optim_table_build(empty_null, 2, out, nbytes, C.byref(nc)) == 0 and nc.value == 1      # numel 0: nothing to point at
    # the device entries validate before any device work
    st, h = (C.c_uint8 * 64)(), _lib.DinerAdamHyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, 0)
    assert lib.diner_adam_step_f32(None, 1, st, C.byref(h), None) == _lib.E_INVALID
    assert lib.diner_adam_step_f32(out, 0, st, C.byref(h), None) == _lib.E_INVALID
    assert lib.diner_optim_grad_stats(out, 0, st, None) == _lib.E_INVALID
    for bad_h in (_lib.DinerAdamHyper(1e-4, 1.0, 0.999, 1e-8, 0.0, 0.0, 0, 0), _lib.DinerAdamHyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, 2),
                  _lib.DinerAdamHyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 0.0, _lib.ADAM_CLIP, 0), _lib.DinerAdamHyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 0.0, 16, 0)):
        assert lib.diner_adam_step_f32(out, 1, st, C.byref(bad_h), None) == _lib.E_INVALID


def _cpu_adam_state(steps=2):
    params, grads = U.make_inputs(5, steps=steps)
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.Adam(ps, lr=1e-3)
    for s in range(steps):
        for p, g in zip(ps, grads[s]):
            p.grad = g.clone()
        opt.step()
    return ps, opt


def test_state_dict_mapping_round_trips_on_cpu_tensors():
    from diner_amd import optim
    ps, opt = _cpu_adam_state()
    sd = opt.state_dict()
    shapes = [tuple(p.shape) for p in ps]
    offsets, total = optim.flat_layout([p.numel() for p in ps])
    assert all(o % 4 == 0 for o in offsets) and total >= sum(p.numel() for p in ps)
    assert all(offsets[k + 1] - offsets[k] >= ps[k].numel() for k in range(len(ps) - 1))
    m, v = torch.full((total,), 7.0), torch.full((total,), 7.0)
    step, group = optim.state_to_flat(sd, shapes, offsets, m, v)
    assert step == 2 and group["lr"] == 1e-3 and group["betas"] == (0.9, 0.999)
    back = optim.flat_to_state(step, shapes, offsets, m, v, group)
    assert set(back) == {"state", "param_groups"} and back["param_groups"] == sd["param_groups"]
    assert set(back["state"]) == set(sd["state"]) == set(range(len(ps)))
    for i, s in sd["state"].items():
        assert set(back["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} and float(back["state"][i]["step"]) == float(s["step"]) == 2.0
        assert torch.equal(back["state"][i]["exp_avg"], s["exp_avg"]) and torch.equal(back["state"][i]["exp_avg_sq"], s["exp_avg_sq"])
    # torch takes the dict as its own
    opt2 = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=5.0)
    opt2.load_state_dict(back)
    assert opt2.param_groups[0]["lr"] == 1e-3
    # unequal per-parameter steps are refused, and the message says so
    uneven = copy.deepcopy(sd)                     # (state_dict() hands out the optimiser's own inner dicts)
    uneven["state"][3]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="step counts differ"):
        optim.state_to_flat(uneven, shapes, offsets, m, v)
    # a parameter without an entry gets zero moments; before the first step the state is empty
    sd = copy.deepcopy(opt.state_dict())
    del sd["state"][4]
    optim.state_to_flat(sd, shapes, offsets, m, v)
    assert float(m[offsets[4]:offsets[4] + ps[4].numel()].abs().max()) == 0.0
    assert optim.flat_to_state(0, shapes, offsets, m, v, group)["state"] == {}


def test_checkpoint_keys_and_prefix_on_a_cpu_module(tmp_path):
    from diner_amd import fit
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    net(torch.randn(4, 3)).square().sum().backward()
    opt.step()
    path = str(tmp_path / "a.ckpt")
    fit.save_checkpoint(path, net, opt, 7, znear=0.5, zfar=1.5)
    ckpt = torch.load(path, weights_only=False)
    assert set(ckpt) == {"state_dict", "optimizer_states", "global_step"} and ckpt["global_step"] == 7
    assert set(ckpt["state_dict"]) == {"nerf." + k for k in net.state_dict()} | {"znear", "zfar"}
    assert float(ckpt["state_dict"]["znear"]) == 0.5 and float(ckpt["state_dict"]["zfar"]) == 1.5
    assert isinstance(ckpt["optimizer_states"], list) and set(ckpt["optimizer_states"][0]) == {"state", "param_groups"}
    fresh = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    fresh_opt = torch.optim.Adam(fresh.parameters(), lr=1.0)
    assert fit.load_checkpoint(path, fresh, fresh_opt) == 7
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), net.state_dict().values()))
    assert fresh_opt.param_groups[0]["lr"] == 1e-3 and torch.equal(fresh_opt.state_dict()["state"][0]["exp_avg"], opt.state_dict()["state"][0]["exp_avg"])
    # a state dict without the prefix loads as well
    bare = str(tmp_path / "b.ckpt")
    torch.save(dict(state_dict=net.state_dict(), optimizer_states=[], global_step=3), bare)
    fresh2 = torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.Linear(5, 2))
    assert fit.load_checkpoint(bare, fresh2) == 3
    assert all(torch.equal(a, b) for a, b in zip(fresh2.state_dict().values(), net.state_dict().values()))
    with pytest.raises(ValueError, match="optimizer_states"):
        fit.load_checkpoint(bare, fresh2, fresh_opt)


@pytest.mark.parametrize("hyper", range(len(U.HYPERS)))
@pytest.mark.parametrize("clip", [None, 3.0])
def test_float64_restatement_agrees_with_torch(hyper, clip):
    """Pins the yardstick: three steps of torch.optim.Adam / AdamW in float64 on the CPU against optim_util.adam64, to 1e-12 relative."""
    h = dict(U.HYPERS[hyper])
    params, grads = U.make_inputs(11, sizes=[1, 3, 5, 512, 4101])
    ps = [torch.nn.Parameter(p.double()) for p in params]
    cls = torch.optim.AdamW if h.pop("decoupled") else torch.optim.Adam
    opt = cls(ps, **h)
    p64, m64, v64 = [p.double() for p in params], [torch.zeros_like(p, dtype=torch.float64) for p in params], [torch.zeros_like(p, dtype=torch.float64) for p in params]
    for s in range(3):
        for p, g in zip(ps, grads[s]):
            p.grad = g.double()
        if clip is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, clip))
        opt.step()
        p64, m64, v64, info = U.adam64(p64, grads[s], m64, v64, s + 1, **U.HYPERS[hyper], max_grad_norm=clip)
        if clip is not None:
            assert abs(info["grad_norm"] - norm) <= 1e-12 * norm and info["clip"] < 1.0
        for k, p in enumerate(ps):
            st = opt.state[p]
            for got, ref in ((p64[k], p.detach()), (m64[k], st["exp_avg"]), (v64[k], st["exp_avg_sq"])):
                assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (s, k)
    # a skipped step changes nothing and says so
    bad = [g.clone() for g in grads[0]]
    bad[3][7] = float("inf")
    q, m, v, info = U.adam64(p64, bad, m64, v64, 4, **U.HYPERS[hyper], skip_nonfinite=True)
    assert info["skipped"] and info["nonfinite"] == 1 and all(torch.equal(a, b) for a, b in zip(q + m + v, p64 + m64 + v64))
