"""The optimiser step on the device: torch.optim.Adam / AdamW over all parameter tensors of a model in ONE launch of csrc/optim.hip (C ABI:
diner_optim_table_bytes / _build, diner_optim_grad_stats, diner_adam_step_f32) -- the reference's
`torch.optim.Adam(self.nerf.parameters(), lr=self.lr)` (src/models/diner.py:332-334).  Enqueue-only on the current stream; like
diner_amd.ops there is no CPU fallback for the step.

    opt = DeviceAdam(nerf.parameters(), lr=1e-4)
    losses["total"].backward()
    opt.step(zero_grads=True)

The state dict is torch.optim.Adam's, so `optimizer_states[0]` of a checkpoint written by the reference's training loads, and the reverse.
The dict <-> flat-buffer mapping (`flat_layout`, `state_to_flat`, `flat_to_state`) is plain torch and works on CPU tensors.
"""
import ctypes as C
import math

import torch

from . import _lib

lib = _lib.load()

_ALIGN = 4           # elements: every tensor's slice of a flat buffer starts on a 16-byte boundary


# ---- torch.optim.Adam's state dict <-> flat buffers (plain torch, any device) ----------------------------------------------------------
def flat_layout(numels):
    """-> (offsets, total): element offset of every tensor's slice in a flat fp32 buffer whose slices start on 16-byte boundaries."""
    offsets, total = [], 0
    for n in numels:
        offsets.append(total)
        total += (int(n) + _ALIGN - 1) // _ALIGN * _ALIGN
    return offsets, max(total, _ALIGN)


def _step_of(v):
    return int(round(float(v)))


def state_to_flat(state_dict, shapes, offsets, exp_avg, exp_avg_sq):
    """Copies a torch.optim.Adam state dict's moments into the flat buffers (slices `offsets` of tensors shaped `shapes`) and returns
    (step, param_group).  Parameters without an entry (torch creates one at a parameter's first step) get zero moments.  This optimiser
    keeps ONE step count for all parameters: a dict whose per-parameter steps differ is refused."""
    groups = state_dict["param_groups"]
    order = [i for g in groups for i in g["params"]]
    if len(order) != len(shapes):
        raise ValueError(f"load_state_dict: the state dict lists {len(order)} parameters, the optimiser has {len(shapes)}")
    if len(groups) != 1:
        raise ValueError(f"load_state_dict: {len(groups)} parameter groups; this optimiser has one set of hyper-parameters for all parameters")
    state = state_dict["state"]
    steps = {_step_of(state[i]["step"]) for i in order if i in state}
    if len(steps) > 1:
        raise ValueError(f"load_state_dict: the per-parameter step counts differ ({sorted(steps)}); this optimiser keeps one step count "
                         f"for all parameters")
    exp_avg.zero_()
    exp_avg_sq.zero_()
    for k, i in enumerate(order):
        if i not in state:
            continue
        n = 1
        for d in shapes[k]:
            n *= int(d)
        for flat, name in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            src = state[i][name]
            if tuple(src.shape) != tuple(shapes[k]):
                raise ValueError(f"load_state_dict: {name} of parameter {i} has shape {tuple(src.shape)}, the parameter {tuple(shapes[k])}")
            flat[offsets[k]:offsets[k] + n].copy_(src.detach().reshape(-1).to(torch.float32))
    return (steps.pop() if steps else 0), dict(groups[0])


def flat_to_state(step, shapes, offsets, exp_avg, exp_avg_sq, group):
    """The reverse: a torch.optim.Adam state dict ({state: {i: {step, exp_avg, exp_avg_sq}}, param_groups: [group]}) from the flat
    buffers; the moments are copies.  Before the first step the state is empty, as torch's."""
    state = {}
    if step > 0:
        for k, shape in enumerate(shapes):
            n = 1
            for d in shape:
                n *= int(d)
            state[k] = dict(step=torch.tensor(float(step)), exp_avg=exp_avg[offsets[k]:offsets[k] + n].clone().view(tuple(shape)),
                            exp_avg_sq=exp_avg_sq[offsets[k]:offsets[k] + n].clone().view(tuple(shape)))
    group = dict(group)
    group["params"] = list(range(len(shapes)))
    return dict(state=state, param_groups=[group])


def _group(lr, betas, eps, weight_decay, decoupled):
    """torch.optim.Adam's param_group keys (torch 2.x), so that torch.optim.Adam.load_state_dict takes the dict as its own."""
    return dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay), amsgrad=False,
                maximize=False, foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled))


# ---- the chunk table (host arithmetic: works without a device) -----------------------------------------------------------------------
def build_table(records, out=None):
    """records: (param, grad, exp_avg, exp_avg_sq, numel) device addresses per tensor -> (host buffer, n_chunks, bytes): the chunk table of
    diner_optim_table_build in `out` (a uint8 tensor of at least that size, e.g. pinned) or a new ctypes buffer."""
    n = len(records)
    arr = (_lib.DinerOptimTensor * max(n, 1))()
    for k, r in enumerate(records):
        arr[k] = _lib.DinerOptimTensor(*[int(x) if x else None for x in r[:4]], int(r[4]))
    nbytes = int(lib.diner_optim_table_bytes(arr, n))          # 0 for bad records: the build below then refuses them with the message
    if out is None:
        out = (C.c_uint8 * max(nbytes, 1))()
        ptr = C.addressof(out)
    else:
        ptr = out.data_ptr()
    n_chunks = C.c_int(0)
    _lib.check(lib.diner_optim_table_build(arr, n, C.c_void_p(ptr), nbytes, C.byref(n_chunks)))
    return out, int(n_chunks.value), nbytes


class DeviceAdam:
    """torch.optim.Adam (decoupled=True: AdamW) for contiguous fp32 parameters on one HIP device; with the defaults it is the reference's
    optimiser.  It owns flat fp32 buffers for the gradients and both moments and installs every `p.grad` as a view into the gradient buffer
    (autograd accumulates into an existing .grad in place), so zero_grad() is one memset and a step is one launch over a table of
    <= 4096-element chunks of all tensors.  max_grad_norm: torch's clip_grad_norm_ rule inside the step; skip_nonfinite: a step whose
    gradients hold an inf or NaN changes nothing (and does not count).  Both need the statistics pass (two more small launches), which
    step(grad_norm=True) also runs on request."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None,
                 skip_nonfinite=False):
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("DeviceAdam: no parameters")
        dev = self.params[0].device
        for p in self.params:
            if not p.is_cuda or p.device != dev:
                raise RuntimeError("DeviceAdam: parameters must live on one HIP device (MI355X); there is no CPU fallback")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"DeviceAdam: parameters must be contiguous float32 tensors, got {p.dtype} with strides {p.stride()}")
        if not (lr >= 0 and eps >= 0 and weight_decay >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError(f"DeviceAdam: bad hyper-parameters lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"DeviceAdam: max_grad_norm must be > 0, got {max_grad_norm}")
        self.device = dev
        self.group = _group(lr, betas, eps, weight_decay, decoupled)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.shapes = [tuple(p.shape) for p in self.params]
        self.numels = [p.numel() for p in self.params]
        self.offsets, total = flat_layout(self.numels)
        self.grads = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self.state = torch.zeros(8, dtype=torch.int64, device=dev)          # DinerOptimState
        self._calls = 0                                                     # step launches so far: slot = _calls & 1 is the current one
        self._key = self._table = None
        self._n_chunks = 0
        self._live = []
        for p, off, n in zip(self.params, self.offsets, self.numels):
            if p.requires_grad:
                p.grad = self.grads[off:off + n].view(p.shape)

    # -- gradients
    def zero_grad(self):
        """One memset of the flat gradient buffer; a .grad the caller replaced or removed is put back as the view into it."""
        self.grads.zero_()
        for p, off, n in zip(self.params, self.offsets, self.numels):
            if p.requires_grad and (p.grad is None or p.grad.data_ptr() != self.grads.data_ptr() + 4 * off):
                p.grad = self.grads[off:off + n].view(p.shape)

    def _records(self):
        recs, live = [], []
        m0, v0 = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        for k, p in enumerate(self.params):
            g = p.grad
            if g is None or self.numels[k] == 0:
                continue
            if not g.is_cuda or g.device != self.device or g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != self.numels[k]:
                raise ValueError(f"DeviceAdam: the gradient of parameter {k} must be a contiguous float32 tensor of {self.numels[k]} elements "
                                 f"on {self.device}, got {g.dtype} {tuple(g.shape)} on {g.device}")
            off = 4 * self.offsets[k]
            recs.append((p.data_ptr(), g.data_ptr(), m0 + off, v0 + off, self.numels[k]))
            live.append(k)
        return recs, live

    def _bind(self):
        """The table for the addresses as they are now: rebuilt and uploaded again (a stream-ordered copy from pinned memory) if any moved."""
        recs, live = self._records()
        key = tuple(recs)
        if key != self._key:
            self._key, self._live = key, live
            if not recs:
                self._table, self._n_chunks = None, 0
                return
            arr = (_lib.DinerOptimTensor * len(recs))(*[_lib.DinerOptimTensor(*r) for r in recs])
            nbytes = int(lib.diner_optim_table_bytes(arr, len(recs)))
            host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)            # a new one per rebuild: an earlier copy may still be in flight
            n_chunks = C.c_int(0)
            _lib.check(lib.diner_optim_table_build(arr, len(recs), C.c_void_p(host.data_ptr()), nbytes, C.byref(n_chunks)))
            self._table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._table.copy_(host, non_blocking=True)
            self._host = host
            self._n_chunks = int(n_chunks.value)

    # -- the step
    def step(self, lr=None, zero_grads=False, grad_norm=False):
        """One launch (three with clipping, skipping or grad_norm=True: the statistics pass first); no host synchronisation.  lr overrides
        the group's learning rate for this step (the hook for a schedule); zero_grads overwrites every gradient with zero after it has been
        read, which saves the separate zero_grad().  A parameter whose .grad is None is left out, as torch does; a .grad the caller
        replaced is used where it lies.  Every updated parameter's version counter is bumped, so caches keyed on it (ResnetFC's packed
        inference weights) see the write."""
        self._bind()
        if self._n_chunks == 0:
            return
        g = self.group
        flags = (_lib.ADAM_DECOUPLED_WD if g["decoupled_weight_decay"] else 0) | (_lib.ADAM_ZERO_GRADS if zero_grads else 0)
        if self.max_grad_norm is not None:
            flags |= _lib.ADAM_CLIP
        if self.skip_nonfinite:
            flags |= _lib.ADAM_SKIP_NONFINITE
        h = _lib.DinerAdamHyper(float(g["lr"] if lr is None else lr), g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"],
                                self.max_grad_norm or 0.0, flags, self._calls & 1)
        table, state = C.c_void_p(self._table.data_ptr()), C.c_void_p(self.state.data_ptr())
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if grad_norm or self.max_grad_norm is not None or self.skip_nonfinite:
                _lib.check(lib.diner_optim_grad_stats(table, self._n_chunks, state, stream))
            _lib.check(lib.diner_adam_step_f32(table, self._n_chunks, state, C.byref(h), stream))
        self._calls += 1
        torch.autograd.graph.increment_version([self.params[k] for k in self._live])

    # -- what the device knows
    def grad_norm_tensor(self):
        """0-dim float64 device tensor: the gradient norm of the last statistics pass (no wait)."""
        return self.state.view(torch.float64)[4].sqrt()

    def _read_state(self):
        s = self.state.cpu()                                          # the one synchronisation
        f = s.view(torch.float64)
        cur = self._calls & 1
        return dict(step=int(s[cur]), skipped=int(s[2 + cur]), grad_norm=math.sqrt(float(f[4])) if float(f[4]) >= 0 else float("nan"),
                    nonfinite=int(s[5]), clip=float(f[6]))

    def stats(self):
        """{step, skipped, grad_norm, nonfinite, clip} read from the device's state block: one synchronisation."""
        return self._read_state()

    def _write_state(self, step, skipped=0):
        s = torch.zeros(8, dtype=torch.int64)
        s[0] = s[1] = int(step)
        s[2] = s[3] = int(skipped)
        self.state.copy_(s)

    # -- torch.optim.Adam's state dict
    def state_dict(self):
        return flat_to_state(self._read_state()["step"], self.shapes, self.offsets, self.exp_avg, self.exp_avg_sq, self.group)

    def load_state_dict(self, state_dict):
        if any(g.get("amsgrad") or g.get("maximize") for g in state_dict["param_groups"]):
            raise ValueError("DeviceAdam: amsgrad / maximize state dicts are not supported")
        step, group = state_to_flat(state_dict, self.shapes, self.offsets, self.exp_avg, self.exp_avg_sq)
        for k in ("lr", "eps", "weight_decay"):
            if k in group:
                self.group[k] = float(group[k])
        if "betas" in group:
            self.group["betas"] = (float(group["betas"][0]), float(group["betas"][1]))
        if "decoupled_weight_decay" in group:
            self.group["decoupled_weight_decay"] = bool(group["decoupled_weight_decay"])
        self._write_state(step, skipped=0)
