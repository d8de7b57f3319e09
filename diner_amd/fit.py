"""The loop around a training step and its checkpoints: what Lightning's Trainer.fit does for the reference (src/models/diner.py:292-334)
with everything of a step on the stream -- the objective (diner_amd.objective.calc_losses), the backward and the optimiser update
(diner_amd.optim.DeviceAdam).

    history, opt = fit(nerf, renderer, batches, znear=.., zfar=.., steps=1000, lr=1e-4, w_vgg=0.1, vgg_fn=.., w_antibias=1.)
    save_checkpoint("last.ckpt", nerf, opt, step=1000, znear=.., zfar=..)
"""
import itertools

import torch

LOSS_TERMS = ("rgb_fine", "vgg_fine", "antibias", "total")


def fit(nerf, renderer, batches, *, znear, zfar, steps, optimizer=None, lr=1e-4, seed=0, start_step=0, log_every=50, on_log=None,
        **loss_kwargs):
    """`steps` optimisation steps k = start_step, start_step + 1, ...: calc_losses(nerf, renderer, batch, seed=seed, step=k, **loss_kwargs),
    total.backward(), optimizer.step(zero_grads=True).  batches: any iterable of batch dicts, cycled.  optimizer: a DeviceAdam (made
    here over nerf's trainable parameters with `lr` when None).  The loss terms of a step go into a device ring of log_every rows that is
    read back once per log_every steps (and once at the end): the loop's only wait.  on_log(rows) receives the rows just read.
    -> (history, optimizer); history: one dict {step, rgb_fine, vgg_fine, antibias, total} per step."""
    from .objective import calc_losses
    from .optim import DeviceAdam
    if optimizer is None:
        optimizer = DeviceAdam([p for p in nerf.parameters() if p.requires_grad], lr=lr)
    steps, log_every = int(steps), max(1, int(log_every))
    dev = optimizer.device
    ring = torch.zeros(log_every, len(LOSS_TERMS), dtype=torch.float32, device=dev)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    history, first = [], start_step
    optimizer.zero_grad()

    def flush(upto):
        nonlocal first
        rows = ring[:upto - first].cpu()                               # the wait
        new = [dict(step=first + i, **{k: float(rows[i, j]) for j, k in enumerate(LOSS_TERMS)}) for i in range(rows.shape[0])]
        history.extend(new)
        first = upto
        if on_log is not None and new:
            on_log(new)

    source = itertools.cycle(batches)
    for k in range(start_step, start_step + steps):
        losses = calc_losses(nerf, renderer, next(source), znear=znear, zfar=zfar, seed=seed, step=k, **loss_kwargs)
        losses["total"].backward()
        optimizer.step(zero_grads=True)
        terms = [losses[name] for name in LOSS_TERMS]
        ring[k - first].copy_(torch.stack([t.detach().to(torch.float32) if torch.is_tensor(t) else zero for t in terms]))
        if k + 1 - first == log_every:
            flush(k + 1)
    if first < start_step + steps:
        flush(start_step + steps)
    return history, optimizer


def save_checkpoint(path, nerf, optimizer, step, **hparams):
    """torch.save of a dict with the key names Lightning writes for the reference's DINER module -- ONLY these: `state_dict` (nerf's, under
    the `nerf.` prefix, plus `znear` / `zfar` when given), `optimizer_states` ([optimizer.state_dict()]; [] without an optimiser) and
    `global_step`; further hparams go under `hyper_parameters`."""
    sd = {"nerf." + k: v.detach().cpu() for k, v in nerf.state_dict().items()}
    for k in ("znear", "zfar"):
        if k in hparams:
            sd[k] = torch.as_tensor(hparams[k], dtype=torch.float32)
    ckpt = dict(state_dict=sd, optimizer_states=[optimizer.state_dict()] if optimizer is not None else [], global_step=int(step))
    extra = {k: v for k, v in hparams.items() if k not in ("znear", "zfar")}
    if extra:
        ckpt["hyper_parameters"] = extra
    torch.save(ckpt, path)


def load_checkpoint(path, nerf, optimizer=None):
    """Loads what save_checkpoint (or the reference's training) wrote: nerf's weights from `state_dict`, with or without the `nerf.` prefix
    (other entries of a Lightning state dict, `znear` / `zfar` among them, are left aside), and the optimiser's state from
    `optimizer_states[0]` when an optimiser is given.  -> global_step."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    sd = ckpt["state_dict"]
    own = set(nerf.state_dict())
    if any(k.startswith("nerf.") for k in sd):
        sd = {k[len("nerf."):]: v for k, v in sd.items() if k.startswith("nerf.")}
    nerf.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=True)
    if optimizer is not None:
        states = ckpt.get("optimizer_states") or []
        if not states:
            raise ValueError(f"load_checkpoint: {path} holds no optimizer_states")
        optimizer.load_state_dict(states[0])
    return int(ckpt.get("global_step", 0))
