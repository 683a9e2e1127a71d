"""What the fused `torch.optim.Optimizer` classes of this package share.  Each parameter group is one `FlatParamStore`, updated by one
flat optimizer of `neurosis_amd.optim`: a handful of HIP launches for a whole network instead of a Python loop over its tensors.
There is no eager fallback: the parameters must live in a store (the engine's `setup_flat_params()` puts them there; parameters handed
over on a GPU without one are re-homed into a new store at the first step).  Checkpoints keep torch's layout: parameters numbered
through the groups in order, per-parameter entries under the upstream class's keys.  A subclass keeps its upstream constructor and
supplies `_make_flat(group)` and `_push(group, flat)`."""
from __future__ import annotations

from typing import Optional

import torch
from torch.optim import Optimizer


def _group_store(group: dict, who: str):
    """The FlatParamStore that holds exactly this group's parameters (created on a GPU if they have none yet)."""
    from ..nn import FlatParamStore

    params = [p for p in group["params"] if p.requires_grad]
    if not params:
        raise ValueError(f"{who}: a parameter group without trainable parameters")
    stores = {id(getattr(p, "_nk_store", None)): getattr(p, "_nk_store", None) for p in params}
    if None in stores.values():
        if len(stores) > 1:
            raise ValueError(f"{who}: a parameter group mixes store-managed and free parameters")
        if not params[0].is_cuda:
            raise RuntimeError(f"{who}: the fused update runs on HIP buffers; move the model to the GPU (and call "
                               "setup_flat_params()) before the first step -- there is no CPU path")
        return FlatParamStore(params)
    if len(stores) != 1:
        raise ValueError(f"{who}: the parameters of one group live in {len(stores)} different flat stores")
    store = next(iter(stores.values()))
    if len(store.params) != len(params) or any(a is not b for a, b in zip(store.params, params)):
        raise ValueError(f"{who}: a parameter group must cover its flat store exactly ({len(params)} parameters given, "
                         f"{len(store.params)} in the store): the fused kernels update the whole buffer")
    return store


class _FusedOptimizer(Optimizer):
    # refuse a checkpoint whose group count or group sizes differ from this optimizer's.  CAME and AdamW8bit do; Adafactor and AdamW
    # never did and take the groups that pair up (`zip`): kept as it was, to be decided on its own
    _strict_groups = True

    def __init__(self, params, defaults: dict):
        super().__init__(params, defaults)
        self._flat: list = []
        self._pending_state: Optional[dict] = None

    def _make_flat(self, group: dict):
        """The flat optimizer of one parameter group, from the group's hyper-parameters."""
        raise NotImplementedError

    def _push(self, group: dict, flat) -> None:
        """Before a step: the group's hyper-parameters as they are NOW (an LR scheduler or a loaded checkpoint may have changed them)."""

    def _group_extras(self, flat) -> dict:
        """What the flat optimizer adds to its group's entries (after every step, and in state_dict())."""
        return {}

    # -- binding to the flat buffers --------------------------------------------------------------------
    def bind(self) -> list:
        """One flat optimizer per parameter group (each group = one flat store).  Idempotent."""
        if not self._flat:
            self._flat = [self._make_flat(g) for g in self.param_groups]
            if self._pending_state is not None:
                sd, self._pending_state = self._pending_state, None
                self._load_flat(sd)
        return self._flat

    @property
    def flat(self):
        """The fused optimizer of the first (UNet) group."""
        return self.bind()[0]

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for g, f in zip(self.param_groups, self.bind()):
            self._push(g, f)
            f.step(grad_scale)
            g.update(self._group_extras(f))
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Nothing to do, on purpose: `.grad` tensors are views of the store's flat gradient buffer and every gradient is
        OVERWRITTEN by the kernel that produces it on the first micro-batch of a step (FlatParamStore docstring); setting
        them to None -- torch's default -- would detach the parameters from that buffer."""

    # -- checkpointing ------------------------------------------------------------------------------------
    def _slices(self):
        """(group, its flat optimizer or None while unbound, index of its first parameter, number of parameters)"""
        base = 0
        for gi, g in enumerate(self.param_groups):
            n = len(g["params"])
            yield g, self._flat[gi] if gi < len(self._flat) else None, base, n
            base += n

    def state_dict(self) -> dict:
        groups, state = [], {}
        for g, f, base, n in self._slices():
            packed = {k: v for k, v in g.items() if k != "params"}
            packed["params"] = list(range(base, base + n))
            groups.append(packed)
            if f is not None:
                packed.update(self._group_extras(f))
                for i, st in f.state_dict()["state"].items():
                    state[base + i] = st
        if not self._flat and self._pending_state is not None:
            state = self._pending_state["state"]
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict: dict) -> None:
        who = f"{type(self).__name__}.load_state_dict"
        saved_groups = state_dict.get("param_groups", [])
        if self._strict_groups and len(saved_groups) != len(self.param_groups):
            raise ValueError(f"{who}: {len(saved_groups)} parameter groups in the checkpoint, {len(self.param_groups)} here")
        for g, saved in zip(self.param_groups, saved_groups):
            if self._strict_groups and len(saved.get("params", g["params"])) != len(g["params"]):
                raise ValueError(f"{who}: a parameter group's size differs from the checkpoint's")
            for k, v in saved.items():
                if k != "params":
                    g[k] = v
        if self._flat:
            self._load_flat(state_dict)
        else:
            self._pending_state = state_dict      # applied when the flat buffers exist (first step / bind())

    def _load_flat(self, sd: dict) -> None:
        """Each flat optimizer gets its parameters' entries, renumbered from 0, and its group's `step` (where CAME keeps it)."""
        for g, f, base, n in self._slices():
            if f is not None:
                f.load_state_dict({"state": {int(i) - base: st for i, st in sd.get("state", {}).items() if base <= int(i) < base + n},
                                   "param_groups": [{"step": g.get("step", 0)}]})
