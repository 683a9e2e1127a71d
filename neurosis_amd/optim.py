"""Optimizers over the flat parameter store.

`FlatAdafactor` mirrors `neurosis.optimizers.Adafactor` (reference `optimizers/adafactor.py:104-255`: same constructor
arguments and the same per-tensor rule -- factored second moments over the LAST TWO dims of every tensor with >= 2 dims,
RMS-scaled relative step, update clipping) but runs as a handful of multi-tensor HIP launches on the flat fp32 master /
gradient buffers (`csrc/optim.hip`), rewriting the bf16 shadows in the same pass.  `AdafactorScheduler` mirrors :258-291.

`FlatAdafactorMomentum` is the same optimizer with the reference's first moment (`beta1`, adafactor.py:194-196, 242-245): one more flat
fp32 buffer, read and written in the apply pass; `FlatAdafactor` itself refuses `beta1` and names the subclass.

Differences, all deliberate: state lives in flat buffers instead of a
per-parameter dict; `state_dict()` / `load_state_dict()` speak the reference optimizer's checkpoint format (per-parameter
`step`, `exp_avg_sq_row`, `exp_avg_sq_col` / `exp_avg_sq`, `RMS`, with a first moment `exp_avg`) so a run resumes with its moments, step count
(relative-step warm-up, beta2_t) and per-tensor RMS intact.  `FlatEma` is an `nn.Module` carrying `LitEma`'s buffer names
(`decay`, `num_updates`, one shadow per parameter), so `model_ema.*` keys of a reference checkpoint load and save unchanged.
`FlatCAME` mirrors `neurosis.optimizers.came.CAME` (`optimizers/came.py`) the same way, on `csrc/came.hip`.  `FlatAdamW8bit` is
bitsandbytes' blockwise 8-bit AdamW (`AdamW8bit`, named by the reference's sdxl-te config) as one launch of `csrc/adamw8bit.hip`.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import ops
from .lib import call, query

AF_TENSOR_DTYPE = np.dtype([("off", "<i8"), ("row_off", "<i8"), ("col_off", "<i8"), ("ws_row", "<i8"), ("ws_col", "<i8"),
                            ("kind", "<i4"), ("d0", "<i4"), ("d1", "<i4"), ("kh", "<i4"), ("kw", "<i4"), ("item0", "<i4"),
                            ("nitems", "<i4"), ("mr0", "<i4"), ("cnt0", "<i4"), ("pad", "<i4")])
AF_ITEM_DTYPE = np.dtype([("tensor", "<i4"), ("tr", "<i4"), ("tc", "<i4"), ("pad", "<i4")])
AF_TR, AF_TC, AF_CONV_PAIRS, AF_VEC = 256, 64, 1024, 1024


class _Args(C.Structure):
    _fields_ = [("master", C.c_void_p), ("grad", C.c_void_p), ("shadow", C.c_void_p), ("state", C.c_void_p), ("ws", C.c_void_p),
                ("tensors", C.c_void_p), ("items", C.c_void_p), ("u2_part", C.c_void_p), ("p2_part", C.c_void_p),
                ("mean_row", C.c_void_p), ("scale", C.c_void_p), ("lr_t", C.c_void_p),
                ("item_lo", C.c_int), ("item_hi", C.c_int), ("tensor_lo", C.c_int), ("tensor_hi", C.c_int),
                ("beta2t", C.c_float), ("eps1", C.c_float), ("eps2", C.c_float), ("clip_threshold", C.c_float),
                ("rel_step", C.c_float), ("weight_decay", C.c_float), ("grad_scale", C.c_float),
                ("scale_parameter", C.c_int), ("counters", C.c_void_p), ("has_matrix", C.c_int), ("reserved", C.c_int)]


def _align(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


def _default_chunk_bytes() -> int:
    """Gradient bytes per chunk of tensors (NK_AF_CHUNK_MB, default 128), for FlatAdafactor (three launches per chunk) and FlatCAME alike."""
    # A chunk's gradients are re-read (second-moment pass, update-RMS pass, apply pass) out of the 256 MB Infinity Cache instead of HBM
    # while the chunk fits it -- 14 instead of 22 HBM bytes per parameter.  The update runs on its own stream beside the next step's VAE
    # encoder, so what counts is the HBM bandwidth it takes from that encoder: round 3 (five launches per chunk) measured a steady-state
    # step of 172.2 / 172.8 / 173.8 / 174.8 ms at 64 / 128 / 256 / 2048 MB; round 4 (three launches per chunk): step-time p50 164.3 /
    # 165.2 / 165.5 ms at 64 / 128 / 256 MB (one box, back to back) -- the cache-sized chunk still wins although it
    # costs twice the launches.
    # 128 MB (round 5; 64 before): alone on the chip the update takes 20.5 / 17.8 / 13.8 / 12.7 / 12.2 / 11.7 ms at 32 / 64 / 128 / 256 /
    # 512 / 1024 MB chunks (tools/bench_optimizer.py) -- three dependent launches per chunk, each with its ramp and tail -- while the
    # second and third read of a chunk's gradients only stay in the 256 MB Infinity Cache for small chunks; in the step 128 MB measured
    # -0.5 ms against 64, 256 the same as 64, 512 +0.6 ms (profiles/r05_ab_notes.txt)
    return int(os.environ.get("NK_AF_CHUNK_MB", "128")) << 20


# The state vectors a tensor of each kind (0 vector, 1 matrix, 2 conv) owns, in the order they lie in `state`: (table field, length) with
# length one of "numel", "d0", "d1", "row" (conv: O*KH*I) and "col" (conv: O*KW*I).  _plan_tables() lays them out; the kernels find them
# through the C structs that AF_TENSOR_DTYPE / CAME_TENSOR_DTYPE mirror.
_AF_STATE = {0: (("row_off", "numel"),), 1: (("row_off", "d0"), ("col_off", "d1")), 2: (("row_off", "row"), ("col_off", "col"))}
_CAME_STATE = {0: (("m_off", "numel"), ("r_off", "numel")),
              1: (("m_off", "numel"), ("r_off", "d0"), ("c_off", "d1"), ("rr_off", "d0"), ("cr_off", "d1")),
              2: (("m_off", "numel"), ("r_off", "row"), ("c_off", "col"), ("rr_off", "row"), ("cr_off", "col"))}


def _plan_tables(who: str, shapes, offsets, chunk_bytes: int, boundaries, dtype: np.dtype, state_fields: dict, mr_per_strip: int) -> dict:
    """The tensor table, work items and chunks of a factored optimizer over parameters of `shapes` at element `offsets` of the flat
    buffers; pure (no store, no library, no device).  A matrix is tiled AF_TR x AF_TC (one item per tile, partial row / column sums in
    the chunk's workspace, `mr_per_strip` mean_row slots per 256-row strip, one counter per strip and per tile column), a conv weight
    takes one item per AF_CONV_PAIRS (o, i) pairs, anything else one per AF_VEC elements; every tensor has one more counter.  A chunk is
    closed before the tensor that would take its gradients past `chunk_bytes`, and before every tensor index in `boundaries`.
    Returns tensors (`dtype`), items (AF_ITEM_DTYPE), chunks [(tensor_lo, tensor_hi, item_lo, item_hi)] and the sizes state / ws /
    mean_row / counters."""
    bounds = set(int(b) for b in (boundaries or ()))
    tens = np.zeros(len(shapes), dtype=dtype)
    items, chunks = [], []
    state_off = ws_max = mr_slots = n_counters = 0
    c_t0 = c_i0 = c_bytes = c_ws = 0
    for ti, (shape, off) in enumerate(zip(shapes, offsets)):
        t = tens[ti]
        t["off"] = off
        t["cnt0"] = n_counters
        if len(shape) >= 2 and len(shape) not in (2, 4):
            raise NotImplementedError(f"{who}: {len(shape)}-d parameters are not supported")
        numel = math.prod(shape)
        if c_bytes and (c_bytes + numel * 4 > chunk_bytes or ti in bounds):   # close the current chunk before this tensor
            chunks.append((c_t0, ti, c_i0, len(items)))
            ws_max = max(ws_max, c_ws)
            c_t0, c_i0, c_bytes, c_ws = ti, len(items), 0, 0
        t["item0"] = len(items)
        if len(shape) == 2:
            kind, (d0, d1), kh, kw = 1, shape, 1, 1
            if d1 % 4:
                raise NotImplementedError(f"{who}: matrix rows must be a multiple of 4 elements")
            ntr, ntc = -(-d0 // AF_TR), -(-d1 // AF_TC)
            t["ws_row"], t["ws_col"] = c_ws, c_ws + ntc * d0
            c_ws += _align(ntc * d0 + ntr * d1)
            items += [(ti, r, c, 0) for r in range(ntr) for c in range(ntc)]
            t["mr0"] = mr_slots
            mr_slots += mr_per_strip * ntr
            n_counters += ntr + ntc
        elif len(shape) == 4:
            kind, (d0, d1, kh, kw) = 2, shape
            if kh > 3 or kw > 3:
                raise NotImplementedError(f"{who}: conv kernels larger than 3x3 are not supported")
            items += [(ti, r, 0, 0) for r in range(-(-(d0 * d1) // AF_CONV_PAIRS))]
        else:
            kind, d0, d1, kh, kw = 0, numel, 1, 1, 1
            items += [(ti, r, 0, 0) for r in range(-(-numel // AF_VEC))]
        t["kind"], t["d0"], t["d1"], t["kh"], t["kw"] = kind, d0, d1, kh, kw
        length = {"numel": numel, "d0": d0, "d1": d1, "row": d0 * kh * d1, "col": d0 * kw * d1}
        for field, n in state_fields[kind]:
            t[field] = state_off
            state_off += _align(length[n])
        t["nitems"] = len(items) - int(t["item0"])
        n_counters += 1
        c_bytes += numel * 4
    chunks.append((c_t0, len(shapes), c_i0, len(items)))
    ws_max = max(ws_max, c_ws)
    return {"tensors": tens, "items": np.array(items, dtype=np.int32).view(AF_ITEM_DTYPE).reshape(-1), "chunks": chunks,
            "state": state_off, "ws": ws_max, "mean_row": mr_slots, "counters": n_counters}


class _FlatOptimizer:
    """Checkpoints of the fused optimizers, in `torch.optim.Optimizer.state_dict()` layout: {"state": {i: {...}}, "param_groups": [one]},
    parameter i being `store.params[i]` (registration order, as torch numbers them).  A class supplies `param_state(i)` (views of its
    buffers under its upstream class's keys and logical shapes), `_group_dict()`, `reset_state()`, and overrides the hooks below where it
    differs."""

    _matched = ()   # keys of param_state() that a checkpoint has to equal instead of setting them

    def _saved_state(self, i: int) -> dict:
        """parameter i's checkpoint entry: param_state(i) with the tensors copied"""
        return {k: (v.detach().clone().contiguous() if torch.is_tensor(v) else v) for k, v in self.param_state(i).items()}

    def state_dict(self) -> dict:
        state = {i: self._saved_state(i) for i in range(self.ntensors)} if self.step_count > 0 else {}
        return {"state": state, "param_groups": [{**self._group_dict(), "params": list(range(self.ntensors))}]}

    def _accepts_partial_state(self) -> bool:
        return False

    def _check_entry(self, i: int, st: dict, mine: dict) -> None:
        """refuse a checkpoint entry `st` that does not fit parameter i's own state `mine` (shapes are checked by the caller)"""
        if set(mine) != set(k for k in st if k != "step"):
            raise ValueError(f"{type(self).__name__}.load_state_dict: parameter {i} has state {sorted(st)}, expected {sorted(mine)}")

    def _saved_step(self, sd: dict, state: dict) -> Optional[int]:
        """the step count a checkpoint carries: one per parameter, all equal"""
        steps = set(int(st["step"]) for st in state.values())
        if len(steps) != 1:
            raise ValueError(f"{type(self).__name__}.load_state_dict: per-parameter step counts differ ({sorted(steps)}); the fused update keeps one")
        return steps.pop()

    def _copy_state(self, state: dict) -> None:
        with torch.no_grad():
            for i, st in state.items():
                for k, v in self.param_state(i).items():
                    if torch.is_tensor(v) and k not in self._matched:
                        v.copy_(st[k].to(v.device, v.dtype))

    def load_state_dict(self, sd: dict) -> None:
        """Every entry is checked before anything is copied.  A checkpoint without state resets the optimizer."""
        who = f"{type(self).__name__}.load_state_dict"
        state = {int(i): st for i, st in sd.get("state", {}).items()}
        if not state:
            self.reset_state()
            return
        if len(state) != self.ntensors and not self._accepts_partial_state():
            raise ValueError(f"{who}: state for {len(state)} of {self.ntensors} parameters")
        for i, st in state.items():
            if not 0 <= i < self.ntensors:
                raise ValueError(f"{who}: parameter index {i} out of range (0..{self.ntensors - 1})")
            mine = {k: v for k, v in self.param_state(i).items() if torch.is_tensor(v)}
            self._check_entry(i, st, mine)
            for k, v in mine.items():
                if tuple(v.shape) != tuple(st[k].shape):
                    raise ValueError(f"{who}: {k} of parameter {i} has shape {tuple(st[k].shape)}, expected {tuple(v.shape)}")
        step = self._saved_step(sd, state)
        self._copy_state(state)
        if step is not None:
            self.step_count = step


class _FlatFactored(_FlatOptimizer):
    """What FlatAdafactor and FlatCAME share: the tables of _plan_tables() on the device and one flat fp32 `state`."""

    def _plan(self, store, dtype: np.dtype, state_fields: dict, mr_per_strip: int, chunk_bytes: Optional[int], boundaries=None) -> int:
        """Lay out and upload the tables, allocate what both optimizers keep per tensor / item; returns the workspace size (floats)."""
        plan = _plan_tables(type(self).__name__, [tuple(p.shape) for p in store.params], store.offsets,
                           _default_chunk_bytes() if chunk_bytes is None else chunk_bytes, boundaries, dtype, state_fields, mr_per_strip)
        dev = store.master.device
        self.store = store
        self.step_count = 0
        self.chunks = plan["chunks"]   # (tensor_lo, tensor_hi, item_lo, item_hi)
        self._tens_np = plan["tensors"]
        self.tensors = torch.from_numpy(plan["tensors"].view(np.uint8).copy()).to(dev)
        self.items = torch.from_numpy(plan["items"].view(np.uint8).copy()).to(dev)
        # "blocks done" counters of the last-block-done finalisations (optim_common.h): zeroed before every step although every pass
        # leaves them at zero -- a step abandoned half way by the health gate must not poison the next one
        self.counters = torch.zeros(plan["counters"], dtype=torch.int32, device=dev)
        self.nitems, self.ntensors = len(plan["items"]), len(store.params)
        self.state = torch.zeros(max(plan["state"], 1), dtype=torch.float32, device=dev)
        self.u2_part = torch.zeros(self.nitems, dtype=torch.float32, device=dev)
        self.mean_row = torch.zeros(max(plan["mean_row"], 1), dtype=torch.float32, device=dev)
        return max(plan["ws"], 1)

    def reset_state(self) -> None:
        self.step_count = 0
        self.state.zero_()


class FlatAdafactor(_FlatFactored):
    """Adafactor on a FlatParamStore.  Constructor arguments as the reference's (adafactor.py:104-131)."""

    def __init__(self, store, lr: Optional[float] = None, eps: tuple[float, float] = (1e-30, 1e-3), clip_threshold: float = 1.0,
                 decay_rate: float = -0.8, beta1: Optional[float] = None, weight_decay: float = 0.0, scale_parameter: bool = True,
                 relative_step: bool = True, warmup_init: bool = False, chunk_bytes: Optional[int] = None, boundaries=None):
        if lr is not None and relative_step:
            raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
        if warmup_init and not relative_step:
            raise ValueError("`warmup_init=True` requires `relative_step=True`")
        self.beta1 = self._check_beta1(beta1)
        if query("nk_adafactor_tensor_bytes") != AF_TENSOR_DTYPE.itemsize:
            raise RuntimeError("FlatAdafactor: tensor table layout differs from the HIP library's")
        self.lr, self.eps, self.clip_threshold, self.decay_rate = lr, eps, clip_threshold, decay_rate
        self.weight_decay, self.scale_parameter, self.relative_step, self.warmup_init = weight_decay, scale_parameter, relative_step, warmup_init
        # `boundaries`: tensor indices at which a new chunk must begin (the first parameter of every top-level UNet block), so
        # that a block's update can be issued as soon as that block's gradients are final, while backward is still running
        self._ws_stride = self._plan(store, AF_TENSOR_DTYPE, _AF_STATE, 1, chunk_bytes, boundaries)
        dev = store.master.device
        # NK_AF_STREAMS (default 1; 2 = A/B): consecutive chunks alternate between two streams forked from the caller's, so that one chunk's
        # tail (counter round trips, finishing blocks) runs beside the next chunk's loads.  Chunks share nothing but the
        # partial-sum workspace, which then exists once per stream.
        self.nstreams = 2 if os.environ.get("NK_AF_STREAMS", "1") == "2" else 1
        self._side = None
        self.ws = torch.empty(self._ws_stride * self.nstreams, dtype=torch.float32, device=dev)
        self.p2_part = torch.zeros(self.nitems, dtype=torch.float32, device=dev)
        self.scale = torch.zeros(self.ntensors, dtype=torch.float32, device=dev)
        self.lr_t = torch.zeros(self.ntensors, dtype=torch.float32, device=dev)
        self._p2_valid = False
        self.owned = None          # restrict_ranges(): [(tensor_lo, tensor_hi), ...] this process updates; None = everything
        store.add_listener(self)

    def _check_beta1(self, beta1: Optional[float]) -> Optional[float]:
        if beta1 is not None:
            raise NotImplementedError("FlatAdafactor: beta1 (first moment) is FlatAdafactorMomentum's: this class keeps no exp_avg buffer")
        return None

    def restrict(self, tensor_lo: int, tensor_hi: int) -> None:
        self.restrict_ranges([(tensor_lo, tensor_hi)])

    def restrict_ranges(self, ranges) -> None:
        """Update only the tensors inside `ranges` = [(tensor_lo, tensor_hi), ...] from now on (data-parallel rs_ag mode: a rank owns one
        tensor-aligned part of every slice of the flat buffers; the others' updated shadows arrive by all-gather).  Chunks are cut at every
        boundary; per-tensor state never crosses a tensor, so cutting changes no arithmetic."""
        ranges = sorted((int(a), int(b)) for a, b in ranges if b > a)
        bounds = sorted({x for ab in ranges for x in ab})
        cut = []
        for (t0, t1, i0, i1) in self.chunks:
            marks = sorted({t0, t1} | {b for b in bounds if t0 < b < t1})
            for a, b in zip(marks[:-1], marks[1:]):
                ia = i0 if a == t0 else int(self._tens_np[a]["item0"])
                ib = i1 if b == t1 else int(self._tens_np[b]["item0"])
                cut.append((a, b, ia, ib))
        self.chunks = cut
        self.owned = ranges

    def state_span(self, tensor_lo: int, tensor_hi: int) -> tuple[int, int]:
        """[lo, hi) of `self.state` (fp32 second-moment statistics) belonging to tensors [tensor_lo, tensor_hi): state is laid out in
        tensor order, so a tensor-aligned shard's statistics are one contiguous span (rs_ag gathers them for checkpoints)"""
        lo = int(self._tens_np[tensor_lo]["row_off"]) if tensor_lo < self.ntensors else self.state.numel()
        hi = int(self._tens_np[tensor_hi]["row_off"]) if tensor_hi < self.ntensors else self.state.numel()
        return lo, hi

    def _mine(self, ci: int) -> bool:
        return self.owned is None or any(self.chunks[ci][0] >= a and self.chunks[ci][1] <= b for a, b in self.owned)

    def masters_changed(self) -> None:
        """FlatParamStore hook: the fp32 masters were rewritten from outside (checkpoint load, broadcast, EMA swap): the
        per-tile sums of p^2 that scale_parameter uses are stale."""
        self._p2_valid = False

    # -- the update -------------------------------------------------------------------------------
    def _args(self, chunk, beta2t: float, rel_step: float, grad_scale: float, ws_slot: int = 0) -> _Args:
        t0, t1, i0, i1 = chunk
        s = self.store
        has_matrix = int((self._tens_np["kind"][t0:t1] == 1).any())
        return _Args(s.master.data_ptr(), s.grad.data_ptr(), s.shadow.data_ptr(), self.state.data_ptr(), self.ws.data_ptr() + 4 * self._ws_stride * ws_slot,
                     self.tensors.data_ptr(), self.items.data_ptr(), self.u2_part.data_ptr(), self.p2_part.data_ptr(),
                     self.mean_row.data_ptr(), self.scale.data_ptr(), self.lr_t.data_ptr(), i0, i1, t0, t1,
                     beta2t, self.eps[0], self.eps[1], self.clip_threshold, rel_step, self.weight_decay, grad_scale,
                     int(self.scale_parameter), self.counters.data_ptr(), has_matrix, 0)

    def rel_step(self, step: int) -> float:
        """adafactor.py:133-139"""
        if not self.relative_step:
            return float(self.lr)
        min_step = 1e-6 * step if self.warmup_init else 1e-2
        return min(min_step, 1.0 / math.sqrt(step))

    def refresh_param_norms(self) -> None:
        """Recompute the per-tile sums of p^2 (needed once, and again whenever the masters are changed from outside)."""
        a = self._args((0, self.ntensors, 0, self.nitems), 0.0, 0.0, 1.0)
        call("nk_adafactor_init", C.byref(a), ops._stream())
        self._p2_valid = True

    def step(self, grad_scale: float = 1.0) -> None:
        """One Adafactor update of every parameter (adafactor.py:162-255); also rewrites the bf16 shadows."""
        self.begin_step()
        if self.nstreams == 2 and self.store.master.is_cuda:
            cur = torch.cuda.current_stream()
            if self._side is None:
                self._side = [torch.cuda.Stream(device=self.store.master.device) for _ in range(2)]
            for st in self._side:
                st.wait_stream(cur)
            for ci in range(len(self.chunks)):
                with torch.cuda.stream(self._side[ci & 1]):
                    self.step_chunk(ci, grad_scale, ws_slot=ci & 1)
            for st in self._side:
                cur.wait_stream(st)
        else:
            for ci in range(len(self.chunks)):
                self.step_chunk(ci, grad_scale)
        self.end_step()

    # -- the same update, chunk by chunk: a chunk may be issued as soon as ITS gradients are final (DiffusionEngine streams the
    # update of each top-level block behind that block's backward).  Every per-step scalar (step count, beta2_t, relative step)
    # is fixed by begin_step(); the per-tensor statistics never cross a chunk, so the order of chunks does not matter. ------------
    def begin_step(self) -> None:
        if not self._p2_valid:
            self.refresh_param_norms()
        self.counters.zero_()
        self.step_count += 1
        self._beta2t = 1.0 - math.pow(self.step_count, self.decay_rate)
        self._rel = self.rel_step(self.step_count)
        self._done = [False] * len(self.chunks)

    def step_chunk(self, ci: int, grad_scale: float = 1.0, ws_slot: int = 0) -> None:
        if self._done[ci]:
            return
        if not self._mine(ci):          # another rank's shard
            self._done[ci] = True
            return
        self._launch_chunk(self._args(self.chunks[ci], self._beta2t, self._rel, grad_scale, ws_slot))
        self._done[ci] = True

    def _launch_chunk(self, a: _Args) -> None:
        call("nk_adafactor_chunk", C.byref(a), ops._stream())

    def chunks_in(self, tensor_lo: int, tensor_hi: int) -> list:
        """indices of the chunks that lie entirely inside tensors [tensor_lo, tensor_hi)"""
        return [ci for ci, c in enumerate(self.chunks) if c[0] >= tensor_lo and c[1] <= tensor_hi]

    def end_step(self, grad_scale: float = 1.0) -> None:
        for ci in range(len(self.chunks)):
            self.step_chunk(ci, grad_scale)
        self.store._mark_fresh()

    # -- introspection mirroring the reference's per-parameter state --------------------------------
    def current_lrs(self) -> Tensor:
        """Per-tensor lr of the last step (what `_get_lr` returned for each parameter)."""
        return self.lr_t

    def param_state(self, index: int) -> dict:
        t = self._tens_np[index]
        p = self.store.params[index]
        if t["kind"] == 1:
            return {"step": self.step_count, "exp_avg_sq_row": self.state[int(t["row_off"]):int(t["row_off"]) + int(t["d0"])],
                    "exp_avg_sq_col": self.state[int(t["col_off"]):int(t["col_off"]) + int(t["d1"])]}
        if t["kind"] == 2:
            O, I, KH, KW = p.shape
            row = self.state[int(t["row_off"]):int(t["row_off"]) + O * KH * I].view(O, KH, I).permute(0, 2, 1)
            col = self.state[int(t["col_off"]):int(t["col_off"]) + O * KW * I].view(O, KW, I).permute(0, 2, 1)
            return {"step": self.step_count, "exp_avg_sq_row": row, "exp_avg_sq_col": col}
        return {"step": self.step_count, "exp_avg_sq": self.state[int(t["row_off"]):int(t["row_off"]) + p.numel()].view(p.shape)}


    # -- checkpointing (torch.optim.Optimizer.state_dict layout, the reference class's keys: adafactor.py:186-204) ------
    def _rms(self, index: int) -> Tensor:
        p = self.store.params[index]
        return (ops._phys_flat(p).float().norm(2) / (p.numel() ** 0.5)).reshape(())

    def _saved_state(self, i: int) -> dict:
        """Tensors are copies in the reference's logical shapes."""
        st = super()._saved_state(i)
        st["RMS"] = self._rms(i) if self.scale_parameter else 0
        return st

    def _group_dict(self) -> dict:
        return dict(lr=self.lr, eps=self.eps, clip_threshold=self.clip_threshold, decay_rate=self.decay_rate, beta1=self.beta1,
                    weight_decay=self.weight_decay, scale_parameter=self.scale_parameter, relative_step=self.relative_step,
                    warmup_init=self.warmup_init)

    def _accepts_partial_state(self) -> bool:
        return True

    def _check_entry(self, i: int, st: dict, mine: dict) -> None:
        who = f"{type(self).__name__}.load_state_dict"
        if ("exp_avg" in mine) != ("exp_avg" in st):
            raise ValueError(f"{who}: parameter {i} has {'a' if 'exp_avg' in mine else 'no'} first moment here (beta1={self.beta1}) but the "
                             f"checkpoint has {'none' if 'exp_avg' in mine else 'one'} (exp_avg)")
        for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            if (k in mine) != (k in st):
                raise ValueError(f"{who}: parameter {i} is {'not ' if k not in mine else ''}factored here but the checkpoint disagrees ({k})")

    def _copy_state(self, state: dict) -> None:
        super()._copy_state(state)
        self._p2_valid = False       # RMS(p) is recomputed from the (separately restored) parameters


class FlatAdafactorMomentum(FlatAdafactor):
    """FlatAdafactor with the reference's first moment (adafactor.py:194-196, 242-245): after the clipped, scaled update u~ = scale u has
    been formed, exp_avg = beta1 exp_avg + (1 - beta1) u~ (fp32, zero at the first step, no bias correction) and p = p (1 - wd lr_t) - exp_avg.
    Same constructor with a mandatory `beta1` in [0, 1).  `exp_avg` is one flat fp32 buffer with the masters' physical layout and element
    offsets, read and written by the apply pass (`nk_adafactor_chunk_momentum`): 4 B of state and 8 B of traffic more per parameter.  It never
    crosses a tensor, so chunks may go in any order, on one stream or two.  The sharded exchange is refused: its shard gather knows one
    state span per tensor range."""

    def __init__(self, store, *args, **kwargs):
        super().__init__(store, *args, **kwargs)
        self.exp_avg = torch.zeros(store.master.numel(), dtype=torch.float32, device=store.master.device)

    def _check_beta1(self, beta1: Optional[float]) -> float:
        if beta1 is None:
            raise ValueError("FlatAdafactorMomentum: beta1 is required (FlatAdafactor is the optimizer without a first moment)")
        if not 0.0 <= beta1 < 1.0:
            raise ValueError(f"FlatAdafactorMomentum: beta1 must be in [0, 1), got {beta1}")
        return float(beta1)

    def reset_state(self) -> None:
        super().reset_state()
        self.exp_avg.zero_()

    def restrict_ranges(self, ranges) -> None:
        raise NotImplementedError("FlatAdafactorMomentum: the sharded exchange (rs_ag) with a first moment (beta1) is not built: the shard "
                                  "gather knows one state span per tensor range")

    def _launch_chunk(self, a: _Args) -> None:
        call("nk_adafactor_chunk_momentum", C.byref(a), self.exp_avg.data_ptr(), self.beta1, ops._stream())

    def param_state(self, index: int) -> dict:
        """FlatAdafactor's entries and `exp_avg` in the parameter's logical shape (conv weights: an OIHW view of the physical
        [O][KH][KW][I] slice)"""
        st = super().param_state(index)
        st["exp_avg"] = self.store._view(self.exp_avg, int(self._tens_np[index]["off"]), self.store.params[index])
        return st


class AdafactorScheduler:
    """Proxy scheduler (adafactor.py:258-291): reports `initial_lr` before the first step, then the optimizer's own lr of
    the first parameter."""

    def __init__(self, optimizer: FlatAdafactor, initial_lr: float = 0.0):
        self.optimizer, self.initial_lr = optimizer, initial_lr

    def get_lr(self) -> list[float]:
        if self.optimizer.step_count == 0:
            return [self.initial_lr]
        return [float(self.optimizer.lr_t[0])]

    def step(self) -> None:
        pass


CAME_TENSOR_DTYPE = np.dtype([("off", "<i8"), ("m_off", "<i8"), ("r_off", "<i8"), ("c_off", "<i8"), ("rr_off", "<i8"), ("cr_off", "<i8"),
                              ("ws_row", "<i8"), ("ws_col", "<i8"), ("kind", "<i4"), ("d0", "<i4"), ("d1", "<i4"), ("kh", "<i4"), ("kw", "<i4"),
                              ("item0", "<i4"), ("nitems", "<i4"), ("mr0", "<i4"), ("cnt0", "<i4"), ("pad", "<i4")])


class _CameArgs(C.Structure):
    _fields_ = [("master", C.c_void_p), ("grad", C.c_void_p), ("shadow", C.c_void_p), ("state", C.c_void_p), ("ws", C.c_void_p),
                ("tensors", C.c_void_p), ("items", C.c_void_p), ("u2_part", C.c_void_p), ("mean_row", C.c_void_p), ("denom", C.c_void_p),
                ("counters", C.c_void_p), ("item_lo", C.c_int), ("item_hi", C.c_int), ("tensor_lo", C.c_int), ("tensor_hi", C.c_int),
                ("beta1", C.c_float), ("beta2", C.c_float), ("beta3", C.c_float),
                ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float), ("one_minus_beta3", C.c_float), ("eps1", C.c_float), ("eps2", C.c_float),
                ("clip_threshold", C.c_float), ("lr", C.c_float), ("decay", C.c_float), ("grad_scale", C.c_float), ("has_matrix", C.c_int)]


class FlatCAME(_FlatFactored):
    """CAME on a FlatParamStore: the reference's `neurosis.optimizers.came.CAME` (optimizers/came.py:115-224) as up to four
    multi-tensor HIP launches per chunk of tensors (`csrc/came.hip`).  Same rule per tensor: factored (over the last two dims)
    second moment of g^2+eps1, update clipped by its RMS, first moment m, and for tensors with >= 2 dims a factored statistic of
    the residual (u_hat - m)^2 + eps2 that preconditions m; decoupled weight decay; no bias correction.

    Differences, all deliberate: the masters are fp32 and the bf16 shadow the kernels read is written round-to-nearest (the
    reference rounds bf16 parameters stochastically, `copy_stochastic_`), as the fused Adafactor and AdamW do; `ams_bound` is not
    implemented, and neither is `weight_decouple=False` with a weight decay (in the reference that only edits `p.grad` after the
    update has been computed, without effect on the step): both raise.  Conv weights (OIHW) have the shape limits of
    FlatAdafactor (<= 3x3), matrix rows must be a multiple of 4 elements."""

    def __init__(self, store, lr: float = 2e-4, betas: tuple[float, float, float] = (0.9, 0.999, 0.9999), weight_decay: float = 0.0,
                 weight_decouple: bool = True, fixed_decay: bool = False, clip_threshold: float = 1.0, eps1: float = 1e-30,
                 eps2: float = 1e-16, chunk_bytes: Optional[int] = None):
        _came_validate(lr, betas, weight_decay, weight_decouple, eps1, eps2, "FlatCAME")
        if query("nk_came_tensor_bytes") != CAME_TENSOR_DTYPE.itemsize:
            raise RuntimeError("FlatCAME: tensor table layout differs from the HIP library's")
        self.lr, self.betas, self.weight_decay = float(lr), tuple(float(b) for b in betas), float(weight_decay)
        self.weight_decouple, self.fixed_decay = bool(weight_decouple), bool(fixed_decay)
        self.clip_threshold, self.eps1, self.eps2 = float(clip_threshold), float(eps1), float(eps2)
        # mean_row: partial sums of R, then of Rr, per 256-row strip.  No `boundaries`: this update is not streamed behind backward
        ws = self._plan(store, CAME_TENSOR_DTYPE, _CAME_STATE, 2, chunk_bytes)
        dev = store.master.device
        self.ws = torch.empty(ws, dtype=torch.float32, device=dev)
        self.denom = torch.zeros(self.ntensors, dtype=torch.float32, device=dev)
        self._has_matrix = [int((self._tens_np["kind"][t0:t1] == 1).any()) for (t0, t1, _, _) in self.chunks]

    def decay_factor(self, lr: float) -> float:
        """The decoupled weight decay's multiplier of p (pytorch_optimizer BaseOptimizer.apply_weight_decay)."""
        return 1.0 - self.weight_decay * (1.0 if self.fixed_decay else lr)

    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        """One CAME update of every parameter (came.py:136-224) with the gradients multiplied by `grad_scale` (the data-parallel
        mean); `lr` overrides the constructor's (what a torch LR scheduler set on the group).  Also rewrites the bf16 shadows."""
        if lr is not None:
            self.lr = float(lr)
        self.counters.zero_()
        self.step_count += 1
        s = self.store
        b1, b2, b3 = self.betas
        for (t0, t1, i0, i1), has_matrix in zip(self.chunks, self._has_matrix):
            a = _CameArgs(s.master.data_ptr(), s.grad.data_ptr(), s.shadow.data_ptr(), self.state.data_ptr(), self.ws.data_ptr(),
                          self.tensors.data_ptr(), self.items.data_ptr(), self.u2_part.data_ptr(), self.mean_row.data_ptr(),
                          self.denom.data_ptr(), self.counters.data_ptr(), i0, i1, t0, t1, b1, b2, b3, 1.0 - b1, 1.0 - b2, 1.0 - b3, self.eps1, self.eps2,
                          self.clip_threshold, self.lr, self.decay_factor(self.lr), grad_scale, has_matrix)
            call("nk_came_chunk", C.byref(a), ops._stream())
        s._mark_fresh()

    # -- introspection mirroring the reference's per-parameter state (came.py:151-164) ---------------
    def param_state(self, index: int) -> dict:
        """Views of parameter `index`'s state under the reference's keys and logical shapes (conv statistics permuted from the
        physical [O][KH][I] / [O][KW][I] to [O, I, KH] / [O, I, KW])."""
        t = self._tens_np[index]
        p = self.store.params[index]
        st = {"exp_avg": self.store._view(self.state, int(t["m_off"]), p)}
        if t["kind"] == 1:
            d0, d1 = int(t["d0"]), int(t["d1"])
            for k, off, n in (("exp_avg_sq_row", "r_off", d0), ("exp_avg_sq_col", "c_off", d1), ("exp_avg_res_row", "rr_off", d0),
                              ("exp_avg_res_col", "cr_off", d1)):
                st[k] = self.state[int(t[off]):int(t[off]) + n]
        elif t["kind"] == 2:
            O, I, KH, KW = p.shape
            for k, off, K in (("exp_avg_sq_row", "r_off", KH), ("exp_avg_sq_col", "c_off", KW), ("exp_avg_res_row", "rr_off", KH),
                              ("exp_avg_res_col", "cr_off", KW)):
                st[k] = self.state[int(t[off]):int(t[off]) + O * K * I].view(O, K, I).permute(0, 2, 1)
        else:
            st["exp_avg_sq"] = self.state[int(t["r_off"]):int(t["r_off"]) + p.numel()].view(p.shape)
        return st

    # -- checkpointing (torch.optim.Optimizer.state_dict layout, the reference's keys; `step` is the group's) -------------
    def _group_dict(self) -> dict:
        return dict(lr=self.lr, betas=self.betas, weight_decay=self.weight_decay, weight_decouple=self.weight_decouple,
                    fixed_decay=self.fixed_decay, ams_bound=False, eps1=self.eps1, eps2=self.eps2, step=self.step_count)

    def _accepts_partial_state(self) -> bool:
        return self.step_count > 0

    def _saved_step(self, sd: dict, state: dict) -> Optional[int]:
        groups = sd.get("param_groups", [])
        return int(groups[0]["step"]) if groups and "step" in groups[0] else None


def _came_validate(lr, betas, weight_decay, weight_decouple, eps1, eps2, who: str) -> None:
    """The reference constructor's checks (pytorch_optimizer's validate_learning_rate / validate_betas / validate_non_negative),
    plus the refusal of `weight_decouple=False` with a weight decay."""
    if lr < 0.0:
        raise ValueError(f"[-] learning rate must be positive. got {lr}")
    if len(betas) != 3 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"[-] betas must be three values in the range [0, 1). got {tuple(betas)}")
    for name, v in (("weight_decay", weight_decay), ("eps1", eps1), ("eps2", eps2)):
        if v < 0.0:
            raise ValueError(f"[-] {name} must be non-negative. got {v}")
    if not weight_decouple and weight_decay > 0.0:
        raise NotImplementedError(f"{who}: weight_decouple=False with weight_decay > 0 is not implemented (in the reference it adds wd * p "
                                  "to p.grad after the update has been computed, which does not change that step)")


A8_BLOCK = 256
A8_TENSOR_DTYPE = np.dtype([("off", "<i8"), ("soff", "<i8"), ("numel", "<i4"), ("is8", "<i4")])


def create_dynamic_map(signed: bool = True, max_exponent_bits: int = 7, total_bits: int = 8) -> Tensor:
    """The 256-entry quantization map of bitsandbytes' `create_dynamic_map` for 8 bits and 7 exponent bits: for decade i = 0..6, the
    midpoints of linspace(0.1, 1, n + 1) with n = 2**i (signed) or 2**(i + 1) (unsigned), scaled by 10**(i - 6), and for the signed map
    their negations too; then 0 and 1.0; sorted, fp32.  The signed map runs from -0.99297 to 1.0 (asymmetric on purpose)."""
    if (max_exponent_bits, total_bits) != (7, 8):
        raise NotImplementedError("create_dynamic_map: only the 8-bit map with 7 exponent bits is built")
    data = []
    for i in range(max_exponent_bits):
        n = 2 ** i if signed else 2 ** (i + 1)
        bounds = torch.linspace(0.1, 1, n + 1)
        means = ((bounds[:-1] + bounds[1:]) / 2.0).tolist()
        scale = 10 ** (-(max_exponent_bits - 1) + i)
        data += [scale * x for x in means]
        if signed:
            data += [-scale * x for x in means]
    data += [0.0, 1.0]
    assert len(data) == 2 ** total_bits
    return torch.tensor(sorted(data), dtype=torch.float32)


class _A8Args(C.Structure):
    _fields_ = [("master", C.c_void_p), ("grad", C.c_void_p), ("shadow", C.c_void_p), ("code1", C.c_void_p), ("code2", C.c_void_p),
                ("absmax1", C.c_void_p), ("absmax2", C.c_void_p), ("m32", C.c_void_p), ("v32", C.c_void_p), ("qmap1", C.c_void_p),
                ("qmap2", C.c_void_p), ("tensors", C.c_void_p), ("blk_start", C.c_void_p), ("ntensors", C.c_int), ("nblocks", C.c_int),
                ("beta1", C.c_float), ("beta2", C.c_float), ("one_minus_beta1", C.c_float), ("one_minus_beta2", C.c_float), ("eps", C.c_float),
                ("lr", C.c_float), ("decay", C.c_float), ("bc1", C.c_float), ("bc2", C.c_float), ("grad_scale", C.c_float)]


class FlatAdamW8bit(_FlatOptimizer):
    """8-bit blockwise AdamW on a FlatParamStore (`csrc/adamw8bit.hip`, one launch per step): bitsandbytes' `AdamW8bit` algorithm,
    restated here as the definition (bit-for-bit interchange with bitsandbytes itself is not claimed).

    * Maps: qmap1 = create_dynamic_map(signed=True) for m, qmap2 = create_dynamic_map(signed=False) for v.
    * Blocks: 256 consecutive elements of ONE parameter, in its physical order (conv weights [O][KH][KW][I]); the last block of a
      parameter may be short; blocks never straddle parameters, so nothing depends on where a parameter sits in the store.
    * Parameters with fewer than `min_8bit_size` elements keep fp32 m / v and take the plain AdamW step.
    * Per element of an 8-bit parameter: g = grad * grad_scale; m = qmap1[c1] * absmax1[blk], v = qmap2[c2] * absmax2[blk];
      m = b1 m + (1-b1) g; v = b2 v + (1-b2) g g; p = p (1 - lr wd) - lr (m / bc1) / (sqrt(v / bc2) + eps) with the unquantized new m, v;
      then per block absmax = max |m| and c1 = the index of the map entry nearest to m / absmax (lowest index on a tie; absmax 0 stores
      the code of 0.0); the same for v with qmap2.  bc1 = 1 - b1^t, bc2 = 1 - b2^t, 1 - b and 1 - lr wd are computed in double.
    * Initial state: absmax 0 and every code the code of 0.0 (m = v = 0).

    State: one byte each for m and v plus two fp32 absmax per 256 elements (2.03 B/param against AdamW's 8).  `state_dict()` speaks
    bitsandbytes' per-parameter keys (`state1`, `state2`, `absmax1`, `absmax2`, `qmap1`, `qmap2`, `step`; fp32 `state1` / `state2` only
    for small parameters)."""

    def __init__(self, store, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 min_8bit_size: int = 4096):
        _adamw_validate(lr, betas, eps, weight_decay)
        if query("nk_adamw8bit_tensor_bytes") != A8_TENSOR_DTYPE.itemsize:
            raise RuntimeError("FlatAdamW8bit: tensor table layout differs from the HIP library's")
        self.store = store
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), tuple(float(b) for b in betas), float(eps), float(weight_decay)
        self.min_8bit_size = int(min_8bit_size)
        self.step_count = 0
        dev = store.master.device
        layout = self.layout([tuple(p.shape) for p in store.params], self.min_8bit_size)
        tens = np.zeros(len(store.params), dtype=A8_TENSOR_DTYPE)
        tens["off"] = store.offsets
        tens["soff"], tens["numel"], tens["is8"] = layout["soff"], layout["numel"], layout["is8"]
        if int(layout["numel"].max()) >= 2 ** 31 or layout["nblocks"] >= 2 ** 31 - 16:     # the kernel indexes elements of a tensor and blocks in int
            raise NotImplementedError("FlatAdamW8bit: 2^31 or more elements in one parameter, or 2^31 - 16 or more blocks in one store")
        self._tens_np = tens
        self._blk = layout["blk_start"]
        self.ntensors, self.nblocks = len(store.params), int(layout["nblocks"])
        self.tensors = torch.from_numpy(tens.view(np.uint8).copy()).to(dev)
        self.blk_start = torch.from_numpy(self._blk.astype(np.int32)).to(dev)
        self.qmap1 = create_dynamic_map(signed=True).to(dev)
        self.qmap2 = create_dynamic_map(signed=False).to(dev)
        self.code1 = torch.empty(self.nblocks * A8_BLOCK, dtype=torch.uint8, device=dev)
        self.code2 = torch.empty(self.nblocks * A8_BLOCK, dtype=torch.uint8, device=dev)
        self.absmax1 = torch.zeros(self.nblocks, dtype=torch.float32, device=dev)
        self.absmax2 = torch.zeros(self.nblocks, dtype=torch.float32, device=dev)
        self.m32 = torch.zeros(max(int(layout["small"]), 1), dtype=torch.float32, device=dev)
        self.v32 = torch.zeros_like(self.m32)
        self.zero_codes = (int(torch.nonzero(self.qmap1.cpu() == 0)[0]), int(torch.nonzero(self.qmap2.cpu() == 0)[0]))
        self.reset_state()

    @staticmethod
    def layout(shapes, min_8bit_size: int = 4096) -> dict:
        """Per parameter shape: numel, is8, first block (blk_start, with the total appended) and fp32-state offset (soff, 64-aligned);
        plus nblocks and the fp32 state size `small`.  Every parameter has blocks (the fp32 ones leave their codes unused)."""
        numel = np.array([int(np.prod(s)) for s in shapes], dtype=np.int64)
        is8 = (numel >= min_8bit_size).astype(np.int32)
        nblk = -(-numel // A8_BLOCK)
        blk_start = np.concatenate([[0], np.cumsum(nblk)]).astype(np.int64)
        small = np.where(is8 == 0, (numel + 63) // 64 * 64, 0)
        soff = np.concatenate([[0], np.cumsum(small)[:-1]]).astype(np.int64)
        return {"numel": numel, "is8": is8, "blk_start": blk_start, "soff": soff, "nblocks": int(blk_start[-1]), "small": int(small.sum())}

    @classmethod
    def state_bytes(cls, shapes, min_8bit_size: int = 4096) -> int:
        """Bytes of optimizer state for these parameter shapes: the codes (one byte each for m and v, whole blocks) and the two fp32 absmax
        of every 8-bit parameter's blocks, fp32 m and v of the small ones."""
        lay = cls.layout(shapes, min_8bit_size)
        nblk = np.diff(lay["blk_start"])
        return int((nblk * (2 * A8_BLOCK + 8) * lay["is8"]).sum() + 8 * (lay["numel"] * (1 - lay["is8"])).sum())

    def reset_state(self) -> None:
        """Step 0: absmax 0, every code the code of 0.0, fp32 state 0."""
        self.code1.fill_(self.zero_codes[0])
        self.code2.fill_(self.zero_codes[1])
        self.absmax1.zero_()
        self.absmax2.zero_()
        self.m32.zero_()
        self.v32.zero_()
        self.step_count = 0

    def step(self, grad_scale: float = 1.0, lr: Optional[float] = None) -> None:
        """One AdamW8bit update of every parameter with the gradients multiplied by `grad_scale` (the data-parallel mean); `lr` overrides
        the constructor's (what a torch LR scheduler set on the group).  Also rewrites the bf16 shadows."""
        if lr is not None:
            self.lr = float(lr)
        self.step_count += 1
        s = self.store
        b1, b2 = self.betas
        t = self.step_count
        a = _A8Args(s.master.data_ptr(), s.grad.data_ptr(), s.shadow.data_ptr(), self.code1.data_ptr(), self.code2.data_ptr(),
                    self.absmax1.data_ptr(), self.absmax2.data_ptr(), self.m32.data_ptr(), self.v32.data_ptr(), self.qmap1.data_ptr(),
                    self.qmap2.data_ptr(), self.tensors.data_ptr(), self.blk_start.data_ptr(), self.ntensors, self.nblocks,
                    b1, b2, 1.0 - b1, 1.0 - b2, self.eps, self.lr, 1.0 - self.lr * self.weight_decay, 1.0 - b1 ** t, 1.0 - b2 ** t, grad_scale)
        call("nk_adamw8bit_step", C.byref(a), ops._stream())
        s._mark_fresh()

    # -- introspection under bitsandbytes' per-parameter keys ------------------------------------------------------------------------------
    def param_state(self, index: int) -> dict:
        """Views of parameter `index`'s state: `state1` / `state2` in the parameter's shape (uint8 codes, or fp32 m / v for a small
        parameter); for 8-bit parameters also `absmax1` / `absmax2` (one per block) and the maps."""
        t = self._tens_np[index]
        p = self.store.params[index]
        if not t["is8"]:
            return {"state1": self.store._view(self.m32, int(t["soff"]), p), "state2": self.store._view(self.v32, int(t["soff"]), p)}
        b0, b1 = int(self._blk[index]), int(self._blk[index + 1])
        return {"state1": self.store._view(self.code1, b0 * A8_BLOCK, p), "state2": self.store._view(self.code2, b0 * A8_BLOCK, p),
                "absmax1": self.absmax1[b0:b1], "absmax2": self.absmax2[b0:b1], "qmap1": self.qmap1, "qmap2": self.qmap2}

    # -- checkpointing (torch.optim.Optimizer.state_dict layout, bitsandbytes' keys) ---------------------------------------------------------
    _matched = ("qmap1", "qmap2")

    def _saved_state(self, i: int) -> dict:
        return {**super()._saved_state(i), "step": self.step_count}

    def _group_dict(self) -> dict:
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, min_8bit_size=self.min_8bit_size)

    def _check_entry(self, i: int, st: dict, mine: dict) -> None:
        if set(mine) != set(k for k in st if k != "step"):
            raise ValueError(f"FlatAdamW8bit.load_state_dict: parameter {i} has state {sorted(st)}, expected {sorted(mine)} "
                             f"(min_8bit_size {self.min_8bit_size})")
        for k in self._matched:
            if k in mine and not torch.equal(st[k].detach().to("cpu", torch.float32), mine[k].cpu()):
                raise ValueError(f"FlatAdamW8bit.load_state_dict: {k} of parameter {i} differs from this optimizer's quantization map")
        for k in ("absmax1", "absmax2"):
            if k in mine and tuple(st[k].shape) != tuple(mine[k].shape):
                raise ValueError(f"FlatAdamW8bit.load_state_dict: {k} of parameter {i} has {tuple(st[k].shape)} blocks, expected "
                                 f"{tuple(mine[k].shape)} (block size {A8_BLOCK})")
        for k in ("state1", "state2"):
            if tuple(st[k].shape) != tuple(mine[k].shape) or st[k].dtype != mine[k].dtype:
                raise ValueError(f"FlatAdamW8bit.load_state_dict: {k} of parameter {i} is {st[k].dtype} {tuple(st[k].shape)}, "
                                 f"expected {mine[k].dtype} {tuple(mine[k].shape)}")

    def _copy_state(self, state: dict) -> None:
        self.reset_state()          # the codes and absmax that no parameter's views cover (block tails) are those of step 0
        super()._copy_state(state)


def _adamw_validate(lr, betas, eps, weight_decay) -> None:
    """torch.optim.AdamW's constructor checks."""
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if len(betas) != 2:
        raise ValueError(f"Invalid betas: {tuple(betas)}")
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


class FlatEma(torch.nn.Module):
    """`LitEma` (reference modules/ema.py:11-93) for a FlatParamStore: ONE flat fp32 shadow of every trainable parameter,
    updated by one kernel per step.  Same constructor arguments, decay warm-up `min(decay, (1+n)/(10+n))`, and the
    `store` / `copy_to` / `restore` protocol `DiffusionEngine.ema_scope` uses (models/diffusion.py:247-257).

    Checkpoint format = LitEma's: buffers `decay`, `num_updates` and one buffer per parameter named after it with the dots
    removed (ema.py:25-29); here those per-parameter entries are views of the flat shadow, written and read through
    `_save_to_state_dict` / `_load_from_state_dict`.  `names` are the parameter names as LitEma saw them (relative to the
    wrapped model, e.g. `diffusion_model.input_blocks.0.0.weight`); without names, positional `p<i>` keys are used."""

    def __init__(self, store, decay: float = 0.9999, use_num_updates: bool = True, names=None):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.param_store = store
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_updates else -1, dtype=torch.int))
        self._decay = float(decay)                       # host copies: update() must not read the device
        self._num_updates = 0 if use_num_updates else -1
        self.shadow = store.master.detach().clone()      # not a registered buffer: saved per parameter (below)
        self.collected: Optional[Tensor] = None
        names = list(names) if names is not None else [f"p{i}" for i in range(len(store.params))]
        if len(names) != len(store.params):
            raise ValueError("FlatEma: one name per store parameter expected")
        self.m_name2s_name = {n: n.replace(".", "") for n in names}
        self._s_names = [self.m_name2s_name[n] for n in names]
        store.add_listener(self)

    def masters_changed(self) -> None:
        """FlatParamStore hook.  Before the first update the average IS the model (LitEma clones the parameters at
        construction, after the checkpoint is loaded): follow the new weights.  Later the average is training state of its own."""
        if self._num_updates <= 0 and self.collected is None:
            self.shadow.copy_(self.param_store.master)

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self.shadow = fn(self.shadow)
        return out

    def reset_num_updates(self) -> None:
        self._num_updates = 0
        self.num_updates.zero_()

    def update(self) -> None:
        """ema.py:40-59"""
        decay = self._decay
        if self._num_updates >= 0:
            self._num_updates += 1
            self.num_updates += 1
            decay = min(self._decay, (1 + self._num_updates) / (10 + self._num_updates))
        call("nk_ema_flat", self.shadow.data_ptr(), self.param_store.master.data_ptr(), self.shadow.numel(), float(1.0 - decay), ops._stream())

    def forward(self, model=None) -> None:   # LitEma is called as `self.model_ema(self.model)` (models/diffusion.py:244)
        self.update()

    def copy_to(self, model=None) -> None:
        """ema.py:61-68: the averaged weights become the model's (masters and bf16 shadows)."""
        self.param_store.master.copy_(self.shadow)
        self.param_store.refresh()

    def store(self, parameters=None) -> None:
        self.collected = self.param_store.master.detach().clone()

    def restore(self, parameters=None) -> None:
        if self.collected is None:
            raise RuntimeError("FlatEma.restore() without store()")
        self.param_store.master.copy_(self.collected)
        self.param_store.refresh()
        self.collected = None

    # -- LitEma-format checkpoint entries ---------------------------------------------------------------
    def _views(self):
        st = self.param_store
        return [(s, st._view(self.shadow, off, p)) for s, p, off in zip(self._s_names, st.params, st.offsets)]

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        for s_name, view in self._views():
            destination[prefix + s_name] = view if keep_vars else view.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        if prefix + "decay" in state_dict:
            self._decay = float(state_dict[prefix + "decay"])
        if prefix + "num_updates" in state_dict:
            self._num_updates = int(state_dict[prefix + "num_updates"])
        mine = set()
        for s_name, view in self._views():
            key = prefix + s_name
            mine.add(key)
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            src = state_dict[key]
            if tuple(src.shape) != tuple(view.shape):
                error_msgs.append(f"size mismatch for {key}: checkpoint {tuple(src.shape)}, model {tuple(view.shape)}")
                continue
            with torch.no_grad():
                view.copy_(src)
        # the base class reports every key under the prefix that is not a registered buffer: the per-parameter entries are ours
        unexpected_keys[:] = [k for k in unexpected_keys if k not in mine]
