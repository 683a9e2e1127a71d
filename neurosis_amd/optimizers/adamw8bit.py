"""`AdamW8bit`: bitsandbytes' blockwise 8-bit AdamW (`bitsandbytes.optim.AdamW8bit`, the optimizer of the reference's
`configs/sdxl/sdxl-te.example.yaml`): its constructor and defaults over one HIP launch of `neurosis_amd.optim.FlatAdamW8bit`
(`csrc/adamw8bit.hip`) per parameter group.  The algorithm is defined in `FlatAdamW8bit`'s docstring; bit-for-bit interchange with
bitsandbytes itself is not claimed.  Binding, stepping and checkpoints are `_FusedOptimizer`'s.

Not built, and refused loudly: `amsgrad=True`, `block_wise=False` (one absmax per tensor), `percentile_clipping < 100`, `args`
(bitsandbytes' per-module override object) and `is_paged=True` (paged state).  `optim_bits` is accepted and ignored, as in
bitsandbytes' own AdamW8bit, which always keeps 8-bit state.
"""
from __future__ import annotations

from ..optim import FlatAdamW8bit, _adamw_validate
from ._base import _FusedOptimizer, _group_store

__all__ = ["AdamW8bit"]

_WHO = "neurosis_amd.optimizers.AdamW8bit"


class AdamW8bit(_FusedOptimizer):
    """8-bit blockwise AdamW, fused (bitsandbytes.optim.AdamW8bit's constructor)."""

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, optim_bits: int = 32, args=None, min_8bit_size: int = 4096, percentile_clipping: int = 100,
                 block_wise: bool = True, is_paged: bool = False):
        _adamw_validate(lr, betas, eps, weight_decay)
        if amsgrad:
            raise NotImplementedError(f"{_WHO}: amsgrad=True is not implemented (it needs a third, max-of-v state)")
        if not block_wise:
            raise NotImplementedError(f"{_WHO}: block_wise=False (one absmax per tensor) is not implemented; only the blockwise "
                                      "quantization (256 elements per block) is built")
        if percentile_clipping < 100:
            raise NotImplementedError(f"{_WHO}: percentile_clipping={percentile_clipping} is not implemented (gradient-norm history "
                                      "clipping); only 100 (off) is built")
        if args is not None:
            raise NotImplementedError(f"{_WHO}: `args` (a per-module override object) is not implemented; pass the hyper-parameters directly")
        if is_paged:
            raise NotImplementedError(f"{_WHO}: is_paged=True (paged optimizer state) is not implemented")
        if min_8bit_size < 1:
            raise ValueError(f"Invalid min_8bit_size: {min_8bit_size}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults)
        self.min_8bit_size = int(min_8bit_size)

    def _make_flat(self, g: dict) -> FlatAdamW8bit:
        return FlatAdamW8bit(_group_store(g, "AdamW8bit"), lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"],
                             min_8bit_size=self.min_8bit_size)

    def _push(self, g: dict, f: FlatAdamW8bit) -> None:
        _adamw_validate(g["lr"], g["betas"], g["eps"], g["weight_decay"])
        f.lr, f.betas, f.eps, f.weight_decay = float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"])

    def _group_extras(self, f: FlatAdamW8bit) -> dict:
        return {"step": f.step_count}       # the group carries the step count beside the per-parameter ones (which are what a load reads)
