"""Class-label conditioning (`neurosis.modules.encoders.classed`, reference :9-32): `ClassEmbedder` looks a learned row up per class id and
hands it to the UNet through `GeneralConditioner` -- [B, embed_dim] is filed under "vector" (a UNet with num_classes="sequential" and
adm_in_channels=embed_dim), [B, 1, embed_dim] with add_sequence_dim under "crossattn".  The last class, n_classes - 1, is the
unconditional one (`get_unconditional_conditioning`).

The lookup is ops.label_rows on the fp32 table (fp32 out: the rows themselves, bit for bit).  With is_trainable=True the embedder follows
the trainable-embedder contract of DiffusionEngine (as the text towers do): `trained_parameters()` is what the engine puts in the embedder's
flat store and optimizer group, the forward is one autograd node (nn.apply_module) and its backward is ops.label_rows_bwd on the fp32
gradient that arrives -- each class's row the sum of its samples' gradients in batch order, rows of absent classes exactly zero, written in the
store's overwrite / accumulate mode.  ucg_rate stays with GeneralConditioner._drop_rows, as for every non-caption embedder.

`ClassEmbedderForMultiCond` (reference :35-44) is not built: the reference's own forward passes three arguments (batch, key,
disable_dropout) to ClassEmbedder.forward, which takes one, so it cannot run there either; there is no behaviour to mirror.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from ... import ops
from ...nn import apply_module
from .embedding import AbstractEmbModel


class ClassEmbedder(AbstractEmbModel):
    def __init__(self, embed_dim: int, n_classes: int = 1000, add_sequence_dim: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.embedding = nn.Embedding(n_classes, embed_dim)
        self.n_classes = n_classes
        self.add_sequence_dim = add_sequence_dim

    def trained_parameters(self) -> list:
        """What one step gives a gradient: the table.  The engine puts it in the embedder's flat store and optimizer group."""
        return [self.embedding.weight]

    def forward(self, c: Tensor) -> Tensor:
        """c: int64 class ids [B] -> fp32 [B, embed_dim] ([B, 1, embed_dim] with add_sequence_dim).  An id outside [0, n_classes) gives a NaN
        row (ops.label_rows).  Trainable under grad mode: connected to autograd, the backward writes embedding.weight.grad."""
        table = self.embedding.weight

        def run(ids):
            out = ops.label_rows(table, ids, out_dtype=torch.float32)

            def bwd(g: Tensor):
                ops.label_rows_bwd(ids, g.reshape(out.shape).to(torch.float32).contiguous(), table)
                return None

            return (out[:, None, :] if self.add_sequence_dim else out), bwd

        if self.is_trainable and table.requires_grad and torch.is_grad_enabled():
            return apply_module(run, [c], self)
        return run(c)[0]

    def get_unconditional_conditioning(self, bs: int, device="cuda") -> dict:
        """{input_key: int64 [bs]} naming the last class, the one a config reserves for "no label" """
        return {self.input_key: torch.full((bs,), self.n_classes - 1, dtype=torch.int64, device=device)}
