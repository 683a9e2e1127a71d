"""What the text towers (clip.py: CLIP-L in the HuggingFace layout, OpenCLIP bigG; t5.py: T5 / ByT5) share: ONE pre-norm transformer
block over the HIP kernels, once frozen (`block_forward`: x -> x', keeps nothing) and once trained (`block_train`: x -> (x', bwd)), and the
helpers of their forward and training chains.  A tower describes each of its layers by a `Block` record and hands the block its attention
and activation as callables; what is left in the tower files is parameter naming, the embedding and the output selection.

    norm 1        nn.LayerNorm (ops.layernorm_fwd) or T5LayerNorm (ops.rmsnorm / ops.rmsnorm_fwd)
    q | k | v     ONE GEMM through a `Packed` projection; heads * d_kv (`Block.inner`) need not be the model width
    attention     CLIP: ops.attention_fwd(causal=True) / ops.attention_causal_fwd; T5: ops.attention_relbias_fwd / _train
    out           nn.Linear, residual fused in the GEMM
    norm 2, input projection (`Packed`: T5's gated variants stack [wi_0; wi_1]), activation (ops.gelu / gelu_fwd, ops.gated_act /
    gated_act_fwd), output projection with the residual

`Packed` is the one place where several fp32 parameters become one bf16 matrix that is rebuilt when one of them changes.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Union

import numpy as np
import torch
from torch import Tensor, nn

from ... import ops
from ...graphs import ForwardGraphs, graphs_enabled
from ...nn import as_tokens


class T5LayerNorm(nn.Module):
    def __init__(self, width: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(width))
        self.variance_epsilon = eps

    def forward(self, x: Tensor) -> Tensor:
        return ops.rmsnorm(x, self.weight, self.variance_epsilon)


def norm(x: Tensor, layer: Union[nn.LayerNorm, T5LayerNorm]) -> Tensor:
    if isinstance(layer, nn.LayerNorm):
        return ops.layernorm_fwd(x, layer.weight, layer.bias, layer.eps)[0]
    return layer(x)


def norm_train(x: Tensor, layer: Union[nn.LayerNorm, T5LayerNorm]):
    """(y, bwd(dy, dx_add=None) -> dx), the norm's weight (and bias) gradient written by bwd"""
    if isinstance(layer, nn.LayerNorm):
        return ops.layernorm_fwd(x, layer.weight, layer.bias, layer.eps)
    return ops.rmsnorm_fwd(x, layer.weight, layer.variance_epsilon)


def linear(x: Tensor, layer: nn.Linear, residual: Optional[Tensor] = None) -> Tensor:
    return ops.gemm_nt(x, ops.w2d(layer.weight), layer.bias, residual=residual)


class Packed:
    """One or more projections stacked by rows -- each an nn.Linear or a bare (weight, bias) parameter pair, all with a bias or none -- as the
    ONE bf16 matrix [sum n_i, K] and fp32 bias a single GEMM reads: 24 launches fewer per CLIP-L forward than three GEMMs per layer.

    A single projection is read through its own shadow (ops.w2d) and trained through ops.linear_fwd, as any nn.Linear.  Several are packed
    into a copy that is rebuilt only when ops._param_stamp of one of the tensors changes, and whose address is stable until then (captured
    graphs hold it).  Its bits are f2bf(master) either way: parameters of a FlatParamStore are packed from the store's shadows, which the
    fused optimizers rewrite with the masters; all others by one cast of the stacked fp32 matrices, so that a frozen tower keeps ONE bf16
    copy of them and no shadow per matrix.

    Not an nn.Module: the owner keeps it in its __dict__, so that no state_dict gains a key."""

    def __init__(self, *parts):
        self.parts, self.stamp, self.weight, self.bias = parts, None, None, None
        if len({b is None for _, b in self.pairs()}) != 1:
            raise ValueError("Packed: either every stacked projection has a bias or none")

    def pairs(self) -> list:
        return [(p.weight, p.bias) if isinstance(p, nn.Module) else tuple(p) for p in self.parts]

    def matrices(self) -> tuple:
        """(bf16 [sum n_i, K], fp32 [sum n_i] or None): the operands of ops.gemm_nt"""
        pairs = self.pairs()
        if len(pairs) == 1:
            return ops.w2d(pairs[0][0]), pairs[0][1]
        stamp = tuple(ops._param_stamp(t) for pair in pairs for t in pair if t is not None)
        if self.stamp != stamp:
            if all(getattr(w, "_nk_store", None) is not None for w, _ in pairs):
                self.weight = torch.cat([ops.w2d(w) for w, _ in pairs], dim=0)
            else:
                self.weight = ops.cast_bf16(torch.cat([w.detach().float() for w, _ in pairs], dim=0))
            self.bias = None if pairs[0][1] is None else torch.cat([b.detach().float() for _, b in pairs])
            self.stamp = stamp
        return self.weight, self.bias

    def forward(self, h: Tensor) -> Tensor:
        return ops.gemm_nt(h, *self.matrices())

    def train(self, h: Tensor):
        """(y [M, sum n_i], bwd(dy) -> dh): the forward's GEMM (so its bits), the input gradient through the same packed matrix, and every
        projection's weight and bias gradient from its column slice of dy, written to its .grad in the parameter's engine mode"""
        pairs = self.pairs()
        if len(pairs) == 1:
            return ops.linear_fwd(h, *pairs[0])
        weight, bias = self.matrices()
        y = ops.gemm_nt(h, weight, bias)

        def bwd(dy: Tensor) -> Tensor:
            def wgrads():
                off = 0
                for w, b in pairs:
                    n = w.shape[0]
                    ops.gemm_tn_f32(dy[:, off:off + n], h, ops.g2d(w), ops.wgrad_mode(w), dbias=None if b is None else ops.grad_flat(b))
                    off += n

            ops.on_wgrad_stream(wgrads, dy, h, owner=pairs[0][0])
            return ops.gemm_nn(dy, weight)

        return y, bwd


class Block(NamedTuple):
    """the parameters of one pre-norm block; `inner` = heads * per-head width, the column width of each of q, k and v"""
    norm1: nn.Module
    qkv: Packed
    inner: int
    out: nn.Linear
    norm2: nn.Module
    fc_in: Packed
    fc_out: nn.Linear


def block_forward(x: Tensor, p: Block, attend: Callable, act: Callable) -> Tensor:
    """x + out(attend(q, k, v of norm1 x)), then x + fc_out(act(fc_in(norm2 x))), on a dense bf16 token matrix [batch * L, width], frozen:
    attend(q, k, v) -> attended and act(u) -> hidden are the forward-only ops; q, k, v are column slices of the packed projection."""
    w = p.inner
    fused = p.qkv.forward(norm(x, p.norm1))
    x = linear(attend(fused[:, :w], fused[:, w:2 * w], fused[:, 2 * w:]), p.out, residual=x)
    return linear(act(p.fc_in.forward(norm(x, p.norm2))), p.fc_out, residual=x)


def block_train(x: Tensor, p: Block, attend: Callable, act: Callable):
    """block_forward with its backward: (x', bwd(dx') -> dx).  attend(q, k, v) -> (attended, bwd(do, dq=, dk=, dv=)) and act(u) -> (hidden,
    bwd(dhidden) -> du) are the ops with a backward.  Parameter gradients go to .grad in their engine's mode (the closures of
    ops.linear_fwd and of the norms, Packed.train's own)."""
    w = p.inner
    h1, b_norm1 = norm_train(x, p.norm1)
    fused, b_qkv = p.qkv.train(h1)
    attended, b_att = attend(fused[:, :w], fused[:, w:2 * w], fused[:, 2 * w:])
    x1, b_out = ops.linear_fwd(attended, p.out.weight, p.out.bias, residual=x)
    h2, b_norm2 = norm_train(x1, p.norm2)
    u, b_in = p.fc_in.train(h2)
    hidden, b_act = act(u)
    x2, b_fc = ops.linear_fwd(hidden, p.fc_out.weight, p.fc_out.bias, residual=x1)

    def bwd(dx2: Tensor) -> Tensor:
        dx1 = b_norm2(b_in(b_act(b_fc(dx2))), dx_add=dx2)
        dfused = torch.empty_like(fused)
        b_att(b_out(dx1), dq=dfused[:, :w], dk=dfused[:, w:2 * w], dv=dfused[:, 2 * w:])
        return b_norm1(b_qkv(dfused), dx_add=dx1)

    return x2, bwd


# ---------------------------------------------------------------------------------------------------
# the forward and training chains
# ---------------------------------------------------------------------------------------------------
def embed_tokens(ids: Tensor, table: Tensor) -> Tensor:
    """the table's rows for ids [B, L] as bf16 tokens [B * L, width]"""
    return ops.cast_bf16(table[ids].reshape(-1, table.shape[1]).float())


def _chain_train(x: Tensor, blocks, taps):
    """Run `blocks` (callables x -> (x', bwd)) from the embedding output x; returns ({i: state i for i in taps}, last state, bwd(grads, dtop)),
    state i being the input of block i (state len(blocks) the last output).  bwd adds each tap's gradient where its state enters, walks the
    blocks backwards and returns the gradient of x."""
    states, closures = {0: x} if 0 in taps else {}, []
    for i, block in enumerate(blocks):
        x, b = block(x)
        closures.append(b)
        if i + 1 in taps:
            states[i + 1] = x

    def bwd(grads: dict, dtop: Optional[Tensor]) -> Tensor:
        d = dtop
        for i in range(len(closures), -1, -1):
            g = grads.get(i)
            if g is not None:
                d = g if d is None else ops.add(d, g)
            if i > 0:
                d = closures[i - 1](d)
        return d

    return states, x, bwd


def _trainable(embedder, tower: nn.Module) -> bool:
    """the embedder's forward runs the autograd-connected training chain"""
    return embedder.is_trainable and torch.is_grad_enabled() and any(p.requires_grad for p in tower.parameters())


def _out_grads(gouts, n: int):
    """the first n incoming gradients as dense bf16 token matrices (None where autograd passed none)"""
    return [None if g is None else as_tokens(g.contiguous()) for g in gouts[:n]]


def _graphable(tower: nn.Module, ids: Tensor) -> bool:
    """A frozen tower on the GPU runs its ~250-450 dependent small launches from a hipGraph (neurosis_amd/graphs.py): they are
    launch-latency, not work (4-5 ms of the SDXL step for both towers)."""
    return ids.is_cuda and graphs_enabled("te") and not any(p.requires_grad for p in tower.parameters())


def _forward_graphs(tower: nn.Module) -> ForwardGraphs:
    fg = tower.__dict__.get("_nk_fgraphs")
    if fg is None:
        fg = tower.__dict__["_nk_fgraphs"] = ForwardGraphs(next(tower.parameters()).device)
    return fg


def _check_ids(ids: Tensor, device) -> Tensor:
    if ids.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"token ids must be an integer tensor, got {ids.dtype}")
    return ids.to(device=device, dtype=torch.int64)


def _decode_text(text) -> list:
    if isinstance(text, (str, bytes, np.bytes_)):
        text = [text]
    return [t.decode("utf-8") if isinstance(t, (bytes, np.bytes_)) else t for t in text]
