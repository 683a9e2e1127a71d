"""CLIP text towers as frozen embedders: `FrozenCLIPEmbedder` (OpenAI CLIP ViT-L/14 text model in the HuggingFace layout) and
`FrozenOpenCLIPEmbedder2` (OpenCLIP ViT-bigG/14 text model in the open_clip layout), with the constructor arguments, layer
selection and return conventions of `neurosis.models.text_encoder.clip` (:22-388).

The reference delegates the transformer itself to third-party code (transformers' CLIPTextModel, open_clip's CLIP); here both
towers are the pre-norm block of transformer.py (shared with the T5 towers) over the HIP kernels -- LayerNorm, QKV / out / MLP GEMMs
with fused bias and residual, the fused attention kernel with its causal flag (77 tokens: one key tile), GELU (`_clip_ops`).  Each
layer module describes itself to the block by a `Block` record (`.spec`); the HF layout's q / k / v projections run as ONE GEMM through
a `Packed` copy.  What is left here is what differs: parameter names, so that either checkpoint layout loads unchanged, the embedding
and the output selection (hidden-state taps, the final LayerNorm, the end-of-text gather, bigG's projection):

    HF        text_model.embeddings.{token,position}_embedding.weight, text_model.encoder.layers.N.{self_attn.{q,k,v,out}_proj,
              layer_norm1, layer_norm2, mlp.fc1, mlp.fc2}, text_model.final_layer_norm          (transformers 4.x naming;
              the un-prefixed 5.x names load too)
    open_clip token_embedding.weight, positional_embedding, transformer.resblocks.N.{ln_1, attn.in_proj_{weight,bias},
              attn.out_proj, ln_2, mlp.c_fc, mlp.c_proj}, ln_final, text_projection, logit_scale

Frozen towers (the SDXL configs) run their forward under no_grad, replayed from hipGraphs.  An embedder built with is_trainable=True
(configs/sdxl/sdxl-te.example.yaml) returns outputs that autograd connects, through nn.apply_module, to ONE closure chain per tower: the
embedding, every layer's transformer.block_train (LayerNorms, GEMMs, ops.attention_causal_fwd, ops.gelu_fwd), and for bigG's pooled
output ln_final, the end-of-text gather and text_projection -- all HIP kernels forward and backward.  Only the layers the selected
outputs depend on run; parameters they do not depend on get no gradient (trained_parameters(): what DiffusionEngine puts in the tower's
flat store and optimizer group).
Tokenisation needs the CLIP vocabulary files: they are looked up locally through transformers' CLIPTokenizer when text is
passed; token ids (LongTensor [B, 77]) are accepted directly.
"""
from __future__ import annotations

import logging
from typing import Optional, Sequence, Union

import numpy as np
import torch
from torch import Tensor, nn

from ... import ops
from ...graphs import frozen_stamp
from ...nn import apply_module
from ...modules.encoders.embedding import AbstractEmbModel
from .transformer import (Block, Packed, _chain_train, _check_ids, _decode_text, _forward_graphs, _graphable, _out_grads, _trainable, block_forward,
                          block_train, norm)

logger = logging.getLogger(__name__)
LN_EPS = 1e-5


def _clip_ops(B: int, heads: int, width: int, quick_gelu: bool, train: bool):
    """(attend, act) of a CLIP block (transformer.block_forward / block_train): causal attention and GELU, forward-only or with a backward"""
    if train:
        return (lambda q, k, v: ops.attention_causal_fwd(q, k, v, B, heads, width // heads)), (lambda u: ops.gelu_fwd(u, quick_gelu))
    return (lambda q, k, v: ops.attention_fwd(q, k, v, B, heads, width // heads, causal=True)[0]), (lambda u: ops.gelu(u, quick=quick_gelu))


def _embed(ids: Tensor, table: Tensor, positions: Tensor) -> Tensor:
    """token + position embeddings as bf16 tokens [B * L, width]"""
    if ids.dim() != 2 or ids.shape[1] > positions.shape[0]:
        raise ValueError(f"token ids must be [batch, <= {positions.shape[0]}], got {tuple(ids.shape)}")
    summed = table[ids] + positions[: ids.shape[1]]
    return ops.cast_bf16(summed.reshape(-1, summed.shape[-1]).float())


def _embed_train(ids: Tensor, table: Tensor, positions: Tensor):
    """_embed with its backward: (x, bwd(dx)), bwd writing table.grad / positions.grad (ops.embedding_bwd)"""
    x = _embed(ids, table, positions)

    def bwd(dx: Tensor) -> None:
        ops.embedding_bwd(ids.contiguous(), dx, table, positions)

    return x, bwd


def _final_train(x: Tensor, B: int, L: int, ln, eot: Tensor, want_tokens: bool, want_pooled: bool, projection: Optional[Tensor] = None,
                 projection_t: Optional[Tensor] = None):
    """ln(x), then its rows b * L + eot[b] (@ projection when given): (outputs, bwd(dtokens, dpooled) -> dx).  ONE LayerNorm serves both
    outputs, so its gamma / beta gradients have one producer.  projection_t is the bf16 [E, width] matrix the forward reads; the
    projection's own gradient [width, E] contracts over only B rows (ops.wgrad_few_rows)."""
    normed, b_ln = ops.layernorm_fwd(x, ln.weight, ln.bias, ln.eps)
    outs = [normed] if want_tokens else []
    sel = None
    if want_pooled:
        sel = normed[torch.arange(B, device=x.device) * L + eot].contiguous()
        outs.append(sel if projection is None else ops.gemm_nt(sel, projection_t))

    def bwd(dtokens: Optional[Tensor], dpooled: Optional[Tensor]) -> Tensor:
        d = None
        if dpooled is not None:
            if projection is not None:
                ops.wgrad_few_rows(sel, dpooled, ops.grad_flat(projection).view(projection.shape), ops.wgrad_mode(projection) == 1)
                dpooled = ops.gemm_nn(dpooled, projection_t)
            d = ops.gather_rows_bwd(dpooled, eot, L)
        if dtokens is not None:
            d = dtokens if d is None else ops.add(d, dtokens)
        return b_ln(d)

    return outs, bwd


# ---------------------------------------------------------------------------------------------------
# HuggingFace layout (CLIPTextModel)
# ---------------------------------------------------------------------------------------------------
class _HFAttention(nn.Module):
    def __init__(self, width: int):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(width, width) for _ in range(4))


class _HFMLP(nn.Module):
    def __init__(self, width: int, inner: int):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(width, inner), nn.Linear(inner, width)


class _HFLayer(nn.Module):
    def __init__(self, width: int, inner: int):
        super().__init__()
        self.self_attn = _HFAttention(width)
        self.layer_norm1 = nn.LayerNorm(width, eps=LN_EPS)
        self.mlp = _HFMLP(width, inner)
        self.layer_norm2 = nn.LayerNorm(width, eps=LN_EPS)
        a = self.self_attn
        self.__dict__["spec"] = Block(self.layer_norm1, Packed(a.q_proj, a.k_proj, a.v_proj), width, a.out_proj, self.layer_norm2,
                                      Packed(self.mlp.fc1), self.mlp.fc2)


class CLIPTextTower(nn.Module):
    """transformers' CLIPTextModel for the text side of openai/clip-vit-large-patch14 (defaults) -- same state_dict."""

    def __init__(self, vocab_size: int = 49408, hidden_size: int = 768, intermediate_size: int = 3072, num_hidden_layers: int = 12,
                 num_attention_heads: int = 12, max_position_embeddings: int = 77, hidden_act: str = "quick_gelu", eos_token_id: int = 2, **unused):
        super().__init__()
        if hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"hidden_act {hidden_act!r}: the CLIP text models use 'quick_gelu' or 'gelu'")
        self.heads, self.quick_gelu, self.eos_token_id = num_attention_heads, hidden_act == "quick_gelu", eos_token_id
        tm = self.text_model = nn.Module()
        tm.embeddings = nn.Module()
        tm.embeddings.token_embedding = nn.Embedding(vocab_size, hidden_size)
        tm.embeddings.position_embedding = nn.Embedding(max_position_embeddings, hidden_size)
        tm.encoder = nn.Module()
        tm.encoder.layers = nn.ModuleList(_HFLayer(hidden_size, intermediate_size) for _ in range(num_hidden_layers))
        tm.final_layer_norm = nn.LayerNorm(hidden_size, eps=LN_EPS)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # transformers 5.x dropped the "text_model." level from CLIPTextModel's parameter names
        inner = prefix + "text_model."
        if not any(k.startswith(inner) for k in state_dict):
            for key in [k for k in state_dict if k.startswith(prefix)]:
                state_dict[inner + key[len(prefix):]] = state_dict.pop(key)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @torch.no_grad()
    def forward(self, input_ids: Tensor, output_hidden_states: bool = False) -> dict:
        """{"last_hidden_state" [B, L, C], "pooler_output" [B, C], "hidden_states": tuple of L+1 [B, L, C] or None}, fp32;
        what CLIPTextModel returns (hidden_states[0] = embeddings, [i] = output of layer i, none of them final-normed)."""
        tm = self.text_model
        ids = _check_ids(input_ids, tm.embeddings.token_embedding.weight.device)
        if _graphable(self, ids):
            return _forward_graphs(self).run(lambda t: self._forward_ids(t, output_hidden_states), [ids], extra_key=(output_hidden_states, frozen_stamp(self)))
        return self._forward_ids(ids, output_hidden_states)

    def _forward_ids(self, ids: Tensor, output_hidden_states: bool) -> dict:
        tm = self.text_model
        B, L = ids.shape
        x = _embed(ids, tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight)
        states = [x] if output_hidden_states else None
        attend, act = _clip_ops(B, self.heads, x.shape[1], self.quick_gelu, train=False)
        for layer in tm.encoder.layers:
            x = block_forward(x, layer.spec, attend, act)
            if states is not None:
                states.append(x)
        last = norm(x, tm.final_layer_norm).float().reshape(B, L, -1)
        return {"last_hidden_state": last, "pooler_output": last[torch.arange(B, device=last.device), self._eos(ids)],
                "hidden_states": None if states is None else tuple(s.float().reshape(B, L, -1) for s in states)}

    def _eos(self, ids: Tensor) -> Tensor:
        """the pooled vector's position, the end of text: the highest id in the legacy vocabulary (eos_token_id == 2 configs), else the
        first occurrence of eos_token_id"""
        return ids.argmax(-1) if self.eos_token_id == 2 else (ids == self.eos_token_id).int().argmax(-1)

    def train_depth(self, state: Optional[int], want_last: bool, want_pooled: bool) -> int:
        """layers the training forward runs: all of them when the final-normed outputs are wanted, else up to hidden_states[state]"""
        return len(self.text_model.encoder.layers) if (want_last or want_pooled) else state

    def train_outputs(self, ids: Tensor, state: Optional[int], want_last: bool, want_pooled: bool) -> tuple:
        """The training forward, autograd-connected through nn.apply_module: fp32 (hidden_states[state] [B, L, C] if state is not None,
        last_hidden_state [B, L, C] if want_last, pooler_output [B, C] if want_pooled), with forward()'s values."""
        tm = self.text_model
        layers = list(tm.encoder.layers)[: self.train_depth(state, want_last, want_pooled)]
        final = want_last or want_pooled

        def run(ids):
            B, L = ids.shape
            emb = tm.embeddings
            x, b_emb = _embed_train(ids, emb.token_embedding.weight, emb.position_embedding.weight)
            attend, act = _clip_ops(B, self.heads, x.shape[1], self.quick_gelu, train=True)
            blocks = [lambda h, l=l: block_train(h, l.spec, attend, act) for l in layers]
            states, top, b_chain = _chain_train(x, blocks, set() if state is None else {state})
            outs = [] if state is None else [states[state].float().reshape(B, L, -1)]
            b_final = None
            if final:
                fo, b_final = _final_train(top, B, L, tm.final_layer_norm, self._eos(ids), want_last, want_pooled)
                outs += [fo[0].float().reshape(B, L, -1)] if want_last else []
                outs += [fo[-1].float()] if want_pooled else []

            def bwd(*gouts):
                g = _out_grads(gouts, len(outs))
                grads = {} if state is None else {state: g.pop(0)}
                dtop = b_final(g[0] if want_last else None, g[-1] if want_pooled else None) if final else None
                b_emb(b_chain(grads, dtop))
                return None

            return tuple(outs), bwd

        return apply_module(run, [ids], self)


# ---------------------------------------------------------------------------------------------------
# open_clip layout (the text half of open_clip.CLIP)
# ---------------------------------------------------------------------------------------------------
class _PackedAttention(nn.Module):
    """parameter names of nn.MultiheadAttention (what open_clip's ResidualAttentionBlock holds)"""

    def __init__(self, width: int):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * width, width))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * width))
        self.out_proj = nn.Linear(width, width)
        nn.init.normal_(self.in_proj_weight, std=width**-0.5)


class _OpenCLIPMLP(nn.Module):
    def __init__(self, width: int, inner: int):
        super().__init__()
        self.c_fc, self.c_proj = nn.Linear(width, inner), nn.Linear(inner, width)


class _ResBlock(nn.Module):
    def __init__(self, width: int, inner: int):
        super().__init__()
        self.ln_1 = nn.LayerNorm(width, eps=LN_EPS)
        self.attn = _PackedAttention(width)
        self.ln_2 = nn.LayerNorm(width, eps=LN_EPS)
        self.mlp = _OpenCLIPMLP(width, inner)
        a = self.attn
        self.__dict__["spec"] = Block(self.ln_1, Packed((a.in_proj_weight, a.in_proj_bias)), width, a.out_proj, self.ln_2, Packed(self.mlp.c_fc),
                                      self.mlp.c_proj)


class OpenCLIPTextTower(nn.Module):
    """The text tower of open_clip's CLIP (defaults: ViT-bigG-14 -- width 1280, 32 layers, 20 heads, projection to 1280)."""

    def __init__(self, vocab_size: int = 49408, width: int = 1280, layers: int = 32, heads: int = 20, context_length: int = 77, embed_dim: int = 1280,
                 mlp_ratio: float = 4.0, quick_gelu: bool = False):
        super().__init__()
        self.heads, self.quick_gelu, self.context_length = heads, quick_gelu, context_length
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width).normal_(std=0.01))
        self.transformer = nn.Module()
        self.transformer.resblocks = nn.ModuleList(_ResBlock(width, int(width * mlp_ratio)) for _ in range(layers))
        self.transformer.grad_checkpointing = False
        self.ln_final = nn.LayerNorm(width, eps=LN_EPS)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim).normal_(std=width**-0.5))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self._projection_cache = None

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "attn_mask", None)          # a buffer in open_clip; the causal mask is a kernel flag here
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def _projection_t(self) -> Tensor:
        """text_projection^T as the [embed_dim, width] bf16 matrix gemm_nt reads"""
        cached, stamp = self._projection_cache, ops._param_stamp(self.text_projection)
        if cached is None or cached[0] != stamp:
            cached = self._projection_cache = (stamp, ops.cast_bf16(self.text_projection.detach().t().contiguous().float()))
        return cached[1]

    @torch.no_grad()
    def forward(self, text: Tensor) -> dict:
        """{"last", "penultimate": [B, L, width] (neither final-normed), "pooled": [B, embed_dim]}, fp32 -- the dictionary the
        reference's encode_with_transformer builds (models/text_encoder/clip.py:311-343)."""
        ids = _check_ids(text, self.token_embedding.weight.device)
        if _graphable(self, ids):
            return _forward_graphs(self).run(self._forward_ids, [ids], extra_key=(frozen_stamp(self),))
        return self._forward_ids(ids)

    def _forward_ids(self, ids: Tensor) -> dict:
        B, L = ids.shape
        x = _embed(ids, self.token_embedding.weight, self.positional_embedding)
        width = x.shape[1]
        penultimate = x
        attend, act = _clip_ops(B, self.heads, width, self.quick_gelu, train=False)
        for block in self.transformer.resblocks:
            penultimate = x
            x = block_forward(x, block.spec, attend, act)
        normed = norm(x, self.ln_final).reshape(B, L, width)
        eot = normed[torch.arange(B, device=ids.device), ids.argmax(dim=-1)].contiguous()       # highest id = end of text
        pooled = ops.gemm_nt(eot, self._projection_t())
        return {"last": x.float().reshape(B, L, width), "penultimate": penultimate.float().reshape(B, L, width), "pooled": pooled.float()}

    def train_depth(self, want_last: bool, want_pooled: bool) -> int:
        """blocks the training forward runs: all of them for "last" / "pooled", all but the last for "penultimate" alone"""
        n = len(self.transformer.resblocks)
        return n if (want_last or want_pooled) else n - 1

    def train_outputs(self, ids: Tensor, want_penultimate: bool, want_last: bool, want_pooled: bool) -> tuple:
        """The training forward, autograd-connected through nn.apply_module: fp32 (penultimate, last [B, L, width], pooled [B, embed_dim]),
        each only when asked for, with forward()'s values."""
        n = len(self.transformer.resblocks)
        depth = self.train_depth(want_last, want_pooled)
        blocks_ = list(self.transformer.resblocks)[:depth]
        taps = ({n - 1} if want_penultimate else set()) | ({n} if want_last else set())

        def run(ids):
            B, L = ids.shape
            x, b_emb = _embed_train(ids, self.token_embedding.weight, self.positional_embedding)
            width = x.shape[1]
            attend, act = _clip_ops(B, self.heads, width, self.quick_gelu, train=True)
            states, top, b_chain = _chain_train(x, [lambda h, blk=blk: block_train(h, blk.spec, attend, act) for blk in blocks_], taps)
            outs = [states[i].float().reshape(B, L, width) for i in sorted(taps)]
            b_final = None
            if want_pooled:
                fo, b_final = _final_train(top, B, L, self.ln_final, ids.argmax(dim=-1), False, True, self.text_projection, self._projection_t())
                outs.append(fo[0].float())

            def bwd(*gouts):
                g = _out_grads(gouts, len(outs))
                grads = {i: g[j] for j, i in enumerate(sorted(taps))}
                dtop = b_final(None, g[-1]) if want_pooled else None
                b_emb(b_chain(grads, dtop))
                return None

            return tuple(outs), bwd

        return apply_module(run, [ids], self)


# ---------------------------------------------------------------------------------------------------
# embedders
# ---------------------------------------------------------------------------------------------------
class _TokenizingEmbedder(AbstractEmbModel):
    """tokenisation shared by both embedders (reference :156-202 and :348-388 are the same code twice)"""

    tokenizer = None
    max_length = 77
    extended_chunks = 0

    def _load_tokenizer(self, repo: str) -> None:
        try:
            from transformers import CLIPTokenizer

            self.tokenizer = CLIPTokenizer.from_pretrained(repo, local_files_only=True)
        except Exception as err:   # no vocabulary on this machine: token ids can still be passed to forward()
            logger.warning("CLIP tokenizer %s is not available locally (%s); pass token ids instead of text", repo, type(err).__name__)
            self.tokenizer = None

    def _tokenizer_or_raise(self):
        if self.tokenizer is None:
            raise RuntimeError("this embedder has no tokenizer (CLIP vocabulary files not found locally): pass LongTensor token ids [B, 77]")
        return self.tokenizer

    def tokenize(self, text: Sequence[str]) -> dict:
        enc = self._tokenizer_or_raise()(text, truncation=True, max_length=self.max_length, return_length=True, return_overflowing_tokens=False,
                                         padding="max_length", return_tensors="pt")
        return {"input_ids": enc["input_ids"].to(self.device)}

    def tokenize_extended(self, text: Sequence[str]) -> dict:
        """[B, chunks, 77]: the prompt is cut into `extended_chunks` pieces of 75 tokens, each wrapped in BOS / EOS"""
        tok = self._tokenizer_or_raise()
        body = tok.model_max_length - 2
        ids = tok(text, truncation=True, add_special_tokens=False, max_length=self.extended_chunks * body, padding="max_length",
                  return_tensors="pt")["input_ids"].to(self.device)
        ids = ids.view(len(text), self.extended_chunks, body)
        edge = ids.new_ones(ids.shape[:2] + (1,))
        return {"input_ids": torch.cat((edge * tok.bos_token_id, ids, edge * tok.eos_token_id), dim=2)}

    def _ids_for(self, text) -> Tensor:
        """token ids for forward(): [B, 77], or [B, chunks, 77] in extended mode; tensors pass through"""
        if torch.is_tensor(text):
            return text.to(self.device)
        text = _decode_text(text)
        if self.ucg_rate > 0.0 and self.ucg_rate < np.random.rand():       # (the reference's comparison, kept as is)
            text = [""] * len(text)
        return (self.tokenize_extended(text) if self.extended_chunks > 1 else self.tokenize(text))["input_ids"]

    def encode(self, text):
        return self(text)


class FrozenCLIPEmbedder(_TokenizingEmbedder):
    """reference :22-202.  `config` (a dict of CLIPTextTower arguments) replaces the hub lookup of `version`'s config when given."""

    LAYERS = ["last", "pooled", "hidden", "penultimate"]

    def __init__(self, version: str = "openai/clip-vit-large-patch14", device="cuda", max_length: int = 77, freeze: bool = True, layer: str = "last",
                 layer_idx: Optional[int] = None, always_return_pooled: bool = False, extended_chunks: int = 0, load_pretrained: bool = False,
                 config: Optional[dict] = None, **kwargs):
        super().__init__(**kwargs)
        if layer not in self.LAYERS:
            raise ValueError(f"layer must be one of {self.LAYERS}, got {layer=}")
        if load_pretrained:
            raise NotImplementedError("load_pretrained: there is no hub access here; load a state_dict into .transformer instead")
        self.transformer = CLIPTextTower(**(config or {}))
        self._load_tokenizer(version)
        self.device, self.max_length = torch.device(device), max_length
        self.layer, self.return_pooled, self.extended_chunks = layer, always_return_pooled, extended_chunks
        self.output_hidden_states = layer in ("hidden", "penultimate")
        depth = len(self.transformer.text_model.encoder.layers)
        if layer == "hidden":
            if layer_idx is None:
                raise ValueError("layer_idx must be specified for hidden layer")
            if not (0 <= abs(layer_idx) <= depth):
                raise ValueError(f"layer_idx must be between -{depth} and {depth}")
            self.layer_idx = layer_idx + depth if layer_idx < 0 else layer_idx
        elif layer == "penultimate":
            self.layer_idx = depth - 2
        else:
            # the reference raises here for "last" and "pooled" (its match statement has no such arms) although its forward
            # handles both; they are accepted
            self.layer_idx = None
        if self.is_trainable and extended_chunks > 1:
            raise NotImplementedError("a trainable FrozenCLIPEmbedder does not support extended_chunks > 1 (its training chain takes [B, 77] token ids)")
        if not self.is_trainable:
            self.freeze()

    def _train_spec(self):
        """(hidden state index or None, want last_hidden_state, want pooler_output) of the training forward"""
        state = None if self.layer in ("last", "pooled") else self.layer_idx + 1
        return state, self.layer == "last", self.layer == "pooled" or self.return_pooled

    def trained_parameters(self) -> list:
        """The parameters the selected outputs depend on, in registration order: what one step gives a gradient (and what the optimizer
        group holds).  Layers past the selected one and final_layer_norm under layer = "hidden" are not among them."""
        state, want_last, want_pooled = self._train_spec()
        tm = self.transformer.text_model
        used = [tm.embeddings, *list(tm.encoder.layers)[: self.transformer.train_depth(state, want_last, want_pooled)]]
        if want_last or want_pooled:
            used.append(tm.final_layer_norm)
        ids = {id(p) for m in used for p in m.parameters()}
        return [p for p in self.parameters() if id(p) in ids]

    def _forward_trainable(self, text):
        ids = _check_ids(self._ids_for(text), self.transformer.text_model.embeddings.token_embedding.weight.device)
        state, want_last, want_pooled = self._train_spec()
        outs = list(self.transformer.train_outputs(ids, state, want_last, want_pooled))
        pooled = outs[-1] if want_pooled else None
        z = pooled[:, None, :] if self.layer == "pooled" else outs[0]
        return (z, pooled) if self.return_pooled else z

    def _select(self, out: dict) -> Tensor:
        if self.layer == "last":
            return out["last_hidden_state"]
        if self.layer == "pooled":
            return out["pooler_output"][:, None, :]
        return out["hidden_states"][self.layer_idx + 1]

    def forward(self, text: Union[str, list, Tensor]):
        if _trainable(self, self.transformer):
            return self._forward_trainable(text)
        return self._forward_frozen(text)

    @torch.no_grad()
    def _forward_frozen(self, text: Union[str, list, Tensor]):
        ids = self._ids_for(text)
        if ids.dim() == 2:
            out = self.transformer(ids, output_hidden_states=self.output_hidden_states)
            z = self._select(out)
            return (z, out["pooler_output"]) if self.return_pooled else z
        # extended mode: each prompt's chunks run as one mini-batch and are laid end to end along the token axis
        per_prompt, pooled = [], []
        for chunks in ids:
            out = self.transformer(chunks, output_hidden_states=self.output_hidden_states)
            per_prompt.append(self._select(out).reshape(-1, out["last_hidden_state"].shape[-1]))
            pooled.append(out["pooler_output"][0])
        z = torch.stack(per_prompt, dim=0)
        return (z, pooled) if self.return_pooled else z


OPENCLIP_TOKENIZERS = {"default": "laion/CLIP-ViT-bigG-14-laion2B-39B-b160k", "ViT-bigG-14": "laion/CLIP-ViT-bigG-14-laion2B-39B-b160k"}
OPENCLIP_ARCHS = {"ViT-bigG-14": dict(width=1280, layers=32, heads=20, embed_dim=1280), "ViT-H-14": dict(width=1024, layers=24, heads=16, embed_dim=1024)}


class FrozenOpenCLIPEmbedder2(_TokenizingEmbedder):
    """reference :205-388.  `arch` selects the text tower's shape from OPENCLIP_ARCHS, or pass `config` (OpenCLIPTextTower arguments)."""

    LAYERS = ["pooled", "last", "penultimate"]

    def __init__(self, arch: str = "ViT-bigG-14", version: Optional[str] = "laion2b_s39b_b160k", device="cuda", max_length: int = 77, layer: str = "last",
                 always_return_pooled: bool = False, legacy: bool = False, extended_chunks: int = 0, config: Optional[dict] = None, freeze: bool = True, **kwargs):
        super().__init__(**kwargs)
        if layer not in self.LAYERS:
            raise ValueError(f"layer must be one of {self.LAYERS}, got {layer=}")
        if always_return_pooled and legacy:
            raise ValueError("legacy mode does not support returning pooled embeddings!")
        if extended_chunks > 1 and legacy:
            raise ValueError("legacy mode does not support extended chunks!")
        if config is None and arch not in OPENCLIP_ARCHS:
            raise ValueError(f"unknown arch {arch!r}: pass config= or one of {sorted(OPENCLIP_ARCHS)}")
        self.model = OpenCLIPTextTower(**(config if config is not None else OPENCLIP_ARCHS[arch]))
        repo = OPENCLIP_TOKENIZERS.get(arch)
        if repo is None:
            logger.warning(f"Could not find tokenizer for {arch=} and {version=}, using default")
            repo = OPENCLIP_TOKENIZERS["default"]
        self._load_tokenizer(repo)
        self.device, self.max_length = torch.device(device), max_length
        self.layer, self.return_pooled, self.legacy, self.extended_chunks = layer, always_return_pooled, legacy, extended_chunks
        self.embed_dim = self.model.text_projection.shape[-1]
        if self.is_trainable and (legacy or extended_chunks > 1):
            raise NotImplementedError("a trainable FrozenOpenCLIPEmbedder2 supports neither legacy=True nor extended_chunks > 1")
        if not self.is_trainable:
            self.freeze()

    def _train_spec(self):
        """(want penultimate, want last, want pooled) of the training forward"""
        return self.layer == "penultimate", self.layer == "last", self.layer == "pooled" or self.return_pooled

    def trained_parameters(self) -> list:
        """The parameters the selected outputs depend on, in registration order (logit_scale never is; ln_final and text_projection only
        with the pooled output; the last block not for "penultimate" alone)."""
        _, want_last, want_pooled = self._train_spec()
        m = self.model
        used = [m.token_embedding, *list(m.transformer.resblocks)[: m.train_depth(want_last, want_pooled)]]
        ids = {id(p) for mod in used for p in mod.parameters()} | {id(m.positional_embedding)}
        if want_pooled:
            ids |= {id(p) for p in m.ln_final.parameters()} | {id(m.text_projection)}
        return [p for p in self.parameters() if id(p) in ids]

    def _forward_trainable(self, text):
        ids = _check_ids(self._ids_for(text), self.model.token_embedding.weight.device)
        want = self._train_spec()
        outs = dict(zip([k for k, w in zip(("penultimate", "last", "pooled"), want) if w], self.model.train_outputs(ids, *want)))
        return (outs[self.layer], outs["pooled"]) if self.return_pooled else outs[self.layer]

    def encode_with_transformer(self, text: Tensor):
        out = self.model(text)
        if not self.legacy:
            return out
        # legacy: the chosen layer's tokens through ln_final, nothing else
        chosen = out[self.layer]
        B, L, width = chosen.shape
        return norm(ops.cast_bf16(chosen.reshape(B * L, width)), self.model.ln_final).float().reshape(B, L, width)

    def forward(self, text: Union[str, list, Tensor]):
        if _trainable(self, self.model):
            return self._forward_trainable(text)
        return self._forward_frozen(text)

    @torch.no_grad()
    def _forward_frozen(self, text: Union[str, list, Tensor]):
        ids = self._ids_for(text)
        if ids.dim() == 2:
            out = self.encode_with_transformer(ids)
            if self.legacy:
                return out
            return (out[self.layer], out["pooled"]) if self.return_pooled else out[self.layer]
        per_prompt, pooled = [], []
        for chunks in ids:
            out = self.encode_with_transformer(chunks)
            per_prompt.append(out[self.layer].reshape(-1, out[self.layer].shape[-1]))
            pooled.append(out["pooled"][0:1])
        z = torch.stack(per_prompt, dim=0)
        return (z, torch.cat(pooled, dim=0)) if self.return_pooled else z
