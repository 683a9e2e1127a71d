"""T5 / ByT5 encoders as frozen embedders: `FrozenT5Embedder` and `FrozenByT5Embedder`, with the constructor arguments and return
conventions of `neurosis.models.text_encoder.t5` (:14-101), over `T5EncoderTower`, the encoder half of transformers' T5 (T5EncoderModel)
on the HIP kernels.

The reference delegates the transformer to transformers' T5EncoderModel and calls it with `input_ids` only (:38-53), so there is no padding
mask: every position attends to every position.  The block itself is transformer.py's, shared with the CLIP towers (each `_Block`
describes itself by a `Block` record, `.spec`); this file holds T5's parameter names, `rel_table` and the embedders.  What T5 hands
the block that the CLIP towers do not:

    T5LayerNorm           ops.rmsnorm: x * rsqrt(mean(x^2) + eps) * weight, no mean subtraction, no bias
    self-attention        ops.attention_relbias_fwd: softmax(q k^T + bias) v -- NO 1/sqrt(d) scaling, bidirectional, with block 0's
                          relative position bias shared by every layer.  The bias depends only on (key - query) position, so it is
                          handed to the kernel as one fp32 row of 2 L - 1 entries per head (`T5EncoderTower.rel_table`)
    FeedForward           T5 v1.1 / ByT5 "gated-gelu": wo(gelu_new(wi_0 x) * wi_1 x), [wi_0; wi_1] as ONE `Packed` projection + ops.gated_act;
                          T5 v1.0 "relu": wo(relu(wi x))

Projections carry no bias; num_heads * d_kv need not equal d_model (t5-v1.1-small, ByT5).  The state_dict is T5EncoderModel's:

    shared.weight, encoder.embed_tokens.weight (tied), encoder.block.N.layer.0.{SelfAttention.{q,k,v,o}.weight, layer_norm.weight},
    encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight, encoder.block.N.layer.1.{DenseReluDense.{wi_0,wi_1,wo}.weight
    (or wi), layer_norm.weight}, encoder.final_layer_norm.weight

Frozen (the default), the forward runs under no_grad (replayed from hipGraphs under NK_GRAPH "te", as the frozen CLIP towers).  A frozen
tower keeps its fp32 parameters plus one bf16 copy of every matrix the kernels read (6 bytes per parameter: ~28 GB at T5-v1.1-XXL's 4.7 B
encoder parameters).

Trained with the UNet (`is_trainable: true` and `freeze: false` in the conditioner config, the reference's condition), the embedder's forward
runs `T5EncoderTower.train_outputs`: the same kernels and the same bits as the frozen forward, autograd-connected through nn.apply_module to
one closure chain -- per block transformer.block_train (rmsnorm_fwd, the packed q / k / v projection, attention_relbias_train, the o
projection with residual, rmsnorm_fwd, the packed wi projection, gated_act_fwd, wo with residual); then the final rmsnorm.  Every layer's backward adds its gradient
of the bias table into ONE d_rel [heads, 2 L - 1]; after block 0's backward ops.relbias_bucket_sum folds it into
relative_attention_bias.weight's gradient, once, and ops.embedding_bwd writes the (tied) embedding's.  DiffusionEngine gives the tower a
FlatParamStore and an optimizer group of its own, as it does for the CLIP towers.
"""
from __future__ import annotations

import json
import logging
import math
from pathlib import Path
from typing import Optional, Union

import torch
from torch import Tensor, nn

from ... import ops
from ...graphs import frozen_stamp
from ...modules.encoders.embedding import AbstractEmbModel
from ...nn import apply_module
from .transformer import (Block, Packed, T5LayerNorm, _chain_train, _check_ids, _decode_text, _forward_graphs, _graphable, _out_grads, _trainable,
                          block_forward, block_train, embed_tokens, norm_train)

logger = logging.getLogger(__name__)

T5_MAX_TOKENS = ops.ATTN_RELBIAS_MAX_L
FEED_FORWARD_PROJS = ("relu", "gelu_new", "gated-gelu")
CONFIG_KEYS = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets", "relative_attention_max_distance",
               "feed_forward_proj", "layer_norm_epsilon")


def relative_buckets(length: int, num_buckets: int, max_distance: int) -> Tensor:
    """Bucket of every relative position key - query in [-(length - 1), length - 1] (int64 [2 length - 1], index = key - query + length - 1),
    T5's bidirectional map: half of the buckets per sign (keys behind the query take the lower half), distances below num_buckets / 4 one
    bucket each, the rest spread logarithmically up to max_distance, everything beyond in the sign's last bucket.  The logarithm is taken
    in fp32 as transformers does, so the edges fall where a checkpoint was trained with them."""
    rel = torch.arange(-(length - 1), length, dtype=torch.int64)
    half = num_buckets // 2
    exact = half // 2
    dist = rel.abs()
    spread = exact + (torch.log(dist.float() / exact) / math.log(max_distance / exact) * (half - exact)).to(torch.int64)
    spread = spread.clamp(max=half - 1)
    return (rel > 0).to(torch.int64) * half + torch.where(dist < exact, dist, spread)


class _SelfAttention(nn.Module):
    def __init__(self, d_model: int, heads: int, d_kv: int, num_buckets: Optional[int]):
        super().__init__()
        inner = heads * d_kv
        self.q, self.k, self.v = (nn.Linear(d_model, inner, bias=False) for _ in range(3))
        self.o = nn.Linear(inner, d_model, bias=False)
        if num_buckets is not None:
            self.relative_attention_bias = nn.Embedding(num_buckets, heads)


class _Dense(nn.Module):
    def __init__(self, d_model: int, d_ff: int, gated: bool):
        super().__init__()
        if gated:
            self.wi_0, self.wi_1 = nn.Linear(d_model, d_ff, bias=False), nn.Linear(d_model, d_ff, bias=False)
        else:
            self.wi = nn.Linear(d_model, d_ff, bias=False)
        self.wo = nn.Linear(d_ff, d_model, bias=False)


class _AttentionLayer(nn.Module):
    def __init__(self, d_model: int, heads: int, d_kv: int, num_buckets: Optional[int], eps: float):
        super().__init__()
        self.SelfAttention = _SelfAttention(d_model, heads, d_kv, num_buckets)
        self.layer_norm = T5LayerNorm(d_model, eps)


class _DenseLayer(nn.Module):
    def __init__(self, d_model: int, d_ff: int, gated: bool, eps: float):
        super().__init__()
        self.DenseReluDense = _Dense(d_model, d_ff, gated)
        self.layer_norm = T5LayerNorm(d_model, eps)


class _Block(nn.Module):
    def __init__(self, d_model: int, heads: int, d_kv: int, d_ff: int, gated: bool, num_buckets: Optional[int], eps: float):
        super().__init__()
        self.layer = nn.ModuleList([_AttentionLayer(d_model, heads, d_kv, num_buckets, eps), _DenseLayer(d_model, d_ff, gated, eps)])
        att, ff = self.layer
        sa, dense = att.SelfAttention, ff.DenseReluDense
        wi = (dense.wi_0, dense.wi_1) if gated else (dense.wi,)       # [wi_0; wi_1] as ONE stacked projection
        self.__dict__["spec"] = Block(att.layer_norm, Packed(sa.q, sa.k, sa.v), heads * d_kv, sa.o, ff.layer_norm, Packed(*wi), dense.wo)


class T5EncoderTower(nn.Module):
    """transformers' T5EncoderModel (same state_dict) from its config's entries; the defaults are google/t5-v1_1-xl's encoder."""

    def __init__(self, vocab_size: int = 32128, d_model: int = 2048, d_kv: int = 64, d_ff: int = 5120, num_layers: int = 24, num_heads: int = 32,
                 relative_attention_num_buckets: int = 32, relative_attention_max_distance: int = 128, feed_forward_proj: str = "gated-gelu",
                 layer_norm_epsilon: float = 1e-6, **unused):
        super().__init__()
        if feed_forward_proj not in FEED_FORWARD_PROJS:
            raise ValueError(f"feed_forward_proj {feed_forward_proj!r}: the T5 encoders built here use one of {FEED_FORWARD_PROJS}")
        if d_model % 8 or d_kv % 8 or d_ff % 8 or d_kv > 160 or d_model > 4096:
            raise ValueError(f"T5EncoderTower: d_model, d_kv and d_ff must be multiples of 8, d_kv <= 160 and d_model <= 4096 (the kernels' limits), "
                             f"got {d_model=} {d_kv=} {d_ff=}")
        self.heads, self.d_kv, self.act = num_heads, d_kv, feed_forward_proj
        self.num_buckets, self.max_distance = relative_attention_num_buckets, relative_attention_max_distance
        gated = feed_forward_proj.startswith("gated-")
        self.shared = nn.Embedding(vocab_size, d_model)
        self.encoder = nn.Module()
        self.encoder.embed_tokens = self.shared      # tied: one parameter under both names
        self.encoder.block = nn.ModuleList(_Block(d_model, num_heads, d_kv, d_ff, gated, relative_attention_num_buckets if i == 0 else None, layer_norm_epsilon)
                                           for i in range(num_layers))
        self.encoder.final_layer_norm = T5LayerNorm(d_model, layer_norm_epsilon)
        self._rel: dict = {}

    def rel_table(self, length: int) -> Tensor:
        """fp32 [heads, 2 length - 1]: block 0's relative_attention_bias gathered by bucket, entry [h][key - query + length - 1]; built once
        per sequence length (and per version of the weight) and kept, so a captured graph reads a stable address."""
        if length > T5_MAX_TOKENS:
            raise NotImplementedError(f"T5EncoderTower: at most {T5_MAX_TOKENS} tokens per sequence (the relative-bias attention kernel keeps a head's "
                                      f"bias table in LDS), got {length}")
        weight = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
        stamp = ops._param_stamp(weight)
        hit = self._rel.get(length)
        if hit is None or hit[0] != stamp:
            buckets = relative_buckets(length, self.num_buckets, self.max_distance).to(weight.device)
            hit = self._rel[length] = (stamp, weight.detach().float()[buckets].t().contiguous())
        return hit[1]

    @torch.no_grad()
    def forward(self, input_ids: Tensor) -> dict:
        """{"last_hidden_state": fp32 [B, L, d_model]}: T5EncoderModel(input_ids=...) -- no attention mask, as the reference calls it."""
        ids = _check_ids(input_ids, self.shared.weight.device)
        if ids.dim() != 2:
            raise ValueError(f"token ids must be [batch, length], got {tuple(ids.shape)}")
        self.rel_table(ids.shape[1])      # (refuses a length the kernel does not take before anything is launched or captured)
        if _graphable(self, ids):
            return _forward_graphs(self).run(self._forward_ids, [ids], extra_key=frozen_stamp(self))
        return self._forward_ids(ids)

    def _forward_ids(self, ids: Tensor) -> dict:
        B, L = ids.shape
        rel = self.rel_table(L)
        x = embed_tokens(ids, self.shared.weight)      # T5 neither scales the embeddings nor adds positions
        attend, act = (lambda q, k, v: ops.attention_relbias_fwd(q, k, v, B, self.heads, self.d_kv, rel, scale=1.0)), (lambda u: ops.gated_act(u, self.act))
        for block in self.encoder.block:
            x = block_forward(x, block.spec, attend, act)
        return {"last_hidden_state": self.encoder.final_layer_norm(x).float().reshape(B, L, -1)}

    def train_outputs(self, input_ids: Tensor) -> Tensor:
        """The training forward, autograd-connected through nn.apply_module: fp32 [B, L, d_model] with forward()'s values (the same kernels
        on the same bf16 matrices).  Its backward writes every parameter's .grad in the parameter's engine mode; the tied embedding
        (shared.weight = encoder.embed_tokens.weight) is one parameter with one gradient."""
        ids = _check_ids(input_ids, self.shared.weight.device)
        if ids.dim() != 2:
            raise ValueError(f"token ids must be [batch, length], got {tuple(ids.shape)}")
        if ids.numel() > ops.EMBEDDING_BWD_MAX_TOKENS:
            raise NotImplementedError(f"T5EncoderTower.train_outputs: at most {ops.EMBEDDING_BWD_MAX_TOKENS} tokens per batch (the embedding backward's "
                                      f"limit), got {tuple(ids.shape)}")

        def run(ids):
            B, L = ids.shape
            rel = self.rel_table(L)
            d_rel = torch.zeros_like(rel)      # every layer's backward adds into it
            table = self.shared.weight
            x = embed_tokens(ids, table)
            attend, act = (lambda q, k, v: ops.attention_relbias_train(q, k, v, B, self.heads, self.d_kv, rel, 1.0, d_rel)), (lambda u: ops.gated_act_fwd(u, self.act))
            _, top, b_chain = _chain_train(x, [lambda h, blk=blk: block_train(h, blk.spec, attend, act) for blk in self.encoder.block], set())
            y, b_final = norm_train(top, self.encoder.final_layer_norm)

            def bwd(gout):
                dx = b_chain({}, b_final(_out_grads([gout], 1)[0]))
                bias = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
                ops.relbias_bucket_sum(d_rel, relative_buckets(L, self.num_buckets, self.max_distance), bias)
                ops.embedding_bwd(ids.contiguous(), dx, table, None)
                return None

            return y.float().reshape(B, L, -1), bwd

        return apply_module(run, [ids], self)


# ---------------------------------------------------------------------------------------------------
# embedders
# ---------------------------------------------------------------------------------------------------
def _local_config(path: Union[str, Path]) -> Optional[dict]:
    """config.json of a local checkpoint directory (never a hub lookup)"""
    file = Path(path) / "config.json" if path else None
    if file is None or not file.is_file():
        return None
    return json.loads(file.read_text())


class _T5Embedder(AbstractEmbModel):
    """what FrozenT5Embedder and FrozenByT5Embedder share (reference :14-58 and :61-101 are the same code but for the tokenizer)"""

    tokenizer = None

    def __init__(self, model_name_or_path="", max_length: int = 256, model_kwargs: Optional[dict] = None, freeze: bool = True,
                 config: Optional[dict] = None, **kwargs):
        super().__init__(**kwargs)
        if self.is_trainable and freeze:
            raise NotImplementedError(f"{type(self).__name__}(is_trainable=True) with freeze=True: pass freeze=False to train the tower with the UNet "
                                      "(the reference would freeze every parameter and silently train nothing)")
        if config is None:
            config = _local_config(model_name_or_path)
        if config is None:
            raise ValueError(f"{type(self).__name__}: pass config= (T5Config entries) or a local checkpoint directory as model_name_or_path; "
                             f"{str(model_name_or_path)!r} is not one, and there is no hub access here")
        self.model = T5EncoderTower(**{k: v for k, v in config.items() if k in CONFIG_KEYS})
        self.model_name_or_path, self.model_kwargs = str(model_name_or_path), dict(model_kwargs or {})
        self.max_length = max_length
        self.dtype = torch.float32
        self._load_tokenizer()
        self._load_weights()
        if freeze:
            self.freeze()

    @property
    def device(self):
        return self.model.shared.weight.device

    def _load_tokenizer(self) -> None:
        raise NotImplementedError

    def _load_weights(self) -> None:
        """model.safetensors of a local checkpoint directory, when there is one; otherwise the weights are loaded by the caller
        (load_state_dict on the embedder or on .model)"""
        file = Path(self.model_name_or_path) / "model.safetensors" if self.model_name_or_path else None
        if file is None or not file.is_file():
            return
        from safetensors.torch import load_file

        state = {k: v for k, v in load_file(str(file)).items() if k == "shared.weight" or k.startswith("encoder.")}
        state.setdefault("encoder.embed_tokens.weight", state["shared.weight"])
        self.model.load_state_dict(state)

    def _ids_for(self, text) -> Tensor:
        raise NotImplementedError

    def trained_parameters(self) -> list:
        """Every parameter of the tower, once (the tied embedding is one parameter): what one step gives a gradient, and what the engine puts
        in the tower's store and optimizer group."""
        return list(self.model.parameters())

    def forward(self, text: Union[str, list, Tensor]) -> Tensor:
        """fp32 [B, L, d_model] last hidden state; L = max_length when text is given (padded, and the padding attended to: the
        reference passes no mask).  Trainable (is_trainable and freeze=False) under grad mode: the autograd-connected training chain."""
        ids = text if torch.is_tensor(text) else self._ids_for(_decode_text(text))
        if _trainable(self, self.model):
            return self.model.train_outputs(ids.to(self.device))
        return self._forward_frozen(ids)

    @torch.no_grad()
    def _forward_frozen(self, ids: Tensor) -> Tensor:
        return self.model(ids.to(self.device))["last_hidden_state"]

    def encode(self, text):
        return self(text)


class FrozenT5Embedder(_T5Embedder):
    """reference :14-58.  `config` (a dict of T5EncoderTower arguments / T5Config entries) replaces the lookup of a config; otherwise
    `model_name_or_path` must be a local checkpoint directory (config.json, model.safetensors, spiece.model), read with local_files_only --
    there is never a hub access.  The tower is `.model`, so checkpoints keyed `...model.encoder.block...` load unchanged.  Text needs the
    sentencepiece vocabulary through transformers' T5Tokenizer, found locally; LongTensor ids [B, L] are accepted directly.
    `apply_mask` is stored and unused, as in the reference (its forward passes input_ids only)."""

    def __init__(self, model_name_or_path="", max_length: int = 256, model_kwargs: Optional[dict] = None, freeze: bool = True, apply_mask: bool = True,
                 config: Optional[dict] = None, **kwargs):
        super().__init__(model_name_or_path, max_length, model_kwargs, freeze, config, **kwargs)
        self.apply_mask = apply_mask

    def _load_tokenizer(self) -> None:
        self.tokenizer = None
        if not (self.model_name_or_path and Path(self.model_name_or_path).is_dir()):
            return
        try:
            from transformers import T5Tokenizer

            self.tokenizer = T5Tokenizer.from_pretrained(self.model_name_or_path, local_files_only=True)
        except Exception as err:   # no vocabulary on this machine: token ids can still be passed to forward()
            logger.warning("T5 tokenizer %s is not available locally (%s); pass token ids instead of text", self.model_name_or_path, type(err).__name__)

    def _ids_for(self, text: list) -> Tensor:
        if self.tokenizer is None:
            raise RuntimeError("this embedder has no tokenizer (T5 vocabulary files not found locally): pass LongTensor token ids [B, L]")
        enc = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True, return_overflowing_tokens=False,
                             padding="max_length", return_tensors="pt")
        return enc["input_ids"]


BYT5_PAD, BYT5_EOS, BYT5_OFFSET = 0, 1, 3


def byt5_token_ids(text: list, max_length: int) -> Tensor:
    """ByT5Tokenizer(text, truncation=True, max_length=..., padding="max_length") without a vocabulary file: the UTF-8 bytes + 3, cut to
    max_length - 1, then </s> = 1, padded with <pad> = 0.  (Text is taken literally: a literal "</s>" or "<extra_id_0>" is its bytes.)"""
    rows = []
    for t in text:
        ids = [b + BYT5_OFFSET for b in t.encode("utf-8")][: max_length - 1] + [BYT5_EOS]
        rows.append(ids + [BYT5_PAD] * (max_length - len(ids)))
    return torch.tensor(rows, dtype=torch.int64)


class FrozenByT5Embedder(_T5Embedder):
    """reference :61-101: FrozenT5Embedder over a ByT5 checkpoint.  The byte tokenizer needs no vocabulary file, so text is tokenized on any
    machine (byt5_token_ids); `config` / a local directory as for FrozenT5Embedder.  The reference's class takes no apply_mask."""

    def _load_tokenizer(self) -> None:
        self.tokenizer = byt5_token_ids

    def _ids_for(self, text: list) -> Tensor:
        return byt5_token_ids(text, self.max_length)
