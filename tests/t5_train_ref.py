"""A pure-torch restatement of the T5 encoder (transformers' T5EncoderModel called with input_ids only): embedding, T5LayerNorm (RMS norm),
bidirectional self-attention with the relative position bias and NO 1 / sqrt(d) scaling, the relu / gelu_new / gated gelu_new FeedForward,
and the bucket map.  Differentiable, in the dtype of the state it is given (float64 for references; fp32 under torch.autocast for the
bf16 floor), on any device.  test_t5_train_cpu.py holds it to transformers; test_t5_train_gpu.py differentiates it."""
import math

import torch
import torch.nn.functional as F


def relative_buckets(length, num_buckets, max_distance):
    """[length, length] int64: T5's bidirectional bucket of key j minus query i (the logarithm in fp32, as transformers takes it)"""
    pos = torch.arange(length)
    rel = pos[None, :] - pos[:, None]
    half = num_buckets // 2
    exact = half // 2
    dist = rel.abs()
    spread = exact + (torch.log(dist.float() / exact) / math.log(max_distance / exact) * (half - exact)).to(torch.int64)
    spread = torch.min(spread, torch.full_like(spread, half - 1))
    return (rel > 0).to(torch.int64) * half + torch.where(dist < exact, dist, spread)


def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def rms_norm(x, weight, eps):
    return weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def encode(state, config, ids):
    """last hidden state [B, L, d_model] of the encoder whose parameters are `state` (T5EncoderModel's names; the tied embedding is read
    from "shared.weight" alone, so its gradient is one tensor)"""
    H, dkv, eps, act = config["num_heads"], config["d_kv"], config["layer_norm_epsilon"], config["feed_forward_proj"]
    B, L = ids.shape
    x = state["shared.weight"][ids]
    buckets = relative_buckets(L, config["relative_attention_num_buckets"], config["relative_attention_max_distance"]).to(ids.device)
    bias = state["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"][buckets].permute(2, 0, 1)[None]      # [1, H, L, L]
    for i in range(config["num_layers"]):
        a, f = f"encoder.block.{i}.layer.0.", f"encoder.block.{i}.layer.1."
        h = rms_norm(x, state[a + "layer_norm.weight"], eps)
        q, k, v = (F.linear(h, state[a + f"SelfAttention.{n}.weight"]).view(B, L, H, dkv).transpose(1, 2) for n in "qkv")
        scores = torch.matmul(q, k.transpose(-1, -2)) + bias.to(q.dtype)
        attn = torch.softmax(scores.float() if scores.dtype != torch.float64 else scores, dim=-1).to(scores.dtype)
        ctx = torch.matmul(attn, v).transpose(1, 2).reshape(B, L, H * dkv)
        x = x + F.linear(ctx, state[a + "SelfAttention.o.weight"])
        h = rms_norm(x, state[f + "layer_norm.weight"], eps)
        if act.startswith("gated-"):
            hidden = gelu_new(F.linear(h, state[f + "DenseReluDense.wi_0.weight"])) * F.linear(h, state[f + "DenseReluDense.wi_1.weight"])
        else:
            u = F.linear(h, state[f + "DenseReluDense.wi.weight"])
            hidden = torch.relu(u) if act == "relu" else gelu_new(u)
        x = x + F.linear(hidden, state[f + "DenseReluDense.wo.weight"])
    return rms_norm(x, state["encoder.final_layer_norm.weight"], eps)


def trainable_state(state, dtype, device, q_factor=1.0):
    """the fixture state as leaf tensors that require grad (without the tied alias), every SelfAttention.q.weight times q_factor"""
    out = {}
    for k, v in state.items():
        if k == "encoder.embed_tokens.weight":
            continue
        t = v.detach().to(device=device, dtype=dtype)
        if k.endswith("SelfAttention.q.weight"):
            t = t * q_factor
        out[k] = t.clone().requires_grad_(True)
    return out
