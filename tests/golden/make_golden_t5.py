"""Writes tests/golden/t5_tiny*.{safetensors,json} (read back by tests/t5_fixture.py): tiny T5 encoders from transformers, driven the way the reference's FrozenT5Embedder
drives them (models/text_encoder/t5.py:38-53: `model(input_ids=...)`, fp32, last_hidden_state -- no attention mask), for
tests/test_t5_cpu.py and tests/test_t5_gpu.py.  CPU only, fixed seeds, no network: `python tests/golden/make_golden_t5.py`.

Three variants, each at L in {20, 77, 200} and B = 2 (200 reaches past max_distance = 128 and past one 128-row query block):

    v11    T5 v1.1 gated-gelu, d_model 64, 2 heads x d_kv 64
    wide   gated-gelu, d_model 128, 3 heads x 64: the inner width (192) differs from d_model
    relu   T5 v1.0 ReLU, d_model 64, 2 heads x d_kv 128

The weights are made to show mistakes.  transformers' initialisation leaves the relative bias ~0.1 and the scores small, so a tower that
dropped the bias, mirrored its table or scaled the scores by d_kv^-0.5 would still pass at bf16 accuracy.  After init the bias is redrawn
with std 2 and every q and k weight is scaled by 3; the maker then applies those three mutations to the reference itself and ASSERTS that
each moves the output by at least 10 x the case's bf16 floor.

The bf16 floor of a case is the reference's own price for bf16 weights and activations: the same model as .bfloat16() on the same ids,
floor_rms = |y_bf16 - y_fp32| / |y_fp32| and floor_max = max|y_bf16 - y_fp32| / max|y_fp32|.  The GPU test bounds the HIP tower by them.

Also stored: transformers' compute_bias output for L in {20, 200} (variant v11), and ByT5Tokenizer ids for three strings.

Files: t5_tiny (the index: variant names, weight shard counts, the ByT5 ids), t5_tiny_<variant> (config, key list, ids, outputs, floors) and
t5_tiny_<variant>_w<i> (the fp32 weights, cut into shards so that no file passes the repository's 1 MiB limit)."""
from __future__ import annotations

import copy
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from tests.golden.fixture_io import save_fixture  # noqa: E402

VOCAB, LAYERS, BATCH, LENGTHS = 384, 2, 2, (20, 77, 200)
SHARD_BYTES = 900 * 1024
VARIANTS = {
    "v11": dict(d_model=64, d_kv=64, d_ff=128, num_heads=2, feed_forward_proj="gated-gelu"),
    "wide": dict(d_model=128, d_kv=64, d_ff=256, num_heads=3, feed_forward_proj="gated-gelu"),
    "relu": dict(d_model=64, d_kv=128, d_ff=128, num_heads=2, feed_forward_proj="relu"),
}
COMMON = dict(vocab_size=VOCAB, num_layers=LAYERS, relative_attention_num_buckets=32, relative_attention_max_distance=128, layer_norm_epsilon=1e-6)
BYT5_TEXTS = ["a photo of a cat", "naïve café — 東京 \U0001f600", "x" * 40]
BYT5_MAX_LENGTH = 32


def rel_rms(a, b):
    return float((a - b).double().norm() / b.double().norm())


def run(model, ids):
    with torch.no_grad():
        return model(input_ids=ids).last_hidden_state


def build(name: str, seed: int):
    from transformers import T5Config, T5EncoderModel

    torch.manual_seed(seed)
    config = T5Config(**COMMON, **VARIANTS[name], is_encoder_decoder=False, use_cache=False)
    model = T5EncoderModel(config).float().eval()
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for key, p in model.named_parameters():
            if key.endswith("relative_attention_bias.weight"):
                p.copy_(torch.randn(p.shape, generator=gen) * 2.0)
            elif key.endswith((".SelfAttention.q.weight", ".SelfAttention.k.weight")):
                p.mul_(3.0)
            elif key.endswith("layer_norm.weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=gen))      # (init leaves them 1: a tower that ignored them would pass)
    return config, model


def mutated(model, which: str):
    m = copy.deepcopy(model)
    att0 = m.encoder.block[0].layer[0].SelfAttention
    with torch.no_grad():
        if which == "bias_zeroed":
            att0.relative_attention_bias.weight.zero_()
        elif which == "sign_halves_swapped":
            w = att0.relative_attention_bias.weight
            half = w.shape[0] // 2
            w.copy_(torch.cat([w[half:], w[:half]]).clone())
        elif which == "q_scaled":
            for block in m.encoder.block:
                q = block.layer[0].SelfAttention.q.weight
                q.mul_(float(q.shape[0] // att0.n_heads) ** -0.5)
    return m


def main():
    fixture = {"variants": {}, "lengths": list(LENGTHS), "batch": BATCH}
    for old in Path(__file__).resolve().parent.glob("t5_tiny*"):
        old.unlink()
    for n, name in enumerate(VARIANTS):
        config, model = build(name, 1234 + n)
        state = model.state_dict()
        entry = {"config": {k: getattr(config, k) for k in ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_heads", "relative_attention_num_buckets",
                                                             "relative_attention_max_distance", "feed_forward_proj", "layer_norm_epsilon")},
                 "keys": sorted(state), "cases": {}}
        shards, size = [{}], 0
        for k, v in state.items():
            if k == "encoder.embed_tokens.weight":      # tied to shared.weight
                continue
            if size + v.numel() * 4 > SHARD_BYTES:
                shards.append({})
                size = 0
            shards[-1][k.replace(".", "|")] = v.float()
            size += v.numel() * 4
        for i, shard in enumerate(shards):
            save_fixture(shard, f"t5_tiny_{name}_w{i}")
        half = copy.deepcopy(model).bfloat16()
        gen = torch.Generator().manual_seed(77 + n)
        for L in LENGTHS:
            ids = torch.randint(0, VOCAB, (BATCH, L), generator=gen)
            y = run(model, ids)
            y16 = run(half, ids).float()
            floor_rms, floor_max = rel_rms(y16, y), float((y16 - y).abs().max() / y.abs().max())
            moves = {which: rel_rms(run(mutated(model, which), ids), y) for which in ("bias_zeroed", "sign_halves_swapped", "q_scaled")}
            print(f"{name} L={L}: floor rms {floor_rms:.4f} max {floor_max:.4f}; mutations " + ", ".join(f"{k} {v:.3f}" for k, v in moves.items()))
            for which, moved in moves.items():
                assert moved >= 10 * floor_rms, f"{name} L={L}: mutation {which} moves the output by {moved:.4f} < 10 x the bf16 floor {floor_rms:.4f}"
            entry["cases"][str(L)] = {"ids": ids, "out": y, "floor_rms": floor_rms, "floor_max": floor_max, "mutations": moves}
        if name == "v11":
            att0 = model.encoder.block[0].layer[0].SelfAttention
            with torch.no_grad():
                entry["compute_bias"] = {str(L): att0.compute_bias(L, L)[0].float() for L in (20, 200)}
        save_fixture(entry, f"t5_tiny_{name}")
        fixture["variants"][name] = len(shards)

    from transformers.models.byt5 import ByT5Tokenizer

    enc = ByT5Tokenizer()(BYT5_TEXTS, truncation=True, max_length=BYT5_MAX_LENGTH, return_length=True, return_overflowing_tokens=False, padding="max_length",
                          return_tensors="pt")
    fixture["byt5"] = {"texts": BYT5_TEXTS, "max_length": BYT5_MAX_LENGTH, "ids": enc["input_ids"]}
    save_fixture(fixture, "t5_tiny")


if __name__ == "__main__":
    main()
