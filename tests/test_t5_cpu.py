"""The frozen T5 / ByT5 embedders without a GPU: constructor surface, state_dict layout, the host side of the relative position bias,
ByT5 tokenisation, the refusals, the exports and the plan of the relative-bias attention launch (csrc/attn_plan.h)."""
import ctypes as C
import inspect

import pytest
import torch

from neurosis_amd import lib, ops
from neurosis_amd.models.text_encoder import t5 as T
from tests import attn_plan_rows as R
from tests import t5_fixture as F

TINY = dict(vocab_size=384, d_model=64, d_kv=64, d_ff=128, num_layers=2, num_heads=2, relative_attention_num_buckets=32, relative_attention_max_distance=128,
            feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6)
CLIP_TINY = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1)


def _defaults(cls):
    return {n: p.default for n, p in inspect.signature(cls.__init__).parameters.items() if p.default is not inspect.Parameter.empty}


def test_constructor_surface_and_defaults():
    from neurosis_amd.models.text_encoder import FrozenByT5Embedder, FrozenCLIPT5Encoder, FrozenT5Embedder

    d = _defaults(FrozenT5Embedder)
    assert list(d)[:5] == ["model_name_or_path", "max_length", "model_kwargs", "freeze", "apply_mask"]
    assert (d["model_name_or_path"], d["max_length"], d["freeze"], d["apply_mask"], d["config"]) == ("", 256, True, True, None)
    d = _defaults(FrozenByT5Embedder)
    assert list(d)[:4] == ["model_name_or_path", "max_length", "model_kwargs", "freeze"] and (d["max_length"], d["freeze"], d["config"]) == (256, True, None)
    d = _defaults(FrozenCLIPT5Encoder)
    assert list(d)[:5] == ["clip_version", "t5_version", "device", "clip_max_length", "t5_max_length"]
    assert (d["clip_version"], d["t5_version"], d["device"], d["clip_max_length"], d["t5_max_length"]) == ("openai/clip-vit-large-patch14", "google/t5-v1_1-xl",
                                                                                                         "cuda", 77, 77)
    e = FrozenT5Embedder(config=TINY, input_key="caption", max_length=20, apply_mask=False)
    assert isinstance(e.model, T.T5EncoderTower) and e.max_length == 20 and e.apply_mask is False and e.input_key == "caption"
    assert not e.training and not any(p.requires_grad for p in e.parameters()) and e.tokenizer is None
    assert any(p.requires_grad for p in FrozenT5Embedder(config=TINY, freeze=False).parameters())
    both = FrozenCLIPT5Encoder(device="cpu", clip_config=CLIP_TINY, t5_config=TINY)
    assert both.t5_encoder.max_length == 77 and both.clip_encoder.max_length == 77 and isinstance(both.t5_encoder, FrozenT5Embedder)
    # checkpoints keyed ...model.encoder.block... load unchanged
    assert "model.encoder.block.1.layer.0.SelfAttention.q.weight" in e.state_dict()


@pytest.mark.parametrize("name", F.names())
def test_state_dict_is_transformers_layout_and_loads(name):
    fx = F.variant(name)
    tower = T.T5EncoderTower(**fx["config"])
    assert sorted(tower.state_dict()) == fx["keys"]
    tower.load_state_dict(fx["state"])
    assert tower.encoder.embed_tokens.weight is tower.shared.weight
    for key, want in fx["state"].items():
        assert torch.equal(tower.state_dict()[key], want), key
    with torch.device("meta"):
        meta = T.T5EncoderTower(**fx["config"])
    assert sorted(meta.state_dict()) == fx["keys"] and all(v.is_meta for v in meta.state_dict().values())
    gated = fx["config"]["feed_forward_proj"].startswith("gated-")
    assert ("encoder.block.0.layer.1.DenseReluDense.wi_0.weight" in fx["keys"]) == gated
    assert ("encoder.block.0.layer.1.DenseReluDense.wi.weight" in fx["keys"]) == (not gated)
    assert [k for k in fx["keys"] if "relative_attention_bias" in k] == ["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]


@pytest.mark.parametrize("L", [20, 200])
def test_rel_table_equals_transformers_bias_bit_for_bit(L):
    fx = F.variant("v11")
    tower = T.T5EncoderTower(**fx["config"])
    tower.load_state_dict(fx["state"])
    rel = tower.rel_table(L)
    want = fx["compute_bias"][str(L)]                    # [H, L, L]: [h][query i][key j]
    assert rel.dtype == torch.float32 and tuple(rel.shape) == (fx["config"]["num_heads"], 2 * L - 1) and rel.is_contiguous()
    i, j = torch.meshgrid(torch.arange(L), torch.arange(L), indexing="ij")
    assert torch.equal(rel[:, j - i + L - 1], want)
    if L == 200:      # beyond max_distance every distance shares its sign's last bucket, and the two signs differ
        n = L - 128                                   # key - query = -(L - 1) .. -128, and 128 .. L - 1
        assert torch.equal(rel[:, :n], rel[:, :1].expand(-1, n)) and torch.equal(rel[:, -n:], rel[:, -1:].expand(-1, n))
        assert not torch.equal(rel[:, 0], rel[:, -1])
    assert tower.rel_table(L) is rel, "one table per sequence length: a captured graph reads a stable address"
    buckets = T.relative_buckets(L, 32, 128)
    assert int(buckets.min()) == 0 and int(buckets.max()) == (31 if L == 200 else 16 + 10) and int(buckets[L - 1]) == 0 and int(buckets[L]) == 17


def test_byt5_tokenises_text_like_transformers():
    from neurosis_amd.models.text_encoder import FrozenByT5Embedder

    fx = F.index()["byt5"]
    e = FrozenByT5Embedder(config=TINY, max_length=fx["max_length"])
    ids = e._ids_for(fx["texts"])
    assert ids.dtype == torch.int64 and torch.equal(ids, fx["ids"])
    assert torch.equal(T.byt5_token_ids(["ab"], 4), torch.tensor([[100, 101, 1, 0]]))


def test_refusals_by_name():
    from neurosis_amd.models.text_encoder import FrozenByT5Embedder, FrozenCLIPT5Encoder, FrozenT5Embedder

    for cls in (FrozenT5Embedder, FrozenByT5Embedder):
        with pytest.raises(NotImplementedError, match="is_trainable"):
            cls(config=TINY, is_trainable=True)
    with pytest.raises(NotImplementedError, match="is_trainable"):
        FrozenCLIPT5Encoder(device="cpu", clip_config=CLIP_TINY, t5_config=TINY, is_trainable=True)
    tower = T.T5EncoderTower(**TINY)
    with pytest.raises(NotImplementedError, match=f"at most {ops.ATTN_RELBIAS_MAX_L} tokens"):
        tower(torch.zeros(1, ops.ATTN_RELBIAS_MAX_L + 1, dtype=torch.int64))
    with pytest.raises(ValueError, match="feed_forward_proj 'gated-silu'"):
        T.T5EncoderTower(**dict(TINY, feed_forward_proj="gated-silu"))
    with pytest.raises(RuntimeError, match="no tokenizer .*pass LongTensor token ids"):
        FrozenT5Embedder(config=TINY)(["a photo of a cat"])
    with pytest.raises(ValueError, match="no hub access"):
        FrozenT5Embedder("google/t5-v1_1-xl")
    with pytest.raises(TypeError, match="integer tensor"):
        tower(torch.zeros(1, 8))


def test_names_import_from_both_packages_and_load_under_the_prefix_swap():
    import importlib

    import neurosis_amd.models as M
    import neurosis_amd.models.text_encoder as TE

    for name in ("FrozenT5Embedder", "FrozenByT5Embedder", "FrozenCLIPT5Encoder"):
        assert getattr(M, name) is getattr(TE, name) and name in M.__all__ and name in TE.__all__ and name not in M._NOT_BUILT
    assert "FrozenOpenCLIPImageEmbedder" in M._NOT_BUILT
    with pytest.raises(ImportError, match="FrozenOpenCLIPImageEmbedder"):
        M.FrozenOpenCLIPImageEmbedder
    for path in ("neurosis.models.text_encoder.FrozenT5Embedder", "neurosis.models.text_encoder.t5.FrozenByT5Embedder",
                 "neurosis.models.text_encoder.clip_t5.FrozenCLIPT5Encoder", "neurosis.models.FrozenT5Embedder"):
        module, _, cls = path.replace("neurosis.", "neurosis_amd.", 1).rpartition(".")
        built = getattr(importlib.import_module(module), cls)(**({"config": TINY} if "CLIPT5" not in cls else
                                                                 {"device": "cpu", "clip_config": CLIP_TINY, "t5_config": TINY}))
        assert type(built).__name__ == cls


def _planned(dims, env=None):
    """the plan of nk_attention_relbias_fwd in plan-only mode (null pointers: nothing touches a device), None when refused"""
    with R.environment(env or {}):
        lib.launch_log(3)
        try:
            if int(lib.load().nk_attention_relbias_fwd(C.byref(R.desc(dims)), None, None, None, None, None, None)) != 0:
                return None
            log = lib.launched()
        finally:
            lib.launch_log(0)
    assert len(log) == 2 and log[1].startswith(log[0] + " grid=")
    rec, qsplit, part, ws = R.parse(log[1], dims)
    assert (qsplit, part, ws) == (0, -1, 0)
    return rec


@pytest.mark.parametrize("D, dp", [(64, 64), (128, 160), (40, 64), (96, 96)])
@pytest.mark.parametrize("L", [20, 200, 512, 1024])
def test_relbias_attention_plan(D, dp, L):
    B, H = 2, 3
    ring = 2 * 2 * 64 * (2 * dp + 16)
    want_smem = ring + ((2 * L - 1) * 4 + 15) // 16 * 16
    blocks = (L + 127) // 128
    rec = _planned([B, H, L, L, D, 0])
    assert rec == {"name": "attn_fwd_kernel<relbias>", "extent": [blocks, H, B], "grid": [blocks * H * B, 1, 1], "gx": blocks, "block": 256, "smem": want_smem}
    rec = _planned([B, H, L, L, D, 0], {"NK_ATTN_XCD": "0"})
    assert rec["grid"] == [blocks, H, B] and rec["gx"] == 0 and rec["smem"] == want_smem
    assert want_smem <= 160 * 1024
    # the head-dim-64 switch does not move it: there is one kernel for this pass
    assert _planned([B, H, L, L, D, 0], {"NK_ATTN64": "0"})["smem"] == want_smem


def test_relbias_attention_plan_refusals():
    assert _planned([2, 3, 1025, 1025, 64, 0]) is None and "ATTN_RELBIAS_MAX_L" in lib.load().nk_last_error().decode()
    assert _planned([2, 3, 77, 64, 64, 0]) is None, "self-attention only"
    assert _planned([2, 3, 77, 77, 64, 1]) is None, "no causal variant"
    assert _planned([2, 1, 77, 77, 512, 0]) is None and _planned([2, 1, 77, 77, 60, 0]) is None
    # the plans of the other passes are untouched (tests/test_attn_plan_cpu.py pins them all; one here as a canary)
    assert R.planned(lib, [2, 3, 200, 200, 64, 0], {"NK_ATTN64": "0"}, "fwd")["launches"][0]["smem"] == 2 * 2 * 64 * 144
