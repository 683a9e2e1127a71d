"""The T5 / ByT5 training chain without a GPU: the float64 restatement the GPU tests differentiate (tests/t5_train_ref.py) against
transformers; the bounds of tests/relbias_bounds.py against an emulation of the backward's rounding points, with and without planted
faults; the plan rows of the two new attention passes (csrc/attn_plan.h) and of the RMSNorm backward (csrc/norm_plan.h); the embedders'
flags."""
import contextlib
import ctypes as C
from unittest import mock

import pytest
import torch

from neurosis_amd import lib
from tests import attn_plan_rows as R
from tests import relbias_bounds as rb
from tests import t5_fixture as F
from tests import t5_train_ref as ref

F64 = torch.float64
TINY = dict(vocab_size=384, d_model=64, d_kv=64, d_ff=128, num_layers=2, num_heads=2, relative_attention_num_buckets=32, relative_attention_max_distance=128,
            feed_forward_proj="gated-gelu", layer_norm_epsilon=1e-6)


# ---------------------------------------------------------------------------------------------------
# 1. the restatement against transformers
# ---------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _keep_float64():
    """transformers' T5 casts to fp32 inside T5LayerNorm (the variance) and around the softmax whatever the model's dtype, which alone
    leaves ~5e-7; while this is open those casts leave a float64 tensor as it is, so the model's own code runs in float64 throughout"""
    to, as_float = torch.Tensor.to, torch.Tensor.float

    def _to(self, *args, **kwargs):
        if self.dtype == F64 and (args[:1] == (torch.float32,) or kwargs.get("dtype") is torch.float32):
            return self
        return to(self, *args, **kwargs)

    def _float(self, *args, **kwargs):
        return self if self.dtype == F64 else as_float(self, *args, **kwargs)

    with mock.patch.object(torch.Tensor, "to", _to), mock.patch.object(torch.Tensor, "float", _float):
        yield


@pytest.mark.parametrize("L", [20, 77])
@pytest.mark.parametrize("name", ["v11", "wide", "relu"])
def test_restatement_equals_transformers_in_float64(name, L):
    transformers = pytest.importorskip("transformers")
    fx = F.variant(name)
    cfg = transformers.T5Config(**fx["config"], is_encoder_decoder=False, use_cache=False, dropout_rate=0.0)
    model = transformers.T5EncoderModel(cfg).double().eval()
    missing, unexpected = model.load_state_dict({k: v.double() for k, v in fx["state"].items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    ids = fx["cases"][str(L)]["ids"]
    up = torch.randn(*ids.shape, fx["config"]["d_model"], dtype=F64, generator=torch.Generator().manual_seed(L))
    with _keep_float64():
        want = model(input_ids=ids).last_hidden_state
        want.backward(up)
    state = ref.trainable_state(fx["state"], F64, "cpu")
    got = ref.encode(state, fx["config"], ids)
    got.backward(up)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))      # noqa: E731
    assert rel(got.detach(), want.detach()) <= 1e-9
    params = dict(model.named_parameters())        # (named_parameters names a tied parameter once)
    seen = set()
    for key, p in state.items():
        hf = params.get(key)
        if hf is None:
            assert key == "encoder.embed_tokens.weight" or key == "shared.weight", key
            hf = params["shared.weight"] if "shared.weight" in params else params["encoder.embed_tokens.weight"]
        assert p.grad is not None and hf.grad is not None, key
        assert rel(p.grad, hf.grad) <= 1e-9, (key, rel(p.grad, hf.grad))
        seen.add(key)
    assert "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight" in seen


# ---------------------------------------------------------------------------------------------------
# 2. the bounds against the emulated arithmetic
# ---------------------------------------------------------------------------------------------------
def _heads(L, D, scale, samples=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = (3.0 / (scale * D ** 0.5)) ** 0.5          # logits of standard deviation ~3
    rel_h = torch.randn(2 * L - 1, generator=g) * 2.0
    return rel_h, [tuple((torch.randn(L, D, generator=g) * f).to(torch.bfloat16) for f in (s, s, 1.0, 1.0)) for _ in range(samples)]


def _worst(rel_h, heads, scale, fault):
    """worst error / bound over the outputs of one head (its samples, and d_rel summed over them) of the emulation under `fault`"""
    worst, dSs = {}, []
    err_sum = abs_sum = drel = 0
    for q, k, v, do in heads:
        want = rb.head_reference(q, k, v, do, rel_h, scale)
        got = rb.emulate(q, k, v, do, rel_h, scale, fault if fault in ("drop_bias", "mirror", "scale_bias", "lse_unbiased") else None)
        for n in ("o", "lse", "dq", "dk", "dv"):
            r, b = want[n]
            worst[n] = max(worst.get(n, 0.0), float(((got[n].to(F64) - r).abs() / b).max()))
        dSs.append(got["dS"])
        d, e, a = want["d_rel"]
        drel, err_sum, abs_sum = drel + d, err_sum + e, abs_sum + a
    got = rb.emulate_drel(dSs, fault if fault and fault.startswith("drel_") else None)
    worst["d_rel"] = float(((got.to(F64) - drel).abs() / rb.drel_bound(err_sum, abs_sum, len(heads))).max())
    return worst


@pytest.mark.parametrize("L, D, scale", [(20, 64, 1.0), (77, 64, 64 ** -0.5), (130, 128, 1.0)])
def test_emulated_backward_stays_inside_the_bounds_and_planted_faults_leave_them(L, D, scale):
    rel_h, heads = _heads(L, D, scale, seed=L)
    clean = _worst(rel_h, heads, scale, None)
    print(f"L={L} D={D} scale={scale:.4f}: worst err / bound {clean}")
    assert max(clean.values()) <= 1.0, clean
    for fault in rb.FAULTS:
        if fault == "scale_bias" and scale == 1.0:
            continue                            # (no fault at scale 1)
        bad = _worst(rel_h, heads, scale, fault)
        assert max(bad.values()) > 1.0, (fault, bad)
        if fault.startswith("drel_"):
            assert bad["d_rel"] > 1.0 and max(v for n, v in bad.items() if n != "d_rel") <= 1.0, (fault, bad)


# ---------------------------------------------------------------------------------------------------
# 3. plan rows
# ---------------------------------------------------------------------------------------------------
def _planned(entry, dims, nptr):
    with R.environment({}):
        lib.launch_log(3)
        try:
            tail = [None] * nptr + ([0, None] if entry == "nk_attention_relbias_bwd" else [None])
            assert int(getattr(lib.load(), entry)(C.byref(R.desc(dims)), *tail)) == 0, lib.load().nk_last_error()
            log = lib.launched()
        finally:
            lib.launch_log(0)
    return [R.parse(line, dims) for line in log[1::2]]


@pytest.mark.parametrize("L", [20, 200, 1024])
@pytest.mark.parametrize("D", [64, 80, 128])
def test_plan_rows_of_the_relbias_training_passes(D, L):
    B, H = 2, 3
    dims = [B, H, L, L, D, 0]
    dp = 64 if D <= 64 else 96 if D <= 96 else 160
    gx = (L + 127) // 128
    table = ((2 * L - 1) * 4 + 15) & ~15
    ring = 2 * 2 * 64 * (2 * dp + 16)
    width = (L + 63) // 64 * 64 + 64
    (fwd, qsplit, _, ws), = _planned("nk_attention_relbias_fwd_lse", dims, 6)
    assert fwd == {"name": "attn_fwd_kernel<relbias,lse>", "extent": [gx, H, B], "grid": [gx * H * B, 1, 1], "gx": gx, "block": 256, "smem": ring + table}
    assert ws == 0
    frozen, = _planned("nk_attention_relbias_fwd", dims, 5)
    assert {**frozen[0], "name": fwd["name"]} == fwd, "the training forward keeps the frozen forward's launch shape"
    rows = _planned("nk_attention_relbias_bwd", dims, 12)
    want_ws = ((B * H * L + 3) & ~3) + B * H * gx * 4 * width + 64
    assert [r[1:] for r in rows] == [(1, -1, want_ws)] * 3
    dq, dkdv, red = (r[0] for r in rows)
    assert dq == {"name": "attn_bwd_dq_kernel<relbias>", "extent": [gx, H, B], "grid": [gx * H * B, 1, 1], "gx": gx, "block": 256,
                  "smem": ring + table + 4 * 2 * width * 4}
    assert dkdv == {"name": "attn_bwd_dkdv_kernel<relbias>", "extent": [gx, H, B], "grid": [gx * H * B, 1, 1], "gx": gx, "block": 256,
                    "smem": 2 * (2 * 32 * (2 * dp + 16) + 256) + table}
    assert red == {"name": "attn_drel_reduce_kernel", "extent": [(2 * L + 62) // 64, H, 1], "grid": [(2 * L + 62) // 64, H, 1], "gx": 0, "block": 1024, "smem": 0}
    assert max(dq["smem"], dkdv["smem"]) <= 160 * 1024
    assert lib.query("nk_attention_relbias_bwd_ws_floats", C.byref(R.desc(dims))) == want_ws


def test_relbias_training_passes_refuse_what_the_forward_refuses():
    l = lib.load()
    for dims in ([1, 1, 1032, 1032, 64, 0], [1, 1, 64, 77, 64, 0], [1, 1, 64, 64, 64, 1]):
        assert int(l.nk_attention_relbias_fwd_lse(C.byref(R.desc(dims)), *([None] * 7))) == 1
        assert int(l.nk_attention_relbias_bwd(C.byref(R.desc(dims)), *([None] * 12), 0, None)) == 1


@pytest.mark.parametrize("M, C_", [(1, 64), (3, 1472), (600, 4096)])
def test_plan_rows_of_the_rmsnorm_backward(M, C_):
    lib.launch_log(3)
    try:
        assert int(lib.load().nk_rmsnorm_bwd(*([None] * 8), M, C_, 0, None)) == 0
        log = lib.launched()
    finally:
        lib.launch_log(0)
    rows = min(M, 512)
    ws = rows * C_ + 64
    assert log[0::2] == ["rms_bwd_rows_kernel", "rms_colpart_reduce_kernel"]
    assert log[1] == f"rms_bwd_rows_kernel grid={(rows + 3) // 4},1,1 256 0 part=0+{rows * C_} ws={ws}"
    assert log[3] == f"rms_colpart_reduce_kernel grid={(C_ + 63) // 64},1,1 1024 0 part=0+{rows * C_} ws={ws}"
    assert lib.query("nk_rmsnorm_bwd_ws_floats", M, C_) == ws
    assert int(lib.load().nk_rmsnorm_bwd(*([None] * 8), 2, 4104, 0, None)) == 1


# ---------------------------------------------------------------------------------------------------
# 4. the embedders' flags
# ---------------------------------------------------------------------------------------------------
def test_trainable_embedder_flags():
    from neurosis_amd.models.text_encoder import FrozenByT5Embedder, FrozenCLIPT5Encoder, FrozenT5Embedder

    for cls in (FrozenT5Embedder, FrozenByT5Embedder):
        e = cls(config=TINY, is_trainable=True, freeze=False)
        assert e.is_trainable and all(p.requires_grad for p in e.parameters())
        trained = e.trained_parameters()
        assert len({id(p) for p in trained}) == len(trained) == len(list(e.model.parameters()))
        assert sum(p is e.model.shared.weight for p in trained) == 1 and e.model.encoder.embed_tokens.weight is e.model.shared.weight
        assert {id(p) for p in trained} == {id(p) for p in e.model.state_dict(keep_vars=True).values()}
        with pytest.raises(NotImplementedError, match="is_trainable.*freeze=False"):
            cls(config=TINY, is_trainable=True)
        frozen = cls(config=TINY)
        assert not frozen.is_trainable and not any(p.requires_grad for p in frozen.parameters())
    with pytest.raises(NotImplementedError, match="is_trainable"):
        FrozenCLIPT5Encoder(device="cpu", clip_config=dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1),
                            t5_config=TINY, is_trainable=True)
