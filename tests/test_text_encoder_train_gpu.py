"""The trainable text towers (configs/sdxl/sdxl-te.example.yaml: both CLIP towers trained with the UNet) on the GPU: the backward kernels
they add -- causal attention (nk_attention_bwd_causal), GELU (nk_gelu_bwd), the embedding lookups (nk_embedding_bwd), the end-of-text row
gather and the few-row weight gradient of bigG's text_projection -- and every parameter gradient of both full-size towers, all against
float64 computed by torch on the GPU.

Floors:
  causal attention  the first-order bounds of tests/attention_bounds.head_reference for the attn64 family (the same rounding points as the
                    non-causal one-kernel backward; its docstring derives them), plus exact checks: with dO nonzero only in query row i the
                    dK / dV rows of keys j > i are exactly zero, and changing K / V rows beyond i leaves dQ[i] bit-identical.
  GELU              one rounding to bf16 (half a bf16 ulp of the float64 value) plus 64 fp32 unit roundoffs of |dy| (1 + |x|) for the
                    fp32 erf / exp evaluation.
  embedding         fp32 sums in token order of bf16 rows: N u sum |dx| per element, N the number of rows summed.
  towers            measured against the oracle's own deviation: the same oracle run as a bf16 step runs it (fp32 weights under
                    torch's bf16 autocast: every GEMM in bf16) against float64 gives, per parameter, a normalised max error e_bf16 and
                    a cosine c_bf16.  The HIP gradient must reach e <= 4 e_bf16 + u_bf16 and 1 - c <= 4 (1 - c_bf16) + 1e-5: both are
                    bf16 pipelines of the same depth, so their deviations from float64 are of one size.  The u_bf16 (2^-8) term is the
                    one rounding autocast does not make: the tower's incoming gradient enters the chain as bf16 (a final LayerNorm's
                    bias gradient is just its column sum).  CLIP-L's k_proj.bias gradients are analytically zero: held to 2 u_bf16 of
                    the layer's v_proj.bias gradient instead.  Prints "[tower] ..." with the worst ratios.
"""
import math

import pytest
import torch

from tests import attention_bounds as ab
from tests.util import cosine, rel_err

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16
U = 2.0 ** -24
UB = 2.0 ** -8          # bf16 unit roundoff


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _check(label, got, ref, bound):
    got = got.to(F64)
    assert torch.isfinite(got).all(), f"{label}: non-finite output"
    ratio = (got - ref).abs() / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"[bound] {label}: worst error / bound = {worst:.3g}")
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{label}: |got - ref| = {float((got.reshape(-1)[i] - ref.reshape(-1)[i]).abs()):.4g} > bound "
                             f"{float(bound.reshape(-1)[i]):.4g} at flat index {i} (worst error / bound {worst:.3g})")


# ================================================================================================================================
# causal attention backward
# ================================================================================================================================
def _causal_run(ops, heads_qkvdo, B, H, L):
    """q / k / v column slices of one [B L, 3 H 64] buffer and dq / dk / dv of another (the towers' packed projection);
    returns (o, dq, dk, dv) as [B, L, H, 64]"""
    D = 64
    HD = H * D
    qkv = torch.empty(B * L, 3 * HD, dtype=BF16, device="cuda")
    do = torch.empty(B * L, HD, dtype=BF16, device="cuda")
    view = qkv.view(B, L, 3, H, D)
    dov = do.view(B, L, H, D)
    for (b, h), (q, k, v, d) in heads_qkvdo.items():
        view[b, :, 0, h], view[b, :, 1, h], view[b, :, 2, h], dov[b, :, h] = q, k, v, d
    q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    o, bwd = ops.attention_causal_fwd(q, k, v, B, H, D)
    grads = torch.full((B * L, 3 * HD), float("nan"), dtype=BF16, device="cuda")       # every gradient element must be written
    bwd(do, dq=grads[:, :HD], dk=grads[:, HD:2 * HD], dv=grads[:, 2 * HD:])
    torch.cuda.synchronize()
    g = grads.view(B, L, 3, H, D)
    return o.view(B, L, H, D), g[:, :, 0], g[:, :, 1], g[:, :, 2]


CAUSAL_L = [1, 31, 32, 33, 76, 77, 96]


@pytest.mark.parametrize("H", [12, 20])
@pytest.mark.parametrize("L", CAUSAL_L)
def test_causal_backward_bounded(ops, L, H):
    B, D = 4, 64
    std, offsets = (4.0, 60.0) if H == 12 else (8.0, 0.0)
    heads = {(b, h): ab.gaussian_head(L, L, D, std, offsets=offsets, late_max=True, tail_dominant=3, seed=1000 * L + 31 * (b * H + h))
             for b in range(B) for h in range(H)}
    o, dq, dk, dv = _causal_run(ops, heads, B, H, L)
    fam = ab.FAMILIES["attn64"]
    worst = {}
    for (b, h), (q, k, v, do) in heads.items():
        ref = ab.head_reference(q, k, v, do, D ** -0.5, fam, causal=True)
        for name, got in (("o", o), ("dq", dq), ("dk", dk), ("dv", dv)):
            r, bound = ref[name]
            got_h = got[b, :, h].to(F64)
            assert torch.isfinite(got_h).all(), f"L {L} H {H} {name} (b{b} h{h}): non-finite"
            ratio = float(((got_h - r).abs() / bound.clamp_min(1e-300)).max())
            worst[name] = max(worst.get(name, 0.0), ratio)
            if not ratio <= 1.0:
                _check(f"causal L {L} H {H} {name} (b{b} h{h})", got_h, r, bound)
    print(f"[bound] causal backward L {L} H {H}: worst error / bound " + ", ".join(f"{n} {w:.3g}" for n, w in worst.items()))


@pytest.mark.parametrize("L", [33, 77, 96])
def test_causal_backward_masks_exactly(ops, L):
    """dO only in query row i: dK / dV rows of keys j > i are exactly zero.  K / V rows beyond i changed: dQ[i] is bit-identical."""
    B, H, D = 2, 12, 64
    base = {(b, h): ab.gaussian_head(L, L, D, 4.0, seed=77 * (b * H + h) + L) for b in range(B) for h in range(H)}
    for i in sorted({0, L // 2, L - 2}):
        heads = {}
        for key, (q, k, v, do) in base.items():
            do1 = torch.zeros_like(do)
            do1[i] = do[i]
            heads[key] = (q, k, v, do1)
        _, dq, dk, dv = _causal_run(ops, heads, B, H, L)
        assert torch.count_nonzero(dk[:, i + 1:]) == 0 and torch.count_nonzero(dv[:, i + 1:]) == 0, f"L {L}: keys beyond query {i} got a gradient"
        assert torch.count_nonzero(dv[:, : i + 1]) > 0
        _, dq_a, _, _ = _causal_run(ops, base, B, H, L)
        changed = {}
        g = torch.Generator(device="cuda").manual_seed(i)
        for key, (q, k, v, do) in base.items():
            k2, v2 = k.clone(), v.clone()
            k2[i + 1:] = torch.randn(k2[i + 1:].shape, generator=g, device="cuda").to(BF16)
            v2[i + 1:] = torch.randn(v2[i + 1:].shape, generator=g, device="cuda").to(BF16)
            changed[key] = (q, k2, v2, do)
        _, dq_b, _, _ = _causal_run(ops, changed, B, H, L)
        assert torch.equal(dq_a[:, : i + 1], dq_b[:, : i + 1]), f"L {L}: dQ[<= {i}] moved when keys beyond {i} changed"


def test_causal_backward_repeats_bitwise(ops):
    B, H, L, D = 4, 20, 77, 64
    heads = {(b, h): ab.gaussian_head(L, L, D, 8.0, seed=5 + b * H + h) for b in range(B) for h in range(H)}
    first = _causal_run(ops, heads, B, H, L)
    second = _causal_run(ops, heads, B, H, L)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_noncausal_backward_still_refuses_causal(ops):
    """nk_attention_bwd keeps its refusal; the causal backward has its own entry point"""
    from neurosis_amd.lib import NkError

    q = torch.randn(77, 64).to(BF16).cuda()
    _, bwd = ops.attention_fwd(q, q, q, 1, 1, 64, causal=True)
    with pytest.raises(NkError):
        bwd(q)
    with pytest.raises(NotImplementedError):
        ops.attention_causal_fwd(torch.randn(97, 64).to(BF16).cuda(), q, q, 1, 1, 64)


# ================================================================================================================================
# GELU backward
# ================================================================================================================================
@pytest.mark.parametrize("quick", [False, True])
def test_gelu_backward_fp64(ops, quick):
    g = torch.Generator(device="cuda").manual_seed(int(quick))
    n = 308 * 5120
    x = (torch.randn(n, generator=g, device="cuda") * 3).to(BF16)
    x[:16] = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 8.0, -8.0, 12.0, -12.0, 0.5, -0.5, 2.0, -2.0, 3.5, -3.5, 1.0, -1.0], device="cuda").to(BF16)
    dy = torch.randn(n, generator=g, device="cuda").to(BF16)
    y, bwd = ops.gelu_fwd(x.view(308, 5120), quick)
    assert torch.equal(y, ops.gelu(x.view(308, 5120), quick))
    dx = bwd(dy.view(308, 5120)).reshape(-1)
    xd, dyd = x.to(F64), dy.to(F64)
    if quick:
        s = torch.sigmoid(1.702 * xd)
        d = s + 1.702 * xd * s * (1 - s)
    else:
        d = 0.5 * (1 + torch.erf(xd / math.sqrt(2))) + xd * torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    ref = dyd * d
    bound = ab.half_ulp(ref, torch.zeros_like(ref)) * (1 + 2.0 ** -6) + 64 * U * dyd.abs() * (1 + xd.abs())
    _check(f"gelu bwd quick={quick}", dx, ref, bound)


# ================================================================================================================================
# embedding backward
# ================================================================================================================================
def _embedding_case(V, C, B, L, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.randint(0, V, (B, L), generator=g, device="cuda")
    pad = V - 1
    for b in range(B):                       # a short prompt: BOS, a few tokens, EOS, then ~60 repeats of the padding id
        n = 4 + 3 * b
        ids[b, n:] = pad
    ids[:, 0] = 5                            # the same id (BOS) in every prompt
    dx = torch.randn(B * L, C, generator=g, device="cuda").to(BF16)
    return ids, dx


def _embedding_ref(ids, dx, V, P):
    B, L = ids.shape
    C = dx.shape[1]
    d = dx.to(F64)
    tab = torch.zeros(V, C, dtype=F64, device="cuda").index_add_(0, ids.reshape(-1), d)
    tab_abs = torch.zeros(V, C, dtype=F64, device="cuda").index_add_(0, ids.reshape(-1), d.abs())
    cnt = torch.bincount(ids.reshape(-1), minlength=V).to(F64)[:, None]
    pos = torch.zeros(P, C, dtype=F64, device="cuda")
    pos[:L] = d.view(B, L, C).sum(0)
    pos_abs = torch.zeros(P, C, dtype=F64, device="cuda")
    pos_abs[:L] = d.abs().view(B, L, C).sum(0)
    return tab, cnt * U * tab_abs + 1e-300, pos, B * U * pos_abs + 1e-300


@pytest.mark.parametrize("V,C", [(49408, 768), (49408, 1280)])
def test_embedding_backward(ops, V, C):
    from torch import nn

    from neurosis_amd.nn import FlatParamStore

    B, L, P = 4, 77, 77
    table = nn.Parameter(torch.zeros(V, C, device="cuda"))
    pos = nn.Parameter(torch.zeros(P, C, device="cuda"))
    store = FlatParamStore([table, pos])
    ids, dx = _embedding_case(V, C, B, L, seed=C)
    tab_ref, tab_b, pos_ref, pos_b = _embedding_ref(ids, dx, V, P)
    hit = torch.bincount(ids.reshape(-1), minlength=V) > 0
    assert int(torch.bincount(ids.reshape(-1), minlength=V).max()) >= 60

    # overwrite (first micro-batch): garbage in the buffer beforehand, rows nothing hit come out zero
    store.grad.fill_(float("nan"))
    store.state.grad_accumulate = False
    ops.embedding_bwd(ids, dx, table, pos)
    torch.cuda.synchronize()
    first_tab, first_pos = table.grad.clone(), pos.grad.clone()
    assert torch.count_nonzero(first_tab[~hit]) == 0 and not torch.isnan(first_tab).any()
    _check(f"embedding table V {V} C {C}", first_tab[hit], tab_ref[hit], tab_b[hit])
    _check(f"embedding positions C {C}", first_pos, pos_ref, pos_b)

    # the same again: bit-identical (fixed-order sums)
    ops.embedding_bwd(ids, dx, table, pos)
    torch.cuda.synchronize()
    assert torch.equal(table.grad, first_tab) and torch.equal(pos.grad, first_pos)

    # accumulate (later micro-batch): a second batch adds onto the first
    ids2, dx2 = _embedding_case(V, C, B, L, seed=C + 1)
    tab_ref2, tab_b2, pos_ref2, pos_b2 = _embedding_ref(ids2, dx2, V, P)
    store.state.grad_accumulate = True
    ops.embedding_bwd(ids2, dx2, table, pos)
    torch.cuda.synchronize()
    store.state.grad_accumulate = False
    both = hit | (torch.bincount(ids2.reshape(-1), minlength=V) > 0)
    assert torch.count_nonzero(table.grad[~both]) == 0
    _check("embedding table accumulated", table.grad[both], (tab_ref + tab_ref2)[both], (tab_b + tab_b2 + U * (tab_ref + tab_ref2).abs())[both])
    _check("embedding positions accumulated", pos.grad, pos_ref + pos_ref2, pos_b + pos_b2 + U * (pos_ref + pos_ref2).abs())


def test_gather_and_few_row_wgrad(ops):
    B, L, C, E = 4, 77, 1280, 1280
    g = torch.Generator(device="cuda").manual_seed(9)
    idx = torch.tensor([3, 76, 0, 40], device="cuda")
    dsel = torch.randn(B, C, generator=g, device="cuda").to(BF16)
    dx = ops.gather_rows_bwd(dsel, idx, L).view(B, L, C)
    want = torch.zeros(B, L, C, dtype=BF16, device="cuda")
    want[torch.arange(B), idx] = dsel
    assert torch.equal(dx, want)
    x = torch.randn(B, C, generator=g, device="cuda").to(BF16)
    dy = torch.randn(B, E, generator=g, device="cuda").to(BF16)
    dw = torch.full((C, E), float("nan"), device="cuda")
    ops.wgrad_few_rows(x, dy, dw, accumulate=False)
    ref = x.to(F64).T @ dy.to(F64)
    bound = B * U * (x.to(F64).abs().T @ dy.to(F64).abs()) + 1e-300
    _check("few-row weight gradient", dw, ref, bound)
    ops.wgrad_few_rows(x, dy, dw, accumulate=True)
    _check("few-row weight gradient accumulated", dw, 2 * ref, 2 * bound + U * 2 * ref.abs())


# ================================================================================================================================
# full-size towers against float64 autograd through the oracle
# ================================================================================================================================
def _randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("logit_scale"):
                continue
            if p.dim() == 1 and ("norm" in name or "ln_" in name) and name.endswith("weight"):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif "embedding" in name:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)


def _ids(B, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V - 2, (B, L), generator=g)
    for b in range(B):
        n = 6 + 9 * b
        ids[b, 0] = V - 2                # start of text
        ids[b, n] = V - 1                # end of text: the highest id (the pooled row)
        ids[b, n + 1:] = 0               # padding
    return ids


def _oracle_grads(fn, sd_cpu, bf16, upstream):
    """run `fn(sd)` on the GPU -- in float64, or (bf16=True) with fp32 weights under bf16 autocast: every GEMM in bf16, as a bf16 training
    step runs it -- and backpropagate the upstream gradients; returns {name: grad as float64, or None}"""
    dtype = torch.float32 if bf16 else F64
    sd = {k: v.detach().to("cuda", dtype).requires_grad_(True) for k, v in sd_cpu.items()}
    with torch.device("cuda"), torch.autocast("cuda", dtype=BF16, enabled=bf16):
        outs = fn(sd)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward([o.to(dtype) for o in outs], [u.to(dtype) for u in upstream])
    return {k: (v.grad.to(F64) if v.grad is not None else None) for k, v in sd.items()}


def _compare_tower(label, names, ref64, ref16, trained_ids):
    rows, failures = [], []
    for name, p in names.items():
        r = ref64[name]
        if id(p) not in trained_ids:
            assert r is None or torch.count_nonzero(r) == 0, f"{label}: {name} has a gradient but is not trained"
            continue
        got = p.grad.to(F64)
        assert torch.isfinite(got).all(), f"{label}: {name} non-finite"
        if name.endswith("k_proj.bias"):
            # analytically zero (the softmax ignores a constant added to a query's scores: sum_j dK_j = 0); what is left is the rounding of
            # the bf16 dK rows it sums, held to 2 bf16 unit roundoffs of the same layer's v_proj.bias gradient (a sum of the same size)
            vb = float(ref64[name.replace("k_proj", "v_proj")].abs().max())
            assert float(r.abs().max()) <= 1e-9 * vb and float(got.abs().max()) <= 2 * 2.0 ** -8 * vb, (name, float(got.abs().max()), vb)
            continue
        e, c = rel_err(got, r), cosine(got, r)
        e16, c16 = rel_err(ref16[name], r), cosine(ref16[name], r)
        re, rc = e / (4 * e16 + UB), (1 - c) / (4 * (1 - c16) + 1e-5)
        rows.append((max(re, rc), name, e, e16, c, c16))
        if not (re <= 1.0 and rc <= 1.0):
            failures.append(name)
    rows.sort(reverse=True)
    print(f"[tower] {label}: {len(rows)} parameters, worst ratio to the floor {rows[0][0]:.3g}")
    for ratio, name, e, e16, c, c16 in rows[:6]:
        print(f"[tower]   {name}: ratio {ratio:.3g}  error {e:.3e} (oracle bf16 {e16:.3e})  1-cos {1 - c:.3e} (oracle bf16 {1 - c16:.3e})")
    assert not failures, f"{label}: {len(failures)} parameters beyond the floor, e.g. {failures[:6]}"


def test_clip_l_gradients_fp64():
    """CLIP-L at full size (12 x 768, quick_gelu), layer hidden / layer_idx 11 as in sdxl-te: every trained parameter's gradient against
    float64 autograd of oracle.clip_oracle; final_layer_norm is not trained (the output does not depend on it) and gets no gradient"""
    from oracle import clip_oracle as O
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder
    from neurosis_amd.nn import FlatParamStore

    B, L = 4, 77
    torch.manual_seed(0)
    emb = FrozenCLIPEmbedder(device="cuda", layer="hidden", layer_idx=11, is_trainable=True)
    _randomize(emb, 1)
    sd_cpu = {k: v.detach().clone() for k, v in emb.transformer.state_dict().items()}
    emb = emb.cuda()
    trained = emb.trained_parameters()
    names = dict(emb.transformer.named_parameters())
    trained_ids = {id(p) for p in trained}
    assert id(names["text_model.final_layer_norm.weight"]) not in trained_ids and len(trained) == len(names) - 2
    store = FlatParamStore(trained)
    ids = _ids(B, L, 49408, 2)
    upstream = torch.randn(B, L, 768, generator=torch.Generator().manual_seed(3)).cuda()
    cfg = dict(num_attention_heads=12, num_hidden_layers=12, hidden_act="quick_gelu")
    fn = lambda sd: O.frozen_clip_embedder(sd, cfg, ids.cuda(), "hidden", 11, False)
    ref64 = _oracle_grads(fn, sd_cpu, False, [upstream])
    ref16 = _oracle_grads(fn, sd_cpu, True, [upstream])

    z = emb(ids.cuda())
    assert z.requires_grad and z.shape == (B, L, 768)
    store.grad.fill_(float("nan"))
    z.backward(upstream)
    torch.cuda.synchronize()
    _compare_tower("CLIP-L hidden/11", names, ref64, ref16, trained_ids)
    assert names["text_model.final_layer_norm.weight"].grad is None

    # the frozen path gives the same forward values
    frozen = FrozenCLIPEmbedder(device="cuda", layer="hidden", layer_idx=11).cuda()
    frozen.transformer.load_state_dict(sd_cpu)
    assert torch.equal(frozen(ids.cuda()), z.detach())


def test_bigg_gradients_fp64():
    """bigG at full size (32 x 1280, exact GELU), penultimate + pooled as in sdxl-te: every trained parameter's gradient against float64
    autograd of oracle.clip_oracle; logit_scale gets no gradient"""
    from oracle import clip_oracle as O
    from neurosis_amd.models.text_encoder.clip import FrozenOpenCLIPEmbedder2
    from neurosis_amd.nn import FlatParamStore

    B, L = 4, 77
    torch.manual_seed(0)
    emb = FrozenOpenCLIPEmbedder2(device="cuda", layer="penultimate", always_return_pooled=True, is_trainable=True)
    _randomize(emb, 4)
    sd_cpu = {k: v.detach().clone() for k, v in emb.model.state_dict().items()}
    emb = emb.cuda()
    trained = emb.trained_parameters()
    names = dict(emb.model.named_parameters())
    trained_ids = {id(p) for p in trained}
    assert id(names["logit_scale"]) not in trained_ids and len(trained) == len(names) - 1
    store = FlatParamStore(trained)
    ids = _ids(B, L, 49408, 5)
    g = torch.Generator().manual_seed(6)
    up_tok, up_pool = torch.randn(B, L, 1280, generator=g).cuda(), torch.randn(B, 1280, generator=g).cuda()
    cfg = dict(heads=20, width=1280, layers=32)
    fn = lambda sd: O.frozen_openclip_embedder2(sd, cfg, ids.cuda(), "penultimate", True, False)
    ref64 = _oracle_grads(fn, sd_cpu, False, [up_tok, up_pool])
    ref16 = _oracle_grads(fn, sd_cpu, True, [up_tok, up_pool])

    z, pooled = emb(ids.cuda())
    assert z.requires_grad and pooled.requires_grad and pooled.shape == (B, 1280)
    store.grad.fill_(float("nan"))
    torch.autograd.backward([z, pooled], [up_tok, up_pool])
    torch.cuda.synchronize()
    _compare_tower("bigG penultimate+pooled", names, ref64, ref16, trained_ids)
    assert names["logit_scale"].grad is None

    frozen = FrozenOpenCLIPEmbedder2(device="cuda", layer="penultimate", always_return_pooled=True).cuda()
    frozen.model.load_state_dict(sd_cpu)
    fz, fp = frozen(ids.cuda())
    assert torch.equal(fz, z.detach()) and torch.equal(fp, pooled.detach())


def test_tower_gradients_accumulate_and_repeat():
    """two micro-batches accumulated equal the sum of the two (up to fp32 rounding of the adds); the same step twice is bit-identical"""
    from neurosis_amd.models.text_encoder.clip import FrozenOpenCLIPEmbedder2
    from neurosis_amd.nn import FlatParamStore

    torch.manual_seed(0)
    cfg = dict(width=256, layers=3, heads=4, embed_dim=128)
    emb = FrozenOpenCLIPEmbedder2(config=cfg, device="cuda", layer="penultimate", always_return_pooled=True, is_trainable=True)
    _randomize(emb, 8)
    emb = emb.cuda()
    store = FlatParamStore(emb.trained_parameters())
    ids_a, ids_b = _ids(4, 77, 49408, 10).cuda(), _ids(4, 77, 49408, 11).cuda()
    g = torch.Generator().manual_seed(12)
    ups = [(torch.randn(4, 77, 256, generator=g).cuda(), torch.randn(4, 128, generator=g).cuda()) for _ in range(2)]

    def step(ids, up, acc):
        store.state.grad_accumulate = acc
        z, p = emb(ids)
        torch.autograd.backward([z, p], list(up))
        torch.cuda.synchronize()
        return store.grad.clone()

    ga = step(ids_a, ups[0], False)
    assert torch.equal(step(ids_a, ups[0], False), ga)
    gb = step(ids_b, ups[1], False)
    step(ids_a, ups[0], False)
    both = step(ids_b, ups[1], True)
    store.state.grad_accumulate = False
    assert torch.allclose(both, ga + gb, rtol=1e-6, atol=1e-6 * float((ga.abs() + gb.abs()).max()))


def test_clip_l_last_and_pooled_fp64():
    """CLIP-L's final-normed outputs (layer "last" with the pooled vector: ONE final_layer_norm whose backward gets the token gradient
    plus the end-of-text rows') on a small tower (4 layers of 256, head dim 64), against float64 autograd of oracle.clip_oracle"""
    from oracle import clip_oracle as O
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder
    from neurosis_amd.nn import FlatParamStore

    B, L = 4, 77
    cfg = dict(hidden_size=256, intermediate_size=1024, num_hidden_layers=4, num_attention_heads=4, vocab_size=49408)
    emb = FrozenCLIPEmbedder(device="cuda", config=cfg, layer="last", always_return_pooled=True, is_trainable=True)
    _randomize(emb, 13)
    sd_cpu = {k: v.detach().clone() for k, v in emb.transformer.state_dict().items()}
    emb = emb.cuda()
    trained = emb.trained_parameters()
    names = dict(emb.transformer.named_parameters())
    assert len(trained) == len(names)
    store = FlatParamStore(trained)
    ids = _ids(B, L, 49408, 14)
    g = torch.Generator().manual_seed(15)
    up_tok, up_pool = torch.randn(B, L, 256, generator=g).cuda(), torch.randn(B, 256, generator=g).cuda()
    ocfg = dict(num_attention_heads=4, num_hidden_layers=4, hidden_act="quick_gelu")
    fn = lambda sd: O.frozen_clip_embedder(sd, ocfg, ids.cuda(), "last", None, True)
    ref64 = _oracle_grads(fn, sd_cpu, False, [up_tok, up_pool])
    ref16 = _oracle_grads(fn, sd_cpu, True, [up_tok, up_pool])
    z, pooled = emb(ids.cuda())
    store.grad.fill_(float("nan"))
    torch.autograd.backward([z, pooled], [up_tok, up_pool])
    torch.cuda.synchronize()
    _compare_tower("CLIP-L (small) last+pooled", names, ref64, ref16, {id(p) for p in trained})


# ================================================================================================================================
# the UNet's gradient of its conditioning, and the engine step with both towers trained
# ================================================================================================================================
def test_unet_context_and_y_gradients_fp64(monkeypatch):
    """UNetModel returns d(context) (the sum of every cross-attention's K / V input gradients) and d(y) (through label_emb) when they
    require grad, against float64 autograd of oracle.sdxl_oracle.unet_forward on the unet_sdxl_tiny fixture (floors as for the towers);
    asking for them leaves every parameter gradient bit-identical"""
    import json
    from pathlib import Path

    import neurosis_amd.modules.diffusion as D
    from oracle import sdxl_oracle as O
    from tests.golden.fixture_io import load_fixture
    from tests.golden.make_golden import UNET_TINY, synth_state_dict

    G = Path(__file__).resolve().parent / "golden"
    fx = load_fixture("unet_sdxl_tiny")
    sd = synth_state_dict(json.loads((G / "unet_sdxl_tiny_keys.json").read_text()))
    net = D.UNetModel(**UNET_TINY)
    net.load_state_dict(sd)
    net = net.cuda()
    x, ctx, y = fx["x"].cuda(), fx["context"].cuda(), fx["y"].cuda()
    t = torch.tensor([17.0, 640.0], device="cuda")
    up = torch.randn(x.shape, generator=torch.Generator().manual_seed(21)).cuda()

    def hip(requires):
        c, yy = ctx.clone().requires_grad_(requires), y.clone().requires_grad_(requires)
        out = net(x, t, c, yy)
        out.float().backward(up)
        torch.cuda.synchronize()
        return c.grad, yy.grad, [p.grad.clone() for p in net.parameters()]

    _, _, plain = hip(False)
    dctx, dy, grads = hip(True)
    assert all(torch.equal(a, b) for a, b in zip(plain, grads)), "asking for d(context) / d(y) moved a parameter gradient"

    def oracle(bf16):
        dtype = torch.float32 if bf16 else F64
        s = {k: v.to("cuda", dtype) for k, v in sd.items()}
        c, yy = ctx.to(dtype).requires_grad_(True), y.to(dtype).requires_grad_(True)
        with torch.device("cuda"), torch.autocast("cuda", dtype=BF16, enabled=bf16):
            out = O.unet_forward(s, UNET_TINY, x.to(dtype), t.to(dtype), c, yy)
        out.to(dtype).backward(up.to(dtype))
        return c.grad.to(F64), yy.grad.to(F64)

    # the timestep embedding is fp32 by definition (the reference's and the kernel's): hand it on in the oracle's working dtype
    fp32_embedding = O.timestep_embedding
    monkeypatch.setattr(O, "timestep_embedding", lambda ts, *a, **k: fp32_embedding(ts, *a, **k).to(ts.dtype))
    (c64, y64), (c16, y16) = oracle(False), oracle(True)
    for name, got, r, r16 in (("d(context)", dctx, c64, c16), ("d(y)", dy, y64, y16)):
        assert got is not None and torch.isfinite(got).all(), name
        e, c = rel_err(got, r), cosine(got, r)
        e16, cs16 = rel_err(r16, r), cosine(r16, r)
        print(f"[unet] {name}: error {e:.3e} (oracle bf16 {e16:.3e}), 1-cos {1 - c:.3e} (oracle bf16 {1 - cs16:.3e})")
        assert e <= 4 * e16 + UB and 1 - c <= 4 * (1 - cs16) + 1e-5, name


def _te_engine(optimizer, scheduler=None):
    """a small SDXL-shaped engine whose conditioner is both towers, trainable (CLIP-L hidden / 0 of 2 layers -> crossattn [B, 77, 64];
    bigG penultimate + pooled -> crossattn [B, 77, 64] and vector [B, 48])"""
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models.diffusion import DiffusionEngine
    from neurosis_amd.models.text_encoder.clip import FrozenCLIPEmbedder, FrozenOpenCLIPEmbedder2
    from neurosis_amd.modules.encoders.embedding import GeneralConditioner

    torch.manual_seed(0)
    cfg = dict(in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2], num_head_channels=16,
               use_linear_in_transformer=True, transformer_depth=1, context_dim=128, adm_in_channels=48, num_classes="sequential", use_checkpoint=False)
    clip_l = FrozenCLIPEmbedder(device="cuda", config=dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1),
                                layer="hidden", layer_idx=0, input_key="caption", is_trainable=True, base_lr=1.0)
    bigg = FrozenOpenCLIPEmbedder2(config=dict(width=64, layers=2, heads=1, embed_dim=48), device="cuda", layer="penultimate", always_return_pooled=True,
                                   input_key="caption", is_trainable=True, base_lr=1.0)
    _randomize(clip_l, 31)
    _randomize(bigg, 32)
    net = D.UNetModel(**cfg)
    with torch.no_grad():
        for p in net.parameters():                   # (zero_module'd outputs would give the conditioning no gradient at all)
            if p.dim() >= 2 and not p.abs().sum():
                p.normal_(std=0.05)
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=None, conditioner=GeneralConditioner([clip_l, bigg]), optimizer=optimizer,
                          scheduler=scheduler, loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting()))
    eng = eng.cuda()
    eng.setup_flat_params()
    return eng


def _te_batch(seed):
    g = torch.Generator().manual_seed(seed)
    ids = _ids(2, 77, 49408, seed).cuda()
    return ({"caption": ids}, torch.randn(2, 4, 16, 16, generator=g).cuda(), torch.tensor([0.5, 3.0]).cuda(),
            torch.randn(2, 4, 16, 16, generator=g).cuda())


def _te_step(eng, seed, micro=0):
    batch, x, sigma, noise = _te_batch(seed)
    eng.accumulate(micro)
    loss = eng(x, batch, sigmas=sigma, noise=noise)
    loss.mean().backward()
    torch.cuda.synchronize()
    return loss.detach()


def test_engine_step_trains_both_towers():
    """the sdxl-te step on a small engine: AdamW8bit over three groups (UNet, CLIP-L, bigG) under LegacyCosineAnnealingWarmupRestarts.  The
    towers' stores get finite nonzero gradients from the UNet's d(context) / d(y); the update moves every trained parameter and leaves the
    ones without a gradient (CLIP-L's second layer and final_layer_norm, bigG's logit_scale) bit-identical; graph replay of the UNet chain
    (third pass of one signature) gives the gradients of the eager first pass bit for bit; two accumulated micro-batches give the sum"""
    from functools import partial

    from neurosis_amd.optimizers import AdamW8bit
    from neurosis_amd.schedulers import LegacyCosineAnnealingWarmupRestarts

    eng = _te_engine(partial(AdamW8bit, lr=1e-3, weight_decay=0.01), partial(LegacyCosineAnnealingWarmupRestarts, first_cycle_steps=10,
                                                                                   warm_up_steps=2, min_lr=1e-6))
    opt = eng._torch_optimizer
    assert [g["name"] for g in opt.param_groups] == ["UNet", "FrozenCLIPEmbedder", "FrozenOpenCLIPEmbedder2"]
    stores = [eng.store, *eng.embedder_stores]
    clip_l, bigg = eng.conditioner.embedders
    frozen = [clip_l.transformer.text_model.final_layer_norm.weight, clip_l.transformer.text_model.encoder.layers[1].mlp.fc2.weight,
              bigg.model.logit_scale]
    frozen0 = [p.detach().clone() for p in frozen]

    runs = []
    for _ in range(3):                  # eager, capture, replay of the UNet chain: one signature
        _te_step(eng, 40)
        runs.append([s.grad.clone() for s in stores])
    for i, (a, b) in enumerate(zip(runs[0], runs[2])):
        assert torch.equal(a, b), f"store {i}: graph replay differs from the eager pass"
    for s in eng.embedder_stores:
        assert torch.isfinite(s.grad).all() and float(s.grad.abs().max()) > 0

    ga = runs[0]
    _te_step(eng, 41)
    gb = [s.grad.clone() for s in stores]
    _te_step(eng, 40, micro=0)
    _te_step(eng, 41, micro=1)
    for a, b, s in zip(ga, gb, stores):
        assert torch.allclose(s.grad, a + b, rtol=1e-6, atol=1e-6 * float((a.abs() + b.abs()).max()))

    before = [s.master.clone() for s in eng.embedder_stores]
    eng.optimizer_step()
    eng.join_optimizer()
    torch.cuda.synchronize()
    for s, m in zip(eng.embedder_stores, before):
        moved = [not torch.equal(p.detach(), m[o:o + p.numel()].view(p.shape)) for p, o in zip(s.params, s.offsets)]
        assert all(moved), "a trained tower parameter did not move"
    for p, p0 in zip(frozen, frozen0):
        assert torch.equal(p.detach(), p0), "a parameter without a gradient changed"
    assert [g["lr"] for g in opt.param_groups][1:] == pytest.approx([0.5, 0.5])      # warm-up step 1 of 2 from min_lr 1e-6 to 1.0
