"""The kernels the T5 / ByT5 training chain adds, each against float64: the relative-bias attention forward with log-sum-exp and its backward
with the gradient of the bias table (csrc/attention.hip), the bucket sum, the RMSNorm backward (csrc/norm.hip), the gated gelu_new / gelu_new
/ ReLU backward and the embedding backward without positions (csrc/elementwise.hip).  Outputs are prefilled with NaN: every element must
be written.

Bounds, from where the kernels round (U = 2^-24, bf16 outputs rounded once):
  attention   tests/relbias_bounds.py (its docstring has the rounding points).
  rmsnorm dx  dx = t1 - t2, t1 = rstd g dy, t2 = rstd xhat s2, s2 = mean_c(g dy xhat).  rstd carries the forward's r1 = (0.5 (8 ceil(C / 512)
              + 8) + 3) U; xhat = x rstd one more U; every product one U.  s2 is a per-lane sum in chunk order then six butterfly adds:
              |d s2| <= (r1 + 3 U + (8 ceil(C / 512) + 8) U) mean_c |g dy xhat|.  So |d dx| <= (r1 + 4 U) |t1| + (2 r1 + 5 U) |t2| +
              rstd |xhat| |d s2| (+ U |dx_add|: added in fp32 before the one rounding), times SAFETY, plus half a bf16 ulp.
  dgamma      sum over M rows of dy xhat in fp32, each term within (r1 + 2 U): ((M + 8) U + r1 + 2 U) sum_m |dy xhat| (any order of M adds).
  activations one bf16 rounding plus 64 U of the magnitude terms |dy| |b| (1 + |a|) (du_a) and |dy| (1 + |a|) (du_b, modes 2 / 3), the form of
              the GELU backward test of test_text_encoder_train_gpu.py; the ReLU backward is exact.
  bucket sum  n U sum |terms| for a bucket of n table entries; embedding N U sum |dx| for an id that occurs N times."""
import ctypes as C
import math

import pytest
import torch

from tests import attention_bounds as ab
from tests import attn_plan_rows as R
from tests import relbias_bounds as rb
from tests.test_t5_kernels_gpu import _inputs

pytestmark = pytest.mark.gpu
U, F64, BF16 = ab.U, torch.float64, torch.bfloat16
NAN = float("nan")


def _ops():
    from neurosis_amd import ops

    return ops


def _within(got, ref, bound, what):
    err = (got.to(F64) - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max |err| {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all() and worst <= 1.0, f"{what}: error {worst:.3f} x its bound"
    return worst


# ---------------------------------------------------------------------------------------------------
# relative-bias attention: forward with lse, backward with d_rel
# ---------------------------------------------------------------------------------------------------
def _run(B, H, D, L, scale, dense, kind="gauss", seed=None):
    """(fused, rel, do, o, lse, dq, dk, dv, d_rel) of one forward + backward; gradients and d_rel prefilled with NaN"""
    ops = _ops()
    fused, rel = _inputs(B, H, D, L, seed=(D * 10000 + L * 10 + dense) if seed is None else seed, kind=kind, scale=scale)
    HD = H * D
    do = torch.randn(B * L, HD, generator=torch.Generator(device="cuda").manual_seed(L + D), device="cuda").to(BF16)
    q, k, v = fused[:, :HD], fused[:, HD:2 * HD], fused[:, 2 * HD:]
    grads = torch.full((B * L, 3 * HD), NAN, dtype=BF16, device="cuda")
    dq, dk, dv = grads[:, :HD], grads[:, HD:2 * HD], grads[:, 2 * HD:]
    if dense:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        dq, dk, dv = (torch.full((B * L, HD), NAN, dtype=BF16, device="cuda") for _ in range(3))
    d_rel = torch.full((H, 2 * L - 1), NAN, device="cuda")
    o, bwd = ops.attention_relbias_train(q, k, v, B, H, D, rel, scale, d_rel)
    bwd(do, dq=dq, dk=dk, dv=dv, accumulate=False)
    assert torch.equal(o, ops.attention_relbias_fwd(q, k, v, B, H, D, rel, scale=scale)), "o differs from the frozen forward's"
    return dict(q=q, k=k, v=v, rel=rel, do=do, o=o, lse=bwd.lse, dq=dq, dk=dk, dv=dv, d_rel=d_rel, bwd=bwd)


def _check(B, H, D, L, scale, dense, kind="gauss"):
    r = _run(B, H, D, L, scale, dense, kind)
    worst = {}
    for h in range(H):
        cols = slice(h * D, (h + 1) * D)
        drel = err_sum = abs_sum = 0
        for b in range(B):
            rows = slice(b * L, (b + 1) * L)
            want = rb.head_reference(r["q"][rows, cols], r["k"][rows, cols], r["v"][rows, cols], r["do"][rows, cols], r["rel"][h], scale)
            got = {"o": r["o"][rows, cols], "lse": r["lse"][b, h], "dq": r["dq"][rows, cols], "dk": r["dk"][rows, cols], "dv": r["dv"][rows, cols]}
            for n, g in got.items():
                assert torch.isfinite(g.float()).all(), f"{n} of head ({b}, {h}) is not finite (an element was not written?)"
                ref, bound = want[n]
                worst[n] = max(worst.get(n, 0.0), ((g.to(F64) - ref).abs() / bound).max().item())
            d, e, a = want["d_rel"]
            drel, err_sum, abs_sum = drel + d, err_sum + e, abs_sum + a
        assert torch.isfinite(r["d_rel"][h]).all(), f"d_rel of head {h} is not finite"
        worst["d_rel"] = max(worst.get("d_rel", 0.0), ((r["d_rel"][h].to(F64) - drel).abs() / rb.drel_bound(err_sum, abs_sum, B)).max().item())
    print(f"relbias training B={B} H={H} D={D} L={L} scale={scale:.4f} {'dense' if dense else 'sliced'} {kind}: worst err / bound "
          + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    return r


@pytest.mark.parametrize("dense", [False, True], ids=["sliced", "dense"])
@pytest.mark.parametrize("unit_scale", [True, False], ids=["scale1", "scaleD"])
@pytest.mark.parametrize("L", [1, 20, 64, 65, 77, 200, 512])
@pytest.mark.parametrize("D", [64, 128])
def test_relbias_forward_and_backward_against_float64(D, L, unit_scale, dense):
    _check(2, 3, D, L, 1.0 if unit_scale else D ** -0.5, dense)


@pytest.mark.parametrize("unit_scale", [True, False], ids=["scale1", "scaleD"])
def test_relbias_forward_and_backward_at_the_longest_sequence(unit_scale):
    _check(1, 2, 64, 1024, 1.0 if unit_scale else 0.125, False)


@pytest.mark.parametrize("D, L", [(64, 20), (64, 77), (128, 200)])
def test_relbias_backward_masks_the_key_tail(D, L):
    """the zero rows that pad the last 64-key tile score 40 above every real key: unmasked they would take all the weight of P"""
    _check(2, 3, D, L, 1.0, False, kind="tail")


@pytest.mark.parametrize("D, L", [(64, 200), (128, 200)])
def test_zero_table_backward_is_the_unbiased_backward_bit_for_bit(D, L):
    """rel = 0 at scale 1 (T5's): fma(s, 1, 0) = s, so P, dS and the three gradients are the generic unbiased kernels' (NK_ATTN64=0 keeps
    head dim 64 on them) bit for bit.  (At a scale that is no power of two the biased kernels round scale * s before the multiply by
    log2 e, the unbiased ones multiply s by the rounded scale * log2 e: equal within the bounds, not bitwise.)"""
    ops = _ops()
    from neurosis_amd.lib import NkAttnDesc, call, query

    B, H, HD = 2, 3, 3 * D
    fused, _ = _inputs(B, H, D, L, seed=11 + D)
    do = torch.randn(B * L, HD, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda").to(BF16)
    q, k, v = fused[:, :HD], fused[:, HD:2 * HD], fused[:, 2 * HD:]
    zero = torch.zeros(H, 2 * L - 1, device="cuda")
    d_rel = torch.zeros_like(zero)
    o, bwd = ops.attention_relbias_train(q, k, v, B, H, D, zero, 1.0, d_rel)
    dq, dk, dv = bwd(do)
    d = NkAttnDesc()
    d.B, d.H, d.Lq, d.Lk, d.D, d.scale, d.causal = B, H, L, L, D, 1.0, 0
    d.sq = d.sk = d.sv = 3 * HD
    d.bq = d.bk = d.bv = L * 3 * HD
    d.so = d.sdq = d.sdk = d.sdv = d.sdo = HD
    d.bo = d.bdq = d.bdk = d.bdv = d.bdo = L * HD
    o2 = torch.full_like(o, NAN)
    lse2 = torch.empty(B, H, L, device="cuda")
    g2 = [torch.full_like(o, NAN) for _ in range(3)]
    st = ops._stream()
    with R.environment({"NK_ATTN64": "0"}):
        call("nk_attention_fwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o2.data_ptr(), lse2.data_ptr(), st)
        ws = torch.empty(query("nk_attention_bwd_ws_floats", C.byref(d)), device="cuda")
        call("nk_attention_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o2.data_ptr(), lse2.data_ptr(), do.data_ptr(),
             g2[0].data_ptr(), g2[1].data_ptr(), g2[2].data_ptr(), ws.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(bwd.lse, lse2)
    assert torch.equal(dq, g2[0]) and torch.equal(dk, g2[1]) and torch.equal(dv, g2[2])


@pytest.mark.parametrize("D, L", [(64, 77), (128, 200)])
def test_d_rel_accumulates_exactly_and_repeats_bitwise(D, L):
    r = _run(2, 3, D, L, 1.0, False)
    first = {n: r[n].clone() for n in ("dq", "dk", "dv", "d_rel")}
    again = _run(2, 3, D, L, 1.0, False)
    for n, t in first.items():
        assert torch.equal(again[n], t), f"{n} differs between two runs"
    r["bwd"](r["do"], accumulate=True)          # once more into the same d_rel: fp32 doubling is exact
    torch.cuda.synchronize()
    assert torch.equal(r["d_rel"], 2 * first["d_rel"])


# ---------------------------------------------------------------------------------------------------
# bucket sum
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [20, 200])
def test_bucket_sum_against_float64(L):
    from torch import nn

    from neurosis_amd.models.text_encoder.t5 import relative_buckets
    from neurosis_amd.nn import FlatParamStore

    ops = _ops()
    H, NB = 3, 32
    g = torch.Generator(device="cuda").manual_seed(L)
    d_rel = torch.randn(H, 2 * L - 1, generator=g, device="cuda")
    buckets = relative_buckets(L, NB, 128)
    weight = nn.Parameter(torch.zeros(NB, H, device="cuda"))
    store = FlatParamStore([weight])
    bk = buckets.cuda()
    ref = torch.zeros(NB, H, dtype=F64, device="cuda").index_add_(0, bk, d_rel.to(F64).T)
    mag = torch.zeros(NB, H, dtype=F64, device="cuda").index_add_(0, bk, d_rel.to(F64).abs().T)
    cnt = torch.bincount(bk, minlength=NB).to(F64)[:, None]
    used = cnt[:, 0] > 0
    # bucket 16 ("ahead by zero") has no position pair at any length; L = 20 stays below max_distance and leaves ten more unused
    assert not used[16] and (int((~used).sum()) > 1) == (L == 20)
    store.grad.fill_(NAN)
    store.state.grad_accumulate = False
    ops.relbias_bucket_sum(d_rel, buckets, weight)
    torch.cuda.synchronize()
    first = weight.grad.clone()
    assert torch.count_nonzero(first[~used]) == 0 and not torch.isnan(first).any(), "unused buckets come out exactly zero"
    _within(first[used], ref[used], (cnt * U * mag)[used] + 1e-300, f"bucket sum L={L}")
    store.state.grad_accumulate = True
    ops.relbias_bucket_sum(d_rel, buckets, weight)
    torch.cuda.synchronize()
    store.state.grad_accumulate = False
    assert torch.equal(weight.grad, 2 * first)


# ---------------------------------------------------------------------------------------------------
# RMSNorm backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, C_", [(1, 64), (3, 1472), (77, 128), (130, 4096)])
def test_rmsnorm_backward_against_float64(M, C_):
    from torch import nn

    from neurosis_amd.nn import FlatParamStore

    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(1000 * M + C_)
    x = (torch.randn(M, C_, generator=g, device="cuda") * torch.logspace(-1, 1, M, device="cuda")[:, None]).to(BF16)
    dy = torch.randn(M, C_, generator=g, device="cuda").to(BF16)
    add = torch.randn(M, C_, generator=g, device="cuda").to(BF16)
    gamma = nn.Parameter(1.0 + 0.3 * torch.randn(C_, generator=g, device="cuda"))
    store = FlatParamStore([gamma])
    eps = 1e-6
    y, bwd = ops.rmsnorm_fwd(x, gamma, eps)
    assert torch.equal(y, ops.rmsnorm(x, gamma.detach(), eps)), "y differs from the frozen forward's"
    store.grad.fill_(NAN)
    store.state.grad_accumulate = False
    dx = bwd(dy)
    dgamma = gamma.grad.clone()
    dx2 = bwd(dy, dx_add=add)
    torch.cuda.synchronize()
    assert torch.equal(gamma.grad, dgamma), "dgamma differs between two runs"

    xd, dyd, gd = x.to(F64), dy.to(F64), gamma.detach().to(F64)
    rstd = torch.rsqrt((xd * xd).mean(1, keepdim=True) + eps)
    xh = xd * rstd
    s2 = (gd * dyd * xh).mean(1, keepdim=True)
    t1, t2 = rstd * gd * dyd, rstd * xh * s2
    ref = t1 - t2
    chain = (8 * math.ceil(C_ / 512) + 8) * U
    r1 = 0.5 * chain + 3 * U
    ds2 = (r1 + 3 * U + chain) * (gd * dyd * xh).abs().mean(1, keepdim=True)
    bound = ab.SAFETY * ((r1 + 4 * U) * t1.abs() + (2 * r1 + 5 * U) * t2.abs() + rstd * xh.abs() * ds2)
    _within(dx, ref, bound + ab.half_ulp(ref, bound), f"rmsnorm dx {M}x{C_}")
    ref2 = ref + add.to(F64)
    bound2 = bound + U * add.to(F64).abs()
    _within(dx2, ref2, bound2 + ab.half_ulp(ref2, bound2), f"rmsnorm dx + dx_add {M}x{C_}")
    terms = dyd * xh
    _within(dgamma, terms.sum(0), ab.SAFETY * ((M + 8) * U + r1 + 2 * U) * terms.abs().sum(0) + 1e-300, f"rmsnorm dgamma {M}x{C_}")
    for row in sorted({0, M // 2, M - 1}):      # the same row alone: the same bits of dx
        _, b1 = ops.rmsnorm_fwd(x[row:row + 1].contiguous(), gamma, eps)
        assert torch.equal(b1(dy[row:row + 1].contiguous())[0], dx[row]), f"row {row} of {M} differs when differentiated alone"
    bwd(dy)                                     # (the rows above overwrote dgamma with their own)
    assert torch.equal(gamma.grad, dgamma)
    store.state.grad_accumulate = True          # a second micro-batch adds
    bwd(dy)
    torch.cuda.synchronize()
    store.state.grad_accumulate = False
    assert torch.equal(gamma.grad, 2 * dgamma)


# ---------------------------------------------------------------------------------------------------
# gated gelu_new, gelu_new and ReLU backward
# ---------------------------------------------------------------------------------------------------
def _gelu_new64(a):
    c = 2.0 * math.sqrt(2.0 / math.pi)
    z = c * (a + 0.044715 * a ** 3)
    s = torch.sigmoid(z)
    return a * s, s + a * s * (1 - s) * c * (1 + 3 * 0.044715 * a * a)


@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_gated_act_and_gelu_new_and_relu_backward_against_float64(n):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(n)
    rows = 1 if n == 8 else 7
    inner = n // rows
    assert rows * inner == n and inner % 8 == 0
    a = ((torch.rand(rows, inner, generator=g, device="cuda") * 2 - 1) * 12).to(BF16)
    a[0, :8] = torch.tensor([-12.0, 12.0, 0.0, -0.0, -11.75, -3.0, 1e-3, -1e-3], device="cuda").to(BF16)
    b = (torch.randn(rows, inner, generator=g, device="cuda") * 2).to(BF16)
    dy = torch.randn(rows, inner, generator=g, device="cuda").to(BF16)
    ad, bd, dyd = a.to(F64), b.to(F64), dy.to(F64)
    act, dact = _gelu_new64(ad)
    rounded = lambda ref: ab.half_ulp(ref, torch.zeros_like(ref)) * (1 + 2.0 ** -6)      # noqa: E731

    u = torch.cat([a, b], dim=1).contiguous()
    y, bwd = ops.gated_act_fwd(u, "gated-gelu")
    assert torch.equal(y, ops.gated_act(u, "gated-gelu"))
    du = bwd(dy)
    assert du.dtype == BF16 and du.shape == u.shape
    ref_a, ref_b = dyd * bd * dact, dyd * act
    _within(du[:, :inner], ref_a, rounded(ref_a) + 64 * U * dyd.abs() * bd.abs() * (1 + ad.abs()), f"gated gelu_new du_a n={n}")
    _within(du[:, inner:], ref_b, rounded(ref_b) + 64 * U * dyd.abs() * (1 + ad.abs()), f"gated gelu_new du_b n={n}")

    _, bwd2 = ops.gated_act_fwd(a, "gelu_new")
    ref = dyd * dact
    _within(bwd2(dy), ref, rounded(ref) + 64 * U * dyd.abs() * (1 + ad.abs()), f"gelu_new backward n={n}")
    _, bwd3 = ops.gated_act_fwd(a, "relu")
    assert torch.equal(bwd3(dy), torch.where(a > 0, dy, torch.zeros_like(dy))), "the ReLU backward is exact"


# ---------------------------------------------------------------------------------------------------
# embedding backward without positions
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [64, 128])
def test_embedding_backward_without_positions(C_):
    from torch import nn

    from neurosis_amd.nn import FlatParamStore

    ops = _ops()
    V, B, L = 384, 3, 50
    g = torch.Generator(device="cuda").manual_seed(C_)
    ids = torch.randint(3, V, (B, L), generator=g, device="cuda")
    for b in range(B):
        ids[b, 10 + 7 * b:] = 0              # the padding id, repeated
        ids[b, 9 + 7 * b] = 1                # end of text in every prompt
    dx = torch.randn(B * L, C_, generator=g, device="cuda").to(BF16)
    table = nn.Parameter(torch.zeros(V, C_, device="cuda"))
    store = FlatParamStore([table])
    flat = ids.reshape(-1)
    ref = torch.zeros(V, C_, dtype=F64, device="cuda").index_add_(0, flat, dx.to(F64))
    mag = torch.zeros(V, C_, dtype=F64, device="cuda").index_add_(0, flat, dx.to(F64).abs())
    cnt = torch.bincount(flat, minlength=V).to(F64)[:, None]
    hit = cnt[:, 0] > 0
    assert int(cnt.max()) >= 60
    store.grad.fill_(NAN)
    store.state.grad_accumulate = False
    ops.embedding_bwd(ids, dx, table, None)
    torch.cuda.synchronize()
    first = table.grad.clone()
    assert torch.count_nonzero(first[~hit]) == 0 and not torch.isnan(first).any()
    _within(first[hit], ref[hit], (cnt * U * mag)[hit] + 1e-300, f"embedding without positions C={C_}")
    store.state.grad_accumulate = True
    ops.embedding_bwd(ids, dx, table, None)
    torch.cuda.synchronize()
    store.state.grad_accumulate = False
    assert torch.equal(table.grad, 2 * first)
    with pytest.raises(NotImplementedError, match="at most 8192 tokens"):
        ops.embedding_bwd(torch.zeros(2, 4097, dtype=torch.int64, device="cuda"), torch.zeros(8194, C_, dtype=BF16, device="cuda"), table, None)
