"""The three kernels of the T5 encoders against float64: RMSNorm (csrc/norm.hip: rms_fwd_kernel), the gated gelu_new / tanh-GELU / ReLU pass
(csrc/elementwise.hip) and the forward attention with a relative position bias (csrc/attention.hip: attn_fwd_kernel<.., RELBIAS>).

Every bound is derived from where the kernel rounds (U = 2^-24 fp32, bf16 outputs rounded once: half a bf16 ulp), not from its output:

  rmsnorm   sum of squares: per lane ceil(C / 512) * 8 fused multiply-adds, then 6 butterfly adds -- a sum of non-negative terms, relative error
            <= (8 ceil(C / 512) + 8) U with the mean's multiply and the eps add; the inverse square root halves it and adds 2 U of its own;
            two multiplies by rstd and gamma, 2 U more (+ 2 U slack): rel = (0.5 (8 ceil(C / 512) + 8) + 6) U.
  gelu_new  y = x / (1 + e), e = exp(-z), z = 2 sqrt(2 / pi) (x + 0.044715 x^3): z carries ~6 U relative, so e carries (6 |z| + 8) U with the
            fast exponential's argument scaling and its own ulp; y then e / (1 + e) <= 1 of that plus 3 U: rel = (6 |z| + 11) U.  Where e
            overflows fp32 (z < -88.72) the kernel returns 0 for a value of magnitude <= |x| e^-88 (times |gate|): an absolute term.
  attention the generic family's forward bound of tests/attention_bounds.py with S = scale q k^T + bias: the bias enters in one fp32 fused
            multiply-add whose rounding is relative to |S| <= M, already inside phi = (D + 8) U (sigma + M) + 4 U."""
import math

import pytest
import torch

from tests import attention_bounds as ab
from tests import attn_plan_rows as R

pytestmark = pytest.mark.gpu
U, F64, BF16 = ab.U, torch.float64, torch.bfloat16


def _ops():
    from neurosis_amd import ops

    return ops


def _within(got, ref, bound, what):
    err = (got.to(F64) - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max |err| {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert torch.isfinite(got.float()).all() and worst <= 1.0, f"{what}: error {worst:.3f} x its bound"


# ---------------------------------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, C", [(1, 64), (3, 1472), (77, 128), (130, 4096)])
def test_rmsnorm_against_float64_and_rows_do_not_depend_on_m(M, C):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(1000 * M + C)
    x = (torch.randn(M, C, generator=g, device="cuda") * torch.logspace(-2, 2, M, device="cuda")[:, None]).to(BF16)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g, device="cuda")
    eps = 1e-6
    y = ops.rmsnorm(x, gamma, eps)
    assert y.dtype == BF16 and y.shape == x.shape
    xd = x.to(F64)
    ref = xd * torch.rsqrt((xd * xd).mean(1, keepdim=True) + eps) * gamma.to(F64)
    rel = (0.5 * (8 * math.ceil(C / 512) + 8) + 6) * U
    bound = ab.SAFETY * rel * ref.abs()
    _within(y, ref, bound + ab.half_ulp(ref, bound), f"rmsnorm {M}x{C}")
    for row in sorted({0, M // 2, M - 1}):      # the same row alone, and as the last row of a shorter matrix: the same bits
        alone = ops.rmsnorm(x[row:row + 1].contiguous(), gamma, eps)
        assert torch.equal(alone[0], y[row]), f"row {row} of {M} differs when normalised alone"
        if row:
            assert torch.equal(ops.rmsnorm(x[:row + 1].contiguous(), gamma, eps)[row], y[row])


def test_rmsnorm_refuses_what_it_does_not_take():
    ops = _ops()
    from neurosis_amd.lib import NkError

    x = torch.zeros(2, 4104, dtype=BF16, device="cuda")
    with pytest.raises(NkError, match="RMS_MAXCH"):
        ops.rmsnorm(x, torch.ones(4104, device="cuda"))
    with pytest.raises(ValueError, match="fp32"):
        ops.rmsnorm(x[:, :64].contiguous(), torch.ones(64, device="cuda", dtype=BF16))


# ---------------------------------------------------------------------------------------------------
# gated gelu_new, tanh GELU, ReLU
# ---------------------------------------------------------------------------------------------------
def _gelu_new_reference(x, gate):
    """float64 gelu_new(x) * gate and its bound (module docstring)"""
    xd, gd = x.to(F64), gate.to(F64)
    z = 2.0 * math.sqrt(2.0 / math.pi) * (xd + 0.044715 * xd ** 3)
    ref = xd * torch.sigmoid(z) * gd
    bound = ab.SAFETY * (6 * z.abs() + 11) * U * ref.abs() + (xd * gd).abs() * math.exp(-88.0)
    return ref, bound + ab.half_ulp(ref, bound)


@pytest.mark.parametrize("n", [8, 8 * 1000 + 8])
def test_gated_act_and_tanh_gelu_against_float64(n):
    ops = _ops()
    g = torch.Generator(device="cuda").manual_seed(n)
    rows = 1 if n == 8 else 7          # n elements as one row, and as 7 rows of 1144: the gate is the second half of every row
    inner = n // rows
    assert rows * inner == n and inner % 8 == 0
    a = ((torch.rand(rows, inner, generator=g, device="cuda") * 2 - 1) * 12).to(BF16)
    a[0, :8] = torch.tensor([-12.0, 12.0, 0.0, -0.0, -11.75, -3.0, 1e-3, -1e-3], device="cuda").to(BF16)      # both ends of the span, zero, tiny
    gate = (torch.randn(rows, inner, generator=g, device="cuda") * 2).to(BF16)
    y = ops.gated_act(torch.cat([a, gate], dim=1).contiguous(), "gated-gelu")
    assert y.dtype == BF16 and tuple(y.shape) == (rows, inner)
    _within(y, *_gelu_new_reference(a, gate), f"gated gelu_new n={n}")
    y1 = ops.gated_act(a, "gelu_new")
    _within(y1, *_gelu_new_reference(a, torch.ones_like(a)), f"gelu_new n={n}")
    assert torch.equal(ops.gated_act(a, "relu"), torch.relu(a)), "ReLU is exact"
    with pytest.raises(ValueError, match="kind must be one of"):
        ops.gated_act(a, "gated-silu")


# ---------------------------------------------------------------------------------------------------
# attention with a relative position bias
# ---------------------------------------------------------------------------------------------------
def _biased_head(q, k, v, rel_h, scale):
    """float64 softmax(scale q k^T + bias) v of one head, bias[i][j] = rel_h[j - i + L - 1], and the generic family's forward bound of
    tests/attention_bounds.py (head_reference, the lines that give `ob`) with the bias inside S"""
    L, D = q.shape
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    idx = torch.arange(L, device=q.device)
    S = scale * (q @ k.T) + rel_h.to(F64)[idx[None, :] - idx[:, None] + L - 1]
    lse = torch.logsumexp(S, 1)
    P = torch.exp(S - lse[:, None])
    o = P @ v
    M = S.abs().amax(1) + lse.abs()
    sigma = scale * (q.abs() @ k.abs().T)
    phi = (D + 8) * U * (sigma + M[:, None]) + 4 * U
    phibar = (P * phi).sum(1)
    gL = (L / 8 + 64) * U
    ob = ab.SAFETY * ((P * (phi + ab.UB + gL)) @ v.abs() + (phibar + gL)[:, None] * o.abs())
    return o, ob + ab.half_ulp(o, ob)


def _inputs(B, H, D, L, seed, kind="gauss", scale=1.0):
    """fused [B * L, 3 H D] bf16 = [q | k | v] with logits of standard deviation ~3 at scale 1, and per-head tables of std 2"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    s = math.sqrt(3.0 / math.sqrt(D))
    fused = torch.randn(B * L, 3 * H * D, generator=g, device="cuda")
    fused[:, :2 * H * D] *= s
    rel = torch.randn(H, 2 * L - 1, generator=g, device="cuda") * 2.0
    if kind == "q0":            # the row maximum comes from the bias alone
        fused[:, :H * D] = 0
    if kind == "tail":          # every real key sits 40 below an all-zero key row: the rows past Lk in the last tile would win if unmasked
        a = math.sqrt(40.0 / scale)
        for h in range(H):
            fused[:, h * D] = a
            fused[:, H * D + h * D] = -a
    return fused.to(BF16), rel


def _check(B, H, D, L, scale, dense, kind="gauss"):
    ops = _ops()
    fused, rel = _inputs(B, H, D, L, seed=D * 10000 + L * 10 + dense, kind=kind, scale=scale)
    HD = H * D
    q, k, v = fused[:, :HD], fused[:, HD:2 * HD], fused[:, 2 * HD:]
    if dense:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    o = ops.attention_relbias_fwd(q, k, v, B, H, D, rel, scale=scale)
    assert o.dtype == BF16 and tuple(o.shape) == (B * L, HD)
    worst = 0.0
    for b in range(B):
        for h in range(H):
            rows, cols = slice(b * L, (b + 1) * L), slice(h * D, (h + 1) * D)
            ref, bound = _biased_head(q[rows, cols], k[rows, cols], v[rows, cols], rel[h], scale)
            err = (o[rows, cols].to(F64) - ref).abs()
            worst = max(worst, (err / bound).max().item())
    print(f"relbias attention B={B} H={H} D={D} L={L} scale={scale:.4f} {'dense' if dense else 'sliced'} {kind}: worst err / bound {worst:.3f}")
    assert torch.isfinite(o.float()).all() and worst <= 1.0
    return fused, rel, o


@pytest.mark.parametrize("dense", [False, True], ids=["sliced", "dense"])
@pytest.mark.parametrize("unit_scale", [True, False], ids=["scale1", "scaleD"])
@pytest.mark.parametrize("L", [20, 77, 200, 512])
@pytest.mark.parametrize("D", [64, 128])
def test_relbias_attention_against_float64(D, L, unit_scale, dense):
    _check(2, 3, D, L, 1.0 if unit_scale else D ** -0.5, dense)


@pytest.mark.parametrize("D, L", [(64, 77), (128, 200)])
def test_relbias_attention_row_maximum_from_the_bias_alone(D, L):
    """q = 0: every score is its bias, so a running max that missed the bias would exponentiate up to ~e^8 unnormalised"""
    _check(2, 3, D, L, 1.0, False, kind="q0")


@pytest.mark.parametrize("D, L", [(64, 20), (64, 77), (128, 200)])
def test_relbias_attention_masks_the_key_tail(D, L):
    """the zero rows that pad the last 64-key tile score 40 above every real key: unmasked they would take all the weight"""
    _check(2, 3, D, L, 1.0, False, kind="tail")
    _check(2, 3, D, L, D ** -0.5, True, kind="tail")


@pytest.mark.parametrize("D, L", [(64, 77), (64, 200), (128, 200), (128, 512)])
def test_zero_table_agrees_with_the_unbiased_forward(D, L):
    """rel = 0 at scale D^-0.5 is nk_attention_fwd's problem; both run the generic kernel (NK_ATTN64=0 keeps head dim 64 off the kernel
    that pre-scales Q), so they agree within the bound of either"""
    ops = _ops()
    B, H = 2, 3
    fused, _ = _inputs(B, H, D, L, seed=7 + L)
    HD = H * D
    q, k, v = fused[:, :HD], fused[:, HD:2 * HD], fused[:, 2 * HD:]
    zero = torch.zeros(H, 2 * L - 1, device="cuda")
    o = ops.attention_relbias_fwd(q, k, v, B, H, D, zero, scale=D ** -0.5)
    with R.environment({"NK_ATTN64": "0"}):
        plain = ops.attention_fwd(q, k, v, B, H, D)[0]
    for b in range(B):
        for h in range(H):
            rows, cols = slice(b * L, (b + 1) * L), slice(h * D, (h + 1) * D)
            _, bound = _biased_head(q[rows, cols], k[rows, cols], v[rows, cols], zero[h], D ** -0.5)
            assert ((o[rows, cols].to(F64) - plain[rows, cols].to(F64)).abs() <= bound).all()


def test_relbias_attention_refusals():
    ops = _ops()
    L = ops.ATTN_RELBIAS_MAX_L + 8
    x = torch.zeros(L, 64, dtype=BF16, device="cuda")
    with pytest.raises(NotImplementedError, match=f"at most {ops.ATTN_RELBIAS_MAX_L} tokens"):
        ops.attention_relbias_fwd(x, x, x, 1, 1, 64, torch.zeros(1, 2 * L - 1, device="cuda"))
    x = torch.zeros(16, 64, dtype=BF16, device="cuda")
    with pytest.raises(ValueError, match="rel must be a dense fp32"):
        ops.attention_relbias_fwd(x, x, x, 1, 1, 64, torch.zeros(1, 30, device="cuda"))
