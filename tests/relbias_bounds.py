"""Float64 reference, first-order error bounds and a small emulation of the rounding points for ONE head of the relative-bias attention under
training (csrc/attention.hip: attn_fwd_kernel<.., RELBIAS, RB_LSE>, attn_bwd_dq_kernel<.., RELBIAS>, attn_bwd_dkdv_kernel<.., RELBIAS>,
attn_drel_reduce_kernel).  Shared by test_t5_train_kernels_gpu.py (the kernels against float64) and test_t5_train_cpu.py (the bounds against
the emulated arithmetic, with and without planted faults).

Rounding points, read from the kernels (bf16 = round to nearest even, UB = 2^-8; fp32 unit roundoff U = 2^-24):
  forward   S = fma(q k^T, scale, rel[h][j - i + L - 1]) in fp32 (the products q k^T accumulate in fp32 MFMAs); p = exp2(S log2 e - m log2 e)
            against the running maximum m of S; the row sum l adds the unrounded p in fp32; P is rounded to bf16 for P V; o = bf16(acc / l);
            lse = m + log l in fp32.
  backward  both kernels rebuild S the same way and P = exp2(S log2 e - lse log2 e); dP = dO V^T in fp32; delta = rowsum(dO o O) reads the
            STORED bf16 O; dS = P (dP - delta) in fp32.  d_rel adds THAT fp32 dS along the diagonals (per wave in LDS, then the fixed-order
            reducer over batch and query waves: all fp32).  dS is rounded to bf16 for dQ = scale dS K and dK = scale dS^T Q, P to bf16
            for dV = P^T dO; dQ, dK, dV are rounded once to bf16.  The bias carries no scale and gets none in dS.

Bounds: the generic family's lines of tests/attention_bounds.head_reference (E = 0: no pre-scaled Q') with the bias inside S -- the bias
enters in one fused multiply-add whose rounding is relative to |S| <= M, already inside phi = (D + 8) U (sigma + M) + 4 U.
  d_rel     the diagonal sum of the dS bound WITHOUT dS's bf16 rounding, P (eps |dP - delta| + psi + d_delta), times SAFETY, plus
            (n / 8 + 64) U sum |dS| for the fp32 summation of the diagonal's n terms (n = samples x queries on the diagonal; the kernels'
            longest chain is 16 + 16 + rows / 16 + 1 additions, below n / 8 + 64 for every admitted shape)."""
import torch

from tests.attention_bounds import BF16, F64, LOG2E, SAFETY, U, UB, half_ulp


def bias_matrix(rel_h, L):
    """bias[i][j] = rel_h[j - i + L - 1]"""
    idx = torch.arange(L, device=rel_h.device)
    return rel_h[idx[None, :] - idx[:, None] + L - 1]


def diag_sums(x):
    """[2 L - 1]: entry d + L - 1 = sum_i x[i, i + d]"""
    L = x.shape[0]
    idx = torch.arange(L, device=x.device)
    out = torch.zeros(2 * L - 1, dtype=x.dtype, device=x.device)
    return out.index_add_(0, (idx[None, :] - idx[:, None] + L - 1).reshape(-1), x.reshape(-1))


def head_reference(q, k, v, do, rel_h, scale):
    """q, k, v, do [L, D], rel_h [2 L - 1]: any float type, promoted to float64.  Returns {name: (reference, bound)} for o, lse, dq, dk, dv
    and "d_rel": (this sample's diagonal sums of dS, of the dS error bound without the bf16 rounding, of |dS|) -- drel_bound() combines
    the samples of a head."""
    L, D = q.shape
    q, k, v, do = q.to(F64), k.to(F64), v.to(F64), do.to(F64)
    qa, ka, doa = q.abs(), k.abs(), do.abs()
    gL = (L / 8 + 64) * U
    S = scale * (q @ k.T) + bias_matrix(rel_h.to(F64), L)
    lse = torch.logsumexp(S, 1)
    P = torch.exp(S - lse[:, None])
    o = P @ v
    M = S.abs().amax(1) + lse.abs()
    sigma = scale * (qa @ ka.T)
    phi = (D + 8) * U * (sigma + M[:, None]) + 4 * U
    phibar = (P * phi).sum(1)
    ob = SAFETY * ((P * (phi + UB + gL)) @ v.abs() + (phibar + gL)[:, None] * o.abs())
    ob = ob + half_ulp(o, ob)
    lse_rest = phibar + gL + 8 * U * M
    lseb = SAFETY * lse_rest + U * lse.abs()
    eps = phi + SAFETY * lse_rest[:, None] + U * lse.abs()[:, None]
    dP = do @ v.T
    psi = (D + 2) * U * (doa @ v.abs().T)
    delta = (do * o).sum(1)
    ddelta = (doa * ob).sum(1) + (D + 2) * U * (doa * o.abs()).sum(1)
    A = dP - delta[:, None]
    dS = P * A
    dsa = dS.abs()
    ddS32 = P * (eps * A.abs() + psi)          # the fp32 dS: what d_rel sums
    ddS = ddS32 + P * UB * A.abs()             # ... rounded to bf16: what dQ and dK multiply
    dq = scale * (dS @ k)
    dqb = SAFETY * scale * (ddS @ ka + ddelta[:, None] * (P @ k).abs() + gL * (dsa @ ka))
    shift = P * ddelta[:, None]
    dk = scale * (dS.T @ q)
    dkb = SAFETY * scale * ((ddS + shift).T @ qa + gL * (dsa.T @ qa))
    dv = P.T @ do
    dvb = SAFETY * ((P * (eps + UB + gL)).T @ doa)
    return {"o": (o, ob), "lse": (lse, lseb), "dq": (dq, dqb + half_ulp(dq, dqb)), "dk": (dk, dkb + half_ulp(dk, dkb)),
            "dv": (dv, dvb + half_ulp(dv, dvb)), "d_rel": (diag_sums(dS), diag_sums(ddS32 + shift), diag_sums(dsa))}


def drel_bound(err_sum, abs_sum, samples):
    """bound of a head's d_rel [2 L - 1] from the sums over its samples of head_reference()["d_rel"][1] and [2]"""
    L = (err_sum.numel() + 1) // 2
    n = samples * (L - (torch.arange(2 * L - 1, device=err_sum.device) - (L - 1)).abs()).to(F64)
    return SAFETY * err_sum + (n / 8 + 64) * U * abs_sum


# ================================================================================================================================
# emulation of the rounding points (CPU, small shapes)
# ================================================================================================================================
def _bf(x):
    return x.to(BF16).to(torch.float32)


FAULTS = ("drop_bias", "mirror", "scale_bias", "lse_unbiased", "drel_shift", "drel_last_tile", "drel_sample")


def emulate(q, k, v, do, rel_h, scale, fault=None):
    """the kernels' arithmetic on one head in torch (fp32 products, bf16 where the kernels round); returns o, lse, dq, dk, dv and the fp32
    dS.  Faults of the backward's recomputation: 'drop_bias' (P without the bias), 'mirror' (the table read at query - key), 'scale_bias'
    (the bias multiplied by scale), 'lse_unbiased' (the forward's lse from the unbiased scores)."""
    f32 = torch.float32
    q, k, v, do, rel_h = (t.to(f32) for t in (q, k, v, do, rel_h))
    L = q.shape[0]
    sc, l2e = torch.tensor(scale, dtype=f32), torch.tensor(LOG2E, dtype=f32)
    raw = q @ k.T
    bias = bias_matrix(rel_h, L)
    S = raw * sc + bias
    m = S.amax(1, keepdim=True)
    p = torch.exp2(S * l2e - m * l2e)
    l = p.sum(1, keepdim=True)
    o = _bf((_bf(p) @ v) / l)
    lse = m[:, 0] + torch.log(l[:, 0])
    if fault == "lse_unbiased":
        lse = torch.logsumexp(raw * sc, 1)
    Sb = S
    if fault == "drop_bias":
        Sb = raw * sc
    elif fault == "mirror":
        Sb = raw * sc + bias.T
    elif fault == "scale_bias":
        Sb = (raw + bias) * sc
    P = torch.exp2(Sb * l2e - (lse * l2e)[:, None])
    dP = do @ v.T
    delta = (do * o).sum(1, keepdim=True)
    dS = P * (dP - delta)
    dSb = _bf(dS)
    return {"o": o, "lse": lse, "dq": _bf((dSb @ k) * sc), "dk": _bf((dSb.T @ q) * sc), "dv": _bf(_bf(P).T @ do), "dS": dS}


def emulate_drel(dS_samples, fault=None):
    """a head's d_rel from its samples' fp32 dS (fp32 sums).  Faults: 'drel_shift' (every diagonal one entry off), 'drel_last_tile' (the keys
    of the last 64-key tile not added), 'drel_sample' (the last sample not added)."""
    L = dS_samples[0].shape[0]
    total = torch.zeros(2 * L - 1, dtype=torch.float32)
    for n, dS in enumerate(dS_samples):
        if fault == "drel_sample" and n == len(dS_samples) - 1:
            continue
        if fault == "drel_last_tile":
            dS = dS.clone()
            dS[:, ((L - 1) // 64) * 64:] = 0
        total += diag_sums(dS.to(torch.float32))
    return torch.roll(total, 1) if fault == "drel_shift" else total
