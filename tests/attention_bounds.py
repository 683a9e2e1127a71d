"""Float64 references, error bounds, input generators, the path each case takes (asked of the library's planner) and a small emulation of the
kernels' rounding points for the attention kernels of csrc/attention.hip, attn512.h and attn512_bwd.h.  Shared by test_attention_fp64_gpu.py (the kernels against
float64) and test_attention_bounds_cpu.py (the bounds against the emulated arithmetic, with and without planted faults).

Rounding points, read from the kernels (bf16 = round to nearest even, unit roundoff UB = 2^-8; fp32 unit roundoff U = 2^-24):
  attn64   (d = 64: attn64_fwd_kernel, attn64_bwd_dq_kernel, attn64_bwd_dkdv_kernel, attn64_bwd_small_kernel)
           Q' = bf16(Q * scale * log2 e); scores K Q'^T in fp32 from the deferred reference point m; P rounded to bf16 for P V and for
           dV = P^T dO; dS = P (dP - delta) rounded to bf16 for dQ = scale dS K and dK = ln 2 dS^T Q'; delta = rowsum(dO o O) reads the
           STORED bf16 O; the backward rebuilds the same Q' bit for bit, so the Q' error common to a row cancels against the forward's lse;
           O, dQ, dK, dV rounded once to bf16 (dK / dV after the fp32 sum of the query splits' partials).
  generic  (head dims 40 / 80 / 160 at DP 64 / 96 / 160, and d = 64 under NK_ATTN64=0: attn_fwd_kernel, attn_bwd_dq_kernel,
           attn_bwd_dkdv_kernel) as attn64 without Q': scores Q K^T in fp32 times scale log2 e; dK = scale dS^T Q.
  attn512  (attn512_fwd_kernel; attn512_delta_kernel + attn512_bwd_kernel<0/1>) forward as attn64 (Q'); the backward recomputes scores
           from the raw Q (so the forward lse's Q' error reaches P in full), dS = bf16(P (dP - delta) scale), dK = dS^T Q.
  recompute (ops._attention_recompute_bwd): log p = bf16(scale q.k - lse) (the scores GEMM writes bf16), P = bf16(softmax of those),
           dP = bf16(dO V^T), dS = bf16(P (dP - rowsum(P o dP)) scale) (nk_softmax_rows_bwd), dQ = bf16(dS K), dK, dV fp32 sums of
           dS^T Q, P^T dO rounded once.

Bounds (first order in those roundings and in fp32 accumulation, evaluated in float64 as products of absolute values, so that they stay
meaningful where sums cancel; SAFETY = 1.25 covers the second-order terms):
  E_ij    the Q' rounding, a known function of the input (Q' = bf16(fp32(q) * fp32(scale log2 e)), e = ln 2 Q' - scale q): its exact
          first-order shift of logit ij is E = e k^T.  Ebar_i = sum_j P_ij E_ij moves a whole row (and so lse) and cancels in P.
  phi_ij  (D + 8) U (sigma_ij + M_i) + 4 U: the fp32 score chain and exp2 (sigma = scale |q| |k|^T, M_i = max_j |S_ij| + |lse_i|).
  rho_ij  |E_ij - Ebar_i| + phi_ij, the relative error of the normalised p_ij (E = 0 off the Q' paths); phibar_i = sum_j P_ij phi_ij.
  o       (P o (rho + UB + gL)) |V| + (phibar + gL) |o|, gL = (Lk / 8 + 64) U for the fp32 row sum and P V chains; UB is the rounding of
          P for P V (the row sum l adds the unrounded p, so that rounding is not renormalised).
  lse     |Ebar| + phibar + gL + 8 U M  (+ U |lse| for the fp32 store).
  eps_ij  relative error of the backward's P: rho_ij + the lse bound without |Ebar| where the backward rebuilds the forward's Q' (attn64),
          phi_ij + the whole lse bound where it does not (generic: Ebar = 0; attn512: the forward's Ebar stays in lse).
  dS      |dS~ - dS| <= P ((eps + UB) |dP - delta| + psi) + P d_delta, psi = (D + 2) U |dO| |V|^T,
          d_delta = |dO| . bound(o) + (D + 2) U |dO| . |o|: delta reads the STORED O.  A row's d_delta shifts its dS by P d_delta, which
          moves dQ_i by d_delta |P_i K| (not d_delta P_i |K|).
  dQ      scale (|d dS| |K| + d_delta |P K| + gL |dS| |K|);  dK  scale (|d dS|^T |Q| + gQ |dS|^T |Q|) [+ |dS|^T |e| where dK reads Q'];
  dV      (P o (eps + UB + gQ))^T |dO|, gQ = (Lq / 8 + 64) U.
  recompute: tau = UB (|log P| + bound(lse)) + phi (the bf16 log p), renormalised by the row softmax: eps_P = tau + taubar + UB
          (P stored bf16); dP stored bf16 (UB |dP|); delta = rowsum(P~ o dP~) carries both.
  Every stored bf16 output adds half a bf16 ulp of (|ref| + its bound).
"""
import math
from dataclasses import dataclass

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
SAFETY = 1.25
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
F64 = torch.float64
BF16 = torch.bfloat16


@dataclass(frozen=True)
class Family:
    name: str
    qp_fwd: bool        # forward scores from Q' = bf16(Q scale log2 e)
    qp_bwd: bool        # backward scores from the SAME Q' (its row-common error cancels against the forward lse)
    dk_qp: bool         # dK = ln 2 dS^T Q'
    recompute: bool = False


FAMILIES = {
    "attn64": Family("attn64", True, True, True),
    "generic": Family("generic", False, False, False),
    "attn512": Family("attn512", True, False, False),
    "recompute": Family("recompute", True, False, False, True),     # attn512 forward, ops._attention_recompute_bwd
}


# ================================================================================================================================
# properties of the kernels' loops (the dispatch is asked of the library: case_path, at the end of this file)
# ================================================================================================================================
def empty_split(Lq, qsplit):
    """True if the last query split of the dK / dV kernels owns no 32-query tile"""
    nt_all = (Lq + 31) // 32
    per = (nt_all + qsplit - 1) // qsplit
    return qsplit > 1 and (qsplit - 1) * per >= nt_all


def nwhole(fwd, Lk, D, causal):
    """key tiles the forward takes without a tail mask: the head-dim-64 instances only, none under the causal mask; None at head dim 512"""
    if fwd.startswith("attn512"):
        return None
    return Lk // 64 if (D == 64 and not causal) else 0


# ================================================================================================================================
# helpers
# ================================================================================================================================
def ulp_bf16(x):
    """one bf16 ulp (8 significant bits) of each element of a float64 tensor"""
    a = x.abs().clamp_min(2.0 ** -126)
    mant, _ = torch.frexp(a)
    return a / mant * 2.0 ** -8


def half_ulp(ref, bound):
    return 0.5 * ulp_bf16(ref.abs() + bound)


def family_of(path):
    if path.startswith("attn64"):
        return FAMILIES["attn64"]
    if path.startswith("generic"):
        return FAMILIES["generic"]
    if path == "attn512_recompute":
        return FAMILIES["recompute"]
    return FAMILIES["attn512"]


# ================================================================================================================================
# float64 reference and bounds of one head
# ================================================================================================================================
def head_reference(q, k, v, do, scale, fam, *, causal=False, rows_per_block=None):
    """q [Lq, D], k / v [Lk, D], do [Lq, D] or None: any float type, promoted to float64 on their device.
    Returns {name: (reference, bound)} for o, lse and (with do) dq, dk, dv."""
    Lq, D = q.shape
    e = None
    if fam.qp_fwd:       # the Q' rounding, a known function of the input: ln 2 Q' = scale q + e
        c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
        qp = (q.to(torch.float32) * c.to(q.device)).to(BF16)
        e = LN2 * qp.to(F64) - scale * q.to(F64)
    q, k, v = q.to(F64), k.to(F64), v.to(F64)
    Lk = k.shape[0]
    R = rows_per_block or max(1, min(Lq, (1 << 25) // max(Lk, 1)))        # <= 256 MB per [R, Lk] float64 block
    ka = k.abs()
    gL, gQ = (Lk / 8 + 64) * U, (Lq / 8 + 64) * U
    out = {n: [] for n in ("o", "ob", "lse", "lseb", "dq", "dqb")}
    if do is not None:
        do = do.to(F64)
        dk, dkb, dv, dvb = (torch.zeros(Lk, D, dtype=F64, device=q.device) for _ in range(4))
    for r0 in range(0, Lq, R):
        r1 = min(Lq, r0 + R)
        qb = q[r0:r1]
        qa = qb.abs()
        S = scale * (qb @ k.T)
        if causal:
            S = S.masked_fill(torch.arange(Lk, device=q.device)[None, :] > torch.arange(r0, r1, device=q.device)[:, None], -math.inf)
        lse = torch.logsumexp(S, 1)
        P = torch.exp(S - lse[:, None])
        o = P @ v
        Sf = torch.where(P > 0, S, torch.zeros_like(S))
        M = Sf.abs().amax(1) + lse.abs()
        sigma = scale * (qa @ ka.T)
        phi = (D + 8) * U * (sigma + M[:, None]) + 4 * U
        phibar = (P * phi).sum(1)
        Ebar = torch.zeros_like(lse)
        EE = torch.zeros_like(S)
        if e is not None:
            E = e[r0:r1] @ k.T
            Ebar = (P * E).sum(1)
            EE = (E - Ebar[:, None]).abs()
        rho = EE + phi
        ob = SAFETY * ((P * (rho + UB + gL)) @ v.abs() + (phibar + gL)[:, None] * o.abs())
        ob = ob + half_ulp(o, ob)
        lse_rest = phibar + gL + 8 * U * M
        lseb = SAFETY * (Ebar.abs() + lse_rest) + U * lse.abs()
        out["o"].append(o); out["ob"].append(ob); out["lse"].append(lse); out["lseb"].append(lseb)
        if do is None:
            continue
        dob = do[r0:r1]
        doa = dob.abs()
        dP = dob @ v.T
        psi = (D + 2) * U * (doa @ v.abs().T)
        if fam.recompute:
            tau = UB * ((S - lse[:, None]).abs() + lseb[:, None]) + (D + 16) * U * (sigma + M[:, None])
            tau = torch.where(P > 0, tau, torch.zeros_like(tau))
            epsP = tau + (P * tau).sum(1, keepdim=True) + UB + 8 * U
            delta = (P * dP).sum(1)
            ddelta = (P * (epsP * dP.abs() + psi + UB * dP.abs())).sum(1) + gL * (P * dP.abs()).sum(1)
            A = dP - delta[:, None]
            dS = scale * P * A
            ddS = scale * P * ((epsP + UB) * A.abs() + psi + UB * dP.abs())
            eps_v = epsP
            dsa = dS.abs()
            dqr = dS @ k
            # a row's delta error moves its dS by -P delta: dQ by -scale d_delta (P K), not by scale d_delta (P |K|)
            dqb = SAFETY * (ddS @ ka + scale * ddelta[:, None] * (P @ k).abs() + gL * (dsa @ ka))
            ddS = ddS + scale * P * ddelta[:, None]
            dk += dS.T @ qb
            dkb += ddS.T @ qa + gQ * (dsa.T @ qa)
        else:
            eps = (rho if fam.qp_bwd else phi + Ebar.abs()[:, None]) + SAFETY * lse_rest[:, None] + U * lse.abs()[:, None]
            delta = (dob * o).sum(1)
            ddelta = (doa * ob).sum(1) + (D + 2) * U * (doa * o.abs()).sum(1)
            A = dP - delta[:, None]
            dS = P * A
            ddS = P * ((eps + UB) * A.abs() + psi)
            eps_v = eps
            dsa = dS.abs()
            dqr = scale * (dS @ k)
            dqb = SAFETY * scale * (ddS @ ka + ddelta[:, None] * (P @ k).abs() + gL * (dsa @ ka))
            ddS = ddS + P * ddelta[:, None]
            dk += scale * (dS.T @ qb)
            dkb += scale * (ddS.T @ qa + gQ * (dsa.T @ qa))
            if fam.dk_qp:
                dkb += dsa.T @ e[r0:r1].abs()
        dv += P.T @ dob
        dvb += (P * (eps_v + UB + gQ)).T @ doa
        out["dq"].append(dqr); out["dqb"].append(dqb + half_ulp(dqr, dqb))
    res = {"o": (torch.cat(out["o"]), torch.cat(out["ob"])), "lse": (torch.cat(out["lse"]), torch.cat(out["lseb"]))}
    if do is not None:
        res["dq"] = (torch.cat(out["dq"]), torch.cat(out["dqb"]))
        dkb, dvb = SAFETY * dkb, SAFETY * dvb
        res["dk"] = (dk, dkb + half_ulp(dk, dkb))
        res["dv"] = (dv, dvb + half_ulp(dv, dvb))
    return res


# ================================================================================================================================
# inputs
# ================================================================================================================================
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def gaussian_head(Lq, Lk, D, logit_std, *, offsets=0.0, late_max=False, tail_dominant=0, seed=0, device="cuda"):
    """bf16 q, k, v, dO of one head: logits scale q.k of standard deviation ~logit_std; `offsets` adds a per-row constant of up to
    +-offsets natural units (a constant key component); late_max makes the second half of the rows find their maximum in the last key
    tile only; tail_dominant keys of the ragged last tile get a large score for every row."""
    g = _gen(seed, device)
    scale = D ** -0.5
    s = math.sqrt(logit_std / (scale * math.sqrt(D)))      # scale * s^2 * sqrt(D) = logit_std
    q = torch.randn(Lq, D, generator=g, device=device) * s
    k = torch.randn(Lk, D, generator=g, device=device) * s
    if offsets:
        off = (torch.rand(Lq, generator=g, device=device) * 2 - 1) * offsets
        k[:, 0] = 1.0
        q[:, 0] = off / scale
    if late_max and Lk > 64:
        last = ((Lk - 1) // 64) * 64
        rows = torch.arange(Lq // 2, Lq, device=device)
        k[last:, 1] = 4.0 * s
        q[rows, 1] = abs(logit_std) * 2.0 / (scale * 4.0 * s)
    if tail_dominant:
        j = torch.arange(max(0, Lk - tail_dominant), Lk, device=device)
        k[j, 2] = 2.0 * s
        q[:, 2] = q[:, 2].abs() + logit_std * 1.5 / (scale * 2.0 * s)
    v = torch.randn(Lk, D, generator=g, device=device)
    do = torch.randn(Lq, D, generator=g, device=device)
    return q.to(BF16), k.to(BF16), v.to(BF16), do.to(BF16)


MARGIN = 120.0      # natural units: exp(-120) underflows fp32, so every non-target weight is exactly zero in the kernels


def retrieval_targets(Lq, Lk, *, causal=False, seed=0, device="cuda"):
    """target key per query: every key is someone's target when Lq >= Lk (else the first key of every 64-key tile, every 32-key tile
    boundary and the last key come first); causal: pi(i) <= i, the diagonal included"""
    g = _gen(seed, device)
    if causal:
        i = torch.arange(Lq, device=device)
        r = (torch.rand(Lq, generator=g, device=device) * (i + 1)).long()
        return torch.where(i % 2 == 0, i, r)
    must = torch.unique(torch.cat([torch.arange(0, Lk, 32, device=device), torch.tensor([Lk - 1], device=device)]))
    rest = torch.randperm(Lk, generator=g, device=device)
    rest = rest[~torch.isin(rest, must)]
    order = torch.cat([must, rest])
    reps = (Lq + Lk - 1) // Lk
    t = order.repeat(reps)[:Lq]
    return t[torch.randperm(Lq, generator=g, device=device)] if Lq >= Lk else t


def retrieval_base(Lq, Lk, D, *, two=False, causal=False, seed=0, device="cuda"):
    """dense +-1 keys k [Lk, D] (float64), targets [Lq, 2] (b = -1: one target) and alpha: query i = alpha k_a, or alpha (k_a + k_b), a
    tie; alpha a power of two with every target ahead of every other visible key by >= MARGIN natural units (asserted in float64 on the
    integer scores).  Causal two-key rows pair a visible key a <= i with a masked key b > i: the output must be v_a.  Heads derive from
    this by flipping the signs of key columns (head_flip), which leaves every score, tie and margin as it is."""
    g = _gen(seed, device)
    scale = D ** -0.5
    k = torch.randint(0, 2, (Lk, D), generator=g, device=device).to(F64) * 2 - 1
    ta = retrieval_targets(Lq, Lk, causal=causal, seed=seed + 1, device=device)
    tb = torch.full_like(ta, -1)
    i = torch.arange(Lq, device=device)
    if two and Lk > 1:
        if causal:
            nb = (Lk - 1 - i).clamp_min(0)
            tb = torch.where(nb > 0, i + 1 + (torch.rand(Lq, generator=g, device=device) * nb).long().clamp_max(nb - 1), torch.full_like(i, -1))
        else:
            tb = (ta + 1 + (torch.rand(Lq, generator=g, device=device) * (Lk - 1)).long().clamp_max(Lk - 2)) % Lk
    def row_gaps(ta, tb):
        gaps = torch.empty(Lq, dtype=F64, device=device)
        for r0 in range(0, Lq, 2048):
            r = slice(r0, min(Lq, r0 + 2048))
            rows = i[r]
            a, bb = ta[r], tb[r]
            direction = k[a] + torch.where(bb[:, None] >= 0, k[bb.clamp_min(0)], torch.zeros_like(k[a]))
            raw = direction @ k.T                                          # integers: exact in float64
            vis = torch.ones_like(raw, dtype=torch.bool)
            if causal:
                vis = torch.arange(Lk, device=device)[None, :] <= rows[:, None]
            tgt = torch.zeros_like(vis)
            n = torch.arange(raw.shape[0], device=device)
            tgt[n, a] = True
            top = raw[n, a]
            if two and not causal:
                assert torch.equal(raw[n[bb >= 0], bb[bb >= 0]], top[bb >= 0]), "tie broken"
                tgt[n[bb >= 0], bb[bb >= 0]] = True
            gaps[r] = top - torch.where(vis & ~tgt, raw, torch.full_like(raw, -math.inf)).amax(1)
        return gaps

    gaps = row_gaps(ta, tb)
    for _ in range(20):         # a tie whose sum direction another key matches as well: draw another partner for that row
        redo = (gaps < 4) & (tb >= 0) & (not causal)
        if not bool(redo.any()):
            break
        nb = (ta + 1 + (torch.rand(Lq, generator=g, device=device) * (Lk - 1)).long().clamp_max(Lk - 2)) % Lk
        tb = torch.where(redo, nb, tb)
        gaps = row_gaps(ta, tb)
    gap = float(gaps.min())
    assert gap > 0, "a non-target key scores as high as a target"
    alpha = 2.0 ** math.ceil(math.log2(MARGIN / (scale * gap))) if math.isfinite(gap) else 1.0
    assert alpha * scale * gap >= MARGIN
    return k, torch.stack([ta, tb], 1), alpha


def retrieval_query(k, targets, alpha):
    ta, tb = targets[:, 0], targets[:, 1]
    return alpha * (k[ta] + torch.where(tb[:, None] >= 0, k[tb.clamp_min(0)], torch.zeros_like(k[ta])))


# ================================================================================================================================
# emulation of the rounding points (CPU, small shapes)
# ================================================================================================================================
def _bf(x):
    return x.to(BF16).to(torch.float32)


def _trunc_bf(x):
    return (x.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32)


def emulate(q, k, v, do, fam, *, causal=False, qsplit=1, fault=None):
    """the kernels' arithmetic on one head in torch: fp32 matrix products, bf16 where the family rounds.  fault: None, 'drop_tail_key'
    (the forward masks key Lk - 1), 'lse_neighbour' (the backward reads row i + 1's lse), 'split_missing' (dK / dV without the last
    query split), 'truncate_p' (P truncated to bf16, not rounded)."""
    f32 = torch.float32
    q, k, v = q.to(f32), k.to(f32), v.to(f32)
    do = None if do is None else do.to(f32)
    Lq, D = q.shape
    Lk = k.shape[0]
    scale = D ** -0.5
    c = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    rp = _trunc_bf if fault == "truncate_p" else _bf
    qp = _bf(q * c) if fam.qp_fwd else None
    s2 = qp @ k.T if fam.qp_fwd else (q @ k.T) * c
    mask = torch.zeros(Lq, Lk, dtype=torch.bool)
    if causal:
        mask = torch.arange(Lk)[None, :] > torch.arange(Lq)[:, None]
    if fault == "drop_tail_key":
        mask[:, Lk - 1] = True
    s2 = s2.masked_fill(mask, -1e30)
    m = s2.amax(1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(1, keepdim=True)
    o = _bf((rp(p) @ v) / l)
    lse = ((m[:, 0] + torch.log2(l[:, 0])) * torch.tensor(LN2, dtype=f32))
    res = {"o": o, "lse": lse}
    if do is None:
        return res
    lse_b = torch.roll(lse, -1) if fault == "lse_neighbour" else lse
    if fam.recompute:
        logp = _bf((q @ k.T) * torch.tensor(scale, dtype=f32) - lse_b[:, None])
        P = _bf(torch.softmax(logp, 1))
        dP = _bf(do @ v.T)
        dS = _bf(P * (dP - (P * dP).sum(1, keepdim=True)) * scale)
        dq = _bf(dS @ k)
        dkp, dvp = dS.T, rp(P).T
        kq = q
        post_k = 1.0
    else:
        sb = (qp @ k.T) if fam.qp_bwd else (q @ k.T) * c
        P = torch.exp2(sb - lse_b[:, None] * torch.tensor(LOG2E, dtype=f32))
        dP = do @ v.T
        delta = (do * o).sum(1, keepdim=True)
        dS = P * (dP - delta)
        if fam.name == "attn512":
            dS = _bf(dS * scale)
            dq = _bf(dS @ k)
            post_k = 1.0
        else:
            dS = _bf(dS)
            dq = _bf((dS @ k) * scale)
            post_k = LN2 if fam.dk_qp else scale
        kq = qp if fam.dk_qp else q
        dkp, dvp = dS.T, rp(P).T
    nt_all = (Lq + 31) // 32
    per = (nt_all + qsplit - 1) // qsplit
    dk = torch.zeros(Lk, D)
    dv = torch.zeros(Lk, D)
    for s in range(qsplit):
        if fault == "split_missing" and s == qsplit - 1:
            continue
        rows = slice(min(Lq, s * per * 32), min(Lq, (s + 1) * per * 32))
        dk += (dkp[:, rows] @ kq[rows]) * post_k
        dv += dvp[:, rows] @ do[rows]
    res.update(dq=dq, dk=_bf(dk), dv=_bf(dv))
    return res


# ================================================================================================================================
# the GPU test's cases: (id, env, B, H, Lq, Lk, D, causal, layout, backward) -- layout "self" (slices of one [B L, 3 H D] buffer),
# "cross" (dense q, k / v slices of [B Lk, 2 H D]) or "dense"; env {"NK_ATTN64": "0"} / {"NK_ATTN64_SMALL": "0"}; D = 512 with
# backward "recompute" takes ops.attention512_fwd beyond 2 048 tokens; backward None = forward only, lse dropped for D = 512
# ================================================================================================================================
A64_OFF = {"NK_ATTN64": "0"}
SMALL_OFF = {"NK_ATTN64_SMALL": "0"}
REAL_CASES = [
    ("sdxl-self-L4096", {}, 4, 10, 4096, 4096, 64, False, "self", True),            # attn64 fwd nwhole 64; dQ + dK/dV, qsplit 1
    ("sdxl-self-L1024", {}, 4, 20, 1024, 1024, 64, False, "self", True),
    ("sdxl-self-L3952", {}, 4, 10, 3952, 3952, 64, False, "self", True),            # ragged: 61 whole tiles + 48 keys
    ("sdxl-self-L988", {}, 4, 20, 988, 988, 64, False, "self", True),               # ragged: 15 whole tiles + 28 keys
    ("sdxl-cross-L4096", {}, 4, 10, 4096, 77, 64, False, "cross", True),            # one kernel, small qsplit 8
    ("sdxl-cross-L1024", {}, 4, 20, 1024, 77, 64, False, "cross", True),            # small qsplit 4
    ("sdxl-cross-L3952", {}, 4, 10, 3952, 77, 64, False, "cross", True),            # small qsplit 8
    ("sdxl-cross-L988", {}, 4, 20, 988, 77, 64, False, "cross", True),              # small qsplit 4
    ("sdxl-cross-L4096-2k", SMALL_OFF, 4, 10, 4096, 77, 64, False, "cross", True),  # attn64 dQ + dK/dV + reduce, qsplit 16
    ("sdxl-cross-L1024-2k", SMALL_OFF, 4, 20, 1024, 77, 64, False, "cross", True),  # qsplit 8
    ("sdxl-cross-L3952-2k", SMALL_OFF, 4, 10, 3952, 77, 64, False, "cross", True),  # qsplit 16
    ("sdxl-cross-L988-2k", SMALL_OFF, 4, 20, 988, 77, 64, False, "cross", True),    # qsplit 4
    ("clip-l-causal", {}, 4, 12, 77, 77, 64, True, "self", None),                   # attn64 causal forward + lse
    ("bigg-causal", {}, 4, 20, 77, 77, 64, True, "self", None),
    ("sd15-self-d40", {}, 2, 8, 4096, 4096, 40, False, "self", True),               # generic DP 64
    ("sd15-self-d80", {}, 2, 8, 1024, 1024, 80, False, "self", True),               # generic DP 96
    ("sd15-self-d160", {}, 2, 8, 256, 256, 160, False, "self", True),               # generic DP 160
    ("sd15-cross-d40", {}, 2, 8, 4096, 77, 40, False, "cross", True),               # generic qsplit 16 + reduce
    ("sd15-cross-d80", {}, 2, 8, 1024, 77, 80, False, "cross", True),               # generic qsplit 8 + reduce
    ("sd15-cross-d160", {}, 2, 8, 256, 77, 160, False, "cross", True),              # generic, no split
    ("generic64-self", A64_OFF, 2, 10, 1024, 1024, 64, False, "self", True),        # NK_ATTN64=0: generic DP 64, nwhole 16
    ("generic64-cross", A64_OFF, 2, 10, 1024, 77, 64, False, "cross", True),        # generic qsplit 8
    ("empty-split-small", {}, 2, 20, 1040, 77, 64, False, "cross", True),           # small qsplit 8: 33 tiles, 5 per split, split 7 none
    ("empty-split-dkdv", {}, 2, 20, 1040, 120, 64, False, "cross", True),           # attn64 dK/dV qsplit 8, split 7 none
    ("vae-enc-L16384", {}, 1, 1, 16384, 16384, 512, False, "dense", None),          # attn512 forward without lse
    ("vae-enc-L15808", {}, 1, 1, 15808, 15808, 512, False, "dense", None),
    ("vae-train-L1024", {}, 4, 1, 1024, 1024, 512, False, "dense", True),           # attn512 forward + flash backward
    ("vae-train-L200", {}, 2, 1, 200, 200, 512, False, "dense", True),
    ("vae-recompute-L4096", {}, 1, 1, 4096, 4096, 512, False, "dense", "recompute"),
]
EDGE_LQ = (1, 31, 33, 129)
EDGE_LK = (1, 3, 63, 64, 65, 96, 97, 127, 128, 129)
EDGE_CASES = [(f"edge-d{D}-{Lq}x{Lk}", env, 3, 3, Lq, Lk, D, False, "cross", True)
              for D, env in ((64, {}), (64, SMALL_OFF), (80, {})) for Lq in EDGE_LQ for Lk in EDGE_LK]
EDGE_CASES += [(f"edge-d512-{L}", {}, 3, 1, L, L, 512, False, "dense", True) for L in (1, 31, 33, 129)]


LABEL = {"attn64_fwd_kernel": "attn64_fwd", "attn_fwd_kernel": "generic_fwd_dp", "attn512_fwd_kernel": "attn512_fwd", "attn64_bwd_small_kernel": "attn64_small",
         "attn64_bwd_dq_kernel": "attn64_dq_dkdv", "attn_bwd_dq_kernel": "generic_bwd_dp", "attn512_delta_kernel": "attn512_flash"}


def _generic_dp(launch):
    """the DP instance of a generic kernel, from the LDS bytes of its query-block ring [2 stages][K, V][64][2 DP + 16] (csrc/attn_plan.h)"""
    dp = (launch["smem"] // 256 - 16) // 2
    assert dp in (64, 96, 160) and launch["smem"] == 256 * (2 * dp + 16), launch
    return dp


def case_path(case):
    """(forward path, backward path, query splits of the dK / dV partials, nwhole of the forward, empty split): kernels and splits are what
    the library plans for the case under its environment (plan-only mode: tests/attn_plan_rows.py), mapped to the labels the tests use"""
    from neurosis_amd import lib, ops
    from tests import attn_plan_rows as R

    _, env, B, H, Lq, Lk, D, causal, _, bwd = case
    dims = [B, H, Lq, Lk, D, int(causal)]
    label = lambda l: LABEL[l["name"]] + (str(_generic_dp(l)) if l["name"].startswith("attn_") else "")
    fwd = label(R.planned(lib, dims, env, "fwd")["launches"][0])
    fwd += "_causal" if causal and fwd == "attn64_fwd" else ("_nolse" if D == 512 and bwd is None else "")
    nw = nwhole(fwd, Lk, D, causal)
    if not bwd:
        return fwd, None, 1, nw, False
    if D == 512 and Lq > ops.ATTN512_FLASH_MAX_L:       # ops.attention512_fwd: beyond that, the chunked recompute through the tile engine
        return fwd, "attn512_recompute", 1, nw, False
    plan = R.planned(lib, dims, env, "bwd")
    s = max(plan["qsplit"], 1)
    assert (s > 1) == (plan["launches"][-1]["name"] == "attn_dkv_reduce_kernel"), plan
    return fwd, label(plan["launches"][0]) + ("_qsplit" if s > 1 else ""), s, nw, empty_split(Lq, s)
