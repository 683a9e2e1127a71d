"""The float64 yardstick of the Gumbel-softmax quantizer (csrc/gumbel.hip, GumbelQuantizer): the reference's forward restated with injected
noise under float64 autograd, the noise generator restated from tests/dropout_ref, and the rule that says which indices an fp32 evaluation
may return.  No GPU, and nothing of the reference is imported.

Notation: U = 2^-24 (the unit roundoff of fp32), h the latent width, h4 = h rounded up to 4 (the MFMA's k step: the zero tail adds exactly),
n the number of codes, l = logits, g = noise, s = l + g, a = s / tau.

LOGITS.  l_j = fadd(chain_j, b_j) with chain_j the fma chain of h4 links over z_k w_jk.  A chain of m fused links errs by at most
m U sum_k |z_k w_jk| (1 + O(m U)); the bias add by U |l_j| <= U (|b_j| + sum |z w|)(1 + ...).  So
    |l_j - l64_j| <= (h4 + 1) U (|b_j| + sum_k |z_k w_jk|),      and   logit_bound = 2 (h4 + 6) U (|b_j| + sum_k |z_k w_jk|)
holds it with a safety factor of more than 2.

ACCEPTABLE INDEX.  s_j = fadd(l_j, g_j) adds U |s_j| <= U (|l_j| + |g_j|); a_j = fmul(s_j, fp32(1 / tau)) is a monotone map of s_j, so it
can only tie two scores that were one rounding apart (U |s_j| more).  In all |s_j - s64_j| <= (h4 + 3) U (|b_j| + sum |z w| + |g_j|) and
    bound_j = 2 (h4 + 6) U (|b_j| + sum_k |z_k w_jk| + |g_j|).
The rule is applied to s (the argmax of a = s / tau is the argmax of s for every tau > 0): index j is ACCEPTABLE iff
s64_j >= s64_max - bound_j - bound_max, and a row is DECIDED iff exactly one index is acceptable; any correct fp32 evaluation then returns
float64's argmax.

SOFTMAX.  y_j = exp(a_j - a_max) / sum.  The exponent carries the error of a_j and a_max, 2 U (|s_j| + |s_max|) / tau with the bounds above
taken at injected logits (where the chain is not part of it: the logits are the kernel's input, 2 roundings per score), and one subtraction,
U |a_j - a_max|; the library expf is within 1 ulp (2 U); the sum of n terms in [0, 1] through per-thread chains of at most ceil(n / 256) + 3
links, a 6-level butterfly and 3 wave additions errs by (ceil(n / 256) + 12) U relative; the quotient by U.  Relative to y64_j:
    softmax_rel_j = 2 * (2 (|a_j| + |a_max|) + |a_j - a_max| + ceil(n / 256) + 16) U              (safety factor 2)
and the bf16 store adds 2^-8 (round to nearest at 8 significant bits: half a unit in the last place, relative to the value).

KL.  The issue's bound: |kl - kl64| <= 2 (n + 8) U max(|kl64|, 1).

BACKWARD (d against float64 ON THE SAME bf16-rounded y and G, fp32 logits): the two row sums sum G y and sum q h are fp32 chains as above:
each errs by (ceil(n / 256) + 12) U sum |terms|; q_j carries the relative error of its normaliser and exponent, (c + 16 + l_range) U, which
moves q_j (h_j - sum q h) by that times q_j (1 + |h_j|); the two logs (2 ulp each, on values that are O(log n)) sit inside the same factor.  The result is stored as bf16: 2^-8 |d_j|.  So
    |d_j - d64_j| <= 2^-8 |d64_j| + 2 U [ (c + 12) (inv_tau |y_j| (|G_j| + sum |G y|) + k q_j (|h_j| + sum q |h|)) + (c + 8) k q_j (1 + |h_j|) (1 + l_range) ] + tiny
with c = ceil(n / 256), k = w_kl / N and l_range = max l - min l bounding the exponent's own rounding; `tiny` = 2^-126 covers a
flush of a subnormal result.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import dropout_ref
from tests.vq_reference import rows_of  # noqa: F401  (b c h w -> (b h w) c)

U = 2.0 ** -24
KEY_XOR = 0x47554D42
MASK64 = (1 << 64) - 1


def inv_tau32(tau: float) -> float:
    """the fp32 value of 1 / tau the launch passes"""
    return float(np.float32(1.0 / float(tau)))


# ---- noise ---------------------------------------------------------------------------------------------------------------------------
def noise_words(n_elems: int, seed: int, step: int, site: int) -> np.ndarray:
    """[n_elems] uint32: element e takes word e % 4 of Philox4x32-10 at counter (e / 4 lo, e / 4 hi, site, step lo), key (seed lo, seed hi ^ KEY_XOR)"""
    seed = (seed & MASK64) ^ (KEY_XOR << 32)
    return dropout_ref.philox_words((n_elems + 3) // 4, seed, step & MASK64, site).reshape(-1)[:n_elems]


def uniform_of(words: np.ndarray) -> np.ndarray:
    """u = (2 (w >> 9) + 1) 2^-24 in float64 (exact, and exactly an fp32 value): an odd 24-bit integer scaled, never 0 or 1"""
    return (2.0 * (words >> np.uint32(9)).astype(np.float64) + 1.0) * U


def noise64(rows: int, cols: int, seed: int, step: int, site: int) -> torch.Tensor:
    """float64 [rows, cols]: g = -log(-log(u)) of the generator of nk_gumbel_noise"""
    u = uniform_of(noise_words(rows * cols, seed, step, site))
    return torch.from_numpy(-np.log(-np.log(u))).view(rows, cols)


def noise_tol(g64: torch.Tensor) -> torch.Tensor:
    """|g - g64| <= 6 * 2^-23 (1 + |g64|): logf is inside the 3 ulp of the OpenCL full profile, applied twice (the inner one's relative
    error e on t = -log u moves log t by e: absolute, hence the 1 +), safety factor 2.  (The ROCm device-library documentation on the
    build machine states no tighter figure for logf than the OpenCL table.)"""
    return 6.0 * 2.0 ** -23 * (1.0 + g64.abs())


# ---- acceptable indices ----------------------------------------------------------------------------------------------------------------
def h4_of(h: int) -> int:
    return (h + 3) // 4 * 4


def abs_dot(rows: torch.Tensor, W: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|b_j| + sum_k |z_k w_jk|, float64 [N, n]"""
    return rows.double().abs() @ W.double().abs().T + b.double().abs()


def logit_bound(rows, W, b) -> torch.Tensor:
    return 2.0 * (h4_of(rows.shape[1]) + 6) * U * abs_dot(rows, W, b)


def logits64(rows, W, b) -> torch.Tensor:
    return rows.double() @ W.double().T + b.double()


def acceptable(rows, W, b, g):
    """(ok [N, n] bool, argmax64 [N], decided [N] bool) for latent rows [N, h], W [n, h], b [n] and noise g [N, n]"""
    s = logits64(rows, W, b) + g.double()
    bound = 2.0 * (h4_of(rows.shape[1]) + 6) * U * (abs_dot(rows, W, b) + g.double().abs())
    smax, jmax = s.max(dim=1)
    ok = s >= smax[:, None] - bound - bound.gather(1, jmax[:, None])
    return ok, jmax, ok.sum(1) == 1


def acceptable_scores(logits: torch.Tensor, g: torch.Tensor):
    """the rule for INJECTED fp32 logits (the row kernel's own input): s = fadd(l, g), a = fmul(s, inv_tau): two roundings,
    bound_j = 2 * 2 U (|l_j| + |g_j|)"""
    s = logits.double() + g.double()
    bound = 4.0 * U * (logits.double().abs() + g.double().abs())
    smax, jmax = s.max(dim=1)
    ok = s >= smax[:, None] - bound - bound.gather(1, jmax[:, None])
    return ok, jmax, ok.sum(1) == 1


# ---- the forward and its gradients in float64 -------------------------------------------------------------------------------------------------
def kl64(logits: torch.Tensor) -> torch.Tensor:
    """mean_rows sum_j q_j log(q_j n + 1e-10), q = softmax(logits) (reference quantize.py:136-137)"""
    q = torch.softmax(logits, dim=1)
    return (q * torch.log(q * logits.shape[1] + 1e-10)).sum(1).mean()


def h_of(q: torch.Tensor) -> torch.Tensor:
    """d/dq_j of sum_j q_j log(q_j n + 1e-10):  h_j = log(q_j n + 1e-10) + q_j n / (q_j n + 1e-10)"""
    x = q * q.shape[1]
    return torch.log(x + 1e-10) + x / (x + 1e-10)


def softmax_bwd64(logits, y, G, tau, w_kl) -> torch.Tensor:
    """nk_gumbel_softmax_bwd's formula in float64 on the given (bf16-valued) y and G"""
    l, y, G = logits.double(), y.double(), G.double()
    q = torch.softmax(l, dim=1)
    h = h_of(q)
    return inv_tau32(tau) * y * (G - (G * y).sum(1, keepdim=True)) + (w_kl / l.shape[0]) * q * (h - (q * h).sum(1, keepdim=True))


def restate64(z, W, b, E, g, tau, hard, kl_weight, upstream=None, w=1.0) -> dict:
    """GumbelQuantizer.forward (reference quantize.py:114-148) with injected noise g [N, n], in float64: z [B, h, H, W] or rows [N, h],
    W [n, h], b [n], E [n, d].  With `upstream` (shaped like z_q) also autograd's dz, dW, db, dE of <upstream, z_q> + w * loss.
    F.gumbel_softmax(hard=True) is y_hard - sg[y] + y."""
    four = z.ndim == 4
    rows = (rows_of(z, W.shape[1]) if four else z).double().clone().requires_grad_(True)
    W64, b64, E64 = (t.double().clone().requires_grad_(True) for t in (W, b, E))
    logits = rows @ W64.T + b64
    y = torch.softmax((logits + g.double()) * inv_tau32(tau), dim=1)
    idx = y.argmax(1)
    S = (torch.nn.functional.one_hot(idx, W.shape[0]).double() - y.detach()) + y if hard else y
    zq_rows = S @ E64
    loss = kl_weight * kl64(logits)

    def shaped(t, c):
        return t.view(z.shape[0], z.shape[2], z.shape[3], c).permute(0, 3, 1, 2) if four else t

    out = {"z_q": shaped(zq_rows, E.shape[1]).detach(), "loss": loss.detach(), "indices": idx, "logits": logits.detach(), "y": y.detach()}
    if upstream is not None:
        up = (rows_of(upstream, E.shape[1]) if four else upstream).double()
        dz, dW, db, dE = torch.autograd.grad((up * zq_rows).sum() + w * loss, (rows, W64, b64, E64))
        out.update(dz=shaped(dz, W.shape[1]), dW=dW, db=db, dE=dE)
    return out


# ---- tolerances --------------------------------------------------------------------------------------------------------------------------------
def softmax_tol(a64: torch.Tensor, y64: torch.Tensor) -> torch.Tensor:
    """|y - y64| allowed for the bf16 y of the row kernel (the SOFTMAX paragraph above); a64 the float64 scores (l + g) / tau"""
    n = a64.shape[1]
    amax = a64.max(1, keepdim=True).values
    rel = 2.0 * (2.0 * (a64.abs() + amax.abs()) + (a64 - amax).abs() + math.ceil(n / 256) + 16) * U
    return (2.0 ** -8 + rel) * y64 + 2.0 ** -126


def kl_tol(kl: float, n: int) -> float:
    return 2.0 * (n + 8) * U * max(abs(kl), 1.0)


def softmax_bwd_tol(logits, y, G, tau, w_kl, d64) -> torch.Tensor:
    """the BACKWARD paragraph above"""
    l, y, G = logits.double(), y.double(), G.double()
    N, n = l.shape
    c = math.ceil(n / 256)
    q = torch.softmax(l, dim=1)
    h = h_of(q)
    k = abs(w_kl) / N
    lr = (l.max(1, keepdim=True).values - l.min(1, keepdim=True).values)
    t1 = inv_tau32(tau) * y.abs() * (G.abs() + (G * y).abs().sum(1, keepdim=True))
    t2 = k * q * (h.abs() + (q * h.abs()).sum(1, keepdim=True))
    return 2.0 ** -8 * d64.abs() + 2.0 * U * ((c + 12) * (t1 + t2) + (c + 8.0) * k * q * (1.0 + h.abs()) * (1.0 + lr)) + 2.0 ** -126
