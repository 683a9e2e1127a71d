"""Float64 references, per-element error bounds and the shared inputs for the hand-written glue kernels: the second half of
csrc/elementwise.hip (row softmax and its backward, EDM prepare / loss, AdamW, the timestep embedding), csrc/sampling.hip and
nk_ema_flat of csrc/optim.hip.  Shared by test_glue_kernels_gpu.py (the kernels against float64) and test_glue_bounds_cpu.py (the
bounds against an fp32 restatement of each kernel, with and without planted errors).  Pure torch, no GPU.

Conventions (those of tests/attention_bounds.py): U = 2^-24 per fp32 rounding; a sum or difference that can cancel is charged to the
MAGNITUDES of its terms, never to its result; a bf16 output adds one final half bf16 ulp of (|ref| + bound); SAFETY = 1.25 covers the
second-order terms.  Every count below is read from the kernel source and allows the compiler to contract a multiply-add into one
fused operation (which only removes roundings).  A C `float` argument holds f32(value): the references take that value.
Every *_expected function returns {output name: (float64 reference, bound)}; a padding channel has reference 0 and bound 0, so the
one comparer (`_check`) rejects anything but a zero there.

  softmax   e_j = __expf(x_j - max): the subtraction rounds once, the fast exponential is v_exp_f32(d * log2 e): the product and the
            fp32 constant move the exponent by 2 U |d log2 e|, i.e. e_j by 2 U |d| relative, and the instruction itself is good to
            EXP_ULPS = 1 ulp = 2 U (the documented accuracy of v_exp_f32, not a count of roundings): eps_j = (3 |d_j| + 2) U, and a
            result below 2^-126 may be flushed (TINY, absolute).  The fp32 sum of non-negative terms: a serial chain of 8 NPT adds per
            thread (8 ceil(L / 2048) in the general kernel), six butterfly steps, three adds of the four partials: gamma = (chain + 9) U
            relative, on top of the p-weighted mean ebar of eps_j.  The reciprocal and the product round once each:
            |p~ - p| <= p (eps_j + ebar + gamma + 2 U) + TINY.
  softmax'  dS_j = p_j (dp_j - dot) scale, dot = sum p dp: chain + 9 adds and one rounding per product, charged to sum |p dp|;
            the difference, the two products: 3 U (|dp_j| + sum |p dp|).  Absolute: where dp is constant along a row dS cancels to ~0.
  prepare   z = x + sigma eps: at most two roundings, 2 U (|x| + |sigma eps|); net_in = bf16(z c_in): |c_in| times that, one rounding.
  loss      D = net c_out + z c_skip (2 U (a + b), a = |net c_out|, b = |z c_skip|), diff = D - target (U (a + b + |t|)):
            delta = 3 U (a + b + |t|) ABSOLUTE per element.  dnet = diff g, g = upstream w 2 / (C HW) c_out: four roundings in g, one
            product: |g| delta + 5 U |ref|.  loss: each term diff^2 is off by 2 |diff| delta + delta^2; the sum of non-negative terms
            runs a chain of ceil(HW / 1024) C fused adds per thread, six butterfly steps and 16 partials: gamma = (chain + 22) U
            relative; the reciprocal count and two products 3 U more.  (So the loss bound cannot be below ~30 U: the planted
            two-ulp error is applied to the per-element outputs.)
  sampler   F = F_u + s (F_c - F_u): the difference and its product round once each, relative to |s (F_c - F_u)|, the sum relative to
            its result: dF = U (2 |s| |F_c - F_u| + |F|) (under guidance 7.5 that alone is ~20 U of the halves' distance: more than
            two fp32 ulps of F).  D = c_skip x + c_out F: dD = |c_out| dF + U (|c_out F| + |c_skip x|) + U |D|: the kernel factors x
            out of the reference's D_u + s (D_c - D_u), the same value, so the bound is the kernel's own and charges the
            cancellation between the two products to their magnitudes.  Euler: r = x - D inherits dD and rounds, d = r / sigma_hat,
            dt = sigma_next - sigma_hat and dt d round once each, all relative to the step, then x' = x + dt d rounds relative to
            its result: |dt / sigma_hat| dD + 4 U |dt d| + U |x'|.  sample_prepare: one product, one bf16 rounding.
  adamw     g' = g grad_scale; m' = b1 m + (1 - b1) g': 2 U |b1 m| + 4 U |(1 - b1) g'| absolute; v' = b2 v + (1 - b2) g'^2:
            2 U b2 v + 6 U (1 - b2) g'^2 + TINY (g'^2 may underflow); the host's bc = 1 - powf(b, t): powf to 1 ulp and the
            subtraction, rho = (2 U b^t + U bc) / bc relative; m' / bc1: dm / bc1 + |mhat| (rho1 + U); sqrt(v' / bc2) + eps: relative
            (dv / v' + rho2 + U) / 2 + 2 U; the quotient U; p' = p (1 - lr wd) - lr upd: 3 U |p| + lr d_upd + 2 U lr |upd|.
  ema       e' = e - omd (e - p): 2 U |omd (e - p)| + U |e'|.
  timestep  arg = t exp(a), a = -logf(P) k / half: logf to 1 ulp (2 U), the product and the quotient, so a carries 4 U |a|; expf 1 ulp:
            |d arg| <= (4 |a| + 3) U |arg|; cosf / sinf of a value <= 1 to 2 ulp: 4 U absolute (library accuracy, not counted).

Largest error / bound observed, MI355X | the fp32 restatement of tests/test_glue_bounds_cpu.py (printed by both tests as "[bound] ..."):
  nk_softmax_rows        softmax_rows_reg_kernel<2> 0.998 | 0.998, <4> 0.998 | 0.998, <8> 0.997 | 0.997, softmax_rows_kernel 0.997 | 0.997
  nk_softmax_rows_bwd    1.000 | 1.000
  nk_edm_prepare         z_t 0.482 | 0.829, net_in 1.000 | 1.000
  nk_edm_loss            loss 0.056 | 0.056, dnet 1.000 | 1.000
  nk_sample_prepare      1.000 | 1.000
  nk_sample_denoise      0.639 | 0.727        nk_sample_euler_step   x_next 0.559 | 0.586, denoised 0.639 | 0.727
  nk_adamw_flat          p 0.31 | 0.55, m 0.38 | 0.60, v 0.40 | 0.66        nk_ema_flat  0.797 | 0.797
  nk_timestep_embedding  0.999 | 0.999
Every bf16 output sits at ~1 on both sides: the leading term of its bound is the half ulp of the final rounding, and among thousands of
values some lie next to a tie, where a correctly rounded result is half an ulp off.  The figure says that no output is a whole ulp off; it
says nothing about the fp32 terms beneath, which the fp32 outputs of the same kernels (z_t, loss, the sampler, AdamW) show at 0.06 to 0.8.
The fp32 ratios above 0.5 (denoised, x_next, EMA) come from bounds of three to five roundings: with so few, a few elements in a thousand
have them all aligned, in the restatement as on the GPU (whose fused multiply-adds make it the lower of the two).  The constant of the fast
exponential (EXP_ULPS) is the documented accuracy of the instruction; it was not enlarged.
"""
import functools
import math

import numpy as np
import torch

from tests import attention_bounds as ab

U, SAFETY = ab.U, ab.SAFETY
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
TINY = 2.0 ** -126
EXP_ULPS = 1          # v_exp_f32: 1 ulp (documented instruction accuracy)
NAN = float("nan")


def f32(v):
    """the value a C float argument holds"""
    return float(torch.tensor(v, dtype=F32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=_gen(seed)) * scale


def _bf16_out(ref, pre):
    return ref, pre + ab.half_ulp(ref, pre)


def _tokens(nchw, Cpad, fill=0.0):
    """[B, C, HW] -> channels-last [B, HW, Cpad], padding channels = fill"""
    B, C, HW = nchw.shape
    out = torch.full((B, HW, Cpad), fill, dtype=nchw.dtype)
    out[:, :, :C] = nchw.permute(0, 2, 1)
    return out


def _pad_mask(B, HW, C, Cpad):
    m = torch.zeros(B, HW, Cpad, dtype=torch.bool)
    m[:, :, :C] = True
    return m


# ================================================================================================================================
# row softmax and its backward
# ================================================================================================================================
SOFTMAX_L = (8, 200, 2048, 2056, 4096, 4104, 8192, 8200, 16384, 16392, 18440)
SOFTMAX_M = (1, 3)
SOFTMAX_KINDS = ("normal", "equal", "dominant", "tail")
SOFTMAX_BWD_SHAPES = ((1, 8), (3, 200), (2, 2048), (2, 2056), (1, 16392))
SOFTMAX_BWD_SCALES = (1.0, 0.37)


def softmax_chain(L):
    """(kernel that nk_softmax_rows launches, serial adds per thread in its sum)"""
    for npt, top in ((2, 4096), (4, 8192), (8, 16384)):
        if L <= top:
            return f"softmax_rows_reg_kernel<{npt}>", 8 * npt
    return "softmax_rows_kernel", 8 * math.ceil(L / 2048)


def exp_term(d):
    """relative error of __expf(fp32(d)) against exp(d), d a difference of two bf16 values"""
    return (3 * d.abs() + 2 * EXP_ULPS) * U


@functools.lru_cache(maxsize=None)
def softmax_inputs(M, L, variant):
    """bf16 logits [M, L]; row r is of kind SOFTMAX_KINDS[(variant + r) % 4]: normal (sigma 4, and a 14 in the last 16-byte piece, so
    that the piece carries a tenth or more of the row's mass and, mostly, its maximum), all equal, one +80 among -80, normal with a
    tail of -60000 over the last 16-byte piece and half of the one before"""
    x = _randn(M, L, seed=1000 * L + 10 * M + variant, scale=4.0)
    for r in range(M):
        kind = SOFTMAX_KINDS[(variant + r) % 4]
        if kind == "normal":
            x[r, L - 3] = 14.0
        elif kind == "equal":
            x[r] = 1.375 * (r + 1)
        elif kind == "dominant":
            x[r] = -80.0
            x[r, (7 * L) // 11] = 80.0
        elif kind == "tail":
            x[r, L - min(12, L // 2):] = -60000.0
    return x.to(BF16)


def softmax_expected(x):
    M, L = x.shape
    xd = x.to(F64)
    d = xd - xd.amax(1, keepdim=True)
    p = torch.softmax(xd, 1)
    eps = exp_term(d)
    ebar = (p * eps).sum(1, keepdim=True)
    gamma = (softmax_chain(L)[1] + 9) * U
    return {"p": _bf16_out(p, SAFETY * (p * (eps + ebar + gamma + 2 * U) + TINY))}


@functools.lru_cache(maxsize=None)
def softmax_bwd_inputs(M, L, kind):
    """p = bf16(float64 softmax) [M, L] and dp [M, L] bf16: kind "random", or "const" (constant along each row: dS = 0 up to rounding)"""
    p = torch.softmax(_randn(M, L, seed=7 * L + M, scale=3.0).to(F64), 1).to(BF16)
    if kind == "const":
        dp = (torch.arange(M).double()[:, None] * 1.25 - 1.5).expand(M, L).contiguous()
    else:
        dp = _randn(M, L, seed=7 * L + M + 1, scale=2.0)
    return p, dp.to(BF16)


def softmax_bwd_expected(p, dp, scale):
    M, L = p.shape
    s = f32(scale)
    pd, dd = p.to(F64), dp.to(F64)
    dot = (pd * dd).sum(1, keepdim=True)
    mag = (pd * dd).abs().sum(1, keepdim=True)
    chain = 8 * math.ceil(L / 2048)
    ref = pd * (dd - dot) * s
    pre = SAFETY * abs(s) * pd * ((chain + 10) * U * mag + 3 * U * (dd.abs() + mag))
    return {"ds": _bf16_out(ref, pre)}


# ================================================================================================================================
# EDM prepare and loss
# ================================================================================================================================
EDM_PREPARE_SHAPES = ((1, 4, 1, 8), (3, 4, 30, 8), (2, 9, 257, 16), (2, 8, 33, 8), (2, 5, 7, 5))
EDM_LOSS_SHAPES = ((1, 4, 30, 8), (3, 4, 1025, 8), (2, 9, 64, 16), (2, 8, 2050, 8), (1, 3, 5, 3))
EDM_UPSTREAMS = (1.0, 0.25, -3.0)
SIGMA_DATA = 0.5


def _sigmas(B, seed):
    return torch.exp(_randn(B, seed=seed, scale=1.2) - 0.4).to(F32)


def _precond(sigma):
    """fp32 EDM coefficients (c_in, c_skip, c_out) of fp32 sigmas"""
    s2 = sigma * sigma + SIGMA_DATA ** 2
    return 1.0 / s2.sqrt(), SIGMA_DATA ** 2 / s2, sigma * SIGMA_DATA / s2.sqrt()


@functools.lru_cache(maxsize=None)
def edm_prepare_inputs(B, C, HW, Cpad):
    sigma = _sigmas(B, seed=B + C + HW)
    return dict(x=_randn(B, C, HW, seed=HW + 1), eps=_randn(B, C, HW, seed=HW + 2), sigma=sigma, c_in=_precond(sigma)[0])


def edm_prepare_expected(x, eps, sigma, c_in, Cpad):
    B, C, HW = x.shape
    sg, ci = sigma.to(F64)[:, None, None], c_in.to(F64)[:, None, None]
    noise = sg * eps.to(F64)
    z = x.to(F64) + noise
    zb = 2 * U * (x.to(F64).abs() + noise.abs())
    n = z * ci
    nref, nb = _bf16_out(_tokens(n, Cpad), _tokens(ci.abs() * zb + U * n.abs(), Cpad))
    return {"zt": (z, zb), "net_in": (nref, torch.where(_pad_mask(B, HW, C, Cpad), nb, torch.zeros_like(nb)))}


@functools.lru_cache(maxsize=None)
def edm_loss_inputs(B, C, HW, Cpad, kind):
    """kind "plain": independent draws; "cancel": target = fp32(D), the difference is rounding only.  The padding channels of net_out
    are NaN (nothing may read them); the last of several samples has w = 0."""
    sigma = _sigmas(B, seed=2 * B + C + HW)
    _, c_skip, c_out = _precond(sigma)
    net = _randn(B, C, HW, seed=HW + 3).to(BF16)
    zt = _randn(B, C, HW, seed=HW + 4) * (1 + sigma)[:, None, None]
    target = _randn(B, C, HW, seed=HW + 5)
    if kind == "cancel":
        target = (net.to(F64) * c_out.to(F64)[:, None, None] + zt.to(F64) * c_skip.to(F64)[:, None, None]).to(F32)
    w = (1.0 / (sigma * sigma) + 4.0).to(F32)
    if B > 1:
        w[B - 1] = 0.0
    return dict(net_out=_tokens(net, Cpad, NAN), zt=zt, target=target, c_out=c_out, c_skip=c_skip, w=w)


def edm_loss_expected(net_out, zt, target, c_out, c_skip, w, C, upstream):
    B, HW, Cpad = net_out.shape
    up = f32(upstream)
    co, cs, wd = (t.to(F64)[:, None, None] for t in (c_out, c_skip, w))
    net = net_out[:, :, :C].to(F64).permute(0, 2, 1).contiguous().requires_grad_(True)      # [B, C, HW]
    a, b = net * co, zt.to(F64) * cs
    diff = a + b - target.to(F64)
    loss = w.to(F64) * (diff * diff).mean((1, 2))
    (up * loss.sum()).backward()
    grad, diff, a, b, loss = net.grad, diff.detach(), a.detach().abs(), b.abs(), loss.detach()
    delta = 3 * U * (a + b + target.to(F64).abs())
    cnt = C * HW
    g = (up * wd * 2.0 / cnt * co).abs()
    dref, db = _bf16_out(_tokens(grad, Cpad), _tokens(SAFETY * (g * delta + 5 * U * grad.abs()), Cpad))
    gamma = (math.ceil(HW / 1024) * C + 22 + 3) * U
    T = (diff * diff).sum((1, 2))
    lb = SAFETY * w.to(F64).abs() / cnt * (gamma * T + (1 + gamma) * (2 * diff.abs() * delta + delta * delta).sum((1, 2))) + U * loss.abs()
    return {"loss": (loss, lb), "dnet": (dref, torch.where(_pad_mask(B, HW, C, Cpad), db, torch.zeros_like(db)))}


# ================================================================================================================================
# sampler
# ================================================================================================================================
SAMPLE_SHAPES = ((1, 4, 1, 8), (3, 4, 255, 8), (2, 9, 257, 16), (2, 8, 30, 8), (1, 16, 5, 16))
SAMPLE_REPS = (1, 2)
SAMPLE_SCALES = (0.0, 1.0, 7.5)
SAMPLE_KINDS = ("random", "equal", "opposite")


@functools.lru_cache(maxsize=None)
def sample_inputs(B, C, HW, Cpad, rep, kind):
    """x fp32 [B, C, HW]; net_out bf16 [rep B, HW, Cpad] laid out [unconditional | conditional], its padding channels NaN; kind "equal":
    both halves the same (F is exact), "opposite": F_c = -F_u; per-sample coefficients; the last of several samples steps to sigma_next = 0"""
    sigma = _sigmas(B, seed=3 * B + C + HW) + 0.05
    c_in, c_skip, c_out = _precond(sigma)
    nxt = (sigma * torch.linspace(0.8, 0.3, B)).to(F32)
    if B > 1:
        nxt[B - 1] = 0.0
    fu = _randn(B, C, HW, seed=HW + 6).to(BF16)
    fc = {"random": _randn(B, C, HW, seed=HW + 7).to(BF16), "equal": fu, "opposite": -fu}[kind]
    net = torch.cat([_tokens(f, Cpad, NAN) for f in ((fu, fc) if rep == 2 else (fc,))], 0)
    x = _randn(B, C, HW, seed=HW + 8) * (1 + sigma)[:, None, None]
    return dict(x=x, net_out=net, c_in=c_in, c_skip=c_skip, c_out=c_out, sigma_hat=sigma, sigma_next=nxt)


def sample_prepare_expected(x, c_in, Cpad, rep):
    B, C, HW = x.shape
    n = x.to(F64) * c_in.to(F64)[:, None, None]
    ref, bound = _bf16_out(_tokens(n, Cpad), _tokens(U * n.abs(), Cpad))
    bound = torch.where(_pad_mask(B, HW, C, Cpad), bound, torch.zeros_like(bound))
    return {"net_in": (ref.repeat(rep, 1, 1), bound.repeat(rep, 1, 1))}


def sample_expected(x, net_out, c_skip, c_out, sigma_hat, sigma_next, scale, rep):
    """denoised and the Euler step in the reference's order: D_u, D_c per half, D = D_u + s (D_c - D_u)"""
    B, C, HW = x.shape
    s = f32(scale)
    xd = x.to(F64)
    cs, co, sh, sn = (t.to(F64)[:, None, None] for t in (c_skip, c_out, sigma_hat, sigma_next))
    halves = [net_out[r * B:(r + 1) * B, :, :C].to(F64).permute(0, 2, 1) for r in range(rep)]
    if rep == 2:
        fu, fc = halves
        du, dc = fu * co + xd * cs, fc * co + xd * cs
        D = du + s * (dc - du)
        F = fu + s * (fc - fu)
        dF = U * (2 * abs(s) * (fc - fu).abs() + F.abs())
    else:
        F = halves[0]
        D = F * co + xd * cs
        dF = torch.zeros_like(F)
    dD = co.abs() * dF + U * ((co * F).abs() + (cs * xd).abs() + D.abs())
    r = xd - D
    step = (sn - sh) * (r / sh)
    xn = xd + step
    dxn = ((sn - sh) / sh).abs() * dD + 4 * U * step.abs() + U * xn.abs()
    return {"denoised": (D, SAFETY * dD), "x_next": (xn, SAFETY * dxn)}


# ================================================================================================================================
# AdamW, EMA
# ================================================================================================================================
FLAT_N = (4, 1028)
ADAMW_HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01, grad_scale=0.25)
ADAMW_STEPS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def adamw_inputs(n):
    """fp32 p, m, v (non-zero moments) and one gradient per step: 0, +-1e-12, 1e-25 (whose square underflows fp32), order one and 1e4"""
    special = torch.tensor([0.0, 1e-12, -1e-12, 1e-25])
    grads = []
    for t in ADAMW_STEPS:
        g = _randn(n, seed=n + t)
        g[1::3] *= 1e4
        g[torch.arange(n) % 7 == (t % 7)] = 0.0
        g[:4] = special.roll(t)
        grads.append(g)
    return dict(p=_randn(n, seed=n + 10), m=_randn(n, seed=n + 11, scale=0.1), v=torch.rand(n, generator=_gen(n + 12)) * 1e-2 + 1e-9, grads=grads)


def adamw_expected(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """one float64 step from the fp32 state (p, m, v)"""
    lr, b1, b2, eps, wd, gs = (f32(h) for h in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    gr = g * gs
    A, Bm = (b1 * m).abs(), ((1 - b1) * gr).abs()
    m1 = b1 * m + (1 - b1) * gr
    dm = 2 * U * A + 4 * U * Bm
    Bv = (1 - b2) * gr * gr
    v1 = b2 * v + Bv
    dv = 2 * U * b2 * v + 6 * U * Bv + TINY
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    rho1, rho2 = (2 * U * b1 ** step + U * bc1) / bc1, (2 * U * b2 ** step + U * bc2) / bc2
    mhat = m1 / bc1
    den = (v1 / bc2).sqrt() + eps
    upd = mhat / den
    dupd = (dm / bc1 + mhat.abs() * (rho1 + U)) / den + upd.abs() * ((dv / v1.clamp_min(TINY) + rho2 + U) / 2 + 3 * U)
    p1 = p * (1 - lr * wd) - lr * upd
    dp = 3 * U * p.abs() + lr * dupd + 2 * U * lr * upd.abs()
    return {"p": (p1, SAFETY * dp), "m": (m1, SAFETY * dm), "v": (v1, SAFETY * dv)}


@functools.lru_cache(maxsize=None)
def ema_inputs(n):
    p = _randn(n, seed=n + 20)
    return dict(ema=p + _randn(n, seed=n + 21, scale=1e-3), p=p)


def ema_expected(ema, p, omd):
    o = f32(omd)
    e, q = ema.to(F64), p.to(F64)
    step = o * (e - q)
    ref = e - step
    return {"ema": (ref, SAFETY * (2 * U * step.abs() + U * ref.abs()))}


# ================================================================================================================================
# timestep embedding
# ================================================================================================================================
TIMESTEP_SHAPES = ((1, 2), (4, 320), (3, 256), (5, 7), (2, 1280))
TIMESTEPS = (0.0, 1.0, 0.5, 37.25, 500.0, 999.0, 1024.0)
MAX_PERIODS = (10000.0, 100.0)


def timestep_expected(t, dim, max_period):
    """[cos | sin] of t * exp(-ln(P) k / half), an odd dim's last column exactly zero (reference 0, bound 0)"""
    half = dim // 2
    k = torch.arange(half, dtype=F64)
    a = -math.log(f32(max_period)) * k / half
    arg = t.to(F64)[:, None] * torch.exp(a)[None, :]
    darg = (4 * a.abs()[None, :] + 3) * U * arg.abs()
    ref = torch.zeros(t.shape[0], dim, dtype=F64)
    ref[:, :half], ref[:, half:2 * half] = torch.cos(arg), torch.sin(arg)
    pre = torch.zeros_like(ref)
    pre[:, :2 * half] = SAFETY * (torch.cat([darg, darg], 1) + 4 * U)
    bound = pre + ab.half_ulp(ref, pre)
    bound[:, 2 * half:] = 0.0
    return {"emb": (ref, bound)}


# ================================================================================================================================
# layout and casts (bit for bit: the references are torch's own roundings)
# ================================================================================================================================
LAYOUT_SHAPES = ((1, 3, 1, 8), (3, 4, 31, 8), (2, 33, 33, 40), (2, 70, 45, 72), (1, 8, 32, 8))
LAYOUT_SCALES = (1.0, 0.5, 0.13025)
CAST_N = (1, 7, 8, 9, 8 * 256 + 3)


def nchw_to_nhwc_reference(src, Cpad, scale):
    """bf16(fp32(src) * f32(scale)) as channels-last tokens [N, HW, Cpad]: the kernel's two roundings, so equality is expected"""
    prod = src.to(F32) * torch.tensor(scale, dtype=F32)
    return _tokens(prod.to(BF16), Cpad)


def cast_inputs(n):
    """fp32 values with +-0, subnormals, +-inf, NaN, ties to bf16 that round down and up, and the largest finite fp32 among normals"""
    special = torch.from_numpy(np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F808000,
                                         0x3F818000, 0xBF808000, 0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F807FFF, 0x3F808001, 0x7FA00001],
                                        dtype=np.uint32).view(np.float32).copy())
    x = _randn(n, seed=n, scale=3.0)
    k = min(n, special.numel())
    idx = torch.arange(k) if n <= special.numel() else torch.randperm(n, generator=_gen(n + 1))[:k]
    x[idx] = special.roll(n)[:k]
    return x


# ================================================================================================================================
# the comparison (one comparer: _check of tests/test_text_encoder_train_gpu.py) and the ratio log
# ================================================================================================================================
RATIOS = {}      # entry point -> largest error / bound seen by verify() in this process


def verify(entry, label, got, expected, check, record=True):
    """`check` (the suite's _check) on every output of `expected`; records the worst error-to-bound ratio per entry point"""
    for name, (ref, bound) in expected.items():
        g = got[name].detach().cpu()
        assert g.shape == ref.shape, (label, name, tuple(g.shape), tuple(ref.shape))
        if record and g.numel():
            worst = float(((g.to(F64) - ref).abs() / bound.clamp_min(1e-300)).max())
            RATIOS[entry] = max(RATIOS.get(entry, 0.0), worst)
        check(f"{label} {name}", g, ref, bound)


def report(entry):
    print(f"[glue ratio] {entry}: largest error / bound {RATIOS.get(entry, float('nan')):.3f}")
