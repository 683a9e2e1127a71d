"""Float64 references, per-element error bounds and the shared inputs for the two factored optimizers: csrc/optim.hip (Adafactor) and
csrc/came.hip (CAME), both on the factored-statistics core of csrc/optim_common.h.  Shared by test_optim_kernels_gpu.py (the kernels,
through FlatAdafactor / FlatCAME, against float64) and test_optim_bounds_cpu.py (the bounds against an fp32 restatement of every pass, with
and without planted errors).  Pure torch, no GPU.

Single-step chaining: a reference step starts from the fp32 masters and the fp32 optimizer state as the device holds them, so every
bound is a one-step bound and nothing compounds.  `adafactor_expected` / `came_expected` return {output: (float64 reference, bound)} for
one tensor; the references are the float64 restatements of oracle/adafactor_oracle.py (below) and tests/test_came_cpu.py::came_ref_step.

How the bounds are made.  The kernels' arithmetic is restated operation by operation on pairs `V` = (float64 value, bound on the
kernel's absolute error against it).  Every operation propagates its operands' bounds to first order (divisors and radicands with their
bound taken off, so those steps are rigorous) and adds its own rounding:
  U = 2^-24 |result|  per fp32 multiply, add, subtract, correctly rounded divide and sqrtf (the library is built without fast-math:
      clang's HIP default keeps fp32 divide and sqrt correctly rounded); nothing where an operand is exactly 1 or exactly 0;
  RSQ_ULPS = 1 ulp = 2 U  for rsqrtf (v_rsq_f32; the documented accuracy of the instruction and of HIP's rsqrtf, not a count);
  U |c|  for a constant that reaches the kernel as a C float and is not fp32-representable (beta, 1 - beta, lr, eps, clip, grad_scale:
      the references take the double values, as the oracles do);
  depth * U * sum |terms|  for a sum whose terms pass through at most `depth` additions.  The depths are the kernels' real orders:
      row sum        4 serial terms per lane + the 4-step shuffle tree over the 16 column lanes + ntc serial partials   (8 + ntc)
      column sum     16 serial rows per lane + 16 serial LDS rows + ntr serial partials                               (32 + ntr)
      mean of rows   block_sum_256 (6 butterfly steps, two levels of pair sums) + ntr serial slots                     (8 + ntr)
      u^2, p^2       the thread's serial chain (64 for a tile, 4 KH KW for conv pairs, 4 for a vector) + block_sum_256 (8), then
                     in the tensor's last block ceil(nitems / 256) serial partials + block_sum_256 (8)
      conv pair      KW - 1, KH - 1 (the first addition is to zero).
All statistics are sums of positive terms (g^2 + eps, u^2, p^2, (u - m)^2 + eps, the EMAs), so these are relative bounds of a few tens
of U; the one difference that can cancel (CAME's u_hat - m) is charged to its operands' bounds.  SAFETY = 1.25 (tests/attention_bounds.py)
covers the second-order terms.  A compiler-fused multiply-add only removes roundings.  No constant was fitted to the kernels.

What the honest bound of p_new is: the update passes through both factors, the mean, the clip denominator and the step size.  With zero
masters that is, relative to the update, 32 U for Adafactor's vectors, 81 U for its 3 x 3 convs and 167 U for its matrices at best, and
for CAME, whose update passes through a second pair of factors made of the squared difference u_hat - m, 36 U for vectors and up to
about 900 U for matrices (test_optim_bounds_cpu.py prints them); two fp32 ulps (4 U) cannot be told from rounding there.  The two-ulp plant of
test_optim_bounds_cpu.py therefore goes to an output whose bound allows it -- a vector's second moment on the first step (beta2_t = 0,
grad_scale = 1: one square and one sum, 2 U) -- and the file says so.

The largest error / bound per output on the MI355X and by the fp32 restatement (both print "[optim ratio] ...") stand in the docstring of
tests/test_optim_kernels_gpu.py, next to the test that prints them: 0.06 to 0.8, the same on both sides.
"""
import functools
import math

import torch

from oracle import adafactor_oracle as AO
from tests import attention_bounds as ab
from tests.test_came_cpu import came_ref_step

U, SAFETY = ab.U, ab.SAFETY
F64, F32 = torch.float64, torch.float32
RSQ_ULPS = 1           # rsqrtf = v_rsq_f32: 1 ulp (documented instruction accuracy)
AF_TR, AF_TC, AF_CONV_PAIRS, AF_VEC = 256, 64, 1024, 1024
FIN = 8                # block_sum_256: six butterfly steps and (r0 + r1) + (r2 + r3)


def f32(v):
    """the value a C float argument holds"""
    return float(torch.tensor(v, dtype=F32))


# ================================================================================================================================
# values with error bounds
# ================================================================================================================================
class V:
    """a float64 value and a bound on the kernel's absolute error against it (same shape)"""

    def __init__(self, ref, err=0.0):
        ref, err = torch.as_tensor(ref, dtype=F64), torch.as_tensor(err, dtype=F64)
        self.ref, self.err = (t.contiguous() for t in torch.broadcast_tensors(ref, err))

    def _is(self, c):
        return (self.ref == c) & (self.err == 0)

    def map(self, f):
        return V(f(self.ref), f(self.err))


def const(c):
    """a C float argument: the reference takes the double, the kernel its fp32 rounding"""
    return V(c, 0.0 if f32(c) == c else U * abs(c))


def _rounded(ref, exact):
    return torch.where(exact, torch.zeros_like(ref), U * ref.abs())


def mul(a, b):
    ref = a.ref * b.ref
    a, b = V(a.ref + 0 * ref, a.err), V(b.ref + 0 * ref, b.err)
    err = a.ref.abs() * b.err + b.ref.abs() * a.err + a.err * b.err
    return V(ref, err + _rounded(ref, a._is(1) | b._is(1) | a._is(0) | b._is(0)))


def add(a, b):
    ref = a.ref + b.ref
    a, b = V(a.ref + 0 * ref, a.err), V(b.ref + 0 * ref, b.err)
    return V(ref, a.err + b.err + _rounded(ref, a._is(0) | b._is(0)))


def sub(a, b):
    return add(a, V(-b.ref, b.err))


def div(a, b):
    ref = a.ref / b.ref
    a, b = V(a.ref + 0 * ref, a.err), V(b.ref + 0 * ref, b.err)
    assert bool((b.ref.abs() > b.err).all()), "divisor not bounded away from zero"
    err = (a.err + ref.abs() * b.err) / (b.ref.abs() - b.err)
    return V(ref, err + _rounded(ref, b._is(1) | a._is(0)))


def _rel(a):
    assert bool((a.ref > a.err).all()), "radicand not bounded away from zero"
    return a.err / (a.ref - a.err)


def rsqrt(a):
    ref = a.ref.rsqrt()
    return V(ref, ref * (0.5 * _rel(a) + 2 * RSQ_ULPS * U))


def sqrt(a):
    """sqrtf of a non-negative value (a zero stays within sqrt of its bound)"""
    ref = a.ref.sqrt()
    pos = a.ref > a.err
    safe = V(torch.where(pos, a.ref, torch.ones_like(a.ref)), torch.where(pos, a.err, torch.zeros_like(a.err)))
    return V(ref, torch.where(pos, ref * (0.5 * _rel(safe) + U), (a.ref + a.err).sqrt() * (1 + U)))


def fmax(a, b):
    """fmaxf: the larger reference; the kernel may pick either where they are closer than their bounds"""
    return V(torch.maximum(a.ref, b.ref), torch.maximum(a.err, b.err))


def psum(a, dim, depth):
    """a sum over `dim` (None: everything) whose terms pass through at most `depth` fp32 additions"""
    kw = {} if dim is None else {"dim": dim}
    return V(a.ref.sum(**kw), a.err.sum(**kw) + depth * U * (a.ref.abs() + a.err).sum(**kw))


def unsq(a, dim):
    return a.map(lambda t: t.unsqueeze(dim))


# ================================================================================================================================
# the host planner's partition of a tensor (neurosis_amd/optim.py::_plan_tables) and the serial chains it implies
# ================================================================================================================================
def nitems_of(shape):
    if len(shape) == 2:
        return math.ceil(shape[0] / AF_TR) * math.ceil(shape[1] / AF_TC)
    if len(shape) == 4:
        return math.ceil(shape[0] * shape[1] / AF_CONV_PAIRS)
    return math.ceil(shape[0] / AF_VEC)


def chain_of(shape):
    """serial additions of one thread's partial sum of u^2 / p^2 over a work item"""
    if len(shape) == 2:
        return (AF_TR // 16) * 4
    if len(shape) == 4:
        return (AF_CONV_PAIRS // 256) * shape[2] * shape[3]
    return AF_VEC // 256


def tensor_sum_depth(shape):
    return chain_of(shape) + FIN + math.ceil(nitems_of(shape) / 256) + FIN


# ================================================================================================================================
# the factored statistics (optim_common.h), shared by both optimizers
# ================================================================================================================================
def _ema(old, beta, x, omb):
    return add(mul(V(old), beta), mul(x, omb))


def _scaled_grad(g, grad_scale, eps1):
    """g' = g grad_scale and q = g'^2 + eps1: grad_scale enters g' once and q squared"""
    gg = mul(V(g), const(grad_scale))
    return gg, add(mul(gg, gg), const(eps1))


def _matrix_stats(q, old_row, old_col, beta, omb):
    d0, d1 = q.ref.shape
    ntr, ntc = math.ceil(d0 / AF_TR), math.ceil(d1 / AF_TC)
    row = _ema(old_row, beta, div(psum(q, 1, 8 + ntc), V(float(d1))), omb)
    col = _ema(old_col, beta, div(psum(q, 0, 32 + ntr), V(float(d0))), omb)
    mean = div(psum(row, 0, FIN + ntr), V(float(d0)))
    return row, col, mean


def _matrix_factor(row, col, mean):
    """rsqrt(row / mean row) * rsqrt(col), [d0, d1]"""
    return mul(unsq(rsqrt(div(row, mean)), 1), unsq(rsqrt(col), 0))


def _conv_stats(q, old_row, old_col, beta, omb):
    """logical [O, I, KH, KW]: row statistics [O, I, KH] (mean over KW), column statistics [O, I, KW] (mean over KH)"""
    KH, KW = q.ref.shape[2:]
    row = _ema(old_row, beta, div(psum(q, 3, KW - 1), V(float(KW))), omb)
    col = _ema(old_col, beta, div(psum(q, 2, KH - 1), V(float(KH))), omb)
    return row, col


def _conv_factor(row, col):
    KH = row.ref.shape[2]
    mean = div(psum(row, 2, KH - 1), V(float(KH)))
    return mul(unsq(rsqrt(div(row, unsq(mean, 2))), 3), unsq(rsqrt(col), 2))


def _numel(shape):
    return float(math.prod(shape))


def _out(v):
    return v.ref, SAFETY * v.err


# ================================================================================================================================
# Adafactor: one float64 step of one tensor (oracle/adafactor_oracle.py and the header of csrc/optim.hip)
# ================================================================================================================================
AF_DEFAULTS = dict(lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, weight_decay=0.0, scale_parameter=True,
                   relative_step=True, warmup_init=False)


def adafactor_ref_step(p, g, st, step, grad_scale=1.0, **kw):
    """Plain float64 Adafactor step of one tensor from the state `st` (the reference's keys, not modified): returns
    {"p", "lr_t", "scale", "denom", and "row" + "col" or "v"}.  `_get_lr` is the oracle's own (AO.rel_lr)."""
    h = {**AF_DEFAULTS, **kw}
    p, g = p.double(), g.double() * grad_scale
    beta = 1.0 - math.pow(step, h["decay_rate"])
    rms_p = float(p.norm() / math.sqrt(p.numel()))
    lr_t = AO.rel_lr(step, rms_p, h["lr"], h["eps"][1], h["scale_parameter"], h["relative_step"], h["warmup_init"])
    q = g * g + h["eps"][0]
    out = {}
    if p.dim() >= 2:
        row = beta * st["exp_avg_sq_row"].double() + (1 - beta) * q.mean(-1)
        col = beta * st["exp_avg_sq_col"].double() + (1 - beta) * q.mean(-2)
        u = (row / row.mean(-1, keepdim=True)).rsqrt().unsqueeze(-1) * col.unsqueeze(-2).rsqrt() * g
        out["row"], out["col"] = row, col
    else:
        v = beta * st["exp_avg_sq"].double() + (1 - beta) * q
        u = v.rsqrt() * g
        out["v"] = v
    denom = max(1.0, float(u.norm() / math.sqrt(u.numel())) / h["clip_threshold"])
    scale = lr_t / denom
    out.update(p=p * (1.0 - h["weight_decay"] * lr_t) - scale * u, lr_t=torch.tensor(lr_t, dtype=F64), scale=torch.tensor(scale, dtype=F64),
               denom=torch.tensor(denom, dtype=F64))
    return out


def _agree(name, mine, ref, cancels=0.0):
    """the error-tracking restatement and the plain reference are the same function (`cancels`: the magnitude of the terms of a
    difference, whose float64 roundings are absolute)"""
    assert torch.allclose(mine, ref, rtol=1e-11, atol=1e-290 + 1e-13 * cancels), f"{name}: the bound's reference and the float64 reference differ"


def adafactor_expected(p, g, st, step, grad_scale=1.0, **kw):
    """{output: (float64 reference, bound)} of one FlatAdafactor step of one tensor (logical shapes; conv [O, I, KH, KW]) from the fp32
    master `p`, gradient `g` and state `st` under the reference's keys: p, lr_t, scale, and row + col (factored) or v"""
    h = {**AF_DEFAULTS, **kw}
    shape = tuple(p.shape)
    beta = const(1.0 - math.pow(step, h["decay_rate"]))
    omb = sub(V(1.0), beta)
    gg, q = _scaled_grad(g, grad_scale, h["eps"][0])
    out = {}
    if len(shape) == 2:
        row, col, mean = _matrix_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], beta, omb)
        u = mul(_matrix_factor(row, col, mean), gg)
        out["row"], out["col"] = row, col
    elif len(shape) == 4:
        row, col = _conv_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], beta, omb)
        u = mul(_conv_factor(row, col), gg)
        out["row"], out["col"] = row, col
    else:
        v = _ema(st["exp_avg_sq"], beta, q, omb)
        u = mul(gg, rsqrt(v))
        out["v"] = v
    depth, numel = tensor_sum_depth(shape), V(_numel(shape))
    P = V(p)
    rms_u = sqrt(div(psum(mul(u, u), None, depth), numel))
    denom = fmax(div(rms_u, const(h["clip_threshold"])), V(1.0))
    rms_p = div(sqrt(psum(mul(P, P), None, depth)), sqrt(numel))
    rel = AO.rel_lr(step, 1.0, h["lr"], 1.0, False, h["relative_step"], h["warmup_init"])
    lr_t = mul(fmax(rms_p, const(h["eps"][1])) if h["scale_parameter"] else V(1.0), const(rel))
    scale = div(lr_t, denom)
    decay = sub(V(1.0), mul(const(h["weight_decay"]), lr_t))
    out.update(p=sub(mul(P, decay), mul(scale, u)), lr_t=lr_t, scale=scale)
    ref = adafactor_ref_step(p, g, st, step, grad_scale, **kw)
    for k, v in out.items():
        _agree(k, v.ref, ref[k], float(max(p.abs().max(), ref["p"].abs().max())) if k == "p" else 0.0)
    return {k: _out(v) for k, v in out.items()}


def p2_expected(p, shape):
    """RMS(p) from the partial sums of p^2 that pass C leaves for the next step (summed in float64 by the test): p is exact, one square
    and the thread's chain + block_sum_256 per partial; the square root halves it"""
    rms = float(p.double().norm() / math.sqrt(p.numel()))
    return torch.tensor(rms, dtype=F64), torch.tensor(SAFETY * 0.5 * (chain_of(shape) + FIN + 1) * U * rms, dtype=F64)


# ================================================================================================================================
# CAME: one float64 step of one tensor (tests/test_came_cpu.py::came_ref_step) with the kernels' bounds (csrc/came.hip)
# ================================================================================================================================
CAME_DEFAULTS = dict(lr=2e-4, betas=(0.9, 0.999, 0.9999), weight_decay=0.0, weight_decouple=True, fixed_decay=False, clip_threshold=1.0,
                     eps1=1e-30, eps2=1e-16)
CAME_KEYS = {"exp_avg": "exp_avg", "R": "exp_avg_sq_row", "C": "exp_avg_sq_col", "Rr": "exp_avg_res_row", "Cr": "exp_avg_res_col", "v": "exp_avg_sq"}


def came_expected(p, g, st, grad_scale=1.0, **kw):
    """{output: (float64 reference, bound)} of one FlatCAME step of one tensor from the fp32 master, gradient and state `st` (the
    reference's keys, not modified): p, exp_avg, denom, and R, C, Rr, Cr (factored) or v"""
    h = {**CAME_DEFAULTS, **kw}
    shape = tuple(p.shape)
    b1, b2, b3 = (const(b) for b in h["betas"])
    o1, o2, o3 = (const(1.0 - b) for b in h["betas"])          # the host passes float(1.0 - beta)
    lr = const(h["lr"])
    decay = const(1.0 - h["weight_decay"] * (1.0 if h["fixed_decay"] else h["lr"]))
    gg, q = _scaled_grad(g, grad_scale, h["eps1"])
    out = {}
    if len(shape) == 2:
        R, C, mean = _matrix_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], b2, o2)
        u = mul(_matrix_factor(R, C, mean), gg)
    elif len(shape) == 4:
        R, C = _conv_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], b2, o2)
        u = mul(_conv_factor(R, C), gg)
    else:
        v = _ema(st["exp_avg_sq"], b2, q, o2)
        u = mul(rsqrt(v), gg)
        out["v"] = v
    rms = div(sqrt(psum(mul(u, u), None, tensor_sum_depth(shape))), sqrt(V(_numel(shape))))
    denom = fmax(div(rms, const(h["clip_threshold"])), V(1.0))
    uh = div(u, denom)
    m = _ema(st["exp_avg"], b1, uh, o1)
    P = V(p)
    if len(shape) == 1:
        pn = sub(mul(P, decay), mul(m, lr))
    else:
        d = sub(uh, m)
        res = add(mul(d, d), const(h["eps2"]))
        if len(shape) == 2:
            Rr, Cr, mean = _matrix_stats(res, st["exp_avg_res_row"], st["exp_avg_res_col"], b3, o3)
            f = _matrix_factor(Rr, Cr, mean)
        else:
            Rr, Cr = _conv_stats(res, st["exp_avg_res_row"], st["exp_avg_res_col"], b3, o3)
            f = _conv_factor(Rr, Cr)
        pn = sub(mul(P, decay), mul(mul(f, m), lr))
        out.update(R=R, C=C, Rr=Rr, Cr=Cr)
    out.update(p=pn, exp_avg=m, denom=denom)
    rst = {k: v.clone() for k, v in st.items()}
    want = came_ref_step(p, g.double() * grad_scale, rst, **kw)
    _agree("p", pn.ref, want, float(max(p.abs().max(), want.abs().max())))
    for k, v in out.items():
        if k in CAME_KEYS:
            _agree(k, v.ref, rst[CAME_KEYS[k]])
    return {k: _out(v) for k, v in out.items()}


def zero_state(shape, came):
    """the optimizer state before the first step, under the reference's keys and in its logical shapes"""
    st = {"exp_avg": torch.zeros(shape)} if came else {}
    if len(shape) >= 2:
        for k in ("exp_avg_sq",) + (("exp_avg_res",) if came else ()):
            st[k + "_row"], st[k + "_col"] = torch.zeros(shape[:-1]), torch.zeros(shape[:-2] + shape[-1:])
    else:
        st["exp_avg_sq"] = torch.zeros(shape)
    return st


# ================================================================================================================================
# the shared inputs: the smallest shapes that reach every edge of the core, in one store
# ================================================================================================================================
MATRICES = [(1, 4), (255, 60), (256, 64), (257, 68), (513, 132), (300, 8), (3, 1284)]
CONVS = [(33, 31, 3, 3), (32, 32, 3, 3), (41, 25, 3, 3), (8, 16, 1, 1), (8, 8, 1, 3), (8, 8, 3, 1), (8, 8, 2, 2), (8, 8, 2, 3)]
VECTORS = [(1,), (7,), (1023,), (1024,), (1025,), (2049,)]
# kinds interleaved, so that a small chunk size puts tensors of every kind into a second and a third chunk
SHAPES = [s for trio in zip(MATRICES, CONVS, VECTORS) for s in trio] + [MATRICES[6], CONVS[6], CONVS[7]]
CHUNK_BYTES = 40 << 10
STEPS = 3
ZERO_LINES = ((257, 68), 100, 65)      # this matrix has an all-zero gradient row and column on every step (the eps1 path: q = 1e-30)
ZERO_GRAD = {1: ((300, 8), (7,))}      # step index -> tensors whose whole gradient is zero on that step
STEP_MAG = (1.0, 30.0, 0.03)           # the second step's gradients are large (clip denominator > 1), the third's small (exactly 1)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def inputs():
    """(init, grads): fp32 masters N(0, 0.05^2) per tensor of SHAPES, and STEPS gradient sets whose normal values are spread over
    10^-2 .. 10^2 per element (times STEP_MAG), with the zero row / column and the zero tensors above"""
    init = [torch.randn(*s, generator=_gen(100 + i)) * 0.05 for i, s in enumerate(SHAPES)]
    grads = []
    for t in range(STEPS):
        gs = []
        for i, s in enumerate(SHAPES):
            g = torch.randn(*s, generator=_gen(1000 * (t + 1) + i))
            g = g * 10.0 ** torch.randint(-2, 3, s, generator=_gen(5000 * (t + 1) + i)).float() * STEP_MAG[t]
            if s == ZERO_LINES[0]:
                g[ZERO_LINES[1], :] = 0.0
                g[:, ZERO_LINES[2]] = 0.0
            if s in ZERO_GRAD.get(t, ()):
                g.zero_()
            gs.append(g)
        grads.append(gs)
    return init, grads


AF_CASES = {
    # masters zeroed before every step: p_new = -scale u, rounded once; lr_t sits on the eps2 floor of scale_parameter
    "zero": dict(kwargs=dict(scale_parameter=True, relative_step=True, warmup_init=False), zero=True, grad_scale=1.0),
    # |update| = lr |u| ~ 3e-2 against |p| ~ 5e-2; weight decay on; grad_scale != 1
    "manual": dict(kwargs=dict(lr=3e-2, relative_step=False, scale_parameter=False, weight_decay=0.1), zero=False, grad_scale=0.37),
    # |update| = 1e-2 RMS(p) |u|; weight decay on
    "relative": dict(kwargs=dict(scale_parameter=True, relative_step=True, warmup_init=False, weight_decay=1e-2), zero=False, grad_scale=1.0),
    # the warm-up regime: the update is below an ulp of most masters; lr_t, scale and the states carry the check, and p must move
    "warmup": dict(kwargs=dict(scale_parameter=True, relative_step=True, warmup_init=True), zero=False, grad_scale=1.0),
}
CAME_CASES = {
    "zero": dict(kwargs=dict(lr=1e-2), zero=True, grad_scale=1.0),
    "decay": dict(kwargs=dict(lr=3e-2, weight_decay=0.1), zero=False, grad_scale=1.0),
    "fixed": dict(kwargs=dict(lr=3e-2, betas=(0.9, 0.99, 0.999), weight_decay=1e-2, fixed_decay=True), zero=False, grad_scale=0.37),
}


# ================================================================================================================================
# the comparison (one comparer: _check of tests/test_text_encoder_train_gpu.py) and the ratio log
# ================================================================================================================================
RATIOS = {}      # (optimizer, output) -> largest error / bound seen by verify() in this process


def verify(who, label, got, expected, check, record=True):
    """`check` (the suite's _check) on every output of `expected` that `got` must have; records the worst error / bound per output"""
    for name, (ref, bound) in expected.items():
        g = torch.as_tensor(got[name]).detach().cpu().to(F64).reshape(ref.shape)
        if record and g.numel():
            worst = float(((g - ref).abs() / bound.clamp_min(1e-300)).max())
            RATIOS[(who, name)] = max(RATIOS.get((who, name), 0.0), worst)
        check(f"{label} {name}", g, ref, bound)


def report(who):
    for (w, name), r in sorted(RATIOS.items()):
        if w == who:
            print(f"[optim ratio] {who} {name}: largest error / bound {r:.3f}")


def must_move(p0, ref, bound):
    """the masters a step cannot leave where they were: the reference update exceeds its bound by more than an ulp of p"""
    return (ref - p0.double()).abs() > bound + 2.0 ** -23 * p0.double().abs()
