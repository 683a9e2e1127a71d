"""Float64 reference and per-element bounds of the Adafactor step with the first moment (csrc/optim.hip: af_apply_momentum_kernel behind
the unchanged statistics passes), on the primitives of tests/optim_bounds.py.  Shared by test_adafactor_momentum_cpu.py (the fixture, the
fp32 restatement, the planted errors) and test_adafactor_momentum_gpu.py (the kernels through FlatAdafactorMomentum).  Pure torch, no GPU.

Single-step chaining as in optim_bounds.py: a reference step starts from the fp32 masters, the fp32 state and the fp32 `exp_avg` as the
device holds them.

The bounds.  Everything up to the clipped, scaled update is the momentum-free step's: row / col / v, lr_t and scale keep the bounds of
`ob.adafactor_expected`, taken from its result, and u~ = scale u is rebuilt from them with the same helpers, as that function builds it.
Then
    m_new = m_old beta1 + u~ (1 - beta1)        one product with const(beta1), one with 1 - beta1, one sum
    p_new = p decay - m_new                     one product and one difference
beta1 reaches the kernel as a C float and the entry point forms 1 - beta1 from that float, as pass A forms 1 - beta2_t: its bound is
sub(1, const(beta1)), i.e. U |beta1| where beta1 is not fp32-representable, and nothing at beta1 = 0 (then m_new = u~ with u~'s bound and
p_new has the bound of the momentum-free step).  No constant is fitted; SAFETY is optim_bounds.py's.
"""
import math

import torch

from tests import optim_bounds as ob
from tests.optim_bounds import F64, V, add, const, div, mul, psum, rsqrt, sub


def _u_ref(g, row, col, v):
    """float64 u = g / sqrt(v^) from the new statistics (factored over the last two dims, or the full second moment)"""
    if row is not None:
        return (row / row.mean(-1, keepdim=True)).rsqrt().unsqueeze(-1) * col.unsqueeze(-2).rsqrt() * g
    return v.rsqrt() * g


def adafactor_m_ref_step(p, g, st, m_old, step, beta1, grad_scale=1.0, **kw):
    """Plain float64 Adafactor step with a first moment (reference adafactor.py:221-250) of one tensor from the state `st` (the
    reference's keys) and `m_old`; nothing is modified.  Returns ob.adafactor_ref_step's entries, with "p" the momentum step's, and
    "exp_avg"."""
    h = {**ob.AF_DEFAULTS, **kw}
    out = ob.adafactor_ref_step(p, g, st, step, grad_scale, **kw)
    u = _u_ref(g.double() * grad_scale, out.get("row"), out.get("col"), out.get("v"))
    m = beta1 * m_old.double() + (1.0 - beta1) * (out["scale"] * u)
    out["p"] = p.double() * (1.0 - h["weight_decay"] * out["lr_t"]) - m
    out["exp_avg"] = m
    return out


def adafactor_m_expected(p, g, st, m_old, step, beta1, grad_scale=1.0, **kw):
    """{output: (float64 reference, bound)} of one FlatAdafactorMomentum step of one tensor (logical shapes; conv [O, I, KH, KW]) from the
    fp32 master `p`, gradient `g`, state `st` under the reference's keys and first moment `m_old`: p, exp_avg, lr_t, scale, and
    row + col (factored) or v"""
    h = {**ob.AF_DEFAULTS, **kw}
    shape = tuple(p.shape)
    base = ob.adafactor_expected(p, g, st, step, grad_scale, **kw)
    val = lambda k: V(base[k][0], base[k][1] / ob.SAFETY)         # an output of the momentum-free step with its own bound
    gg, _ = ob._scaled_grad(g, grad_scale, h["eps"][0])
    if len(shape) == 2:
        row = val("row")
        mean = div(psum(row, 0, ob.FIN + math.ceil(shape[0] / ob.AF_TR)), V(float(shape[0])))      # (ob._matrix_stats' mean of the row EMA)
        u = mul(ob._matrix_factor(row, val("col"), mean), gg)
    elif len(shape) == 4:
        u = mul(ob._conv_factor(val("row"), val("col")), gg)
    else:
        u = mul(gg, rsqrt(val("v")))
    lr_t = val("lr_t")
    ut = mul(val("scale"), u)
    b1 = const(beta1)
    m = add(mul(V(m_old), b1), mul(ut, sub(V(1.0), b1)))
    decay = sub(V(1.0), mul(const(h["weight_decay"]), lr_t))
    pn = sub(mul(V(p), decay), m)
    ref = adafactor_m_ref_step(p, g, st, m_old, step, beta1, grad_scale, **kw)
    ob._agree("p", pn.ref, ref["p"], float(max(p.abs().max(), ref["p"].abs().max())))
    ob._agree("exp_avg", m.ref, ref["exp_avg"], float(max(m_old.abs().max(), ref["exp_avg"].abs().max())))
    out = {k: v for k, v in base.items() if k != "p"}
    out.update(p=ob._out(pn), exp_avg=ob._out(m))
    return out


def float64_chain(init, grads, beta1, **kw):
    """the float64 step chained over `grads` (one list of gradients per step) from fp32 `init`, state and moment kept in float64:
    (parameters after every step, final states under the reference's keys, with exp_avg)"""
    ps = [t.double() for t in init]
    sts = [{k: v.double() for k, v in ob.zero_state(tuple(t.shape), False).items()} for t in init]
    ms = [torch.zeros_like(t, dtype=F64) for t in init]
    after = []
    for s, gs in enumerate(grads):
        for i, g in enumerate(gs):
            r = adafactor_m_ref_step(ps[i], g, sts[i], ms[i], s + 1, beta1, **kw)
            ps[i], ms[i] = r["p"], r["exp_avg"]
            sts[i] = {"exp_avg_sq_row": r["row"], "exp_avg_sq_col": r["col"]} if "row" in r else {"exp_avg_sq": r["v"]}
        after.append([t.clone() for t in ps])
    return after, [{**st, "exp_avg": m} for st, m in zip(sts, ms)]
