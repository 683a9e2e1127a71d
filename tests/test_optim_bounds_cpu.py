"""The bounds of tests/optim_bounds.py, tested without a GPU.

  finite            the float64 references are finite on every input of every case (zero rows and columns, zero tensors, large and small
                    gradients), the clip denominator exceeds 1 on some steps and equals 1 on others, and the chunk size of the GPU test
                    puts tensors of every kind into a second and a third chunk.
  fp32 restatement  every pass of csrc/optim.hip and csrc/came.hip in numpy fp32 with the kernels' tile partials and summation order
                    (four serial terms per lane, the shuffle tree over the 16 column lanes, the serial tile partials, block_sum_256, the
                    per-item partials and the tensor's last block) must lie within the bounds against float64, chained step by step as the
                    GPU test chains the device: a bound is not too tight for honest fp32.  Prints "[optim ratio] ..." per output.
  planted errors    each of these, planted into the restatement, must be rejected by the same verify() the GPU test uses: the last four
                    columns of a ragged tile missing from the row sums, the last row of a strip tail missing from the column sums, the row
                    mean divided by the tile-padded width, the second strip's mean_row slot left out, eps1 left out, the column factor of
                    the neighbouring tile column, KH and KW swapped on the 1x3 and 3x1 convs, the clip numel without KH KW, weight decay
                    without lr_t (Adafactor) or with it under fixed_decay (CAME), beta2_t of step - 1, grad_scale not squared in q,
                    CAME's residual from the first moment before its update, and an element moved by two ulps.  The honest bound of p_new
                    is 30 to 900 U (optim_bounds.py), so two ulps there are NOT rejected (asserted below, so the statement stays true);
                    the two-ulp plant is applied where the bound allows it: a vector's second moment on the first step, and the
                    zero-master p_new is shown to reject a plant of the bound's own size."""
import math

import numpy as np
import pytest
import torch

from tests import optim_bounds as ob
from tests.test_text_encoder_train_gpu import _check

f = np.float32
TR, TC = ob.AF_TR, ob.AF_TC


# ================================================================================================================================
# the kernels' reductions
# ================================================================================================================================
def _serial(a, axis=-1):
    """acc = 0; acc += a[k] left to right, fp32"""
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros(a.shape[1:], f)
    for k in range(a.shape[0]):
        acc = acc + a[k]
    return acc


def _butterfly(a):
    """xor butterfly over the last axis (a power of two); lane 0's total"""
    n = a.shape[-1]
    idx, o = np.arange(n), n // 2
    while o:
        a = a + a[..., idx ^ o]
        o //= 2
    return a[..., 0]


def _block_sum(per):
    """block_sum_256 over the last axis (256 threads)"""
    w = _butterfly(per.reshape(per.shape[:-1] + (4, 64)))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _pad(a, shape):
    out = np.zeros(shape, f)
    out[tuple(slice(0, n) for n in a.shape)] = a
    return out


def _rsqrt(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return f(1) / np.sqrt(x)


def _tiles(shape):
    return math.ceil(shape[0] / TR), math.ceil(shape[1] / TC)


def tile_stats(v, old_row, old_col, beta, omb, plant=None):
    """fac_tile_add_row + fac_strip_finish: the row / column EMAs of a matrix of non-negative terms and the mean of the row EMA"""
    d0, d1 = v.shape
    ntr, ntc = _tiles(v.shape)
    vp = _pad(v, (ntr * TR, ntc * TC))
    vr = vp.copy()
    if plant == "drop_cols" and d1 % TC:
        vr[:, d1 - 4:d1] = 0
    rs = _serial(_butterfly(_serial(vr.reshape(ntr * TR, ntc, 16, 4))))[:d0]
    row = old_row * beta + (rs / f(ntc * TC if plant == "padded_width" else d1)) * omb
    vc = vp.copy()
    if plant == "drop_row" and d0 % TR:
        vc[d0 - 1] = 0
    cs = _serial(_serial(_serial(vc.reshape(ntr, 16, 16, ntc * TC), axis=1), axis=1), axis=0)[:d1]      # lane rows i, LDS rows ry, strips
    col = old_col * beta + (cs / f(d0)) * omb
    slots = _block_sum(_pad(row, (ntr * TR,)).reshape(ntr, TR))
    if plant == "one_slot":
        slots = slots[:1]
    return row, col, _serial(slots) / f(d0)


def tile_factor(row, col, mean, plant=None):
    ci = _rsqrt(col)
    if plant == "neighbour_col":
        j = np.arange(col.shape[0]) ^ TC
        ci = ci[np.where(j < col.shape[0], j, np.arange(col.shape[0]))]
    return _rsqrt(row / mean)[:, None] * ci[None, :]


def pair_stats(v, old_row, old_col, beta, omb):
    KH, KW = v.shape[2:]
    row = old_row * beta + (_serial(v, axis=3) / f(KW)) * omb
    col = old_col * beta + (_serial(v, axis=2) / f(KH)) * omb
    return row, col


def pair_factor(row, col):
    mean = _serial(row, axis=2) / f(row.shape[2])
    return _rsqrt(row / mean[:, :, None])[:, :, :, None] * _rsqrt(col)[:, :, None, :]


def parts_of(sq):
    """the per-item partial sums of a tensor of squares, in item order"""
    if sq.ndim == 2:
        ntr, ntc = _tiles(sq.shape)
        t = _pad(sq, (ntr * TR, ntc * TC)).reshape(ntr, 16, 16, ntc, 16, 4).transpose(0, 3, 2, 4, 1, 5).reshape(ntr, ntc, 256, 64)
        return _block_sum(_serial(t)).reshape(-1)
    if sq.ndim == 4:
        O, I, KH, KW = sq.shape
        nit = math.ceil(O * I / ob.AF_CONV_PAIRS)
        t = _pad(sq.reshape(O * I, KH * KW), (nit * 1024, KH * KW)).reshape(nit, 4, 256, KH * KW).transpose(0, 2, 1, 3).reshape(nit, 256, -1)
        return _block_sum(_serial(t))
    nit = math.ceil(sq.shape[0] / ob.AF_VEC)
    return _block_sum(_serial(_pad(sq, (nit * 1024,)).reshape(nit, 4, 256).transpose(0, 2, 1)))


def total_of(parts):
    """af_tensor_scale / cm_tensor_denom: thread tid sums parts tid, tid + 256, ...; block_sum_256"""
    k = math.ceil(parts.shape[0] / 256)
    return _block_sum(_serial(_pad(parts, (k * 256,)).reshape(k, 256), axis=0))


def _np(t):
    return t.detach().cpu().numpy().astype(f)


def _state(st):
    return {k: _np(v) for k, v in st.items()}


def _out(d):
    return {k: torch.from_numpy(np.asarray(v, dtype=f)) for k, v in d.items()}


# ================================================================================================================================
# the restatements
# ================================================================================================================================
def restate_adafactor(p, g, st, step, grad_scale=1.0, plant=None, **kw):
    """af_stats_kernel, af_u2_kernel, af_apply_kernel on one tensor; returns the outputs of ob.adafactor_expected, the new state under
    the reference's keys ("state") and the partial sums of p^2 ("p2")"""
    h = {**ob.AF_DEFAULTS, **kw}
    p, g, st = _np(p), _np(g), _state(st)
    shape = p.shape
    bstep = step - 1 if plant == "beta_step" and step > 1 else step
    beta = f(1.0 - math.pow(bstep, h["decay_rate"]))
    omb = f(1) - beta
    gs, eps1 = f(grad_scale), f(0.0 if plant == "eps1" else h["eps"][0])
    gg = g * gs
    q = (gg * g if plant == "gs_once" else gg * gg) + eps1
    out = {}
    if p.ndim == 2:
        row, col, mean = tile_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], beta, omb, plant)
        u = tile_factor(row, col, mean, plant) * gg
        out["row"], out["col"] = row, col
    elif p.ndim == 4:
        row, col = pair_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], beta, omb)
        u = pair_factor(row, col) * gg
        out["row"], out["col"] = row, col
    else:
        v = st["exp_avg_sq"] * beta + q * omb
        u = gg * _rsqrt(v)
        out["v"] = v
    numel = f(math.prod(shape[:2] if plant == "numel_taps" else shape))
    su, sp = total_of(parts_of(u * u)), total_of(parts_of(p * p))
    denom = np.maximum(f(1), np.sqrt(su / numel) / f(h["clip_threshold"]))
    rms_p = np.sqrt(sp) / np.sqrt(f(math.prod(shape)))
    rel = f(ob.AO.rel_lr(step, 1.0, h["lr"], 1.0, False, h["relative_step"], h["warmup_init"]))
    lr_t = (np.maximum(f(h["eps"][1]), rms_p) if h["scale_parameter"] else f(1)) * rel
    scale = lr_t / denom
    decay = f(1) - f(h["weight_decay"]) * (f(1) if plant == "wd_no_lr" else lr_t)
    pn = p * decay - scale * u
    out.update(p=p if plant == "no_apply" else pn, lr_t=lr_t, scale=scale)
    res = _out(out)
    res["state"] = _out({{"row": "exp_avg_sq_row", "col": "exp_avg_sq_col", "v": "exp_avg_sq"}[k]: out[k] for k in ("row", "col", "v") if k in out})
    res["p2"] = torch.from_numpy(parts_of(pn * pn))
    return res


def restate_came(p, g, st, grad_scale=1.0, plant=None, **kw):
    """came_stats_kernel, came_u2_kernel, came_moment_kernel, came_apply_kernel on one tensor"""
    h = {**ob.CAME_DEFAULTS, **kw}
    p, g, st = _np(p), _np(g), _state(st)
    shape = p.shape
    b1, b2, b3 = (f(b) for b in h["betas"])
    o1, o2, o3 = (f(1.0 - b) for b in h["betas"])
    lr = f(h["lr"])
    fixed = h["fixed_decay"] != (plant == "fixed_decay_lr")
    decay = f(1.0 - h["weight_decay"] * (1.0 if fixed else h["lr"]))
    gs, eps1, eps2 = f(grad_scale), f(h["eps1"]), f(h["eps2"])
    gg = g * gs
    q = gg * gg + eps1
    out = {}
    if p.ndim == 2:
        R, C, mean = tile_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], b2, o2, plant)
        u = tile_factor(R, C, mean) * gg
    elif p.ndim == 4:
        R, C = pair_stats(q, st["exp_avg_sq_row"], st["exp_avg_sq_col"], b2, o2)
        u = pair_factor(R, C) * gg
    else:
        v = st["exp_avg_sq"] * b2 + q * o2
        u = _rsqrt(v) * gg
        out["v"] = v
    su = total_of(parts_of(u * u))
    denom = np.maximum(f(1), (np.sqrt(su) / np.sqrt(f(math.prod(shape)))) / f(h["clip_threshold"]))
    uh = u / denom
    m = st["exp_avg"] * b1 + uh * o1
    if p.ndim == 1:
        pn = p * decay - m * lr
    else:
        d = uh - (st["exp_avg"] if plant == "res_old_m" else m)
        res = d * d + eps2
        if p.ndim == 2:
            Rr, Cr, mean = tile_stats(res, st["exp_avg_res_row"], st["exp_avg_res_col"], b3, o3)
            fac = tile_factor(Rr, Cr, mean)
        else:
            Rr, Cr = pair_stats(res, st["exp_avg_res_row"], st["exp_avg_res_col"], b3, o3)
            fac = pair_factor(Rr, Cr)
        pn = p * decay - (fac * m) * lr
        out.update(R=R, C=C, Rr=Rr, Cr=Cr)
    out.update(p=p if plant == "no_apply" else pn, exp_avg=m, denom=denom)
    ret = _out(out)
    ret["state"] = _out({ob.CAME_KEYS[k]: out[k] for k in ob.CAME_KEYS if k in out})
    return ret


def _swap_taps(t):
    """a [O, I, KH, KW] tensor as a kernel with KH and KW exchanged sees its [O][KH][KW][I] memory: [O, I, KW, KH]"""
    O, I, KH, KW = t.shape
    return t.permute(0, 2, 3, 1).reshape(O, KW, KH, I).permute(0, 3, 1, 2).contiguous()


def _swapped_step(p, g, step, c):
    """The first step of a kernel that exchanges KH and KW, as the test sees it.  With a tap dimension of 1 the factored second moment is
    exact and symmetric -- u, and so p, are those of the honest kernel -- and what gives the exchange away is the state: the kernel
    writes its [O][KW][I] row statistics at row_off and its [O][KH][I] column statistics at col_off of the planner's layout (row region,
    64-aligned, then the column region), and the test reads [O][KH][I] and [O][KW][I] back from there.  With two real tap dimensions
    (2 x 3) p itself differs."""
    O, I, KH, KW = p.shape
    sw = restate_adafactor(_swap_taps(p), _swap_taps(g), ob.zero_state(tuple(_swap_taps(p).shape), False), step, c["grad_scale"], **c["kwargs"])
    got = {"p": _unswap_taps(sw["p"], KH, KW)}
    if 1 in (KH, KW):
        col_off = (O * KH * I + 63) // 64 * 64
        buf = torch.zeros(col_off + 4 * O * KH * KW * I)
        for off, t in ((0, sw["row"]), (col_off, sw["col"])):
            buf[off:off + t.numel()] = t.permute(0, 2, 1).reshape(-1)
        got["row"] = buf[:O * KH * I].view(O, KH, I).permute(0, 2, 1)
        got["col"] = buf[col_off:col_off + O * KW * I].view(O, KW, I).permute(0, 2, 1)
    return got


def _unswap_taps(t, KH, KW):
    """the [O][KW][KH][I] memory a swapped kernel wrote, read as the [O, I, KH, KW] tensor it is"""
    O, I = t.shape[:2]
    return t.permute(0, 2, 3, 1).reshape(O, KH, KW, I).permute(0, 3, 1, 2).contiguous()


# ================================================================================================================================
# the chain: what the GPU test does with the device, done with the restatement
# ================================================================================================================================
def run_chain(who, case, plant=None, only=None, record=True, steps=ob.STEPS, edit=None):
    """STEPS single steps of every tensor of ob.SHAPES (or those in `only`) of one case, each verified against float64 from the
    restatement's own fp32 state; `edit(step, shape, got, expected)` may tamper with an output before it is verified"""
    came = who == "came"
    c = (ob.CAME_CASES if came else ob.AF_CASES)[case]
    init, grads = ob.inputs()
    info = {"denoms": [], "must_move": 0}
    for i, shape in enumerate(ob.SHAPES):
        if only is not None and shape not in only:
            continue
        p, st = init[i].clone(), ob.zero_state(shape, came)
        for s in range(steps):
            if c["zero"]:
                p = torch.zeros_like(p)
            g = grads[s][i]
            if came:
                want = ob.came_expected(p, g, st, c["grad_scale"], **c["kwargs"])
                got = restate_came(p, g, st, c["grad_scale"], plant, **c["kwargs"])
                info["denoms"].append(float(want["denom"][0]))
            else:
                want = ob.adafactor_expected(p, g, st, s + 1, c["grad_scale"], **c["kwargs"])
                if plant == "swap_taps":
                    got = _swapped_step(p, g, s + 1, c)
                    want = {k: want[k] for k in got}
                else:
                    got = restate_adafactor(p, g, st, s + 1, c["grad_scale"], plant, **c["kwargs"])
                    info["denoms"].append(float(ob.adafactor_ref_step(p, g, st, s + 1, c["grad_scale"], **c["kwargs"])["denom"]))
            for k, (ref, bound) in want.items():
                assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), (who, case, shape, s, k)
            if edit is not None:
                edit(s, shape, got, want)
            ob.verify(who, f"{who} {case} step {s + 1} {shape}", got, want, _check, record)
            info["must_move"] += int(ob.must_move(p, *want["p"]).sum())
            if "p2" in got:
                ref, bound = ob.p2_expected(got["p"], shape)
                rms = (got["p2"].double().sum() / math.prod(shape)).sqrt()
                ob.verify(who, f"{who} {case} step {s + 1} {shape}", {"rms_p": rms}, {"rms_p": (ref, bound)}, _check, record)
            if "state" not in got:
                break
            p, st = got["p"], got["state"]
    return info


# ================================================================================================================================
# tests
# ================================================================================================================================
def test_chunk_size_puts_every_kind_into_a_second_and_a_third_chunk():
    from neurosis_amd import optim as O

    offs = np.cumsum([0] + [(math.prod(s) + 63) // 64 * 64 for s in ob.SHAPES])[:-1].tolist()
    for order in (ob.SHAPES, ob.SHAPES[::-1]):
        for dtype, fields, mr in ((O.AF_TENSOR_DTYPE, O._AF_STATE, 1), (O.CAME_TENSOR_DTYPE, O._CAME_STATE, 2)):
            plan = O._plan_tables("test", order, offs, ob.CHUNK_BYTES, None, dtype, fields, mr)
            assert [int(t["nitems"]) for t in plan["tensors"]] == [ob.nitems_of(s) for s in order]
            for kind in (0, 1, 2):
                later = [ci for ci, (t0, t1, i0, _) in enumerate(plan["chunks"]) if ci > 0 and i0 > 0 and (plan["tensors"]["kind"][t0:t1] == kind).any()]
                assert len(later) >= 2, (kind, plan["chunks"])
    conv_pairs = sorted(s[0] * s[1] for s in ob.CONVS[:3])
    assert conv_pairs == [1023, 1024, 1025]


@pytest.mark.parametrize("case", list(ob.AF_CASES))
def test_adafactor_restatement_is_within_the_bounds(case):
    info = run_chain("adafactor", case)
    assert max(info["denoms"]) > 1.5 and min(info["denoms"]) == 1.0, "the clip denominator must exceed 1 on some steps and equal 1 on others"
    ob.report("adafactor")


@pytest.mark.parametrize("case", list(ob.CAME_CASES))
def test_came_restatement_is_within_the_bounds(case):
    info = run_chain("came", case)
    assert max(info["denoms"]) > 1.5 and min(info["denoms"]) == 1.0
    ob.report("came")


def test_float64_restatement_follows_the_fp32_oracle():
    """adafactor_ref_step is the oracle's step (fp32 torch) in float64: the same lr and parameters to fp32 accuracy"""
    init, grads = ob.inputs()
    kw = ob.AF_CASES["relative"]["kwargs"]
    for i, shape in enumerate(ob.SHAPES):
        p, st = init[i].clone(), ob.AO.new_state(init[i])
        lr = ob.AO.step_tensor(p, grads[0][i].clone(), st, **kw)
        ref = ob.adafactor_ref_step(init[i], grads[0][i], ob.zero_state(shape, False), 1, **kw)
        assert abs(lr - float(ref["lr_t"])) <= 1e-5 * lr
        d_ref = ref["p"] - init[i].double()
        assert float(((p.double() - init[i].double()) - d_ref).abs().max()) <= 1e-4 * float(d_ref.abs().max()) + 2 ** -23 * float(init[i].abs().max()), shape


@pytest.mark.parametrize("who,case", [("adafactor", "warmup"), ("adafactor", "relative"), ("came", "decay")])
def test_an_apply_pass_that_does_nothing_is_rejected(who, case):
    """also in the warm-up regime: there are masters whose update exceeds its bound by more than an ulp, on every kind of tensor"""
    for shape in ((256, 64), (32, 32, 3, 3), (1024,)):
        assert run_chain(who, case, only=[shape], record=False)["must_move"] > 0
        with pytest.raises(AssertionError):
            run_chain(who, case, plant="no_apply", only=[shape], record=False)


AF_PLANTS = {
    "drop_cols": [(257, 68), (513, 132), (255, 60)],
    "drop_row": [(257, 68), (513, 132), (300, 8)],
    "padded_width": [(257, 68), (255, 60), (1, 4)],
    "one_slot": [(513, 132), (300, 8)],
    "eps1": [(257, 68)],
    "neighbour_col": [(513, 132), (257, 68)],
    "swap_taps": [(8, 8, 1, 3), (8, 8, 3, 1), (8, 8, 2, 3)],
    "numel_taps": [(33, 31, 3, 3), (8, 8, 2, 3)],
    "wd_no_lr": [(256, 64), (8, 16, 1, 1), (1025,)],
    "beta_step": [(256, 64), (32, 32, 3, 3), (1024,)],
    "gs_once": [(256, 64), (41, 25, 3, 3), (1023,)],
}


@pytest.mark.filterwarnings("ignore:invalid value encountered")      # without eps1 the zero row's factor is 0 * inf
@pytest.mark.parametrize("plant", list(AF_PLANTS))
def test_adafactor_planted_errors_are_rejected(plant):
    """every tensor named for the plant rejects it (on its own), in the case with weight decay and grad_scale != 1"""
    for shape in AF_PLANTS[plant]:
        run_chain("adafactor", "manual", only=[shape], record=False)
        with pytest.raises(AssertionError):
            run_chain("adafactor", "manual", plant=plant, only=[shape], record=False)


CAME_PLANTS = {
    "drop_cols": [(257, 68)],
    "one_slot": [(513, 132)],
    "fixed_decay_lr": [(256, 64), (8, 16, 1, 1), (1025,)],
    "res_old_m": [(256, 64), (32, 32, 3, 3)],
}


@pytest.mark.parametrize("plant", list(CAME_PLANTS))
def test_came_planted_errors_are_rejected(plant):
    for shape in CAME_PLANTS[plant]:
        with pytest.raises(AssertionError):
            run_chain("came", "fixed", plant=plant, only=[shape], record=False)


def _move(name, ulps, at_step=0):
    """tamper: the element of `name` whose bound is tightest against its value moves by `ulps` fp32 ulps, away from the reference"""
    def edit(s, shape, got, want):
        if s != at_step or name not in want:
            return
        ref, bound = want[name]
        t = got[name].clone().reshape(-1)
        i = int((bound / ref.abs().clamp_min(1e-300) + (ref == 0) * 1e30).reshape(-1).argmin())
        up = bool(t[i].double() >= ref.reshape(-1)[i])
        for _ in range(ulps):
            t[i] = torch.nextafter(t[i], torch.tensor(math.inf if up else -math.inf))
        got[name] = t.reshape(got[name].shape)
    return edit


def test_two_ulps_are_rejected_where_the_bound_allows_it():
    """A vector's second moment on the first step is one square and one sum (beta2_t = 0, grad_scale = 1): bound 2.5 U, and two ulps
    are rejected.  In p_new the honest bound is 30 to 900 U (printed): two ulps pass (asserted, so that the docstrings stay true), and a plant of
    the size of the bound itself -- 2 x bound / ulp, rounded up -- is rejected there."""
    for who in ("adafactor", "came"):
        vec = [(1025,)]
        if who == "adafactor":
            with pytest.raises(AssertionError):
                run_chain(who, "zero", only=vec, record=False, steps=1, edit=_move("v", 2))
        run_chain(who, "zero", only=vec, record=False, steps=1, edit=_move("p", 2))
        for shape in ((1025,), (257, 68), (41, 25, 3, 3)):
            c = (ob.CAME_CASES if who == "came" else ob.AF_CASES)["zero"]
            p, g = torch.zeros(shape), ob.inputs()[1][0][ob.SHAPES.index(shape)]
            st = ob.zero_state(shape, who == "came")
            want = ob.came_expected(p, g, st, **c["kwargs"]) if who == "came" else ob.adafactor_expected(p, g, st, 1, **c["kwargs"])
            ref, bound = want["p"]
            nz = ref != 0
            rel = float((bound[nz] / ref[nz].abs()).min())
            ulps = math.ceil(2 * rel / 2.0 ** -24) + 1            # an ulp is at least 2^-24 relative
            print(f"[optim ratio] {who} zero-master p_new {shape}: bound {rel / ob.U:.0f} U relative; planted {ulps} ulps")
            with pytest.raises(AssertionError):
                run_chain(who, "zero", only=[shape], record=False, steps=1, edit=_move("p", ulps))
