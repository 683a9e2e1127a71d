"""The Adafactor and CAME kernels (csrc/optim.hip, csrc/came.hip on the core of csrc/optim_common.h) against float64, per element, on
the update itself.  Both go through FlatAdafactor / FlatCAME: their tensor, item and chunk tables are the host planner's.

Every step is a single step: the masters and the optimizer state are read back from the device, one float64 step is taken from exactly
those values (tests/optim_bounds.py), and every output -- p_new, the row / column / vector statistics, the first moment, lr_t, scale, the
clip denominator, RMS(p) from the partial sums of p^2 -- is compared per element at its derived bound.  The cases make the update the
thing that is measured: zero masters (p_new = -scale u, rounded once; the eps2 floor of scale_parameter), a step of 1e-2 |p| or more with
weight decay (bound(update) + half an ulp of p), and the warm-up regime, where lr_t, scale and the states carry the check and every
element whose update exceeds its bound by an ulp must have moved.  The store holds the smallest shapes that reach every edge of the
core (ob.SHAPES); gradients span four decades with a zero row and column, zero tensors, a clipped and an unclipped step.  After every
step the "blocks done" counters are all zero.  The same steps in small chunks (tensors of every kind in a second and third chunk:
non-zero item_lo), on two streams (Adafactor) and with the store in reverse order give the same bits.

Largest error / bound on the MI355X | by the fp32 restatement of tests/test_optim_bounds_cpu.py ("[optim ratio] ..." in both):
  Adafactor  p 0.797 | 0.797, row 0.662 | 0.662, col 0.656 | 0.656, v 0.634 | 0.634, lr_t 0.300 | 0.300, scale 0.300 | 0.300, rms_p 0.109 | 0.094
  CAME       p 0.523 | 0.572, exp_avg 0.630 | 0.636, R 0.544 | 0.544, C 0.559 | 0.559, Rr 0.564 | 0.564, Cr 0.527 | 0.531, v 0.551 | 0.551,
             denom 0.056 | 0.088
The ratios above 0.5 are the same on both sides, and all of one kind: bounds of three to six roundings, in which a few elements among 10^5
have them all aligned.  p 0.797 is the warm-up case, where the update is a few ulps of p and the leading term of the bound is the half ulp
of the final rounding of p itself: next to a tie a correctly rounded result is half an ulp off, 1 / SAFETY = 0.8 of the bound.  row, col, v,
R .. Cr and exp_avg (0.53 .. 0.66) are EMAs on the third step, whose gradients are small: old * beta + new * (1 - beta) is then the old
value through the fp32 rounding of beta (a common offset of up to U), one product and one sum, a bound of 3 to 4 U of which 2.5 U are
reached.  The reductions (lr_t, scale, denom, rms_p: 0.06 .. 0.3) stay far inside their worst-case chains, as sums of positive terms do.
"""
import pytest
import torch

from tests import optim_bounds as ob
from tests.test_text_encoder_train_gpu import _check

pytestmark = pytest.mark.gpu
AF_KEYS = {"row": "exp_avg_sq_row", "col": "exp_avg_sq_col", "v": "exp_avg_sq"}


@pytest.fixture(autouse=True)
def _clean_health():
    from neurosis_amd import lib

    lib.call("nk_health_clear")
    yield
    lib.call("nk_health_clear")


def make_store(tensors):
    from neurosis_amd.nn import FlatParamStore

    # conv weights live channels-last (the store's physical layout is [O][KH][KW][I])
    params = [torch.nn.Parameter(t.clone().cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.clone().cuda()) for t in tensors]
    return FlatParamStore(params), params


def _host(t):
    return t.detach().cpu().contiguous().clone()


def _state(opt, j):
    return {k: _host(v) for k, v in opt.param_state(j).items() if torch.is_tensor(v)}


def _kinds_in_later_chunks(opt):
    """per kind, the number of chunks after the first (non-zero item_lo) that hold a tensor of it"""
    return [sum(1 for (t0, t1, i0, _) in opt.chunks[1:] if i0 > 0 and (opt._tens_np["kind"][t0:t1] == k).any()) for k in (0, 1, 2)]


def _run(who, case, order, chunk_bytes, verify):
    """ob.STEPS steps of one case over the tensors ob.SHAPES[i], i in `order`; with `verify` every step is checked against float64 from
    the device's own masters and state.  Returns, per index of ob.SHAPES, (master, state, shadow) after the last step, and the per-tensor
    scalars"""
    from neurosis_amd.optim import FlatAdafactor, FlatCAME

    came = who == "came"
    c = (ob.CAME_CASES if came else ob.AF_CASES)[case]
    init, grads = ob.inputs()
    store, params = make_store([init[i] for i in order])
    opt = (FlatCAME if came else FlatAdafactor)(store, chunk_bytes=chunk_bytes, **c["kwargs"])
    if chunk_bytes is None:
        assert len(opt.chunks) == 1
    else:
        assert min(_kinds_in_later_chunks(opt)) >= 2, opt.chunks
    must_move = 0
    for s in range(ob.STEPS):
        if c["zero"]:
            store.master.zero_()
            store.masters_changed()
        for p, i in zip(params, order):
            p.grad.copy_(grads[s][i].cuda())
        torch.cuda.synchronize()
        before = [(_host(p), _state(opt, j)) for j, p in enumerate(params)] if verify else None
        opt.step(grad_scale=c["grad_scale"])
        torch.cuda.synchronize()
        assert not bool(opt.counters.any()), f"{who} {case} step {s + 1}: a 'blocks done' counter is not back at zero"
        if not verify:
            continue
        for j, (p, i) in enumerate(zip(params, order)):
            shape, (p0, st0) = ob.SHAPES[i], before[j]
            label = f"{who} {case} step {s + 1} {shape}"
            st1, p1 = _state(opt, j), _host(p)
            if came:
                want = ob.came_expected(p0, grads[s][i], st0, c["grad_scale"], **c["kwargs"])
                got = {k: st1[key] for k, key in ob.CAME_KEYS.items() if key in st1 and k in want}
                got.update(p=p1, denom=opt.denom[j].cpu())
            else:
                want = ob.adafactor_expected(p0, grads[s][i], st0, s + 1, c["grad_scale"], **c["kwargs"])
                got = {k: st1[key] for k, key in AF_KEYS.items() if key in st1}
                got.update(p=p1, lr_t=opt.lr_t[j].cpu(), scale=opt.scale[j].cpu())
            assert set(got) == set(want), (label, sorted(got), sorted(want))
            ob.verify(who, label, got, want, _check)
            must = ob.must_move(p0, *want["p"])
            must_move += int(must.sum())
            assert bool((p1 != p0)[must].all()), f"{label}: {int((p1 == p0)[must].sum())} masters whose update exceeds its bound by an ulp did not move"
            if not came:
                t = opt._tens_np[j]
                parts = opt.p2_part[int(t["item0"]):int(t["item0"]) + int(t["nitems"])].double().sum().cpu()
                ob.verify(who, label, {"rms_p": (parts / p1.numel()).sqrt()}, {"rms_p": ob.p2_expected(p1, shape)}, _check)
    if verify:
        assert must_move > 0, "no update of this case can be told from rounding: the case checks nothing"
    torch.cuda.synchronize()
    tensors = {i: (_host(p), _state(opt, j), _host(p._nk_shadow)) for j, (p, i) in enumerate(zip(params, order))}
    scalars = {i: [_host(t[j]) for t in ((opt.denom,) if came else (opt.lr_t, opt.scale))] for j, i in enumerate(order)}
    return tensors, scalars


def _same(label, a, b):
    for i in a[0]:
        (pa, sa, ha), (pb, sb, hb) = a[0][i], b[0][i]
        assert torch.equal(pa, pb) and torch.equal(ha, hb), f"{label}: masters or shadows of {ob.SHAPES[i]} differ"
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), f"{label}: state of {ob.SHAPES[i]} differs"
        assert all(torch.equal(x, y) for x, y in zip(a[1][i], b[1][i])), f"{label}: per-tensor scalars of {ob.SHAPES[i]} differ"


@pytest.mark.parametrize("case", list(ob.AF_CASES))
def test_adafactor_steps_per_element(case, monkeypatch):
    order = list(range(len(ob.SHAPES)))
    monkeypatch.setenv("NK_AF_STREAMS", "1")
    base = _run("adafactor", case, order, None, True)
    ob.report("adafactor")
    _same("small chunks", base, _run("adafactor", case, order, ob.CHUNK_BYTES, False))
    _same("reversed store", base, _run("adafactor", case, order[::-1], ob.CHUNK_BYTES, False))
    monkeypatch.setenv("NK_AF_STREAMS", "2")
    _same("two streams", base, _run("adafactor", case, order, ob.CHUNK_BYTES, False))


@pytest.mark.parametrize("case", list(ob.CAME_CASES))
def test_came_steps_per_element(case):
    order = list(range(len(ob.SHAPES)))
    base = _run("came", case, order, None, True)
    ob.report("came")
    _same("small chunks", base, _run("came", case, order, ob.CHUNK_BYTES, False))
    _same("reversed store", base, _run("came", case, order[::-1], ob.CHUNK_BYTES, False))
