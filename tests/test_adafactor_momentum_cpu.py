"""Adafactor's first moment (beta1) without a GPU: the float64 reference of tests/optim_momentum_bounds.py against the reference class's
own fp32 steps (tests/golden/adafactor_beta1_steps, written by make_golden_adafactor_beta1.py), the bounds against an fp32 restatement of
af_apply_momentum_kernel with and without planted errors, and the public surface (constructors, refusals, the ABI entry).

Largest error / bound of the fp32 restatement ("[optim ratio] adafactor-m ...", the GPU's stand in tests/test_adafactor_momentum_gpu.py):
  beta1 = 0.9   p 0.798, exp_avg 0.637, row 0.662, col 0.656, v 0.634, lr_t 0.300, scale 0.300
  beta1 = 0.0   p 0.797, exp_avg 0.199, row 0.662, col 0.656, v 0.634, lr_t 0.300, scale 0.300
p 0.80 is the warm-up case (half an ulp of p itself, 1 / SAFETY of the bound, as in tests/test_optim_kernels_gpu.py); exp_avg 0.64 at beta1 = 0.9
is the moment on the third step, whose update is small: old * beta1 through the fp32 rounding of beta1, one product and one sum.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import optim_bounds as ob
from tests import optim_momentum_bounds as omb
from tests import test_optim_bounds_cpu as T
from tests.golden.fixture_io import load_fixture
from tests.test_text_encoder_train_gpu import _check
from tests.util import rel_err

f = np.float32
BETA1 = 0.9

# rel_err of a step's delta (p_after - p_before) between the reference class's fp32 run (the fixture) and the float64 chain on the same
# inputs (omb.float64_chain), measured here on the CPU, largest of the three steps: `relative` 8.79e-5 (steps: 8.79e-5 / 6.25e-5 / 4.36e-5),
# `manual` 1.64e-3 (1.64e-3 / 9.08e-4 / 7.36e-4: the step is lr (1 - beta1) |u| = 1e-4 against |p| = 0.5, so a delta between fp32 masters carries
# an ulp of |p|).  DELTA_DEV is that value rounded up; the tolerance of a comparison with the fixture is
# twice it (the rule of tests/test_optim_gpu.py: the kernels' deviation and the reference's are independent and of the same kind).  A step
# that leaves the masters alone has rel_err 1.
DELTA_DEV = {"relative": 8.8e-5, "manual": 1.65e-3}
DELTA_TOL = {tag: 2 * v for tag, v in DELTA_DEV.items()}
PARAM_TOL = 2e-5           # parameters, relative (tests/test_optim_gpu.py)
STATE_TOL = 1e-4           # exp_avg and the factored states


def delta_err(p_before, p_after, ref_before, ref_after) -> float:
    return rel_err(p_after.double() - p_before.double(), ref_after.double() - ref_before.double())


# ================================================================================================================================
# 1. the float64 reference against the reference class's own steps
# ================================================================================================================================
@pytest.mark.parametrize("tag", ["relative", "manual"])
def test_float64_reference_reproduces_the_fixture(tag):
    """Three chained float64 steps from the fixture's inputs: parameters after every step (PARAM_TOL), each step's delta (DELTA_DEV, the
    measured deviation itself: see above), exp_avg and the factored states after the last (STATE_TOL)."""
    c = load_fixture("adafactor_beta1_steps")[tag]
    assert c["kwargs"]["beta1"] == BETA1 and all("exp_avg" in st for st in c["states"])
    kw = {k: v for k, v in c["kwargs"].items() if k != "beta1"}
    after, states = omb.float64_chain(c["init"], c["grads"], BETA1, **kw)
    worst = []
    for s in range(3):
        errs = []
        for i, want in enumerate(c["after"][s]):
            assert rel_err(after[s][i], want) <= PARAM_TOL, (s, tuple(want.shape))
            p0, w0 = (after[s - 1][i], c["after"][s - 1][i]) if s else (c["init"][i], c["init"][i])
            errs.append(delta_err(p0, after[s][i], w0, want))
        worst.append(max(errs))
    print(f"[adafactor-m delta] {tag}: largest rel_err of a step's delta, fixture against float64, per step: " + " / ".join(f"{e:.3g}" for e in worst))
    assert max(worst) <= DELTA_DEV[tag], worst
    for i, want in enumerate(c["states"]):
        for k in ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            if k in want:
                assert rel_err(states[i][k], want[k]) <= STATE_TOL, (i, k)


# ================================================================================================================================
# 2. the fp32 restatement of the momentum pass, and planted errors
# ================================================================================================================================
def restate_momentum(p, g, st, m_old, step, beta1, grad_scale=1.0, plant=None, **kw):
    """af_stats_kernel, af_u2_kernel (T.restate_adafactor: statistics, lr_t, scale) and af_apply_momentum_kernel on one tensor in numpy fp32"""
    h = {**ob.AF_DEFAULTS, **kw}
    base = T.restate_adafactor(p, g, st, step, grad_scale, **kw)
    pp, gg, m = T._np(p), T._np(g) * f(grad_scale), T._np(m_old)
    if pp.ndim == 2:
        row, col = T._np(base["row"]), T._np(base["col"])
        ntr = T._tiles(pp.shape)[0]
        mean = T._serial(T._block_sum(T._pad(row, (ntr * T.TR,)).reshape(ntr, T.TR))) / f(pp.shape[0])      # (tile_stats' mean of the row EMA)
        u = T.tile_factor(row, col, mean) * gg
    elif pp.ndim == 4:
        u = T.pair_factor(T._np(base["row"]), T._np(base["col"])) * gg
    else:
        u = gg * T._rsqrt(T._np(base["v"]))
    lr_t, scale = T._np(base["lr_t"]), T._np(base["scale"])
    b1 = f(beta1)
    o1 = f(1) - b1
    if plant == "swap_betas":
        b1, o1 = o1, b1
    ut = (lr_t if plant == "unclipped" else scale) * u
    decay = f(1) - f(h["weight_decay"]) * lr_t
    mn = m * b1 + ut * o1
    if plant == "wd_on_m":
        mn = mn * decay
    pn = pp * decay - (ut if plant == "p_minus_u" else mn)
    out = T._out({k: T._np(base[k]) for k in ("row", "col", "v", "lr_t", "scale") if k in base})
    out.update(T._out(dict(p=pn, exp_avg=mn)))
    out["state"] = base["state"]
    return out


def run_chain(case, beta1, plant=None, only=None, record=True):
    """ob.STEPS single steps of every tensor of ob.SHAPES (or those in `only`) of one case of ob.AF_CASES, each verified against float64
    from the restatement's own fp32 masters, state and moment (what the GPU test does with the device)"""
    c = ob.AF_CASES[case]
    init, grads = ob.inputs()
    info = {"denoms": [], "must_move": 0, "m_nonzero": 0}
    who = f"adafactor-m{beta1}"
    for i, shape in enumerate(ob.SHAPES):
        if only is not None and shape not in only:
            continue
        p, st, m = init[i].clone(), ob.zero_state(shape, False), torch.zeros(shape)
        for s in range(ob.STEPS):
            if c["zero"]:
                p = torch.zeros_like(p)
            g = grads[s][i]
            info["m_nonzero"] += int(s > 0 and bool(m.any()))
            want = omb.adafactor_m_expected(p, g, st, m, s + 1, beta1, c["grad_scale"], **c["kwargs"])
            got = restate_momentum(p, g, st, m, s + 1, beta1, c["grad_scale"], plant, **c["kwargs"])
            info["denoms"].append(float(ob.adafactor_ref_step(p, g, st, s + 1, c["grad_scale"], **c["kwargs"])["denom"]))
            for k, (ref, bound) in want.items():
                assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(bound).all()), (case, shape, s, k)
            ob.verify(who, f"{who} {case} step {s + 1} {shape}", got, want, _check, record)
            info["must_move"] += int(ob.must_move(p, *want["p"]).sum())
            p, st, m = got["p"], got["state"], got["exp_avg"]
    return info


@pytest.mark.parametrize("beta1", [BETA1, 0.0])
@pytest.mark.parametrize("case", list(ob.AF_CASES))
def test_momentum_restatement_is_within_the_bounds(case, beta1):
    info = run_chain(case, beta1)
    assert max(info["denoms"]) > 1.5 and min(info["denoms"]) == 1.0, "the clip denominator must exceed 1 on some steps and equal 1 on others"
    assert info["must_move"] > 0 and (beta1 == 0.0 or info["m_nonzero"] > 0)
    ob.report(f"adafactor-m{beta1}")


def test_without_beta1_the_bounds_are_the_momentum_free_step_s():
    """beta1 = 0 and m_old = 0: m_new = u~ and p_new is ob.adafactor_expected's, reference and bound"""
    init, grads = ob.inputs()
    c = ob.AF_CASES["manual"]
    for shape in ((257, 68), (41, 25, 3, 3), (1025,)):
        i = ob.SHAPES.index(shape)
        st = ob.zero_state(shape, False)
        base = ob.adafactor_expected(init[i], grads[0][i], st, 1, c["grad_scale"], **c["kwargs"])
        mine = omb.adafactor_m_expected(init[i], grads[0][i], st, torch.zeros(shape), 1, 0.0, c["grad_scale"], **c["kwargs"])
        assert torch.allclose(mine["p"][0], base["p"][0], rtol=1e-13, atol=0) and torch.allclose(mine["p"][1], base["p"][1], rtol=1e-9, atol=0)
        assert set(mine) == set(base) | {"exp_avg"}


PLANTS = {
    "swap_betas": [(256, 64), (32, 32, 3, 3), (1024,)],          # beta1 and 1 - beta1 exchanged
    "unclipped": [(257, 68), (33, 31, 3, 3), (1025,)],           # the moment of lr_t u where the clip denominator is above 1 (the second step)
    "p_minus_u": [(255, 60), (8, 16, 1, 1), (2049,)],            # p - u~ applied instead of p - m_new
    "wd_on_m": [(513, 132), (41, 25, 3, 3), (1023,)],            # weight decay applied to m
}


@pytest.mark.parametrize("plant", list(PLANTS))
def test_planted_errors_are_rejected(plant):
    """every tensor named for the plant accepts the honest pass and rejects the plant (on its own), in the case with weight decay and
    grad_scale != 1, whose second step is clipped"""
    for shape in PLANTS[plant]:
        info = run_chain("manual", BETA1, only=[shape], record=False)
        assert max(info["denoms"]) > 1.1, "the clip denominator must be above 1 on some step of this tensor"
        with pytest.raises(AssertionError):
            run_chain("manual", BETA1, plant=plant, only=[shape], record=False)


# ================================================================================================================================
# 3. - 6. the public surface
# ================================================================================================================================
def test_public_adafactor_takes_beta1():
    from neurosis_amd.optimizers import Adafactor

    opt = Adafactor([torch.nn.Parameter(torch.zeros(8, 8))], beta1=BETA1)
    assert opt.param_groups[0]["beta1"] == BETA1 and opt.defaults["beta1"] == BETA1
    assert Adafactor([torch.nn.Parameter(torch.zeros(8, 8))]).param_groups[0]["beta1"] is None


def _cpu_store():
    """what a FlatAdafactor constructor touches before it refuses: nothing of a store"""
    return SimpleNamespace()


def test_flat_adafactor_still_refuses_beta1_and_names_the_subclass():
    from neurosis_amd.optim import FlatAdafactor, FlatAdafactorMomentum

    assert issubclass(FlatAdafactorMomentum, FlatAdafactor)
    with pytest.raises(NotImplementedError, match="FlatAdafactorMomentum"):
        FlatAdafactor(_cpu_store(), beta1=BETA1)


@pytest.mark.parametrize("beta1", [1.0, -0.1])
def test_invalid_beta1_raises(beta1):
    from neurosis_amd.optim import FlatAdafactorMomentum
    from neurosis_amd.optimizers import Adafactor

    with pytest.raises(ValueError, match="beta1"):
        Adafactor([torch.nn.Parameter(torch.zeros(8, 8))], beta1=beta1)
    with pytest.raises(ValueError, match="beta1"):
        FlatAdafactorMomentum(_cpu_store(), beta1=beta1)
    with pytest.raises(ValueError, match="beta1"):
        FlatAdafactorMomentum(_cpu_store())                      # mandatory


def test_abi_entry_is_bound():
    from neurosis_amd import lib

    assert lib.SIGNATURES["nk_adafactor_chunk_momentum"] == [lib.vp, lib.vp, lib.f32, lib.vp]
    assert hasattr(lib.load(), "nk_adafactor_chunk_momentum")
    assert lib.SIGNATURES["nk_adafactor_chunk"] == [lib.vp, lib.vp]


def test_momentum_checkpoint_entries_must_match():
    """_check_entry refuses, by name, a checkpoint without exp_avg for a momentum optimizer, and one with exp_avg for a momentum-free one"""
    from neurosis_amd.optim import FlatAdafactor, FlatAdafactorMomentum

    z = torch.zeros(4)
    with_m, without = {"exp_avg": z, "exp_avg_sq": z}, {"exp_avg_sq": z}
    for cls, mine, st in ((FlatAdafactorMomentum, with_m, without), (FlatAdafactor, without, with_m)):
        opt = cls.__new__(cls)
        opt.beta1 = BETA1 if cls is FlatAdafactorMomentum else None
        opt._check_entry(0, dict(mine, step=1), mine)
        with pytest.raises(ValueError, match="exp_avg"):
            opt._check_entry(0, dict(st, step=1), mine)
