"""Fused multi-tensor Adafactor on the flat buffers (csrc/optim.hip) against the reference's own steps (golden fixture)
and against the CPU oracle on a larger, SDXL-like parameter set.  fp32 throughout: tolerance 2e-5 relative on parameters
(reduction orders differ), 1e-4 on the factored states.  One step moves a parameter by far less than it is wide, so each step's delta
(p_after - p_before) is compared with the reference's delta as well, at DELTA_TOL / SDXL_DELTA_TOL."""
from pathlib import Path

import pytest
import torch

from tests.util import rel_err
from tests.golden.fixture_io import load_fixture

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"


# rel_err of a step's delta.  Measured on the CPU: the fp32 reference's own delta against the delta of a float64 chain on the same inputs
# (tests/optim_bounds.py::adafactor_ref_step) is at most 6.6e-2 / 4.7e-2 / 3.6e-2 over the three steps of the `relative` fixture (the step
# is 1e-6 of max |p| there: a delta between fp32 masters carries an ulp of |p|) and 1.85e-4 / 1.93e-4 / 1.96e-4 for `manual`; for the
# SDXL-like set and the fp32 CPU oracle 1.12e-1, 3.36e-1, 3.73e-2, 1.64e-1, 1.91e-2 for its five steps.  The tolerance is twice the largest
# measured value (per step for the SDXL-like set): the kernels' deviation and the reference's are independent and of the same kind.
# A step that leaves the masters alone has rel_err 1.
DELTA_TOL = {"relative": 2 * 6.6e-2, "manual": 2 * 1.97e-4}
SDXL_DELTA_TOL = [2 * t for t in (1.12e-1, 3.36e-1, 3.73e-2, 1.64e-1, 1.91e-2)]


def delta_err(p_before, p_after, ref_before, ref_after) -> float:
    return rel_err(p_after.double() - p_before.double(), ref_after.double() - ref_before.double())


def make_store(tensors):
    from neurosis_amd.nn import FlatParamStore

    # conv weights live channels-last (the store's physical layout is [O][KH][KW][I])
    params = [torch.nn.Parameter(t.clone().cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.clone().cuda()) for t in tensors]
    return FlatParamStore(params), params


def set_grads(params, grads, scale=1.0):
    for p, g in zip(params, grads):
        p.grad.copy_(g.cuda() * scale)


@pytest.mark.parametrize("streams", ["1", "2"])
@pytest.mark.parametrize("tag", ["relative", "manual"])
def test_flat_adafactor_matches_reference_steps(tag, streams, monkeypatch):
    """(streams = 2: NK_AF_STREAMS=2, consecutive chunks alternating between two streams with a workspace each)"""
    from neurosis_amd.optim import FlatAdafactor

    monkeypatch.setenv("NK_AF_STREAMS", streams)
    c = load_fixture("adafactor_steps")[tag]
    store, params = make_store(c["init"])
    opt = FlatAdafactor(store, chunk_bytes=8 << 10, **c["kwargs"])   # tiny chunks: several chunks even for this small set
    assert len(opt.chunks) > 2
    for s in range(3):
        set_grads(params, c["grads"][s])
        before = [p.detach().cpu().clone() for p in params]
        opt.step()
        torch.cuda.synchronize()
        for p, want in zip(params, c["after"][s]):
            assert rel_err(p.detach().cpu(), want) <= 2e-5, (s, tuple(p.shape))
        for p, p0, want0, want in zip(params, before, c["after"][s - 1] if s else c["init"], c["after"][s]):
            assert delta_err(p0, p.detach().cpu(), want0, want) <= DELTA_TOL[tag], (s, tuple(p.shape))
        # the bf16 shadows the kernels read follow the masters
        for p in params:
            from neurosis_amd import ops

            assert rel_err(ops._phys_flat(p).float().cpu(), p._nk_shadow.float().cpu()) <= 1e-2
    for i, want in enumerate(c["states"]):
        got = opt.param_state(i)
        for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            if k in want:
                assert rel_err(got[k].cpu(), want[k]) <= 1e-4, (i, k)
    # grad_scale (the data-parallel mean): scaled gradients + grad_scale == unscaled gradients
    store2, params2 = make_store(c["init"])
    opt2 = FlatAdafactor(store2, **c["kwargs"])
    set_grads(params2, c["grads"][0], scale=4.0)
    opt2.step(grad_scale=0.25)
    for p, p0, want in zip(params2, c["init"], c["after"][0]):
        assert rel_err(p.detach().cpu(), want) <= 2e-5
        assert delta_err(p0, p.detach().cpu(), p0, want) <= DELTA_TOL[tag], tuple(p.shape)


def _adafactor_run(c, steps, scale=1.0, grad_scale=1.0):
    """master, shadow and state after `steps` steps of the golden case `c` in 8 KiB chunks (the fixture has three steps of gradients: a
    fourth step takes the first's again)"""
    from neurosis_amd.optim import FlatAdafactor

    store, params = make_store(c["init"])
    opt = FlatAdafactor(store, chunk_bytes=8 << 10, **c["kwargs"])
    assert len(opt.chunks) > 2
    for s in range(steps):
        set_grads(params, c["grads"][s % len(c["grads"])], scale=scale)
        opt.step(grad_scale=grad_scale)
    torch.cuda.synchronize()
    return store.master.clone(), store.shadow.clone(), opt.state.clone()


@pytest.mark.parametrize("streams", ["1", "2"])
@pytest.mark.parametrize("tag", ["relative", "manual"])
def test_bitwise_deterministic(tag, streams, monkeypatch):
    """Fixed-order partial sums, no atomics on values: two runs give the same bits."""
    monkeypatch.setenv("NK_AF_STREAMS", streams)
    c = load_fixture("adafactor_steps")[tag]
    for a, b in zip(_adafactor_run(c, 4), _adafactor_run(c, 4)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("streams", ["1", "2"])
@pytest.mark.parametrize("tag", ["relative", "manual"])
def test_grad_scale_is_exact(tag, streams, monkeypatch):
    """grad_scale (the data-parallel mean): 4 g with grad_scale 0.25 is g, bit for bit."""
    monkeypatch.setenv("NK_AF_STREAMS", streams)
    c = load_fixture("adafactor_steps")[tag]
    for a, b in zip(_adafactor_run(c, 4), _adafactor_run(c, 4, scale=4.0, grad_scale=0.25)):
        assert torch.equal(a, b)


def test_flat_adafactor_sdxl_like_shapes_vs_oracle():
    """Real channel counts (ragged tiles: 1280x2048 context projections, 320-channel convs, 4-channel conv_out, 2816 label
    input), five steps, against the CPU oracle: parameters, each step's delta (SDXL_DELTA_TOL), lr, and the factored states at the end."""
    from neurosis_amd.optim import AdafactorScheduler, FlatAdafactor
    from oracle import adafactor_oracle as AO

    g = torch.Generator().manual_seed(7)
    shapes = [(1280, 2048), (2560, 640), (640, 2560), (1280, 2816), (330, 1284), (320, 320, 3, 3), (640, 320, 1, 1), (8, 320, 3, 3),
              (320, 8, 3, 3), (1280,), (5000,), (3,)]
    init = [torch.randn(*s, generator=g) * 0.05 for s in shapes]
    store, params = make_store(init)
    kw = dict(scale_parameter=True, relative_step=True, warmup_init=True)
    opt = FlatAdafactor(store, **kw)
    sched = AdafactorScheduler(opt, initial_lr=4e-7)
    assert sched.get_lr() == [4e-7]
    ref = [t.clone() for t in init]
    sts = [AO.new_state(p) for p in ref]
    for s in range(5):
        grads = [torch.randn(*sh, generator=g) * (0.1 if s % 2 else 3.0) for sh in shapes]
        set_grads(params, grads)
        before, ref_before = [p.detach().cpu().clone() for p in params], [t.clone() for t in ref]
        opt.step()
        lrs = [AO.step_tensor(p, gr, st, **kw) for p, gr, st in zip(ref, grads, sts)]
        torch.cuda.synchronize()
        for p, want in zip(params, ref):
            assert rel_err(p.detach().cpu(), want) <= 2e-5, (s, tuple(p.shape))
        for p, p0, want0, want in zip(params, before, ref_before, ref):
            assert delta_err(p0, p.detach().cpu(), want0, want) <= SDXL_DELTA_TOL[s], (s, tuple(p.shape))
        # lr = max(eps2, RMS(p)) * rel_step: torch's CPU norm over 2-4 M elements carries ~1e-5..1e-4 of fp32 accumulation noise
        assert rel_err(opt.current_lrs().cpu(), torch.tensor(lrs)) <= 3e-4
    assert abs(sched.get_lr()[0] - lrs[0]) <= 3e-4 * lrs[0]
    for i, want in enumerate(sts):
        got = opt.param_state(i)
        for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            if k in want:
                assert tuple(got[k].shape) == tuple(want[k].shape), (i, k)
                assert rel_err(got[k].cpu(), want[k]) <= 1e-4, (i, k)


def test_flat_adafactor_argument_errors():
    from neurosis_amd.optim import FlatAdafactor

    store, _ = make_store([torch.zeros(8, 8)])
    with pytest.raises(ValueError):
        FlatAdafactor(store, lr=1e-3, relative_step=True)
    with pytest.raises(ValueError):
        FlatAdafactor(store, lr=1e-3, relative_step=False, warmup_init=True)
    with pytest.raises(NotImplementedError):
        FlatAdafactor(store, beta1=0.9)


def test_flat_ema_matches_lit_ema_rule():
    """modules/ema.py:40-59: shadow -= (1 - d) * (shadow - p), d = min(decay, (1+n)/(10+n)); store / copy_to / restore."""
    from neurosis_amd.optim import FlatEma

    g = torch.Generator().manual_seed(3)
    init = [torch.randn(40, 24, generator=g), torch.randn(8, 8, 3, 3, generator=g), torch.randn(17, generator=g)]
    store, params = make_store(init)
    ema = FlatEma(store, decay=0.999)
    ref = [t.clone() for t in init]
    cur = [t.clone() for t in init]
    for n in range(1, 4):
        cur = [c + 0.1 * torch.randn(c.shape, generator=g) for c in cur]
        with torch.no_grad():
            for p, c in zip(params, cur):
                p.copy_(c.cuda())
        ema.update()
        d = min(0.999, (1 + n) / (10 + n))
        ref = [r - (1.0 - d) * (r - c) for r, c in zip(ref, cur)]
    torch.cuda.synchronize()
    ema.store()
    ema.copy_to()
    for p, want in zip(params, ref):
        assert rel_err(p.detach().cpu(), want) <= 1e-6
    ema.restore()
    for p, want in zip(params, cur):
        assert rel_err(p.detach().cpu(), want) <= 1e-6
