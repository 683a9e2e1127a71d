"""Fused multi-tensor CAME on the flat buffers (csrc/came.hip) against the reference's own steps (golden fixture came_steps), against
an fp64 restatement of the reference step on a larger SDXL-like parameter set, and inside the engine (hipGraph replay, gradient
accumulation, the backward-health gate).  fp32 throughout: 2e-5 relative on parameters (reduction orders differ), 1e-4 on states.  One
step moves a parameter by far less than it is wide, so each step's delta (p_after - p_before) is compared with the reference's as well."""
import json
import os
from functools import partial
from pathlib import Path

import pytest
import torch

from tests.test_came_cpu import came_ref_step, load_came_case
from tests.util import rel_err

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
KEYS = ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col", "exp_avg_sq")


@pytest.fixture(autouse=True)
def _clean_health():
    from neurosis_amd import lib

    lib.call("nk_health_clear")
    yield
    lib.call("nk_health_clear")


# rel_err of a step's delta.  For the fixture, measured on the CPU: the fp32 reference's deltas against the deltas of the float64 chain of
# came_ref_step on the same inputs are at most 1.03e-3 (default), 1.76e-3 (decay) and 9.7e-5 (fixed) over the four steps; the tolerance
# is twice that: the kernels' deviation and the reference's are independent and of the same kind.  A step that leaves the masters alone
# has rel_err 1.
# On the SDXL-like set the reference is float64 itself, so what it lacks is the fp32 format of the masters, and that is computed, not
# sampled: a delta between fp32 masters is off by half an ulp of p twice (the master the step started from against the float64 chain's,
# and the rounding of the new one), 2^-23 max |p| at most, which delta_floor() puts in relation to the reference delta per tensor
# (6e-6 for the matrices, 2e-4 .. 2e-3 for the vectors, whose update is lr m without a second preconditioner).  On top, the arithmetic:
# twice the worst per-element bound of one CAME step's p_new relative to its update, 900 U (tests/optim_bounds.py), the factor two for
# the drift of the states over three steps.  (A first version took twice the floor as sampled from the float64 chain, 2 x 1.95e-4 on the
# third step; the five-element vector came out at 4.8e-4 under a floor of 8.2e-4: rounding luck of five values, not arithmetic.)
DELTA_TOL = {"default": 2 * 1.03e-3, "decay": 2 * 1.76e-3, "fixed": 2 * 9.7e-5}
SDXL_DELTA_ARITH = 2 * 900 * 2.0 ** -24


def delta_floor(ref_before, ref_after) -> float:
    return float(2.0 ** -23 * ref_after.abs().max() / (ref_after - ref_before).abs().max())


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


@pytest.mark.parametrize("tag", ["default", "decay", "fixed"])
def test_flat_came_matches_reference_steps(tag):
    from neurosis_amd import ops
    from neurosis_amd.optim import FlatCAME

    c = load_came_case(tag)
    store, params = make_store(c["init"])
    opt = FlatCAME(store, chunk_bytes=8 << 10, **c["kwargs"])      # tiny chunks: several chunks even for this small set
    assert len(opt.chunks) > 2
    for s in range(4):
        set_grads(params, c["grads"][s])
        before = [p.detach().cpu().clone() for p in params]
        opt.step()
        torch.cuda.synchronize()
        for p, want in zip(params, c["after"][s]):
            assert rel_err(p.detach().cpu(), want) <= 2e-5, (s, tuple(p.shape))
        for p, p0, want0, want in zip(params, before, c["after"][s - 1] if s else c["init"], c["after"][s]):
            assert delta_err(p0, p.detach().cpu(), want0, want) <= DELTA_TOL[tag], (s, tuple(p.shape))
        for p in params:          # the bf16 shadows the kernels read follow the masters
            assert rel_err(ops._phys_flat(p).float().cpu(), p._nk_shadow.float().cpu()) <= 1e-2
    for i, want in enumerate(c["states"]):
        got = opt.param_state(i)
        assert set(got) == set(want)
        for k, v in want.items():
            assert tuple(got[k].shape) == tuple(v.shape), (i, k)
            assert rel_err(got[k].cpu(), v) <= 1e-4, (i, k)


def test_grad_scale_is_exact():
    """grad_scale (the data-parallel mean): 4 g with grad_scale 0.25 is g, bit for bit."""
    from neurosis_amd.optim import FlatCAME

    c = load_came_case("fixed")
    runs = []
    for scale, gs in ((1.0, 1.0), (4.0, 0.25)):
        store, params = make_store(c["init"])
        opt = FlatCAME(store, chunk_bytes=8 << 10, **c["kwargs"])
        for s in range(2):
            set_grads(params, c["grads"][s], scale=scale)
            opt.step(grad_scale=gs)
        torch.cuda.synchronize()
        runs.append((store.master.clone(), store.shadow.clone(), opt.state.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_bitwise_deterministic():
    from neurosis_amd.optim import FlatCAME

    c = load_came_case("decay")
    runs = []
    for _ in range(2):
        store, params = make_store(c["init"])
        opt = FlatCAME(store, chunk_bytes=8 << 10, **c["kwargs"])
        for s in range(4):
            set_grads(params, c["grads"][s])
            opt.step()
        torch.cuda.synchronize()
        runs.append((store.master.clone(), store.shadow.clone(), opt.state.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_flat_came_sdxl_like_shapes_vs_fp64():
    """Real channel counts (ragged tiles: a 1000 x 1284 matrix, 320-channel convs, 4-channel conv_out), three steps with update
    clipping on the large one, against the fp64 restatement of the reference step."""
    from neurosis_amd.optim import FlatCAME

    g = torch.Generator().manual_seed(11)
    shapes = [(1280, 1280), (10240, 1280), (640, 2048), (320, 320, 3, 3), (4, 320, 3, 3), (1280,), (5,), (1000, 1284)]
    init = [torch.randn(*s, generator=g) * 0.05 for s in shapes]
    kw = dict(lr=1e-4, betas=(0.9, 0.999, 0.9999), weight_decay=1e-2)
    store, params = make_store(init)
    opt = FlatCAME(store, **kw)
    ref = [t.double() for t in init]
    sts = [{} for _ in shapes]
    for s, mag in enumerate((1.0, 10.0, 0.1)):
        grads = [torch.randn(*sh, generator=g) * mag for sh in shapes]
        set_grads(params, grads)
        before, ref_before = [p.detach().cpu().clone() for p in params], ref
        opt.step()
        ref = [came_ref_step(p, gr, st, **kw) for p, gr, st in zip(ref, grads, sts)]
        torch.cuda.synchronize()
        for p, want in zip(params, ref):
            assert rel_err(p.detach().cpu(), want) <= 1e-5, (s, tuple(p.shape))
        for p, p0, want0, want in zip(params, before, ref_before, ref):
            assert delta_err(p0, p.detach().cpu(), want0, want) <= SDXL_DELTA_ARITH + delta_floor(want0, want), (s, tuple(p.shape))
    for i, st in enumerate(sts):
        got = opt.param_state(i)
        for k, v in st.items():
            assert rel_err(got[k].cpu(), v) <= 1e-4, (i, k)


def test_checkpoint_round_trip_through_the_optimizer_api():
    """state_dict -> a new CAME on a copy of the parameters -> load_state_dict -> one more step: the same bits as the run that
    went on uninterrupted.  Keys and shapes are the reference's."""
    from neurosis_amd.optimizers.came import CAME

    c = load_came_case("fixed")
    store, params = make_store(c["init"])
    opt = CAME(params, **c["kwargs"])
    for s in range(3):
        set_grads(params, c["grads"][s])
        opt.step()
    sd = opt.state_dict()
    assert sd["param_groups"][0]["step"] == 3
    for i, want in enumerate(c["states"]):
        assert {k: tuple(v.shape) for k, v in sd["state"][i].items()} == {k: tuple(v.shape) for k, v in want.items()}
    store2, params2 = make_store([p.detach().cpu() for p in params])
    opt2 = CAME(params2, **c["kwargs"])
    opt2.load_state_dict(sd)
    for o, ps in ((opt, params), (opt2, params2)):
        set_grads(ps, c["grads"][3])
        o.step()
    torch.cuda.synchronize()
    assert torch.equal(store.master, store2.master) and torch.equal(store.shadow, store2.shadow)
    assert opt2.param_groups[0]["step"] == 4
    for i in range(len(params)):
        a, b = opt.flat.param_state(i), opt2.flat.param_state(i)
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_lr_follows_the_group():
    """An LR scheduler edits the group's lr: the next step uses it."""
    from neurosis_amd.optimizers.came import CAME

    c = load_came_case("default")
    store, params = make_store(c["init"])
    opt = CAME(params, lr=1.0)
    torch.optim.lr_scheduler.LambdaLR(opt, lambda _: 1e-3)      # sets the group's lr to 1.0 * 1e-3 = the fixture's
    set_grads(params, c["grads"][0])
    opt.step()
    torch.cuda.synchronize()
    for p, want in zip(params, c["after"][0]):
        assert rel_err(p.detach().cpu(), want) <= 2e-5


# -- inside the engine ---------------------------------------------------------------------------------------------------------------
def _engine():
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models import DiffusionEngine
    from neurosis_amd.optimizers.came import CAME
    from tests.golden.make_golden import UNET_TINY, synth_state_dict

    net = D.UNetModel(**UNET_TINY)
    net.load_state_dict(synth_state_dict(json.loads((G / "unet_sdxl_tiny_keys.json").read_text())))
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=None, optimizer=partial(CAME, lr=1e-4),
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())).cuda()
    eng.setup_flat_params()
    assert isinstance(eng._torch_optimizer, CAME)
    return eng


def _batches(n):
    from tests.golden.make_golden import UNET_TINY

    g = torch.Generator().manual_seed(5)
    return [dict(x=torch.randn(2, 4, 16, 16, generator=g).cuda(), noise=torch.randn(2, 4, 16, 16, generator=g).cuda(),
                 sigma=(torch.rand(2, generator=g) * 5 + 0.1).cuda(),
                 cond={"crossattn": torch.randn(2, 77, UNET_TINY["context_dim"], generator=g).cuda(),
                       "vector": torch.randn(2, UNET_TINY["adm_in_channels"], generator=g).cuda()}) for _ in range(n)]


def _fwd_bwd(eng, b):
    eng(b["x"], b["cond"], sigmas=b["sigma"], noise=b["noise"]).mean().backward()


def _engine_steps(graph: str, batches):
    os.environ["NK_GRAPH"] = graph
    try:
        eng = _engine()
        m0 = eng.store.master.clone()
        for b in batches:
            _fwd_bwd(eng, b)
            eng.optimizer_step()
        eng.join_optimizer()
        torch.cuda.synchronize()
        return eng, m0
    finally:
        os.environ.pop("NK_GRAPH", None)


def test_engine_steps_with_graph_replay_match_the_eager_chain():
    batches = _batches(3)
    eng_g, m0 = _engine_steps("1", batches)
    eng_e, _ = _engine_steps("0", batches)
    cg = eng_g.model.diffusion_model._nk_graphs
    assert cg is not None and cg.replays > 0, "the graphed run did not replay"
    assert eng_e.model.diffusion_model._nk_graphs is None
    assert not torch.equal(eng_g.store.master, m0) and bool(torch.isfinite(eng_g.store.master).all())
    assert eng_g._torch_optimizer.param_groups[0]["step"] == 3
    assert torch.equal(eng_g.store.master, eng_e.store.master)
    assert torch.equal(eng_g.store.shadow, eng_e.store.shadow)


def test_engine_flagged_backward_is_not_applied_and_is_reported():
    from neurosis_amd import lib, ops

    eng = _engine()
    b = _batches(1)[0]

    def step():
        _fwd_bwd(eng, b)
        eng.optimizer_step()

    step()
    torch.cuda.synchronize()
    m0, s0 = eng.store.master.clone(), eng.store.shadow.clone()
    lib.call("nk_debug_raise_health", ops._stream())          # what a give-up inside this step's backward does
    step()                                                      # the update kernels see the word and touch nothing
    torch.cuda.synchronize()
    assert torch.equal(eng.store.master, m0) and torch.equal(eng.store.shadow, s0)
    with pytest.raises(lib.NkError, match="health"):            # ... and the next update refuses on the host
        step()


def test_engine_two_micro_batches_are_one_step_on_the_summed_gradients():
    from neurosis_amd.optim import FlatCAME

    eng = _engine()
    b0, b1 = _batches(2)
    eng.accumulate(0, last=False)
    _fwd_bwd(eng, b0)
    torch.cuda.synchronize()
    g0 = eng.store.grad.clone()
    eng.accumulate(1, last=True)
    _fwd_bwd(eng, b1)
    torch.cuda.synchronize()
    g_sum = eng.store.grad.clone()
    assert not torch.equal(g_sum, g0), "the second micro-batch did not add to the gradients"
    init = [p.detach().cpu() for p in eng.store.params]
    grads = [p.grad.detach().cpu() for p in eng.store.params]
    eng.optimizer_step()
    eng.join_optimizer()
    torch.cuda.synchronize()
    store, params = make_store(init)
    assert store.offsets == eng.store.offsets
    set_grads(params, grads)
    assert torch.equal(store.grad, g_sum)
    FlatCAME(store, lr=1e-4).step()
    torch.cuda.synchronize()
    assert torch.equal(store.master, eng.store.master)
    assert torch.equal(store.shadow, eng.store.shadow)
