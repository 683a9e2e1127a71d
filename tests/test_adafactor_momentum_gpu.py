"""Adafactor's first moment (beta1) on the GPU: af_apply_momentum_kernel (csrc/optim.hip) behind the unchanged statistics passes, through
FlatAdafactorMomentum, the public Adafactor class and DiffusionEngine.

  per element   every step is a single step: masters, state and exp_avg are read back, one float64 step is taken from exactly those values
                (tests/optim_momentum_bounds.py) and p, exp_avg, the statistics, lr_t, scale and RMS(p) from the partial sums of p^2 are
                compared per element at their derived bounds; store, gradients and cases are those of tests/test_optim_kernels_gpu.py
                (ob.SHAPES, ob.inputs(), ob.AF_CASES), at beta1 = 0.9 and beta1 = 0.0.  From the second step on exp_avg is non-zero.
  same bits     small chunks, the store reversed, two streams, the chunks one by one in reverse order, a second run, and 4 g with a quarter
                of the grad_scale give the bits of the one-chunk run: masters, shadows, statistics, exp_avg, lr_t, scale.
  the fixture   the reference class's own three steps with beta1 = 0.9 (tests/golden/adafactor_beta1_steps), at the tolerances of
                tests/test_adafactor_momentum_cpu.py.
  the engine    a checkpoint after two steps resumes bit for bit, the streamed per-block update gives the same bits, a checkpoint without
                exp_avg is refused by name; the sharded exchange is refused.

Largest error / bound on the MI355X | by the fp32 restatement of tests/test_adafactor_momentum_cpu.py ("[optim ratio] adafactor-m..." in both):
  beta1 = 0.9   p 0.798 | 0.798, exp_avg 0.635 | 0.637, row 0.662 | 0.662, col 0.656 | 0.656, v 0.634 | 0.634, lr_t 0.300 | 0.300, scale 0.300 | 0.300, rms_p 0.100
  beta1 = 0.0   p 0.797 | 0.797, exp_avg 0.199 | 0.199, row 0.662 | 0.662, col 0.656 | 0.656, v 0.634 | 0.634, lr_t 0.300 | 0.300, scale 0.300 | 0.300, rms_p 0.113
(the restatement does not form RMS(p)).  Against the fixture, largest over tensors and steps: parameters 7.2e-8 / 2.7e-7 (`relative` / `manual`,
tolerance 2e-5), a step's delta 8.9e-5 / 1.95e-3 (tolerance 1.76e-4 / 3.3e-3).
"""
import json
from functools import partial
from types import SimpleNamespace

import pytest
import torch

from tests import optim_bounds as ob
from tests import optim_momentum_bounds as omb
from tests.golden.fixture_io import load_fixture
from tests.test_adafactor_momentum_cpu import BETA1, DELTA_TOL, PARAM_TOL, STATE_TOL, delta_err
from tests.test_optim_kernels_gpu import AF_KEYS, _clean_health, _host, _kinds_in_later_chunks, _same, _state, make_store  # noqa: F401  (_clean_health: autouse)
from tests.test_text_encoder_train_gpu import _check
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def _run(case, beta1, order, chunk_bytes, verify, reverse_chunks=False, gmul=1.0):
    """ob.STEPS steps of one case of ob.AF_CASES over the tensors ob.SHAPES[i], i in `order`, with the gradients times `gmul` and grad_scale
    divided by it; with `verify` every step is checked against float64 from the device's own masters, state and exp_avg.  Returns what
    tests/test_optim_kernels_gpu.py::_run returns (the state includes exp_avg)."""
    from neurosis_amd.optim import FlatAdafactorMomentum

    c = ob.AF_CASES[case]
    who = f"adafactor-m{beta1}"
    init, grads = ob.inputs()
    store, params = make_store([init[i] for i in order])
    opt = FlatAdafactorMomentum(store, beta1=beta1, chunk_bytes=chunk_bytes, **c["kwargs"])
    assert opt.exp_avg.numel() == store.master.numel() and opt.exp_avg.dtype == torch.float32
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
            p.grad.copy_(grads[s][i].cuda() * gmul)
        torch.cuda.synchronize()
        before = [(_host(p), _state(opt, j)) for j, p in enumerate(params)] if verify else None
        if reverse_chunks:
            opt.begin_step()
            for ci in reversed(range(len(opt.chunks))):
                opt.step_chunk(ci, c["grad_scale"] / gmul)
            opt.end_step()
        else:
            opt.step(grad_scale=c["grad_scale"] / gmul)
        torch.cuda.synchronize()
        assert not bool(opt.counters.any()), f"{who} {case} step {s + 1}: a 'blocks done' counter is not back at zero"
        if not verify:
            continue
        for j, (p, i) in enumerate(zip(params, order)):
            shape, (p0, st0) = ob.SHAPES[i], before[j]
            label = f"{who} {case} step {s + 1} {shape}"
            st1, p1 = _state(opt, j), _host(p)
            m0 = st0.pop("exp_avg")
            # (at beta1 = 0 the moment is the last update itself: zero behind a zero gradient)
            moved = s > 0 and not (beta1 == 0.0 and shape in ob.ZERO_GRAD.get(s - 1, ()))
            assert tuple(m0.shape) == tuple(shape) and bool(m0.any()) == moved, f"{label}: exp_avg before the step"
            want = omb.adafactor_m_expected(p0, grads[s][i], st0, m0, s + 1, beta1, c["grad_scale"], **c["kwargs"])
            got = {k: st1[key] for k, key in AF_KEYS.items() if key in st1}
            got.update(p=p1, exp_avg=st1["exp_avg"], lr_t=opt.lr_t[j].cpu(), scale=opt.scale[j].cpu())
            assert set(got) == set(want), (label, sorted(got), sorted(want))
            ob.verify(who, label, got, want, _check)
            must = ob.must_move(p0, *want["p"])
            must_move += int(must.sum())
            assert bool((p1 != p0)[must].all()), f"{label}: {int((p1 == p0)[must].sum())} masters whose update exceeds its bound by an ulp did not move"
            t = opt._tens_np[j]
            parts = opt.p2_part[int(t["item0"]):int(t["item0"]) + int(t["nitems"])].double().sum().cpu()
            ob.verify(who, label, {"rms_p": (parts / p1.numel()).sqrt()}, {"rms_p": ob.p2_expected(p1, shape)}, _check)
    if verify:
        assert must_move > 0, "no update of this case can be told from rounding: the case checks nothing"
    torch.cuda.synchronize()
    tensors = {i: (_host(p), _state(opt, j), _host(p._nk_shadow)) for j, (p, i) in enumerate(zip(params, order))}
    scalars = {i: [_host(t[j]) for t in (opt.lr_t, opt.scale)] for j, i in enumerate(order)}
    return tensors, scalars


@pytest.mark.parametrize("beta1", [BETA1, 0.0])
@pytest.mark.parametrize("case", list(ob.AF_CASES))
def test_momentum_steps_per_element(case, beta1, monkeypatch):
    monkeypatch.setenv("NK_AF_STREAMS", "1")
    _run(case, beta1, list(range(len(ob.SHAPES))), None, True)
    ob.report(f"adafactor-m{beta1}")


@pytest.mark.parametrize("beta1", [BETA1, 0.0])
@pytest.mark.parametrize("case", list(ob.AF_CASES))
def test_momentum_same_bits(case, beta1, monkeypatch):
    """masters, shadows, statistics, exp_avg, lr_t and scale, bit for bit: exp_avg never crosses a tensor, so neither the chunking nor
    the order of the chunks nor the stream they run on can matter"""
    order = list(range(len(ob.SHAPES)))
    monkeypatch.setenv("NK_AF_STREAMS", "1")
    base = _run(case, beta1, order, None, False)
    assert all("exp_avg" in st for _, st, _ in base[0].values())
    _same("a second run", base, _run(case, beta1, order, None, False))
    _same("small chunks", base, _run(case, beta1, order, ob.CHUNK_BYTES, False))
    _same("reversed store", base, _run(case, beta1, order[::-1], ob.CHUNK_BYTES, False))
    _same("chunk by chunk in reverse order", base, _run(case, beta1, order, ob.CHUNK_BYTES, False, reverse_chunks=True))
    _same("4 g with a quarter of the grad_scale", base, _run(case, beta1, order, ob.CHUNK_BYTES, False, gmul=4.0))
    monkeypatch.setenv("NK_AF_STREAMS", "2")
    _same("two streams", base, _run(case, beta1, order, ob.CHUNK_BYTES, False))


@pytest.mark.parametrize("tag", ["relative", "manual"])
def test_momentum_matches_reference_steps(tag):
    """the reference class's own three steps with beta1 = 0.9, through FlatAdafactorMomentum in 8 KiB chunks"""
    from neurosis_amd.optim import FlatAdafactorMomentum

    c = load_fixture("adafactor_beta1_steps")[tag]
    store, params = make_store(c["init"])
    opt = FlatAdafactorMomentum(store, chunk_bytes=8 << 10, **c["kwargs"])
    assert len(opt.chunks) > 2 and opt.beta1 == BETA1
    for s in range(3):
        for p, g in zip(params, c["grads"][s]):
            p.grad.copy_(g.cuda())
        before = [p.detach().cpu().clone() for p in params]
        opt.step()
        torch.cuda.synchronize()
        for p, p0, want0, want in zip(params, before, c["after"][s - 1] if s else c["init"], c["after"][s]):
            err, derr = rel_err(p.detach().cpu(), want), delta_err(p0, p.detach().cpu(), want0, want)
            print(f"[adafactor-m fixture] {tag} step {s + 1} {tuple(p.shape)}: parameters {err:.3g}, delta {derr:.3g}")
            assert err <= PARAM_TOL, (s, tuple(p.shape))
            assert derr <= DELTA_TOL[tag], (s, tuple(p.shape))
    for i, want in enumerate(c["states"]):
        got = opt.param_state(i)
        for k in ("exp_avg", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq"):
            assert (k in want) == (k in got), (i, k)
            if k in want:
                assert tuple(got[k].shape) == tuple(want[k].shape), (i, k)
                assert rel_err(got[k].cpu(), want[k]) <= STATE_TOL, (i, k)


# ================================================================================================================================
# checkpoint and engine
# ================================================================================================================================
def _engine(stream=False, **adafactor):
    """the tiny engine of tests/test_loss_class_gpu.py::_engine with the public Adafactor; `stream`: the per-block update behind backward
    (set before the flat store exists, so that configure_optimizers cuts the chunks at the blocks)"""
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models import AutoencoderKL, DiffusionEngine
    from neurosis_amd.optimizers import Adafactor
    from tests.golden.make_golden import UNET_TINY, VAE_TINY, synth_state_dict
    from tests.test_loss_class_gpu import G

    keys = json.loads((G / "engine_tiny_keys.json").read_text())
    net = D.UNetModel(**UNET_TINY)
    net.load_state_dict(synth_state_dict(keys["unet"]))
    vae = AutoencoderKL(embed_dim=4, ddconfig={k: v for k, v in VAE_TINY.items() if k != "embed_dim"})
    vae.load_state_dict({k: v for k, v in synth_state_dict(keys["vae"]).items() if not k.startswith(("encoder.quant_conv", "decoder.post_quant_conv"))})
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=vae, scale_factor=0.13025, input_key="image", vae_batch_size=2,
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting()),
                          optimizer=partial(Adafactor, **adafactor)).cuda()
    eng.stream_optimizer = stream
    eng.setup_flat_params()
    return eng


# a manual lr: with scale_parameter the resumed run recomputes the partial sums of p^2 with af_init_p2_kernel, whose sums are not pass C's
# bit for bit (RMS(p) agrees to rounding: tests/test_loss_class_gpu.py compares such a resume at 1e-3), and this test is about exp_avg
ENGINE_KW = dict(lr=1e-3, relative_step=False, scale_parameter=False, weight_decay=1e-2)


def test_engine_checkpoint_and_streamed_update_keep_the_bits():
    from neurosis_amd.optim import FlatAdafactorMomentum
    from neurosis_amd.optimizers import Adafactor

    e = load_fixture("engine_tiny")
    batch = lambda: {"image": e["image"].cuda(), "crossattn": e["crossattn"].cuda(), "vector": e["vector"].cuda()}

    def step(eng, seed, streamed=False):
        g = torch.Generator(device="cuda").manual_seed(seed)
        noise = torch.randn(e["noise"].shape, device="cuda", generator=g)
        eng.training_step(batch(), 0, sigmas=e["sigma"].cuda(), noise=noise).backward()
        assert eng._streaming_step is streamed          # the hook fired during backward (or not)
        eng.optimizer_step()
        eng.join_optimizer()
        torch.cuda.synchronize()

    def bits(eng):
        return eng.store.master.clone(), eng.store.shadow.clone(), eng.adafactor.state.clone(), eng.adafactor.exp_avg.clone()

    a = _engine(beta1=BETA1, **ENGINE_KW)
    assert isinstance(a._torch_optimizer, Adafactor) and isinstance(a.adafactor, FlatAdafactorMomentum) and a.adafactor is a._torch_optimizer.flat
    step(a, 1)
    step(a, 2)
    sd = {k: v.detach().clone() for k, v in a.state_dict().items()}
    osd = a._torch_optimizer.state_dict()
    assert osd["param_groups"][0]["beta1"] == BETA1
    st0 = osd["state"][0]
    assert int(st0["step"]) == 2 and tuple(st0["exp_avg"].shape) == tuple(a.store.params[0].shape) and bool(st0["exp_avg"].any())
    step(a, 3)

    b = _engine(beta1=BETA1, **ENGINE_KW)
    b.load_state_dict(sd, strict=True)
    b.store.refresh()
    b._torch_optimizer.load_state_dict(osd)
    assert b.adafactor.step_count == 2 and bool(b.adafactor.exp_avg.any())
    step(b, 3)
    for name, x, y in zip(("master", "shadow", "state", "exp_avg"), bits(a), bits(b)):
        assert torch.equal(x, y), f"the third step after a checkpoint round trip: {name} differs from the uninterrupted run's"

    c = _engine(stream=True, beta1=BETA1, **ENGINE_KW)
    assert len(c.adafactor.chunks) > len(a.adafactor.chunks)
    for seed in (1, 2, 3):
        step(c, seed, streamed=True)
    assert c.adafactor.step_count == 3
    for name, x, y in zip(("master", "shadow", "state", "exp_avg"), bits(a), bits(c)):
        assert torch.equal(x, y), f"three streamed steps: {name} differs from the one-shot update's"

    # a checkpoint without a first moment, and the other way round
    plain = _engine(**ENGINE_KW)
    step(plain, 1)
    with pytest.raises(ValueError, match="exp_avg"):
        b._torch_optimizer.load_state_dict(plain._torch_optimizer.state_dict())
    with pytest.raises(ValueError, match="exp_avg"):
        plain._torch_optimizer.load_state_dict(osd)


def test_sharded_exchange_is_refused():
    from neurosis_amd.optim import FlatAdafactorMomentum

    store, _ = make_store([torch.zeros(8, 8), torch.zeros(16)])
    opt = FlatAdafactorMomentum(store, beta1=BETA1)
    with pytest.raises(NotImplementedError, match="beta1"):
        opt.restrict_ranges([(0, 1)])
    with pytest.raises(NotImplementedError, match="beta1"):
        opt.restrict(0, 1)
    eng = SimpleNamespace(store=store, adafactor=opt, model_ema=None, _streaming_step=False)
    from neurosis_amd.models import DiffusionEngine

    with pytest.raises(NotImplementedError, match="beta1"):
        DiffusionEngine.optimizer_step(eng, dp=SimpleNamespace(sharded=True))
