"""The ADM block family on the GPU: the modulated GroupNorm and resampling kernels against the float64 restatement (tests/adm_ref.py), the
ResBlock variants and a tiny scale-shift + updown UNet against fixtures captured from the reference (tests/golden/make_golden_adm.py).

Tolerances are the ones the unmodulated paths are already held to: TOL_BF16 = 2e-2 / TOL_F32 = 1e-2 of tests/test_kernels_gpu.py for the
kernels (dmod is a bf16 output of fp32 sums: held like dgamma / dbeta, 1e-2 of its own scale), the bounds of
test_blocks_real_width.py::test_hip_blocks_match_the_reference_at_real_widths for the blocks and those of tests/test_modules_gpu.py for the
tiny UNet.  A large activation is compared at the pixels its fixture holds, plus its norm."""
import json
import os
from pathlib import Path

import pytest
import torch

from tests import adm_ref as R
from tests.golden.fixture_io import load_fixture
from tests.golden.make_golden import BLOCK_SAMPLE_ROWS, VAE_TINY, block_inputs, block_upstream, synth_state_dict
from tests.golden.make_golden_adm import ADM_BLOCK_CASES, CONV_SAMPLE_CIN, unet_inputs
from tests.util import _call_into, assert_close, bf16_round, check_grad_cosines, cosine, rel_err

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
BF = torch.bfloat16
TOL_BF16 = 2e-2      # tests/test_kernels_gpu.py
TOL_F32 = 1e-2


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


@pytest.fixture(scope="module")
def blocks():
    return load_fixture("adm_blocks")


@pytest.fixture(scope="module")
def unets():
    return load_fixture("unet_adm_tiny")


def rnd(*shape, seed, scale=1.0):
    return bf16_round(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale)


def tok(t):
    """[N, C, H, W] -> channels-last bf16 tokens on the GPU"""
    return t.detach().to("cuda", BF).permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def untok(t, N, H, W):
    return t.float().cpu().view(N, H, W, -1).permute(0, 3, 1, 2)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


# ------------------------------------------------------------------------------------------------
# 1. the modulated GroupNorm kernels
# ------------------------------------------------------------------------------------------------
GN_SHAPES = [(2, 64, 24, 20), (2, 320, 16, 16), (3, 640, 9, 7)]
_gn_refs = {}


def _gn_case(shape, silu):
    """inputs and the float64 reference (forward, closed-form backward), computed once per (shape, silu)"""
    key = (shape, silu)
    if key not in _gn_refs:
        N, C, H, W = shape
        s = sum(shape)
        x = bf16_round(rnd(N, C, H, W, seed=s) * 2 + 0.5)
        gamma, beta = rnd(C, seed=s + 1) * 0.5 + 1, rnd(C, seed=s + 2) * 0.1
        mod = rnd(N, 2 * C, seed=s + 3, scale=0.7)
        dy, extra = rnd(N, C, H, W, seed=s + 4), rnd(N, C, H, W, seed=s + 5)
        d = lambda t: t.double()
        scale, shift = d(mod[:, :C]), d(mod[:, C:])
        y = R.gn_mod_fwd(d(x), d(gamma), d(beta), scale, shift, 32, 1e-5, silu)
        y_swapped = R.gn_mod_fwd(d(x), d(gamma), d(beta), scale, shift, 32, 1e-5, silu, swap=True)
        dx, dgamma, dbeta, dscale, dshift = R.gn_mod_bwd(d(dy), d(x), d(gamma), d(beta), scale, shift, 32, 1e-5, silu)
        _gn_refs[key] = dict(x=x, gamma=gamma, beta=beta, mod=mod, dy=dy, extra=extra, y=y, y_swapped=y_swapped, dx=dx, dgamma=dgamma, dbeta=dbeta,
                             dmod=torch.cat([dscale, dshift], 1))
    return _gn_refs[key]


def _gn_run(ops, c, shape, silu, from_sums, with_add, mod=None, accumulate=False, prefill=None):
    N, C, H, W = shape
    w, b = torch.nn.Parameter(c["gamma"].cuda()), torch.nn.Parameter(c["beta"].cuda())
    if prefill is not None:
        w.grad, b.grad = torch.full_like(w, prefill), torch.full_like(b, prefill)
    w._nk_state = ops.EngineState()              # an engine of its own: the accumulate flag stays out of the process-wide default
    w._nk_state.grad_accumulate = accumulate
    img = ops.Img(tok(c["x"]), N, H, W)
    if from_sums:
        img.sums = ops.groupnorm_sums(img, 32)
    m = (c["mod"] if mod is None else mod).to("cuda", BF)
    out, bwd = ops.groupnorm_mod_fwd(img, w, b, m, 32, 1e-5, silu)
    dx, dmod = bwd(tok(c["dy"]), tok(c["extra"]) if with_add else None)
    torch.cuda.synchronize()
    return out.t, dx, dmod, w.grad.clone(), b.grad.clone()


@pytest.mark.parametrize("from_sums", [False, True], ids=["one_call", "from_sums"])
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "dx_add"])
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "linear"])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_modulated_groupnorm_against_float64(ops, shape, silu, with_add, from_sums):
    N, C, H, W = shape
    c = _gn_case(shape, silu)
    y, dx, dmod, dg, db = _gn_run(ops, c, shape, silu, from_sums, with_add)
    want_dx = c["dx"] + (c["extra"].double() if with_add else 0)
    errs = dict(y=rel_err(untok(y, N, H, W), c["y"]), dx=rel_err(untok(dx, N, H, W), want_dx), dgamma=rel_err(dg, c["dgamma"]), dbeta=rel_err(db, c["dbeta"]),
                dmod=rel_err(dmod, c["dmod"]))
    print(f"[gn_mod {shape} silu={silu} add={with_add} sums={from_sums}] " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert_close(untok(y, N, H, W), c["y"], TOL_BF16, "gn_mod fwd")
    assert_close(untok(dx, N, H, W), want_dx, TOL_BF16, "gn_mod dx")
    assert_close(dg, c["dgamma"], TOL_F32, "gn_mod dgamma")
    assert_close(db, c["dbeta"], TOL_F32, "gn_mod dbeta")
    assert_close(dmod, c["dmod"], TOL_F32, "gn_mod dmod")
    # the chunk order: a reference that takes the shift for the scale must NOT pass the forward's assertion
    with pytest.raises(AssertionError):
        assert_close(untok(y, N, H, W), c["y_swapped"], TOL_BF16, "gn_mod fwd against the swapped reference")


@pytest.mark.parametrize("from_sums", [False, True], ids=["one_call", "from_sums"])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_zero_modulation_is_the_plain_groupnorm_bit_for_bit(ops, shape, from_sums):
    N, C, H, W = shape
    c = _gn_case(shape, True)
    y, dx, dmod, dg, db = _gn_run(ops, c, shape, True, from_sums, True, mod=torch.zeros(N, 2 * C))
    w, b = torch.nn.Parameter(c["gamma"].cuda()), torch.nn.Parameter(c["beta"].cuda())
    img = ops.Img(tok(c["x"]), N, H, W)
    if from_sums:
        img.sums = ops.groupnorm_sums(img, 32)
    out, bwd = ops.groupnorm_fwd(img, w, b, 32, 1e-5, True)
    dx0 = bwd(tok(c["dy"]), tok(c["extra"]))
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(out.t)) and torch.equal(bits(dx), bits(dx0))
    assert torch.equal(dg, w.grad) and torch.equal(db, b.grad)
    # d_shift is then dbeta per image, d_scale = gamma * B + beta * A: nonzero although the modulation is
    assert float(dmod.float().abs().max()) > 0


def test_modulated_groupnorm_is_reproducible_and_accumulates(ops):
    shape = GN_SHAPES[2]
    c = _gn_case(shape, True)
    a = _gn_run(ops, c, shape, True, False, True)
    b = _gn_run(ops, c, shape, True, False, True)
    for u, v in zip(a, b):
        assert torch.equal(bits(u), bits(v))
    acc = _gn_run(ops, c, shape, True, False, True, accumulate=True, prefill=3.0)
    assert torch.equal(bits(acc[1]), bits(a[1])) and torch.equal(bits(acc[2]), bits(a[2]))
    assert torch.equal(acc[3], a[3] + 3.0) and torch.equal(acc[4], a[4] + 3.0)
    over = _gn_run(ops, c, shape, True, False, True, accumulate=False, prefill=3.0)
    assert torch.equal(over[3], a[3]) and torch.equal(over[4], a[4])


# ------------------------------------------------------------------------------------------------
# 2. the resamplers
# ------------------------------------------------------------------------------------------------
RS_SHAPES = [(2, 8, 7, 10), (1, 320, 16, 16), (2, 64, 5, 5)]


@pytest.mark.parametrize("kind", ["integers", "randn"])
@pytest.mark.parametrize("shape", RS_SHAPES)
def test_resampling_kernels(ops, shape, kind):
    N, C, H, W = shape
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(sum(shape))
    if kind == "integers":      # sums of four small integers and their quarters are exact in fp32 and (here) in bf16 after ONE rounding
        x = torch.randint(-31, 32, shape, generator=g).float()
        dy = torch.randint(-31, 32, (N, C, Ho, Wo), generator=g).float()
    else:
        x, dy = rnd(*shape, seed=1), rnd(N, C, Ho, Wo, seed=2)
    xt, dyt = tok(x), tok(dy)
    y = _call_into(ops, "nk_avgpool2x_fwd", N * Ho * Wo, C, xt, N, H, W, C)
    dx = _call_into(ops, "nk_avgpool2x_bwd", N * H * W, C, dyt, N, H, W, C)
    up = _call_into(ops, "nk_upsample2x_fwd", N * 4 * H * W, C, xt, N, H, W, C)
    want_y = R.avgpool2x(x.double())
    want_dx = R.avgpool2x_bwd(dy.double(), H, W)
    want_up = R.upsample2x(x.double())
    # nearest upsampling copies, the pool's backward scales by a power of two: exact whatever the values
    assert torch.equal(untok(up, N, 2 * H, 2 * W).double(), want_up)
    assert torch.equal(untok(dx, N, H, W).double(), want_dx)
    if H % 2:
        assert float(untok(dx, N, H, W)[:, :, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(untok(dx, N, H, W)[:, :, :, W - 1].abs().max()) == 0.0
    if kind == "integers":      # the pool's forward: the fp32 sum is exact, so the result is ONE round-to-nearest-even of the exact mean
        assert torch.equal(untok(y, N, Ho, Wo), want_y.float().to(BF).float())
    else:                       # within one bf16 ulp (at most 2^-7 of the value) of float64
        assert bool(((untok(y, N, Ho, Wo).double() - want_y).abs() <= want_y.abs() * 2.0 ** -7).all())
    # and the ops layer hands out the same tensors
    yi, bwd = ops.avgpool2x_fwd(ops.Img(xt, N, H, W))
    assert (yi.N, yi.H, yi.W) == (N, Ho, Wo) and torch.equal(bits(yi.t), bits(y)) and torch.equal(bits(bwd(dyt)), bits(dx))
    ui, ubwd = ops.upsample2x_fwd(ops.Img(xt, N, H, W))
    assert (ui.H, ui.W) == (2 * H, 2 * W) and torch.equal(bits(ui.t), bits(up))
    dup = tok(torch.randint(-7, 8, (N, C, 2 * H, 2 * W), generator=g).float())
    assert torch.equal(untok(ubwd(dup), N, H, W).double(), R.upsample2x_bwd(untok(dup, N, 2 * H, 2 * W).double()))


def test_standalone_resampling_modules(ops):
    from neurosis_amd.modules.diffusion.openaimodel import Downsample, Upsample

    x = rnd(2, 16, 7, 10, seed=3)
    for mod, ref in ((Downsample(16, False), R.avgpool2x), (Upsample(16, False), R.upsample2x)):
        xg = x.cuda().requires_grad_(True)
        xr = x.double().requires_grad_(True)
        out, want = mod.cuda()(xg), ref(xr)
        dy = rnd(*want.shape, seed=4)
        out.backward(dy.cuda())
        want.backward(dy.double())
        assert out.shape == want.shape
        assert rel_err(out, want) <= 2.0 ** -8 and rel_err(xg.grad, xr.grad) <= 2.0 ** -8


# ------------------------------------------------------------------------------------------------
# 3. the ResBlock variants against the reference fixtures
# ------------------------------------------------------------------------------------------------
def _hip_resblock(name, fx, **override):
    from neurosis_amd.modules.diffusion.openaimodel import ResBlock

    kw, in_shapes = ADM_BLOCK_CASES[name]
    blk = ResBlock(**{**kw, **override})
    res = blk.load_state_dict(synth_state_dict(fx["shapes"]))
    assert not res.missing_keys and not res.unexpected_keys
    return blk.cuda(), block_inputs(name, in_shapes)


def _run_block(blk, ins, dy):
    dev = {k: v.cuda().requires_grad_(True) for k, v in ins.items()}
    for p in blk.parameters():
        p.grad = None
    out = blk(dev["x"], dev["emb"])
    out.backward(dy.cuda())
    from neurosis_amd import ops

    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    return out.detach(), dev["x"].grad, dev["emb"].grad, {k: p.grad.clone() for k, p in blk.named_parameters()}


@pytest.mark.parametrize("name", list(ADM_BLOCK_CASES))
def test_hip_resblocks_match_the_reference(blocks, name):
    fx = blocks[name]
    blk, ins = _hip_resblock(name, fx)
    dy = block_upstream(name, fx["out_shape"])
    out, dx, demb, grads = _run_block(blk, ins, dy)
    assert list(out.shape) == fx["out_shape"]
    worst = dict(rel=0.0, cos=1.0, norm=0.0, mat=1.0, vec=1.0)
    for label, got_full, entry in (("out", out, fx["out"]), ("d_x", dx, fx["d_x"])):
        got, want = R.stored_view(entry, got_full.float().cpu())
        e, c, dn = rel_err(got, want), cosine(got, want), abs(float(got_full.float().norm()) - entry["norm"]) / entry["norm"]
        worst.update(rel=max(worst["rel"], e), cos=min(worst["cos"], c), norm=max(worst["norm"], dn))
        assert e <= 3e-2 and c >= 0.999, (name, label, e, c)
        assert dn <= 5e-2, (name, label, dn)
    e, c = rel_err(demb, fx["d_emb"]), cosine(demb, fx["d_emb"])
    worst.update(rel=max(worst["rel"], e), cos=min(worst["cos"], c))
    assert e <= 3e-2 and c >= 0.999, (name, "d_emb", e, c)
    nmax = max(fx["grad_norms"].values())
    for k in fx["params"]:
        g, n = grads[k], fx["grad_norms"][k]
        if n <= 1e-5 * nmax:
            assert float(g.norm()) <= 2e-2 * nmax, (name, k, float(g.norm()))
            continue
        dn = abs(float(g.norm()) - n) / n
        worst["norm"] = max(worst["norm"], dn)
        assert dn <= 5e-2, (name, k, float(g.norm()), n)
        c = cosine(R.stored_rows(g, BLOCK_SAMPLE_ROWS, CONV_SAMPLE_CIN), fx["g"][k])
        worst["mat" if g.dim() >= 2 else "vec"] = min(worst["mat" if g.dim() >= 2 else "vec"], c)
        assert c >= (0.999 if g.dim() >= 2 else 0.998), (name, k, c)
    print(f"[adm block {name}] worst: rel {worst['rel']:.3e} cosine {worst['cos']:.6f} norm {worst['norm']:.3e}; sampled gradient cosines "
          f"matrices {worst['mat']:.5f} vectors {worst['vec']:.5f}")


# ------------------------------------------------------------------------------------------------
# 4. checkpointing and dropout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("name", ["ssn_320_640", "down_ssn_odd"])
def test_use_checkpoint_is_bit_identical(ops, blocks, name, dropout):
    fx = blocks[name]
    blk, ins = _hip_resblock(name, fx, dropout=dropout)
    blk.train()
    dy = block_upstream(name, fx["out_shape"])
    res = []
    for ck in (False, True):
        blk.use_checkpoint = ck
        ops.dropout_seed(11, 0)
        dev = {k: v.cuda().requires_grad_(True) for k, v in ins.items()}
        for p in blk.parameters():
            p.grad = None
        out = blk(dev["x"], dev["emb"])
        ops.dropout_draw()               # a later draw must not leak into the re-run
        out.backward(dy.cuda())
        ops.join_wgrad_stream()
        torch.cuda.synchronize()
        res.append((out.detach().clone(), dev["x"].grad.clone(), dev["emb"].grad.clone(), {k: p.grad.clone() for k, p in blk.named_parameters()}))
    (o0, dx0, de0, g0), (o1, dx1, de1, g1) = res
    assert torch.equal(bits(o0), bits(o1)) and torch.equal(bits(dx0), bits(dx1)) and torch.equal(bits(de0), bits(de1))
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    if dropout:
        blk.use_checkpoint = False
        ops.dropout_seed(12, 0)
        with torch.no_grad():
            other = blk(ins["x"].cuda(), ins["emb"].cuda())
        assert not torch.equal(bits(other), bits(o0))        # the mask is live


# ------------------------------------------------------------------------------------------------
# 5. the tiny UNet
# ------------------------------------------------------------------------------------------------
def _unet(fx, store=False):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.nn import FlatParamStore

    net = D.UNetModel(**fx["cfg"])
    res = net.load_state_dict(synth_state_dict(fx["shapes"]))
    assert not res.missing_keys and not res.unexpected_keys
    net = net.cuda()
    return net, (FlatParamStore(net.parameters()) if store else None)


def _unet_call(net, ins):
    return net(ins["x"].cuda(), ins["timesteps"].cuda(), ins["context"].cuda(), ins["y"].cuda())


def _check_unet_against_the_reference(label, fx, store):
    """Forward output and parameter gradients of a tiny UNet against the fixture, at the bounds tests/test_modules_gpu.py::
    test_unet_against_reference_golden uses: output rel <= 3e-2 and cosine >= 0.999, gradient cosines >= 0.9985 / 0.997, gradient norms
    within 5e-2 relative + 5e-4.

    The analytically-zero gradients are held apart.  A bias (without scale-shift: also the emb projection) in front of a
    one-channel-per-group GroupNorm has a zero gradient, 1e-5 in the fp32 reference; the bf16 path returns the sum of bf16-rounded
    gradients there, rounding noise in proportion to the gradient that arrives.  The fixture holds that noise for the reference's own fp32
    gradient rounded to bf16 (bf16_zero_grad_noise, 2.7e-2 .. 2.5e-1 with this fixture's unit-scale upstream; tests/golden/
    make_golden_adm.py::zero_gradient_noise).  The bound is twice that figure per parameter: it is one draw of a norm over >= 32 independent
    channel sums (relative spread about 1 / sqrt(2 * 32) = 12 %), on a gradient that the bf16 chain reproduces to a few percent."""
    net, st = _unet(fx, store)
    f = _unet_call(net, unet_inputs())
    assert f.shape == fx["F_out"].shape
    print(f"[{label}] output rel {rel_err(f, fx['F_out']):.3e} cosine {cosine(f, fx['F_out']):.6f}")
    assert rel_err(f, fx["F_out"]) <= 3e-2 and cosine(f, fx["F_out"]) >= 0.999
    f.backward(block_upstream("unet_adm_tiny", f.shape).cuda())
    torch.cuda.synchronize()
    grads = dict(net.named_parameters())
    zero = fx["bf16_zero_grad_noise"]
    check_grad_cosines(f"{label} golden", grads, fx["grads"], floor_matrix=0.9985, floor_vector=0.997, keep=lambda k, g: k not in zero)
    from tests.util import WORST_COSINES

    w = WORST_COSINES[f"{label} golden"]
    assert w[0] >= 0.9985 and w[2] >= 0.997, w
    assert zero and all(fx["grad_norms"][k] < 1e-4 for k in zero) and all(n > 1.0 for k, n in fx["grad_norms"].items() if k not in zero)
    bad, worst_rel, worst_zero = [], 0.0, 0.0
    for k, n in fx["grad_norms"].items():
        mine = float(grads[k].grad.float().norm())
        if k in zero:
            worst_zero = max(worst_zero, mine / zero[k])
            if mine > 2.0 * zero[k]:
                bad.append((k, mine, n, zero[k]))
            continue
        worst_rel = max(worst_rel, abs(mine - n) / n)
        if abs(mine - n) > 5e-2 * n + 5e-4:
            bad.append((k, mine, n))
    print(f"[{label}] gradient norms: worst relative deviation {worst_rel:.3e}; analytically-zero gradients: at most {worst_zero:.2f} x the "
          f"bf16 rounding noise of the reference's gradient")
    assert not bad, bad[:8]


@pytest.mark.parametrize("store", [True, False], ids=["flat_store", "free_params"])
def test_tiny_unet_against_the_reference(unets, store):
    _check_unet_against_the_reference("adm unet", unets["updown_ssn"], store)


def test_tiny_unet_with_parameter_free_resampling(unets):
    """conv_resample=False: Upsample / Downsample(use_conv=False) inside the chain, forward and backward"""
    _check_unet_against_the_reference("adm unet conv_resample=False", unets["plain_resample"], True)


def _graph_steps(fx, graph: bool, n=4):
    import neurosis_amd.modules.diffusion as D

    os.environ["NK_GRAPH"] = "1" if graph else "0"
    try:
        net, store = _unet(fx, store=True)
        store.state.wgrad_stream = torch.cuda.Stream()
        den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
        lossfn = D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())
        ins = unet_inputs()
        g = torch.Generator().manual_seed(7)
        losses, grads, replays = [], [], []
        for _ in range(n):
            x, noise = torch.randn(ins["x"].shape, generator=g).cuda(), torch.randn(ins["x"].shape, generator=g).cuda()
            loss = lossfn._forward(D.OpenAIWrapper(net), den, {"crossattn": ins["context"].cuda(), "vector": ins["y"].cuda()}, x, {},
                                   sigmas=torch.tensor([0.5, 3.0]).cuda(), noise=noise)
            loss.mean().backward()
            torch.cuda.synchronize()
            losses.append(loss.detach().clone())
            grads.append(store.grad.clone())
            replays.append(net._nk_graphs.replays if net._nk_graphs is not None else 0)
            store.adamw_step(1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0)
        return losses, grads, replays
    finally:
        os.environ.pop("NK_GRAPH", None)


def test_tiny_unet_graph_replay_equals_the_eager_chain(unets):
    fx = unets["updown_ssn"]
    loss_g, grad_g, replays = _graph_steps(fx, True)
    loss_e, grad_e, replays_e = _graph_steps(fx, False)
    assert replays_e == [0] * 4 and replays[0] == 0 and replays[2] > replays[1] > 0 and replays[3] > replays[2]
    for i in range(4):
        assert torch.equal(loss_g[i], loss_e[i]), (i, loss_g[i].tolist(), loss_e[i].tolist())
        # (as tests/test_graphs_gpu.py: equal up to the fp32 atomics of the few split-K weight gradients)
        d = float((grad_g[i] - grad_e[i]).norm() / grad_e[i].norm())
        print(f"[adm unet graphs] step {i + 1}: loss {loss_g[i].tolist()} flat gradient relative distance to the eager chain {d:.3e}")
        assert d <= 1e-5 and float(grad_e[i].norm()) > 0, (i, d)


def test_one_adafactor_step_through_the_engine(unets):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models import AutoencoderKL, DiffusionEngine

    fx = unets["updown_ssn"]
    keys = json.loads((G / "engine_tiny_keys.json").read_text())
    e = load_fixture("engine_tiny")
    net = D.UNetModel(**fx["cfg"])
    net.load_state_dict(synth_state_dict(fx["shapes"]))
    vae = AutoencoderKL(embed_dim=4, ddconfig={k: v for k, v in VAE_TINY.items() if k != "embed_dim"})
    vae.load_state_dict({k: v for k, v in synth_state_dict(keys["vae"]).items() if not k.startswith(("encoder.quant_conv", "decoder.post_quant_conv"))})
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=vae, scale_factor=0.13025, input_key="image", vae_batch_size=2,
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())).cuda()
    eng.setup_flat_params()
    eng.configure_adafactor(scale_parameter=True, relative_step=False, warmup_init=False, lr=1e-3)
    batch = lambda: {"image": e["image"].cuda(), "crossattn": e["crossattn"].cuda(), "vector": e["vector"].cuda()}
    before = eng.store.master.clone()
    losses = []
    for i in range(2):
        loss = eng.training_step(batch(), i, sigmas=e["sigma"].cuda(), noise=e["noise"].cuda())
        loss.backward()
        eng.optimizer_step()
        eng.join_optimizer()
        torch.cuda.synchronize()
        losses.append(float(loss.detach()))
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[0] != losses[1], losses
    assert bool(torch.isfinite(eng.store.master).all()) and bool(torch.isfinite(eng.store.grad).all())
    assert not torch.equal(before, eng.store.master)
    # the [2C, E] scale | shift projection got its update like every other matrix
    w = eng.model.diffusion_model.input_blocks[1][0].emb_layers[1].weight
    assert list(w.shape) == [64, 128] and not torch.equal(w.detach().cpu(), synth_state_dict({"input_blocks.1.0.emb_layers.1.weight": [64, 128]})["input_blocks.1.0.emb_layers.1.weight"])


# ------------------------------------------------------------------------------------------------
# 6. torch.ops.neurosis_hip.*
# ------------------------------------------------------------------------------------------------
def test_dispatcher_ops_through_autograd():
    import neurosis_amd.torch_ops  # noqa: F401  (registers the namespace)

    o = torch.ops.neurosis_hip
    shape = GN_SHAPES[0]
    N, C, H, W = shape
    c = _gn_case(shape, True)
    xt = tok(c["x"]).requires_grad_(True)
    gc, bc = c["gamma"].cuda().requires_grad_(True), c["beta"].cuda().requires_grad_(True)
    mc = c["mod"].to("cuda", BF).requires_grad_(True)
    y = o.groupnorm_mod(xt, gc, bc, mc, N, 32, 1e-5, True)
    y.backward(tok(c["dy"]))
    assert_close(untok(y.detach(), N, H, W), c["y"], TOL_BF16, "op groupnorm_mod")
    assert_close(untok(xt.grad, N, H, W), c["dx"], TOL_BF16, "op groupnorm_mod dx")
    assert_close(gc.grad, c["dgamma"], TOL_F32, "op dgamma")
    assert_close(bc.grad, c["dbeta"], TOL_F32, "op dbeta")
    assert_close(mc.grad, c["dmod"], TOL_F32, "op dmod")
    N, C, H, W = RS_SHAPES[0]
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-31, 32, (N, C, H, W), generator=g).float()
    for op, ref in ((o.avgpool2x, R.avgpool2x), (o.upsample2x_nearest, R.upsample2x)):
        xg, xr = tok(x).requires_grad_(True), x.double().requires_grad_(True)
        out, want = op(xg, N, H, W), ref(xr)
        dy = torch.randint(-7, 8, want.shape, generator=g).float()
        out.backward(tok(dy))
        want.backward(dy.double())
        assert torch.equal(untok(out.detach(), N, want.shape[2], want.shape[3]).double(), want.detach())
        assert torch.equal(untok(xg.grad, N, H, W).double(), xr.grad)
    # shapes without a GPU kernel: the fake (meta) kernels
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        t = torch.empty(N * H * W, C, dtype=BF, device="cuda")
        assert o.avgpool2x(t, N, H, W).shape == (N * (H // 2) * (W // 2), C) and o.upsample2x_nearest(t, N, H, W).shape == (N * 4 * H * W, C)
        assert o.groupnorm_mod(t, torch.empty(C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(N, 2 * C, dtype=BF, device="cuda"), N, 4, 1e-5, True).shape == t.shape
