"""Concat-conditioned UNets (inpainting / edit / upscale models) on the fused training and sampling paths: the two prepare kernels bit for
bit against the kernels they extend, the fused route taken, loss / gradients / guided denoiser output against tests/golden/concat_tiny
(make_golden_concat.py: the reference's own UNetModel(in_channels=9) behind its OpenAIWrapper), hipGraph replay with a new concat tensor
every step, and the engine end to end.

Tolerances: the kernels are bit-exact (the latent channels share their arithmetic with nk_edm_prepare / nk_sample_prepare, the concat
channels are one RNE rounding of an fp32 value); loss, gradients and the denoiser output as test_loss_class_gpu.py / test_sampler_gpu.py
hold the same objectives without a concat entry."""
import json
from pathlib import Path

import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.golden.make_golden import VAE_TINY, synth_state_dict
from tests.golden.make_golden_concat import CONCAT_CASES, grad_rows
from tests.util import check_grad_cosines, cosine, rel_err

pytestmark = pytest.mark.gpu
G = Path(__file__).resolve().parent / "golden"
C = 4
NAN16, NAN32 = 0x7FC1, 0x7FC00123          # quiet-NaN bit patterns the output buffers are pre-filled with
TAIL = 64                                   # sentinel elements behind zt, sentinel rows behind net_in
# cosine floors of the concat columns of d input_blocks.0.0.weight: the generic route's own value less 0.001 (see the test that uses them)
CONCAT_COLUMN_FLOOR = {"edm_l2": 0.998543, "rf_l2": 0.998245}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _nan_tokens(rows: int, cpad: int) -> torch.Tensor:
    return torch.full((rows + TAIL, cpad), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _assert_tail_untouched(buf: torch.Tensor, used: int, pattern: int):
    tail = _bits(buf).reshape(-1)[used:]
    assert tail.numel() > 0 and bool((tail == pattern).all()), "wrote behind the end of the buffer"


def _extra_tokens(extra: torch.Tensor) -> torch.Tensor:
    return extra.permute(0, 2, 3, 1).reshape(-1, extra.shape[1]).to(torch.bfloat16)


# C + Ce = 5 (pad ends inside the first vector), 8 (exactly one vector), 9 (a second vector with 7 pad channels), 16 (two full vectors);
# HW = 35 (less than a wave, odd) and 384 (more than one workgroup, with a tail)
KERNEL_SHAPES = [(2, 5, 7), (3, 16, 24)]


def _kernel_inputs(B, H, W, Ce, seed):
    g = torch.Generator().manual_seed(seed)
    x, eps = torch.randn(B, C, H, W, generator=g).cuda(), torch.randn(B, C, H, W, generator=g).cuda()
    sigma, c_in = (torch.rand(B, generator=g) * 5 + 0.1).cuda(), (torch.rand(B, generator=g) + 0.1).cuda()
    extra_c, extra_u = torch.randn(B, Ce, H, W, generator=g).cuda(), torch.randn(B, Ce, H, W, generator=g).cuda()
    return x, eps, sigma, c_in, extra_c, extra_u


@pytest.mark.parametrize("shape", KERNEL_SHAPES)
@pytest.mark.parametrize("Ce", [1, 4, 5, 12])
def test_training_kernel_bit_for_bit(Ce, shape):
    from neurosis_amd.lib import call

    B, H, W = shape
    HW, cpad = H * W, (C + Ce + 7) // 8 * 8
    x, eps, sigma, c_in, extra, _ = _kernel_inputs(B, H, W, Ce, 21)
    zt_old, net_old = torch.empty_like(x), torch.empty(B * HW, 8, dtype=torch.bfloat16, device="cuda")
    call("nk_edm_prepare", x.data_ptr(), eps.data_ptr(), sigma.data_ptr(), c_in.data_ptr(), zt_old.data_ptr(), net_old.data_ptr(), B, C, HW, 8, _stream())
    zt = torch.full((x.numel() + TAIL,), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
    net_in = _nan_tokens(B * HW, cpad)
    call("nk_edm_prepare_cat", x.data_ptr(), eps.data_ptr(), sigma.data_ptr(), c_in.data_ptr(), extra.data_ptr(), zt.data_ptr(), net_in.data_ptr(),
         B, C, Ce, HW, cpad, _stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(zt[:x.numel()]), _bits(zt_old).reshape(-1))
    got = net_in[:B * HW]
    assert torch.equal(_bits(got[:, :C]), _bits(net_old[:, :C]))
    assert torch.equal(_bits(got[:, C:C + Ce]), _bits(_extra_tokens(extra)))
    assert cpad == C + Ce or bool((_bits(got[:, C + Ce:]) == 0).all())
    _assert_tail_untouched(zt, x.numel(), NAN32)
    _assert_tail_untouched(net_in, B * HW * cpad, NAN16)


@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("shape", KERNEL_SHAPES)
@pytest.mark.parametrize("Ce", [1, 4, 5, 12])
def test_sampling_kernel_bit_for_bit(Ce, shape, rep):
    from neurosis_amd.lib import call

    B, H, W = shape
    HW, cpad = H * W, (C + Ce + 7) // 8 * 8
    x, _, _, c_in, extra_c, extra_u = _kernel_inputs(B, H, W, Ce, 22)
    assert not torch.equal(extra_c, extra_u)
    net_old = torch.empty(rep * B * HW, 8, dtype=torch.bfloat16, device="cuda")
    call("nk_sample_prepare", x.data_ptr(), c_in.data_ptr(), net_old.data_ptr(), B, C, HW, 8, rep, _stream())
    net_in = _nan_tokens(rep * B * HW, cpad)
    # rep == 1 reads extra_c alone: it gets no unconditional tensor at all
    call("nk_sample_prepare_cat", x.data_ptr(), c_in.data_ptr(), extra_u.data_ptr() if rep == 2 else None, extra_c.data_ptr(), net_in.data_ptr(),
         B, C, Ce, HW, cpad, rep, _stream())
    torch.cuda.synchronize()
    got, old = net_in[:rep * B * HW].reshape(rep, B * HW, cpad), net_old.reshape(rep, B * HW, 8)
    for r in range(rep):
        assert torch.equal(_bits(got[r, :, :C]), _bits(old[r, :, :C]))
        want = extra_u if (rep == 2 and r == 0) else extra_c
        assert torch.equal(_bits(got[r, :, C:C + Ce]), _bits(_extra_tokens(want))), f"replica {r} carries the wrong concat tensor"
        assert cpad == C + Ce or bool((_bits(got[r, :, C + Ce:]) == 0).all())
    _assert_tail_untouched(net_in, rep * B * HW * cpad, NAN16)


def test_kernels_refuse_bad_shapes_and_launch_nothing():
    from neurosis_amd import lib
    from neurosis_amd.lib import NkError, call

    x = torch.zeros(1, 4, 2, 2, device="cuda")
    e = torch.zeros(1, 12, 2, 2, device="cuda")
    v = torch.ones(1, device="cuda")
    zt = torch.zeros_like(x)
    buf = torch.zeros(4 * 32, dtype=torch.bfloat16, device="cuda")
    X, E, V, Z, N = x.data_ptr(), e.data_ptr(), v.data_ptr(), zt.data_ptr(), buf.data_ptr()
    # (B, C, Ce, HW, Cpad): Cpad < C+Ce; Cpad % 8 != 0; Cpad - (C+Ce) >= 8; Ce < 0
    bad = [(1, 4, 5, 4, 8), (1, 4, 5, 4, 12), (1, 4, 1, 4, 16), (1, 4, -1, 4, 8)]
    lib.launch_log(1)
    try:
        for B, Cc, Ce, HW, cpad in bad:
            with pytest.raises(NkError):
                call("nk_edm_prepare_cat", X, X, V, V, E, Z, N, B, Cc, Ce, HW, cpad, _stream())
            with pytest.raises(NkError):
                call("nk_sample_prepare_cat", X, V, E, E, N, B, Cc, Ce, HW, cpad, 1, _stream())
        with pytest.raises(NkError):
            call("nk_sample_prepare_cat", X, V, E, E, N, 1, 4, 4, 4, 8, 3, _stream())        # rep must be 1 or 2
        with pytest.raises(NkError):
            call("nk_edm_prepare_cat", X, X, V, V, None, Z, N, 1, 4, 4, 4, 8, _stream())      # no concat tensor, Ce > 0
        with pytest.raises(NkError):
            call("nk_sample_prepare_cat", X, V, E, None, N, 1, 4, 4, 4, 8, 1, _stream())
        with pytest.raises(NkError):
            call("nk_sample_prepare_cat", X, V, None, E, N, 1, 4, 4, 4, 8, 2, _stream())      # rep 2 needs the unconditional one too
        assert lib.launched() == []
        # Ce = 0 with no concat tensor is the old kernel's job done by the new one: accepted
        call("nk_edm_prepare_cat", X, X, V, V, None, Z, N, 1, 4, 0, 4, 8, _stream())
        call("nk_sample_prepare_cat", X, V, None, None, N, 1, 4, 0, 4, 8, 2, _stream())
        assert lib.launched() == ["edm_prepare_cat", "sample_prepare_cat"]
    finally:
        lib.launch_log(0)
    torch.cuda.synchronize()


# ---- the tiny concat UNet of the fixture -------------------------------------------------------------------------------------------------
def _unet(fx, store=True):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.nn import FlatParamStore

    net = D.UNetModel(**fx["cfg"])
    net.load_state_dict(synth_state_dict(fx["shapes"]))
    net = net.cuda()
    return net, (FlatParamStore(net.parameters()) if store else None)


def _loss_setup(kw):
    import neurosis_amd.modules.diffusion as D

    if kw["objective_type"] == "rf":
        den, weighting = D.Denoiser(preconditioning=D.RectifiedFlowXLPreconditioning()), D.RectifiedFlowWeighting()
    else:
        den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
        weighting = D.EpsWeighting()
    return den, weighting, D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=weighting, **kw)


def test_the_fused_route_is_taken():
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd import lib

    fx = load_fixture("concat_tiny")
    case = fx["cases"]["edm_l2"]
    net, st = _unet(fx)
    wrapped = D.OpenAIWrapper(net)
    cond = {"crossattn": fx["context"].cuda(), "vector": fx["y"].cuda(), "concat": fx["concat"].cuda()}
    assert wrapped.fused_unet(fx["x"].cuda(), {"concat": cond["concat"]}, {}) is net
    den, _, lossfn = _loss_setup(case["kwargs"])
    lib.launch_log(1)
    try:
        loss = lossfn._forward(wrapped, den, cond, fx["x"].cuda(), {}, sigmas=case["sigma"].cuda(), noise=case["noise"].cuda())
        names = lib.launched()        # (the log keeps the first 64 launches: the head of the chain, where the network input is built)
    finally:
        lib.launch_log(0)
    torch.cuda.synchronize()
    assert "edm_prepare_cat" in names[:4] and len(names) >= 32
    assert "nchw_to_nhwc" not in names and "edm_prepare" not in names
    assert torch.isfinite(loss).all()


@pytest.mark.parametrize("tag", [t for t, _ in CONCAT_CASES])
def test_loss_and_gradients_match_the_reference(tag):
    import neurosis_amd.modules.diffusion as D

    fx = load_fixture("concat_tiny")
    case = fx["cases"][tag]
    net, st = _unet(fx)
    den, weighting, lossfn = _loss_setup(case["kwargs"])
    assert type(weighting).__name__ == case["weighting"]
    cond = {"crossattn": fx["context"].cuda(), "vector": fx["y"].cuda(), "concat": fx["concat"].cuda()}
    loss = lossfn._forward(D.OpenAIWrapper(net), den, cond, fx["x"].cuda(), {}, sigmas=case["sigma"].cuda(), noise=case["noise"].cuda())
    assert loss.shape == case["loss"].shape and loss.dtype == torch.float32
    print(f"[concat {tag}] loss {loss.tolist()} reference {case['loss'].tolist()} rel {rel_err(loss.detach(), case['loss']):.3e}")
    assert rel_err(loss.detach(), case["loss"]) <= 1e-2, (loss.tolist(), case["loss"].tolist())
    loss.mean().backward()
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    gmax = max(case["grad_norms"].values())
    # measured worst >= 2-D / 1-D on the fused route: edm_l2 0.99868 (time_embed.0.weight) / 0.99908, rf_l2 0.99913 / 0.99903; loss within 2.5e-4 / 7.7e-4,
    # gradient norms within 1.5e-2 / 2.1e-2 (floors and bounds: test_loss_class_gpu.py's for the same objectives)
    fm, fv = {"rf_l2": (0.998, 0.998)}.get(tag, (0.9985, 0.998))
    got = {k: grad_rows(named[k].grad) for k in case["grads"]}
    check_grad_cosines(f"concat {tag}", got, case["grads"], floor_matrix=fm, floor_vector=fv, keep=lambda k, g: float(g.norm()) > 1e-2 * gmax)
    worst_norm = max(abs(float(named[k].grad.norm()) - n) / n for k, n in case["grad_norms"].items() if n > 1e-2 * gmax)
    print(f"[concat {tag}] worst gradient-norm deviation {worst_norm:.4f}")
    for k, n in case["grad_norms"].items():
        if n > 1e-2 * gmax:
            assert abs(float(named[k].grad.norm()) - n) <= 6e-2 * n, (tag, k)
    # the concat columns of the first convolution's weight gradient alone.  The generic route (Denoiser.forward -> torch.cat -> UNetModel.forward)
    # of the commit before the fused one existed measured 0.999543 (edm_l2) / 0.999245 (rf_l2) against this fixture on an MI355X; the floor is
    # 0.001 below that, the distance test_loss_class_gpu.py keeps between its measured worst and its floor.  The fused route measures the same
    # 0.999543 / 0.999245: it feeds the same network the same bf16 input (the latent columns: 0.999752 / 0.999412 on both routes).
    floor = CONCAT_COLUMN_FLOOR[tag]
    c = cosine(named["input_blocks.0.0.weight"].grad[:, C:], case["grads"]["input_blocks.0.0.weight"][:, C:])
    print(f"[concat {tag}] cosine of the concat columns of d input_blocks.0.0.weight: {c:.6f} (floor {floor})")
    assert c >= floor, (tag, c)


# ---- the engine: hipGraph replay with a new concat tensor every step, and the sampling entry points ---------------------------------------
def _engine(**kw):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models import AutoencoderKL, DiffusionEngine
    from neurosis_amd.modules.encoders import GeneralConditioner, IdentityEncoder, PrecomputedEmbedder

    fx = load_fixture("concat_tiny")
    keys = json.loads((G / "engine_tiny_keys.json").read_text())
    net = D.UNetModel(**fx["cfg"])
    net.load_state_dict(synth_state_dict(fx["shapes"]))
    vae = AutoencoderKL(embed_dim=4, ddconfig={k: v for k, v in VAE_TINY.items() if k != "embed_dim"})
    vae.load_state_dict({k: v for k, v in synth_state_dict(keys["vae"]).items() if not k.startswith(("encoder.quant_conv", "decoder.post_quant_conv"))})
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    conditioner = GeneralConditioner([IdentityEncoder(input_key="inpaint"), PrecomputedEmbedder(input_key="crossattn"), PrecomputedEmbedder(input_key="vector")])
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=vae, conditioner=conditioner, scale_factor=0.13025, input_key="image", vae_batch_size=2,
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting()), **kw).cuda()
    eng.setup_flat_params()
    return eng


def _engine_batches(n):
    e = load_fixture("engine_tiny")
    g = torch.Generator().manual_seed(31)
    B, _, H, W = e["latents"].shape
    out = []
    for _ in range(n):
        inpaint = torch.cat(((torch.rand(B, 1, H, W, generator=g) > 0.5).float(), torch.randn(B, 4, H, W, generator=g)), 1)
        out.append(({"image": e["image"].cuda(), "crossattn": e["crossattn"].cuda(), "vector": e["vector"].cuda(), "inpaint": inpaint.cuda()},
                    dict(sigmas=e["sigma"].cuda(), noise=e["noise"].cuda())))
    return out


def test_graph_replay_sees_each_steps_concat_tensor(monkeypatch):
    """Three training steps of the engine (eager warm-up, capture, replay), a different concat tensor in each: the replayed chain must
    give the eager chain's loss bit for bit -- a concat tensor baked into the graph would show in the third step -- and its gradients up
    to the fp32 atomics of the few split-K weight gradients (the bound of tests/test_graphs_gpu.py)."""
    res = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("NK_GRAPH", raising=False)
        else:
            monkeypatch.setenv("NK_GRAPH", mode)
        eng = _engine()
        losses, grads = [], []
        for batch, inject in _engine_batches(3):
            loss = eng.training_step(batch, 0, **inject)
            loss.backward()
            torch.cuda.synchronize()
            losses.append(loss.detach().clone())
            grads.append(eng.store.grad.clone())
            eng.optimizer_step(lr=1e-3)
        eng.join_optimizer()
        torch.cuda.synchronize()
        cg = eng.model.diffusion_model._nk_graphs
        res[mode] = (losses, grads, None if cg is None else cg.replays)
    assert res["0"][2] is None and res[None][2] > 0, "the default run must have replayed the chain"
    assert not torch.equal(res["0"][0][1], res["0"][0][2])
    for i, (a, b) in enumerate(zip(res["0"][0], res[None][0])):
        assert torch.equal(a, b), (i, a.tolist(), b.tolist())
    for i, (a, b) in enumerate(zip(res["0"][1], res[None][1])):
        assert float(a.norm()) > 0 and float((a - b).norm() / a.norm()) <= 1e-5, i


def test_engine_samples_and_logs_images_of_a_concat_model():
    import neurosis_amd.modules.diffusion as D
    import neurosis_amd.modules.diffusion.sampling as S
    from neurosis_amd.modules.guidance import VanillaCFG

    sampler = S.EulerEDMSampler(discretization=D.LegacyDDPMDiscretization(), guider=VanillaCFG(3.0), num_steps=2)
    eng = _engine(sampler=sampler).eval()
    batch, _ = _engine_batches(1)[0]
    calls = []
    original = S.FusedDenoiser.euler
    S.FusedDenoiser.euler = lambda self, *a, **k: calls.append("euler") or original(self, *a, **k)
    try:
        out = eng.log_images(batch, num_img=2)
    finally:
        S.FusedDenoiser.euler = original
    assert calls == ["euler"] * 2, "the sampler must have taken the fused Euler step"
    assert out["samples"].shape == (2, 3, 64, 64) and torch.isfinite(out["samples"]).all()


def _sampling_setup():
    import neurosis_amd.modules.diffusion as D

    fx = load_fixture("concat_tiny")
    net, _ = _unet(fx, store=False)
    net = net.eval()
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
    s = fx["sample"]
    cond, uc = ({k: v.cuda() for k, v in d.items()} for d in (s["cond"], s["uc"]))
    return fx, D.OpenAIWrapper(net), den, s, cond, uc


def test_guided_denoiser_matches_the_reference_with_two_concat_tensors():
    import neurosis_amd.modules.diffusion.sampling as S
    from neurosis_amd.modules.guidance import VanillaCFG

    fx, wrapped, den, s, cond, uc = _sampling_setup()
    guider = VanillaCFG(s["scale"])
    fused = S.FusedDenoiser(wrapped, den, use_graph=False)
    x = s["x"].cuda()
    assert fused.supports(x, guider, cond)
    with torch.no_grad():
        got = fused.guided(x, s["sigma"].cuda(), cond, uc, guider)
    torch.cuda.synchronize()
    # (the tolerance of test_sampler_gpu.py for the fused route against the reference; the two concat tensors swapped are s["swap_distance"] away)
    print(f"[concat guided] rel {rel_err(got, s['denoised']):.4e} cosine {cosine(got, s['denoised']):.6f} swapped assignment {s['swap_distance']:.3f}")
    assert s["swap_distance"] > 10 * 4e-2
    assert rel_err(got, s["denoised"]) <= 4e-2 and cosine(got, s["denoised"]) >= 0.999


def test_captured_euler_step_equals_the_eager_step_and_reloads_the_concat_tensor():
    import neurosis_amd.modules.diffusion.sampling as S
    from neurosis_amd.modules.guidance import VanillaCFG

    fx, wrapped, den, s, cond, uc = _sampling_setup()
    guider = VanillaCFG(s["scale"])
    # the second step's conditioning: another (cond, uc) pair, the concat tensors among what changes
    cond2 = dict(cond, concat=uc["concat"].flip(0).contiguous(), crossattn=cond["crossattn"].flip(0).contiguous())
    uc2 = dict(uc, concat=cond["concat"].flip(0).contiguous())
    sig = [torch.full((2,), v, device="cuda") for v in (2.5, 1.4, 0.7)]
    res = {}
    with torch.no_grad():
        for use_graph in (False, True):
            fused = S.FusedDenoiser(wrapped, den, use_graph=use_graph)
            x1 = fused.euler(s["x"].cuda(), sig[0], sig[1], cond, uc, guider).clone()
            x2 = fused.euler(x1.clone(), sig[1], sig[2], cond2, uc2, guider).clone()
            stale = fused.euler(x1.clone(), sig[1], sig[2], cond, uc, guider).clone()
            res[use_graph] = (x1, x2, stale)
            assert len(fused._captured) == (1 if use_graph else 0)
    torch.cuda.synchronize()
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])
    assert rel_err(res[True][1], res[True][2]) > 1e-2, "the second pair's conditioning must matter"
