"""The bounds of tests/glue_bounds.py, tested without a GPU.

  fp32 restatement  each kernel's formula in torch fp32 on the CPU, in the kernel's order of operations and with its chunked sums (the
                    per-thread serial chain, the xor butterfly over 64 lanes, the serial sum of the per-wave partials), must lie within
                    the bound against float64 on the inputs the GPU test uses: a bound is not too tight for honest fp32.  The stated
                    error term of the fast exponential is checked against torch's fp32 exp.  Prints "[glue ratio] ..." per entry point.
  planted errors    planted into a restatement's output, each of these must be rejected by the same check: one element moved by two
                    output ulps (bf16 ulps; 8 U relative for fp32), a padding channel made non-zero, two neighbouring pixels swapped,
                    bc2 replaced by bc1, beta1 applied to the gradient instead of the old moment, a softmax row normalised by a sum
                    that misses its last 16-byte piece.  The loss VALUE is a reduction whose chain alone allows ~30 U, so the two-ulp
                    plant goes to the per-element outputs (dnet, z_t, net_in, ...); a sample with the wrong loss weight is planted there."""
import math

import pytest
import torch

from tests import attention_bounds as ab
from tests import glue_bounds as gb
from tests.test_text_encoder_train_gpu import _check

U, F64, F32, BF16 = gb.U, gb.F64, gb.F32, gb.BF16
_LANES = torch.arange(64)


def _butterfly(v):
    """wave_sum of csrc/nk_common.h over the last axis (64 lanes): every lane ends with the total; lane 0's is returned"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ o]
    return v[..., 0]


def _serial(t):
    """left-to-right fp32 sum over the last axis"""
    acc = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for k in range(t.shape[-1]):
        acc = acc + t[..., k]
    return acc


def _block_sum(per_thread, waves):
    """per_thread [..., 64 * waves, chain]: the kernels' fixed-order block reduction"""
    acc = _serial(per_thread)
    return _serial(_butterfly(acc.view(*acc.shape[:-1], waves, 64)))


def _t(v):
    return torch.tensor(v, dtype=F32)


# ================================================================================================================================
# restatements
# ================================================================================================================================
def restate_softmax(x, short_sum_row=None):
    M, L = x.shape
    chain = gb.softmax_chain(L)[1]
    width = chain * 256
    xp = torch.cat([x.float(), torch.full((M, width - L), -math.inf)], 1)
    mx = xp.amax(1, keepdim=True)
    e = torch.exp(xp - mx)
    summed = e.clone()
    if short_sum_row is not None:
        summed[short_sum_row, L - 8:L] = 0.0
    per = summed.view(M, chain // 8, 256, 8).permute(0, 2, 1, 3).reshape(M, 256, chain)
    inv = 1.0 / _block_sum(per, 4)
    return {"p": (e[:, :L] * inv[:, None]).to(BF16)}


def restate_softmax_bwd(p, dp, scale):
    M, L = p.shape
    chain = 8 * math.ceil(L / 2048)
    a, b = p.float(), dp.float()
    prod = torch.cat([a * b, torch.zeros(M, chain * 256 - L)], 1)
    dot = _block_sum(prod.view(M, chain // 8, 256, 8).permute(0, 2, 1, 3).reshape(M, 256, chain), 4)
    return {"ds": (a * (b - dot[:, None]) * _t(scale)).to(BF16)}


def restate_edm_prepare(x, eps, sigma, c_in, Cpad):
    z = x + sigma[:, None, None] * eps
    return {"zt": z, "net_in": gb._tokens((z * c_in[:, None, None]).to(BF16), Cpad)}


def restate_edm_loss(net_out, zt, target, c_out, c_skip, w, C, upstream, w_used=None):
    B, HW, Cpad = net_out.shape
    co, cs = c_out[:, None, None], c_skip[:, None, None]
    wb = w if w_used is None else w_used
    inv_cnt = _t(1.0) / (_t(float(C)) * _t(float(HW)))
    gscale = _t(upstream) * wb * 2.0 * inv_cnt * c_out
    D = net_out[:, :, :C].float().permute(0, 2, 1) * co + zt * cs
    diff = D - target                                                   # [B, C, HW]
    sq = diff * diff
    nP = math.ceil(HW / 1024)
    sq = torch.cat([sq, torch.zeros(B, C, nP * 1024 - HW)], 2).view(B, C, nP, 1024).permute(0, 3, 2, 1).reshape(B, 1024, nP * C)
    loss = _block_sum(sq, 16) * inv_cnt * wb
    return {"loss": loss, "dnet": gb._tokens((diff * gscale[:, None, None]).to(BF16), Cpad)}


def restate_sample(x, net_out, c_skip, c_out, sigma_hat, sigma_next, scale, rep):
    B, C, HW = x.shape
    cs, co, sh = c_skip[:, None, None], c_out[:, None, None], sigma_hat[:, None, None]
    F = net_out[:B, :, :C].float().permute(0, 2, 1)
    if rep == 2:
        fc = net_out[B:, :, :C].float().permute(0, 2, 1)
        F = F + _t(scale) * (fc - F)
    D = cs * x + co * F
    dt = (sigma_next - sigma_hat)[:, None, None]
    return {"denoised": D, "x_next": x + dt * ((x - D) / sh)}


def restate_adamw(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, grad_scale, bc2_is_bc1=False, beta1_on_grad=False):
    lr, b1, b2, eps, wd, gs = (_t(h) for h in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    bc1, bc2 = 1.0 - torch.pow(b1, _t(float(step))), 1.0 - torch.pow(b2, _t(float(step)))
    if bc2_is_bc1:
        bc2 = bc1
    gr = g * gs
    m1 = ((1.0 - b1) * m + b1 * gr) if beta1_on_grad else (b1 * m + (1.0 - b1) * gr)
    v1 = b2 * v + (1.0 - b2) * gr * gr
    upd = (m1 / bc1) / (torch.sqrt(v1 / bc2) + eps)
    return {"p": p * (1.0 - lr * wd) - lr * upd, "m": m1, "v": v1}


def restate_ema(ema, p, omd):
    return {"ema": ema - _t(omd) * (ema - p)}


def restate_timestep(t, dim, max_period):
    half = dim // 2
    k = torch.arange(half, dtype=F32)
    freq = torch.exp(-torch.log(_t(max_period)) * k / _t(float(half)))
    arg = t[:, None] * freq[None, :]
    out = torch.zeros(t.shape[0], dim)
    out[:, :half], out[:, half:2 * half] = torch.cos(arg), torch.sin(arg)
    return {"emb": out.to(BF16)}


# ================================================================================================================================
# planted errors
# ================================================================================================================================
def _moved(t, ref, bound):
    """one element (where the bound is tightest against the value) moved by two output ulps, away from the reference"""
    out = t.clone()
    i = int((ref.abs() / bound.clamp_min(1e-300)).masked_fill(bound <= 0, 0).argmax())
    v = out.view(-1)[i].to(F64)
    away = 1.0 if float(v) >= float(ref.reshape(-1)[i]) else -1.0
    out.view(-1)[i] = (v + away * 2 * ab.ulp_bf16(v)) if t.dtype == BF16 else v + away * 8 * U * v.abs()
    return out


def _rejected(entry, label, got, expected):
    with pytest.raises(AssertionError):
        gb.verify(entry, label, got, expected, _check, record=False)


def _plant_all(entry, label, got, expected, pixel_axis=None, padded=None, ulps=True):
    """every output: two ulps; the outputs with a pixel axis: neighbours swapped; the padded outputs: a non-zero padding channel"""
    for name, (ref, bound) in expected.items():
        if ulps:
            _rejected(entry, f"{label} two ulps", {**got, name: _moved(got[name], ref, bound)}, expected)
        ax = (pixel_axis or {}).get(name)
        if ax is not None and ref.shape[ax] >= 2:
            idx = torch.arange(ref.shape[ax])
            idx[0], idx[1] = 1, 0
            _rejected(entry, f"{label} pixels swapped", {**got, name: got[name].index_select(ax, idx)}, expected)
        if name in (padded or ()) and bool((bound == 0).any()):
            bad = got[name].clone()
            bad.view(-1)[int((bound.view(-1) == 0).nonzero()[0])] = 2.0 ** -100
            _rejected(entry, f"{label} padding", {**got, name: bad}, expected)


# ================================================================================================================================
# tests
# ================================================================================================================================
def test_fast_exponential_term_covers_fp32_exp():
    """the stated per-term error of the exponential, (3 |d| + 2) U relative (+ TINY), against torch's fp32 exp of the fp32 difference"""
    x = torch.cat([gb.softmax_inputs(3, 2056, v).view(-1) for v in range(4)])
    d = (x.float() - x.float().max())
    ref = torch.exp(d.to(F64))
    _check("fp32 exp", torch.exp(d), ref, ref * gb.exp_term(d.to(F64)) + gb.TINY)


@pytest.mark.parametrize("L", gb.SOFTMAX_L)
def test_softmax_restatement_and_planted_errors(L):
    for M in gb.SOFTMAX_M:
        for variant in range(4):
            x = gb.softmax_inputs(M, L, variant)
            exp = gb.softmax_expected(x)
            got = restate_softmax(x)
            gb.verify("nk_softmax_rows", f"softmax {M}x{L} v{variant}", got, exp, _check)
            row = [r for r in range(M) if gb.SOFTMAX_KINDS[(variant + r) % 4] == "normal"]
            if row:
                _plant_all("nk_softmax_rows", f"softmax {M}x{L}", got, exp, pixel_axis={"p": 1})
                _rejected("nk_softmax_rows", f"softmax {M}x{L} short sum", restate_softmax(x, short_sum_row=row[0]), exp)
    gb.report("nk_softmax_rows")


@pytest.mark.parametrize("M, L", gb.SOFTMAX_BWD_SHAPES)
def test_softmax_bwd_restatement_and_planted_errors(M, L):
    for scale in gb.SOFTMAX_BWD_SCALES:
        for kind in ("random", "const"):
            p, dp = gb.softmax_bwd_inputs(M, L, kind)
            exp = gb.softmax_bwd_expected(p, dp, scale)
            got = restate_softmax_bwd(p, dp, scale)
            gb.verify("nk_softmax_rows_bwd", f"softmax bwd {M}x{L} {kind} scale {scale}", got, exp, _check)
            if kind == "random":
                _plant_all("nk_softmax_rows_bwd", f"softmax bwd {M}x{L}", got, exp, pixel_axis={"ds": 1})
    gb.report("nk_softmax_rows_bwd")


@pytest.mark.parametrize("shape", gb.EDM_PREPARE_SHAPES)
def test_edm_prepare_restatement_and_planted_errors(shape):
    B, C, HW, Cpad = shape
    inp = gb.edm_prepare_inputs(*shape)
    exp = gb.edm_prepare_expected(**inp, Cpad=Cpad)
    got = restate_edm_prepare(**inp, Cpad=Cpad)
    gb.verify("nk_edm_prepare", f"edm_prepare {shape}", got, exp, _check)
    _plant_all("nk_edm_prepare", f"edm_prepare {shape}", got, exp, pixel_axis={"zt": 2, "net_in": 1}, padded=("net_in",))
    gb.report("nk_edm_prepare")


@pytest.mark.parametrize("shape", gb.EDM_LOSS_SHAPES)
def test_edm_loss_restatement_and_planted_errors(shape):
    B, C, HW, Cpad = shape
    for kind in ("plain", "cancel"):
        inp = gb.edm_loss_inputs(*shape, kind)
        for upstream in gb.EDM_UPSTREAMS:
            exp = gb.edm_loss_expected(**inp, C=C, upstream=upstream)
            got = restate_edm_loss(**inp, C=C, upstream=upstream)
            gb.verify("nk_edm_loss", f"edm_loss {shape} {kind} upstream {upstream}", got, exp, _check)
            if B > 1:
                assert float(got["loss"][B - 1]) == 0.0 and float(exp["loss"][0][B - 1]) == 0.0
            if kind == "plain":
                dn = {"dnet": exp["dnet"]}
                _plant_all("nk_edm_loss", f"edm_loss {shape}", {"dnet": got["dnet"]}, dn, pixel_axis={"dnet": 1}, padded=("dnet",))
                wrong = restate_edm_loss(**inp, C=C, upstream=upstream, w_used=inp["w"].roll(1) + 1.0)
                _rejected("nk_edm_loss", f"edm_loss {shape} wrong weight", wrong, exp)
    gb.report("nk_edm_loss")


@pytest.mark.parametrize("shape", gb.SAMPLE_SHAPES)
def test_sampler_restatement_and_planted_errors(shape):
    B, C, HW, Cpad = shape
    for rep in gb.SAMPLE_REPS:
        for kind in gb.SAMPLE_KINDS:
            inp = gb.sample_inputs(*shape, rep, kind)
            prep = gb.sample_prepare_expected(inp["x"], inp["c_in"], Cpad, rep)
            got_prep = {"net_in": gb._tokens((inp["x"] * inp["c_in"][:, None, None]).to(BF16), Cpad).repeat(rep, 1, 1)}
            gb.verify("nk_sample_prepare", f"sample_prepare {shape} rep {rep}", got_prep, prep, _check)
            args = {k: inp[k] for k in ("x", "net_out", "c_skip", "c_out", "sigma_hat", "sigma_next")}
            for scale in gb.SAMPLE_SCALES:
                exp = gb.sample_expected(**args, scale=scale, rep=rep)
                got = restate_sample(**args, scale=scale, rep=rep)
                label = f"sample {shape} rep {rep} {kind} scale {scale}"
                gb.verify("nk_sample_denoise", label, {"denoised": got["denoised"]}, {"denoised": exp["denoised"]}, _check)
                gb.verify("nk_sample_euler_step", label, got, exp, _check)
                if kind == "random":
                    # under guidance the honest error of F exceeds two fp32 ulps (glue_bounds: dF): the two-ulp plant is for s <= 1
                    _plant_all("nk_sample_euler_step", label, got, exp, pixel_axis={"denoised": 2, "x_next": 2}, ulps=rep == 1 or scale <= 1.0)
            if kind == "random":
                _plant_all("nk_sample_prepare", f"sample_prepare {shape}", got_prep, prep, pixel_axis={"net_in": 1}, padded=("net_in",))
    for entry in ("nk_sample_prepare", "nk_sample_denoise", "nk_sample_euler_step"):
        gb.report(entry)


@pytest.mark.parametrize("n", gb.FLAT_N)
def test_adamw_and_ema_restatement_and_planted_errors(n):
    inp = gb.adamw_inputs(n)
    state = {k: inp[k].clone() for k in ("p", "m", "v")}
    for step, g in zip(gb.ADAMW_STEPS, inp["grads"]):
        exp = gb.adamw_expected(state["p"], g, state["m"], state["v"], step, **gb.ADAMW_HYPER)      # from the restatement's own state
        got = restate_adamw(state["p"], g, state["m"], state["v"], step, **gb.ADAMW_HYPER)
        gb.verify("nk_adamw_flat", f"adamw n={n} step {step}", got, exp, _check)
        _plant_all("nk_adamw_flat", f"adamw n={n} step {step}", got, exp)
        for fault in ("bc2_is_bc1", "beta1_on_grad"):
            _rejected("nk_adamw_flat", f"adamw n={n} step {step} {fault}",
                      restate_adamw(state["p"], g, state["m"], state["v"], step, **gb.ADAMW_HYPER, **{fault: True}), exp)
        state = got
    e = gb.ema_inputs(n)
    for omd in (1e-4, 0.37):
        exp, got = gb.ema_expected(**e, omd=omd), restate_ema(**e, omd=omd)
        gb.verify("nk_ema_flat", f"ema n={n} omd {omd}", got, exp, _check)
        _plant_all("nk_ema_flat", f"ema n={n}", got, exp)
    gb.report("nk_adamw_flat")
    gb.report("nk_ema_flat")


@pytest.mark.parametrize("B, dim", gb.TIMESTEP_SHAPES)
def test_timestep_restatement_and_planted_errors(B, dim):
    for mp in gb.MAX_PERIODS:
        for start in range(0, len(gb.TIMESTEPS), B):
            t = torch.tensor([gb.TIMESTEPS[(start + i) % len(gb.TIMESTEPS)] for i in range(B)], dtype=F32)
            exp, got = gb.timestep_expected(t, dim, mp), restate_timestep(t, dim, mp)
            gb.verify("nk_timestep_embedding", f"timestep {B}x{dim} P={mp} t={t.tolist()}", got, exp, _check)
            if dim % 2:
                assert bool((got["emb"][:, dim - 1] == 0).all())
                bad = got["emb"].clone()
                bad[0, dim - 1] = 2.0 ** -100
                _rejected("nk_timestep_embedding", "odd column", {"emb": bad}, exp)
            _rejected("nk_timestep_embedding", "two ulps", {"emb": _moved(got["emb"], *exp["emb"])}, exp)
    gb.report("nk_timestep_embedding")


def test_layout_and_cast_references():
    """the bit-exact references are torch's own roundings: the specials survive them as the GPU test expects"""
    x = gb.cast_inputs(8 * 256 + 3)
    b = x.to(BF16)
    assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool((x == 0).any())
    assert bool(torch.isinf(b[x == torch.finfo(F32).max]).all()), "the largest finite fp32 rounds to inf"
    one = torch.tensor([0x3F808000, 0x3F818000], dtype=torch.int32).view(F32).to(BF16).view(torch.int16)
    assert one.tolist() == [0x3F80, 0x3F82], "ties round to even: down, then up"
    src = torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(0))
    ref = gb.nchw_to_nhwc_reference(src, 8, 0.13025)
    assert ref.shape == (2, 5, 8) and bool((ref[:, :, 3:] == 0).all())
