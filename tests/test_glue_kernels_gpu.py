"""The hand-written glue kernels through the C ABI, per element against float64 within the derived bounds of tests/glue_bounds.py:
nk_softmax_rows (all four kernels) and nk_softmax_rows_bwd, nk_edm_prepare, nk_edm_loss, nk_sample_prepare / _denoise / _euler_step,
nk_adamw_flat, nk_ema_flat, nk_timestep_embedding, and bit for bit nk_nchw_to_nhwc, nk_nhwc_to_nchw and the two casts.

  guards       every bf16 destination lies between sentinel rows (tests.util._call_into / _guarded), every fp32 destination between NaN
               guard elements: nothing is written outside, nothing inside is left unwritten
  values       tests.glue_bounds: float64 of the exact inputs, bounds from the kernels' operation counts; a padding channel must be 0
  past the cap each kernel's grid cap is exceeded once: one launch equals, bit for bit, the same entry point on the array in two pieces
               (or, for the row kernels, rows past the cap that repeat rows 0, 1, ... equal them)
  refusals     bad sizes and null pointers return NK_ERR_ARG before any launch

The largest error / bound per entry point is printed ("[glue ratio] ...", "[bound] ..."; read with -s) and recorded next to the bounds
in tests/glue_bounds.py."""
import math

import pytest
import torch

from tests import glue_bounds as gb
from tests.test_text_encoder_train_gpu import _check
from tests.util import SENTINEL, _call_into, _guarded

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NK_OK, NK_ERR_ARG = 0, 1
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _cuda(d):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in d.items()}


class _GuardedF32:
    """an fp32 destination of `shape` between 64 NaN guard elements on each side, itself NaN until written"""

    def __init__(self, *shape, init=None):
        self.n = math.prod(shape)
        self.buf = torch.full((self.n + 128,), NAN, dtype=F32, device="cuda")
        self.t = self.buf[64:64 + self.n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def done(self, name, may_hold_nan=False):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:64]).all()) and bool(torch.isnan(self.buf[64 + self.n:]).all()), f"{name} wrote outside its destination"
        assert may_hold_nan or not bool(torch.isnan(self.t).any()), f"{name} left part of its destination unwritten"
        return self.t.clone()


def _in_place(ops, name, x, *tail, src=None):
    """a row kernel that works in place on bf16 [M, L] (argument 0, or argument 1 behind `src`), between sentinel rows"""
    M, L = x.shape
    buf, dst = _guarded(M, L)
    dst.copy_(x)
    ops.call(name, *(() if src is None else (src.data_ptr(),)), dst.data_ptr(), M, L, *tail, ops._stream())
    torch.cuda.synchronize()
    assert bool((buf[:64] == SENTINEL).all()) and bool((buf[64 + M:] == SENTINEL).all()), f"{name} wrote outside its rows"
    return dst.clone()


def _same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.reshape(-1).clone().view(torch.uint8), b.reshape(-1).clone().view(torch.uint8)), what


# ================================================================================================================================
# row softmax
# ================================================================================================================================
@pytest.mark.parametrize("M", gb.SOFTMAX_M)
@pytest.mark.parametrize("L", gb.SOFTMAX_L)
def test_softmax_rows(ops, L, M):
    entry = f"nk_softmax_rows {gb.softmax_chain(L)[0]}"
    for variant in range(4):
        x = gb.softmax_inputs(M, L, variant)
        got = _in_place(ops, "nk_softmax_rows", x.cuda())
        gb.verify(entry, f"softmax {M}x{L} v{variant}", {"p": got}, gb.softmax_expected(x), _check)
    gb.report(entry)


@pytest.mark.parametrize("M, L, cap", [(8193, 8, 8192), (4097, 16392, 4096)])
def test_softmax_rows_past_the_cap(ops, M, L, cap):
    pool = (torch.randn(cap, L, generator=torch.Generator().manual_seed(L)) * 4).to(BF16)
    x = torch.cat([pool, pool[:M - cap]]).cuda()
    got = _in_place(ops, "nk_softmax_rows", x)
    _same_bits(got[cap:], got[:M - cap], "a row past the grid cap differs from its copy among the first rows")
    total = got.float().sum(1)
    assert bool(((total - 1).abs() < 2e-2).all()), "a row was left unnormalised"
    gb.verify("nk_softmax_rows past the cap", f"softmax {M}x{L} rows 0..2", {"p": got[:3]}, gb.softmax_expected(pool[:3]), _check)


@pytest.mark.parametrize("M, L", gb.SOFTMAX_BWD_SHAPES)
def test_softmax_rows_bwd(ops, M, L):
    for scale in gb.SOFTMAX_BWD_SCALES:
        for kind in ("random", "const"):
            p, dp = gb.softmax_bwd_inputs(M, L, kind)
            got = _in_place(ops, "nk_softmax_rows_bwd", dp.cuda(), scale, src=p.cuda())
            gb.verify("nk_softmax_rows_bwd", f"softmax bwd {M}x{L} {kind} scale {scale}", {"ds": got}, gb.softmax_bwd_expected(p, dp, scale), _check)
    gb.report("nk_softmax_rows_bwd")


def test_softmax_rows_bwd_past_the_cap(ops):
    M, L, cap = 4097, 8, 4096
    g = torch.Generator().manual_seed(3)
    p = torch.softmax(torch.randn(cap, L, generator=g).double() * 3, 1).to(BF16)
    dp = torch.randn(cap, L, generator=g).to(BF16)
    p, dp = torch.cat([p, p[:M - cap]]).cuda(), torch.cat([dp, dp[:M - cap]]).cuda()
    got = _in_place(ops, "nk_softmax_rows_bwd", dp, 0.37, src=p)
    _same_bits(got[cap:], got[:M - cap], "a row past the grid cap differs from its copy among the first rows")
    gb.verify("nk_softmax_rows_bwd", "softmax bwd past the cap, rows 0..2", {"ds": got[:3]}, gb.softmax_bwd_expected(p[:3].cpu(), dp[:3].cpu(), 0.37), _check)


# ================================================================================================================================
# EDM prepare and loss
# ================================================================================================================================
def _edm_prepare(ops, x, eps, sigma, c_in, Cpad):
    B, C, HW = x.shape
    zt = _GuardedF32(B, C, HW)
    net_in = _call_into(ops, "nk_edm_prepare", B * HW, Cpad, x, eps, sigma, c_in, zt.t, B, C, HW, Cpad, dst_pos=5)
    return {"zt": zt.done("nk_edm_prepare"), "net_in": net_in.view(B, HW, Cpad)}


@pytest.mark.parametrize("shape", gb.EDM_PREPARE_SHAPES)
def test_edm_prepare(ops, shape):
    B, C, HW, Cpad = shape
    inp = gb.edm_prepare_inputs(*shape)
    assert B == 1 or len(set(inp["sigma"].tolist())) == B
    got = _edm_prepare(ops, **_cuda(inp), Cpad=Cpad)
    gb.verify("nk_edm_prepare", f"edm_prepare {shape}", got, gb.edm_prepare_expected(**inp, Cpad=Cpad), _check)
    gb.report("nk_edm_prepare")


def test_edm_prepare_past_the_cap(ops):
    B, HW, Cpad = 3, 837 * 837, 8
    assert B * HW > 8192 * 256 and HW % 256
    g = torch.Generator(device="cuda").manual_seed(5)
    x, eps = (torch.randn(B, 1, HW, generator=g, device="cuda") for _ in range(2))
    sigma = torch.tensor([0.3, 1.7, 9.0], device="cuda")
    c_in = gb._precond(sigma)[0]
    whole = _edm_prepare(ops, x, eps, sigma, c_in, Cpad)
    parts = [_edm_prepare(ops, x[s], eps[s], sigma[s], c_in[s], Cpad) for s in (slice(0, 1), slice(1, 3))]
    for name in ("zt", "net_in"):
        _same_bits(whole[name], torch.cat([q[name] for q in parts]), f"nk_edm_prepare {name}: a value depends on where its pixel lies in the launch")


def _edm_loss(ops, inp, C, upstream, with_dnet=True):
    B, HW, Cpad = inp["net_out"].shape
    loss = _GuardedF32(B)
    args = (inp["net_out"], inp["zt"], inp["target"], inp["c_out"], inp["c_skip"], inp["w"], loss.t)
    if with_dnet:
        dnet = _call_into(ops, "nk_edm_loss", B * HW, Cpad, *args, B, C, HW, Cpad, upstream, dst_pos=7).view(B, HW, Cpad)
    else:
        ops.call("nk_edm_loss", *(a.data_ptr() for a in args), None, B, C, HW, Cpad, upstream, ops._stream())
        dnet = None
    return {"loss": loss.done("nk_edm_loss"), "dnet": dnet}


@pytest.mark.parametrize("shape", gb.EDM_LOSS_SHAPES)
def test_edm_loss(ops, shape):
    B, C, HW, Cpad = shape
    for kind in ("plain", "cancel"):
        inp = gb.edm_loss_inputs(*shape, kind)
        dev = _cuda(inp)
        for upstream in gb.EDM_UPSTREAMS:
            got = _edm_loss(ops, dev, C, upstream)
            gb.verify("nk_edm_loss", f"edm_loss {shape} {kind} upstream {upstream}", got, gb.edm_loss_expected(**inp, C=C, upstream=upstream), _check)
            again, alone = _edm_loss(ops, dev, C, upstream), _edm_loss(ops, dev, C, upstream, with_dnet=False)
            _same_bits(again["loss"], got["loss"], "two runs of nk_edm_loss give different losses")
            _same_bits(again["dnet"], got["dnet"], "two runs of nk_edm_loss give different gradients")
            _same_bits(alone["loss"], got["loss"], "the loss depends on whether the gradient is asked for")
            if B > 1:
                assert float(got["loss"][B - 1]) == 0.0 and bool((got["dnet"][B - 1] == 0).all()), "w = 0: loss 0, gradient rows zero"
    gb.report("nk_edm_loss")


# ================================================================================================================================
# sampler
# ================================================================================================================================
def _euler(ops, d, scale, rep, Cpad, with_denoised=True, alias=False):
    B, C, HW = d["x"].shape
    x = _GuardedF32(B, C, HW, init=d["x"])
    x_next = x if alias else _GuardedF32(B, C, HW)
    den = _GuardedF32(B, C, HW) if with_denoised else None
    ops.call("nk_sample_euler_step", d["net_out"].data_ptr(), x.t.data_ptr(), d["c_skip"].data_ptr(), d["c_out"].data_ptr(), d["sigma_hat"].data_ptr(),
             d["sigma_next"].data_ptr(), scale, x_next.t.data_ptr(), den.t.data_ptr() if den else None, B, C, HW, Cpad, rep, ops._stream())
    out = {"x_next": x_next.done("nk_sample_euler_step")}
    if den:
        out["denoised"] = den.done("nk_sample_euler_step")
    if not alias:
        _same_bits(x.done("nk_sample_euler_step"), d["x"], "nk_sample_euler_step changed its input latents")
    return out


@pytest.mark.parametrize("rep", gb.SAMPLE_REPS)
@pytest.mark.parametrize("shape", gb.SAMPLE_SHAPES)
def test_sampler_kernels(ops, shape, rep):
    B, C, HW, Cpad = shape
    for kind in gb.SAMPLE_KINDS:
        inp = gb.sample_inputs(*shape, rep, kind)
        d = _cuda(inp)
        assert C == Cpad or bool(torch.isnan(inp["net_out"][:, :, C:].float()).all())
        net_in = _call_into(ops, "nk_sample_prepare", rep * B * HW, Cpad, d["x"], d["c_in"], B, C, HW, Cpad, rep, dst_pos=2).view(rep * B, HW, Cpad)
        gb.verify("nk_sample_prepare", f"sample_prepare {shape} rep {rep}", {"net_in": net_in}, gb.sample_prepare_expected(inp["x"], inp["c_in"], Cpad, rep), _check)
        _same_bits(net_in[:B], net_in[(rep - 1) * B:], "the replicas of nk_sample_prepare differ")
        args = {k: inp[k] for k in ("x", "net_out", "c_skip", "c_out", "sigma_hat", "sigma_next")}
        for scale in gb.SAMPLE_SCALES:
            exp = gb.sample_expected(**args, scale=scale, rep=rep)
            label = f"sample {shape} rep {rep} {kind} scale {scale}"
            den = _GuardedF32(B, C, HW)
            ops.call("nk_sample_denoise", d["net_out"].data_ptr(), d["x"].data_ptr(), d["c_skip"].data_ptr(), d["c_out"].data_ptr(), scale, den.t.data_ptr(),
                     B, C, HW, Cpad, rep, ops._stream())
            den = den.done("nk_sample_denoise")
            gb.verify("nk_sample_denoise", label, {"denoised": den}, {"denoised": exp["denoised"]}, _check)
            got = _euler(ops, d, scale, rep, Cpad)
            gb.verify("nk_sample_euler_step", label, got, exp, _check)
            _same_bits(got["denoised"], den, "nk_sample_euler_step and nk_sample_denoise disagree on the denoised latents")
            _same_bits(_euler(ops, d, scale, rep, Cpad, with_denoised=False)["x_next"], got["x_next"], "x_next depends on whether denoised is asked for")
            _same_bits(_euler(ops, d, scale, rep, Cpad, alias=True)["x_next"], got["x_next"], "x_next written over x differs")
    for entry in ("nk_sample_prepare", "nk_sample_denoise", "nk_sample_euler_step"):
        gb.report(entry)


def test_sample_euler_step_past_the_cap(ops):
    B, HW, Cpad = 2, 8_388_737, 8
    assert HW > 65535 * 256 // 2 and B * HW > 65535 * 256 and HW % 256
    g = torch.Generator(device="cuda").manual_seed(9)
    net = torch.randn(B, HW, Cpad, generator=g, device="cuda", dtype=BF16)
    x = torch.randn(B, 1, HW, generator=g, device="cuda")
    sigma = torch.tensor([0.7, 4.0], device="cuda")
    _, c_skip, c_out = gb._precond(sigma)
    nxt = torch.tensor([0.4, 2.5], device="cuda")
    def run(s):
        xn, den = torch.full_like(x[s], NAN), torch.full_like(x[s], NAN)
        ops.call("nk_sample_euler_step", net[s].data_ptr(), x[s].data_ptr(), c_skip[s].data_ptr(), c_out[s].data_ptr(), sigma[s].data_ptr(), nxt[s].data_ptr(),
                 1.0, xn.data_ptr(), den.data_ptr(), s.stop - s.start, 1, HW, Cpad, 1, ops._stream())
        torch.cuda.synchronize()
        assert not bool(torch.isnan(xn).any()) and not bool(torch.isnan(den).any()), "nk_sample_euler_step left part of its destination unwritten"
        return xn, den
    whole = run(slice(0, 2))
    parts = [run(slice(0, 1)), run(slice(1, 2))]
    for j, name in enumerate(("x_next", "denoised")):
        _same_bits(whole[j], torch.cat([q[j] for q in parts]), f"nk_sample_euler_step {name}: a value depends on where its pixel lies in the launch")


# ================================================================================================================================
# AdamW, EMA
# ================================================================================================================================
def _adamw(ops, p, g, m, v, shadow, step, n=None):
    h = gb.ADAMW_HYPER
    ops.call("nk_adamw_flat", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr(), p.numel() if n is None else n, h["lr"], h["beta1"],
             h["beta2"], h["eps"], h["weight_decay"], step, h["grad_scale"], ops._stream())


@pytest.mark.parametrize("n", gb.FLAT_N)
def test_adamw_flat_three_steps(ops, n):
    inp = gb.adamw_inputs(n)
    state = {k: _GuardedF32(n, init=inp[k].cuda()) for k in ("p", "m", "v")}
    before = {k: inp[k] for k in ("p", "m", "v")}
    for step, g in zip(gb.ADAMW_STEPS, inp["grads"]):
        buf, shadow = _guarded(1, n)
        _adamw(ops, state["p"].t, g.cuda(), state["m"].t, state["v"].t, shadow, step)
        got = {k: s.done("nk_adamw_flat").cpu() for k, s in state.items()}
        assert bool((buf[:64] == SENTINEL).all()) and bool((buf[65:] == SENTINEL).all()), "nk_adamw_flat wrote outside its shadow"
        # the float64 step starts from the kernel's own previous fp32 state: errors do not compound
        gb.verify("nk_adamw_flat", f"adamw n={n} step {step}", got, gb.adamw_expected(before["p"], g, before["m"], before["v"], step, **gb.ADAMW_HYPER), _check)
        assert torch.equal(shadow.view(-1).cpu(), got["p"].to(BF16)), "the bf16 shadow is not the rounded master"
        before = got
    gb.report("nk_adamw_flat")


def test_adamw_flat_past_the_cap(ops):
    n, cut = 4 * (8192 * 256 + 257), 4 * (1000 * 256 + 100)
    g = torch.Generator(device="cuda").manual_seed(13)
    p, grad, m = (torch.randn(n, generator=g, device="cuda") for _ in range(3))
    v = torch.rand(n, generator=g, device="cuda") * 1e-2
    runs = []
    for pieces in ((slice(0, n),), (slice(0, cut), slice(cut, n))):
        q, mm, vv = p.clone(), m.clone(), v.clone()
        shadow = torch.full((n,), NAN, dtype=BF16, device="cuda")
        for s in pieces:
            _adamw(ops, q[s], grad[s], mm[s], vv[s], shadow[s], 2)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(shadow).any()), "nk_adamw_flat left part of its shadow unwritten"
        runs.append((q, mm, vv, shadow))
    for name, a, b in zip(("p", "m", "v", "shadow"), *runs):
        _same_bits(a, b, f"nk_adamw_flat {name}: a value depends on where its element lies in the launch")
    assert not torch.equal(runs[0][0], p), "the step changed nothing"


@pytest.mark.parametrize("n", gb.FLAT_N)
def test_ema_flat(ops, n):
    inp = gb.ema_inputs(n)
    for omd in (1e-4, 0.37):
        ema = _GuardedF32(n, init=inp["ema"].cuda())
        ops.call("nk_ema_flat", ema.t.data_ptr(), inp["p"].cuda().data_ptr(), n, omd, ops._stream())
        gb.verify("nk_ema_flat", f"ema n={n} omd {omd}", {"ema": ema.done("nk_ema_flat")}, gb.ema_expected(**inp, omd=omd), _check)
    gb.report("nk_ema_flat")


def test_ema_flat_past_the_cap(ops):
    n, cut = 4 * (16384 * 256 + 257), 4 * (1000 * 256 + 100)
    g = torch.Generator(device="cuda").manual_seed(17)
    p, ema = torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda")
    whole, parts = ema.clone(), ema.clone()
    ops.call("nk_ema_flat", whole.data_ptr(), p.data_ptr(), n, 0.01, ops._stream())
    for s in (slice(0, cut), slice(cut, n)):
        ops.call("nk_ema_flat", parts[s].data_ptr(), p[s].data_ptr(), s.stop - s.start, 0.01, ops._stream())
    torch.cuda.synchronize()
    _same_bits(whole, parts, "nk_ema_flat: a value depends on where its element lies in the launch")
    assert int((whole != ema).sum()) > n * 0.99, "elements were left unchanged"


# ================================================================================================================================
# timestep embedding
# ================================================================================================================================
@pytest.mark.parametrize("B, dim", gb.TIMESTEP_SHAPES)
def test_timestep_embedding(ops, B, dim):
    for mp in gb.MAX_PERIODS:
        for start in range(0, len(gb.TIMESTEPS), B):
            t = torch.tensor([gb.TIMESTEPS[(start + i) % len(gb.TIMESTEPS)] for i in range(B)], dtype=F32)
            emb = _call_into(ops, "nk_timestep_embedding", B, dim, t.cuda(), B, dim, mp)
            gb.verify("nk_timestep_embedding", f"timestep {B}x{dim} P={mp} t={t.tolist()}", {"emb": emb}, gb.timestep_expected(t, dim, mp), _check)
    gb.report("nk_timestep_embedding")


# ================================================================================================================================
# layout and casts: bit for bit
# ================================================================================================================================
@pytest.mark.parametrize("shape", gb.LAYOUT_SHAPES)
def test_layout_kernels(ops, shape):
    N, C, HW, Cpad = shape
    g = torch.Generator().manual_seed(sum(shape))
    for src_is_f32 in (1, 0):
        src = torch.randn(N, C, HW, generator=g) * 3
        src = src if src_is_f32 else src.to(BF16)
        for scale in gb.LAYOUT_SCALES:
            got = _call_into(ops, "nk_nchw_to_nhwc", N * HW, Cpad, src.cuda(), src_is_f32, N, C, HW, Cpad, scale, dst_pos=2).view(N, HW, Cpad)
            _same_bits(got.cpu(), gb.nchw_to_nhwc_reference(src, Cpad, scale), f"nk_nchw_to_nhwc {shape} f32={src_is_f32} scale {scale}")
    tokens = gb._tokens((torch.randn(N, C, HW, generator=g) * 3).to(BF16), Cpad, NAN)      # NaN padding channels: nothing may read them into the image
    want = tokens[:, :, :C].permute(0, 2, 1).contiguous()
    got = _call_into(ops, "nk_nhwc_to_nchw", N * C, HW, tokens.cuda(), 0, N, C, HW, Cpad, dst_pos=1).view(N, C, HW)
    _same_bits(got.cpu(), want, f"nk_nhwc_to_nchw {shape} to bf16")
    dst = _GuardedF32(N, C, HW)
    ops.call("nk_nhwc_to_nchw", tokens.cuda().data_ptr(), dst.t.data_ptr(), 1, N, C, HW, Cpad, ops._stream())
    _same_bits(dst.done("nk_nhwc_to_nchw").cpu(), want.float(), f"nk_nhwc_to_nchw {shape} to fp32")


def _same_bits_or_nan(got, want, what):
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), nan), f"{what}: NaN positions differ"
    _same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want), what)


@pytest.mark.parametrize("n", gb.CAST_N)
def test_cast_f32_to_bf16(ops, n):
    x = gb.cast_inputs(n)
    got = _call_into(ops, "nk_cast_f32_to_bf16", 1, n, x.cuda(), n).view(-1).cpu()
    _same_bits_or_nan(got, x.to(BF16), f"nk_cast_f32_to_bf16 n={n}")


def test_cast_f32_to_bf16_past_the_cap(ops):
    n, cut = 8 * (8192 * 256) + 13, 8 * (1000 * 256 + 100)
    x = torch.randn(n, generator=torch.Generator(device="cuda").manual_seed(19), device="cuda")
    whole, parts = (torch.full((n,), NAN, dtype=BF16, device="cuda") for _ in range(2))
    ops.call("nk_cast_f32_to_bf16", x.data_ptr(), whole.data_ptr(), n, ops._stream())
    for s in (slice(0, cut), slice(cut, n)):
        ops.call("nk_cast_f32_to_bf16", x[s].data_ptr(), parts[s].data_ptr(), s.stop - s.start, ops._stream())
    torch.cuda.synchronize()
    _same_bits(whole, parts, "nk_cast_f32_to_bf16: a value depends on where its element lies in the launch")
    _same_bits(whole, x.to(BF16), "nk_cast_f32_to_bf16 differs from torch's rounding")


def test_cast_bf16_to_f32_every_bit_pattern(ops):
    src = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16).cuda()
    dst = torch.zeros(65536 + 128, dtype=torch.int32, device="cuda")
    ops.call("nk_cast_bf16_to_f32", src.data_ptr(), dst[64:].data_ptr(), 65536, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(dst[64:64 + 65536].cpu(), torch.arange(65536, dtype=torch.int64).mul(65536).to(torch.int32)), "a bf16 pattern is not its fp32 pattern"
    assert not bool(dst[:64].any()) and not bool(dst[64 + 65536:].any()), "nk_cast_bf16_to_f32 wrote outside its destination"


# ================================================================================================================================
# refusals (each returns before any launch)
# ================================================================================================================================
def test_argument_refusals(ops):
    arena = torch.zeros(8 * 4096, dtype=torch.uint8, device="cuda")
    a = [arena.data_ptr() + 4096 * j for j in range(6)]
    st = ops._stream()
    q = ops.query
    for tail, what in (((1, 12), "L % 8 != 0"), ((0, 8), "M = 0")):
        assert q("nk_softmax_rows", a[0], *tail, st) == NK_ERR_ARG, what
        assert q("nk_softmax_rows_bwd", a[0], a[1], *tail, 1.0, st) == NK_ERR_ARG, what
    assert q("nk_softmax_rows", None, 1, 8, st) == NK_ERR_ARG
    assert q("nk_softmax_rows_bwd", None, a[1], 1, 8, 1.0, st) == NK_ERR_ARG and q("nk_softmax_rows_bwd", a[0], None, 1, 8, 1.0, st) == NK_ERR_ARG
    h = (1e-3, 0.9, 0.95, 1e-8, 0.01)
    assert q("nk_adamw_flat", *a[:5], 6, *h, 1, 1.0, st) == NK_ERR_ARG, "n % 4 != 0"
    assert q("nk_adamw_flat", *a[:5], 8, *h, 0, 1.0, st) == NK_ERR_ARG, "step = 0"
    for j in range(5):
        assert q("nk_adamw_flat", *a[:j], None, *a[j + 1:5], 8, *h, 1, 1.0, st) == NK_ERR_ARG, f"null pointer {j}"
    assert q("nk_ema_flat", a[0], a[1], 6, 0.01, st) == NK_ERR_ARG, "n % 4 != 0"
    assert q("nk_ema_flat", None, a[1], 8, 0.01, st) == NK_ERR_ARG and q("nk_ema_flat", a[0], None, 8, 0.01, st) == NK_ERR_ARG
    torch.cuda.synchronize()
    assert not bool(arena.any()), "a refused call wrote"


def test_report_ratios():
    """the largest error / bound per entry point of this run (read with -s)"""
    for entry in sorted(gb.RATIOS):
        gb.report(entry)
