"""The map kernels on the core of csrc/nk_ew.h (elementwise.hip, and the activation / BatchNorm-apply / pooling half of gan.hip), entry point by
entry point at the smallest shapes that reach every branch of the three index decodes:

  guard rows             every destination lies between sentinel rows: nothing is written outside it, nothing inside is left unwritten
  exact values           where the result is representable (add, concat / split, the resamplers and pools on small integers, LeakyReLU with
                         slope 1/4, ReLU) it equals a float64 torch reference bit for bit, torch's first-maximum tie rule included
  tolerance values       SiLU, GEGLU, the GELU modes, the gated tanh form and BatchNorm against float64, within the tolerance the existing test of
                         the op uses: TOL_BF16 of tests/test_kernels_gpu.py (SiLU, GEGLU; BatchNorm too, test_patchgan_gpu asks no less), the
                         derived gelu_new bound of tests/test_t5_kernels_gpu.py, the half-ulp bound of test_gelu_backward_fp64 from its pieces,
                         and for the GELU forward modes 0 and 1 a per-element half-ulp bound derived here (_gelu_fwd_bound), tighter than the
                         2^-7 max |y| of test_gelu_kernel
  position independence  past the grid cap (8192 blocks of 256 items) one launch equals, bit for bit, the same entry point run on the array in
                         two pieces cut off a block boundary: a wrong stride shows here; both destinations start as NaN, so an item a
                         launch skips shows too
  argument refusals      entry point against bad argument, each row with the return value the hand-written entry points gave (their NK_CHECK_ARG
                         lines); a misaligned pointer is refused only where it always was (nk_gelu_bwd, nk_gated_gelu_tanh_fwd)"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import adm_ref as R
from tests import attention_bounds as ab
from tests.test_adm_gpu import RS_SHAPES, bits, tok, untok
from tests.test_kernels_gpu import TOL_BF16
from tests.test_t5_kernels_gpu import _gelu_new_reference, _within
from tests.test_text_encoder_train_gpu import U, _check
from tests.util import _call_into, assert_close

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64
PAST_CAP = 8192 * 256 + 257          # work items: the stride loop runs a second, ragged round


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


def _randn(*shape, seed, scale=2.0):
    """bf16 normal values on the GPU with zeros (of both signs) among them"""
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)
    flat = x.view(-1)
    flat[::5] = 0.0
    flat[3::10] = -0.0
    return x.cuda()


def _ints(*shape, seed, lo=-7, hi=8):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).to(BF).cuda()


def _erf_gelu(x):
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    return x * cdf, cdf + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)      # value, derivative


def _quick_gelu(x):
    s = torch.sigmoid(1.702 * x)
    return x * s, s + 1.702 * x * s * (1 - s)


def _gelu_fwd_bound(mode, x, ref):
    """Where the forward rounds, U = 2^-24 in fp32, then one rounding to bf16 (half a bf16 ulp of the float64 value):
      mode 0  y = 0.5 x (1 + erf(x / sqrt 2)): the argument's scaling and erff (a few ulp of a value <= 1) leave 1 + erf off by <= 10 U
              ABSOLUTE -- where erf is near -1 the sum cancels, so the error scales with |x|, not with y: 0.5 |x| 10 U, and 2 U |y| for the
              two multiplies
      mode 1  y = x / (1 + e), e = exp(-z), z = 1.702 x: the analysis of gelu_new in tests/test_t5_kernels_gpu.py with this z,
              (6 |z| + 11) U relative"""
    b = ab.SAFETY * U * ((5 * x.abs() + 2 * ref.abs()) if mode == 0 else (6 * (1.702 * x).abs() + 11) * ref.abs())
    return b + ab.half_ulp(ref, b)


# ------------------------------------------------------------------------------------------------
# flat ops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 8 * 257])
def test_flat_ops(ops, n):
    x, dy = _randn(n, seed=n), _randn(n, seed=n + 1)
    xd, dyd = x.to(F64), dy.to(F64)
    run = lambda name, *args, dst_pos=1: _call_into(ops, name, n // 8, 8, *args, dst_pos=dst_pos).view(-1)
    sg = torch.sigmoid(xd)
    assert_close(run("nk_silu_fwd", x, n), xd * sg, TOL_BF16, "silu fwd")
    assert_close(run("nk_silu_bwd", dy, x, n, dst_pos=2), dyd * sg * (1 + xd * (1 - sg)), TOL_BF16, "silu bwd")
    for mode, (ref, dref) in ((0, _erf_gelu(xd)), (1, _quick_gelu(xd))):
        _within(run("nk_gelu_fwd", x, n, mode), ref, _gelu_fwd_bound(mode, xd, ref), f"gelu fwd mode {mode} n={n}")
        want = dyd * dref      # the bound of test_gelu_backward_fp64 (tests/test_text_encoder_train_gpu.py), from its pieces
        _check(f"gelu bwd mode {mode} n={n}", run("nk_gelu_bwd", dy, x, n, mode, dst_pos=2), want,
               ab.half_ulp(want, torch.zeros_like(want)) * (1 + 2.0 ** -6) + 64 * U * dyd.abs() * (1 + xd.abs()))
    _within(run("nk_gelu_fwd", x, n, 2), *_gelu_new_reference(x, torch.ones_like(x)), f"gelu_new n={n}")
    assert torch.equal(run("nk_gelu_fwd", x, n, 3), torch.relu(x)), "ReLU is exact"
    # exact: sums of small integers; a quarter of a bf16 value
    a, b = _ints(n, seed=n + 2, lo=-60, hi=61), _ints(n, seed=n + 3, lo=-60, hi=61)
    assert torch.equal(run("nk_add", a, b, n, dst_pos=2).to(F64), a.to(F64) + b.to(F64))
    y = run("nk_leaky_relu_fwd", x, n, 0.25)
    assert torch.equal(y.to(F64), torch.where(xd >= 0, xd, xd * 0.25))
    assert torch.equal(run("nk_leaky_relu_bwd", dy, y, n, 0.25, dst_pos=2).to(F64), torch.where(y.to(F64) > 0, dyd, dyd * 0.25))


# ------------------------------------------------------------------------------------------------
# rows ops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, I", [(1, 8), (3, 8), (257, 24), (300, 2560)])
def test_gated_activations(ops, M, I):
    u, dy = _randn(M, 2 * I, seed=M + I), _randn(M, I, seed=M + I + 1)
    a, g, dyd = u[:, :I].to(F64), u[:, I:].to(F64), dy.to(F64)
    gelu, dgelu = _erf_gelu(g)
    y = _call_into(ops, "nk_geglu_fwd", M, I, u, M, I)
    assert_close(y, a * gelu, TOL_BF16, "geglu fwd")
    du = _call_into(ops, "nk_geglu_bwd", M, 2 * I, dy, u, M, I, dst_pos=2)
    assert_close(du, torch.cat([dyd * gelu, dyd * a * dgelu], 1), TOL_BF16, "geglu bwd")
    # the saved-derivative form: y and s guarded in turn, then with s = u
    s = torch.empty_like(u)
    ys = _call_into(ops, "nk_geglu_fwd_s", M, I, u, s, M, I)
    assert_close(ys, a * gelu, TOL_BF16, "geglu fwd, saved-derivative form")
    assert_close(s, torch.cat([gelu, a * dgelu], 1), TOL_BF16, "geglu saved derivatives")
    y2 = torch.empty_like(y)
    assert torch.equal(bits(_call_into(ops, "nk_geglu_fwd_s", M, 2 * I, u, y2, M, I, dst_pos=2)), bits(s)) and torch.equal(bits(y2), bits(ys))
    u_in_place = u.clone()
    y3 = _call_into(ops, "nk_geglu_fwd_s", M, I, u_in_place, u_in_place, M, I)
    assert torch.equal(bits(y3), bits(ys)) and torch.equal(bits(u_in_place), bits(s)), "s = u: every item reads its two chunks before it writes them"
    dus = _call_into(ops, "nk_geglu_bwd_s", M, 2 * I, dy, s, M, I, dst_pos=2)
    assert_close(dus, s.to(F64) * torch.cat([dyd, dyd], 1), TOL_BF16, "geglu bwd from saved derivatives")
    # T5's gate: gelu_new(first half) * second half
    x12 = (u[:, :I].float().clamp(-6, 6) * 2).to(BF)
    t5 = _call_into(ops, "nk_gated_gelu_tanh_fwd", M, I, torch.cat([x12, u[:, I:]], 1).contiguous(), M, I)
    _within(t5, *_gelu_new_reference(x12, u[:, I:]), f"gated gelu_new {M}x{I}")


@pytest.mark.parametrize("rows, Ca, Cb", [(70, 320, 640), (5, 8, 8)])
def test_concat_and_split(ops, rows, Ca, Cb):
    a, b = _randn(rows, Ca, seed=Ca), _randn(rows, Cb, seed=Cb + 1)
    out = _call_into(ops, "nk_cat_channels", rows, Ca + Cb, a, b, rows, Ca, Cb, dst_pos=2)
    assert torch.equal(bits(out), bits(torch.cat([a, b], 1)))
    for other_a, other_b in ((torch.empty_like(a), torch.empty_like(b)), (None, None)):      # both sides, then each side alone
        got_a = _call_into(ops, "nk_split_channels", rows, Ca, out, other_b, rows, Ca, Cb, dst_pos=1)
        got_b = _call_into(ops, "nk_split_channels", rows, Cb, out, other_a, rows, Ca, Cb, dst_pos=2)
        assert torch.equal(bits(got_a), bits(a)) and torch.equal(bits(got_b), bits(b))
        if other_a is not None:
            assert torch.equal(bits(other_a), bits(a)) and torch.equal(bits(other_b), bits(b))


@pytest.mark.parametrize("M, C", [(65, 8), (4096, 64)])
@pytest.mark.parametrize("slope", [0.2, 1.0])
def test_batchnorm_apply_and_dx(ops, M, C, slope):
    x, dy = _randn(M, C, seed=M), _randn(M, C, seed=M + 1)
    g = torch.Generator().manual_seed(C)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()
    mean, rstd, dgamma, dbeta = (torch.empty(C, device="cuda") for _ in range(4))
    ws = torch.empty(ops.query("nk_batchnorm_ws_floats", M, C), device="cuda")
    y = _call_into(ops, "nk_batchnorm_fwd", M, C, x, gamma, beta, mean, rstd, None, None, ws, M, C, 1e-5, 0.1, slope, dst_pos=3)
    xr = x.to(F64).requires_grad_(True)
    gr, br = gamma.to(F64).requires_grad_(True), beta.to(F64).requires_grad_(True)
    ref = F.leaky_relu(F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5), slope)
    ref.backward(dy.to(F64))
    assert_close(y, ref, TOL_BF16, "batchnorm fwd")
    dx = _call_into(ops, "nk_batchnorm_bwd", M, C, dy, x, y, gamma, mean, rstd, dgamma, dbeta, ws, M, C, slope, 0, dst_pos=6)
    assert_close(dx, xr.grad, TOL_BF16, "batchnorm dx")


# ------------------------------------------------------------------------------------------------
# pixel ops
# ------------------------------------------------------------------------------------------------
def _ties(shape, seed):
    """half-integers in [-2, 2]: every pooling window holds equal values, so the first-maximum rule decides"""
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).double() / 2


@pytest.mark.parametrize("shape", RS_SHAPES + [(1, 8, 2, 2), (2, 8, 6, 10)])
def test_resamplers_on_small_integers(ops, shape):
    N, C, H, W = shape
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randint(-31, 32, shape, generator=g).double()
    dy = torch.randint(-31, 32, (N, C, Ho, Wo), generator=g).double()
    dup = torch.randint(-7, 8, (N, C, 2 * H, 2 * W), generator=g).double()
    up = _call_into(ops, "nk_upsample2x_fwd", N * 4 * H * W, C, tok(x), N, H, W, C)
    assert torch.equal(untok(up, N, 2 * H, 2 * W).double(), R.upsample2x(x))
    dx = _call_into(ops, "nk_upsample2x_bwd", N * H * W, C, tok(dup), N, H, W, C)
    assert torch.equal(untok(dx, N, H, W).double(), R.upsample2x_bwd(dup))
    y = _call_into(ops, "nk_avgpool2x_fwd", N * Ho * Wo, C, tok(x), N, H, W, C)      # an exact fp32 sum, rounded once
    assert torch.equal(untok(y, N, Ho, Wo), R.avgpool2x(x).float().to(BF).float())
    dx = _call_into(ops, "nk_avgpool2x_bwd", N * H * W, C, tok(dy), N, H, W, C)      # zeros in an odd last row / column
    assert torch.equal(untok(dx, N, H, W).double(), R.avgpool2x_bwd(dy, H, W))


def _maxpool_reference(x, dy_seed, k, s):
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, k, s)
    dy = torch.randint(-7, 8, ref.shape, generator=torch.Generator().manual_seed(dy_seed)).double()      # sums of up to four are exact in bf16
    ref.backward(dy)
    return ref.detach(), dy, xr.grad


@pytest.mark.parametrize("shape, k, s", [(sh, 2, 2) for sh in RS_SHAPES + [(1, 8, 2, 2), (2, 8, 6, 10)]] + [(sh, 3, 2) for sh in RS_SHAPES + [(1, 8, 3, 3), (2, 16, 7, 9)]])
def test_max_pools_with_ties(ops, shape, k, s):
    N, C, H, W = shape
    x = _ties(shape, seed=sum(shape) + k)
    ref, dy, want_dx = _maxpool_reference(x, 5, k, s)
    Ho, Wo = ref.shape[2:]
    y = _call_into(ops, "nk_maxpool_fwd", N * Ho * Wo, C, tok(x), N, H, W, C, k, s)
    assert torch.equal(untok(y, N, Ho, Wo).double(), ref)
    dx = _call_into(ops, "nk_maxpool_bwd", N * H * W, C, tok(dy), tok(x), N, H, W, C, k, s, dst_pos=2)
    assert torch.equal(untok(dx, N, H, W).double(), want_dx)
    if k == 2 and H % 2 == 0 and W % 2 == 0:      # the 2 x 2 kernels take even extents only
        y2 = _call_into(ops, "nk_maxpool2x2_fwd", N * Ho * Wo, C, tok(x), N, H, W, C)
        dx2 = _call_into(ops, "nk_maxpool2x2_bwd", N * H * W, C, tok(dy), tok(x), N, H, W, C, dst_pos=2)
        assert torch.equal(bits(y2), bits(y)) and torch.equal(untok(dx2, N, H, W).double(), want_dx)


# ------------------------------------------------------------------------------------------------
# position independence past the grid cap
# ------------------------------------------------------------------------------------------------
def _in_two_pieces(ops, name, src, dst_like, rows, cut, tail):
    """entry point `name`(src, dst, *tail(rows)) on all `rows` leading slices of src at once, and on [0, cut) and [cut, rows) separately"""
    whole, parts = torch.full_like(dst_like, float("nan")), torch.full_like(dst_like, float("nan"))
    ops.call(name, src.data_ptr(), whole.data_ptr(), *tail(rows), ops._stream())
    ops.call(name, src[:cut].data_ptr(), parts[:cut].data_ptr(), *tail(cut), ops._stream())
    ops.call(name, src[cut:].data_ptr(), parts[cut:].data_ptr(), *tail(rows - cut), ops._stream())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(whole).any()) and not bool(torch.isnan(parts).any()), f"{name} left part of its destination unwritten"
    assert torch.equal(bits(whole), bits(parts)), f"{name}: a value depends on where its item lies in the launch"


def test_results_do_not_depend_on_the_position_in_the_launch(ops):
    pool = torch.randn(1 << 22, generator=torch.Generator().manual_seed(11)).to(BF).cuda()
    fill = lambda *shape: pool[torch.arange(math.prod(shape), device="cuda") % pool.numel()].view(*shape)
    # flat: items of 8 elements, cut 100 items past a block boundary
    x = fill(PAST_CAP, 8)
    _in_two_pieces(ops, "nk_silu_fwd", x, x, PAST_CAP, 1000 * 256 + 100, lambda r: (r * 8,))
    # rows: one chunk per row of the gated input [M][16]
    u = fill(PAST_CAP, 16)
    _in_two_pieces(ops, "nk_geglu_fwd", u, u[:, :8].contiguous(), PAST_CAP, 777_777, lambda r: (r, 8))
    del x, u
    # pixels: three images of 837 x 837 output pixels, one chunk each (2 101 707 items); one image, then two
    Hh = 2 * 837
    assert 3 * 837 * 837 > 8192 * 256 and (837 * 837) % 256
    img = fill(3, Hh * Hh, 8)
    _in_two_pieces(ops, "nk_avgpool2x_fwd", img, torch.empty(3, 837 * 837, 8, dtype=BF, device="cuda"), 3, 1, lambda r: (r, Hh, Hh, 8))


# ------------------------------------------------------------------------------------------------
# argument refusals
# ------------------------------------------------------------------------------------------------
# entry point -> (pointer arguments, a good tail, {bad argument: bad tail}, refuses a misaligned pointer)
_FLAT = {"n % 8 != 0": (12,), "n = 0": (0,)}
_ROWS = {"I % 8 != 0": (1, 12), "M = 0": (0, 8)}
_PIX = {"C % 8 != 0": (1, 2, 2, 12), "N = 0": (0, 2, 2, 8)}
REFUSALS = {
    "nk_silu_fwd": (2, (8,), _FLAT, False),
    "nk_silu_bwd": (3, (8,), _FLAT, False),
    "nk_add": (3, (8,), _FLAT, False),
    "nk_gelu_fwd": (2, (8, 0), {"n % 8 != 0": (12, 0), "mode 4": (8, 4)}, False),
    "nk_gelu_bwd": (3, (8, 0), {"n % 8 != 0": (12, 0), "mode 2": (8, 2)}, True),
    "nk_leaky_relu_fwd": (2, (8, 0.25), {"n % 8 != 0": (12, 0.25), "slope < 0": (8, -0.5)}, False),
    "nk_leaky_relu_bwd": (3, (8, 0.25), {"n % 8 != 0": (12, 0.25), "slope < 0": (8, -0.5)}, False),
    "nk_geglu_fwd": (2, (1, 8), _ROWS, False),
    "nk_geglu_bwd": (3, (1, 8), _ROWS, False),
    "nk_geglu_fwd_s": (3, (1, 8), _ROWS, False),
    "nk_geglu_bwd_s": (3, (1, 8), _ROWS, False),
    "nk_gated_gelu_tanh_fwd": (2, (1, 8), _ROWS, True),
    "nk_cat_channels": (3, (1, 8, 8), {"Ca % 8 != 0": (1, 12, 8), "Cb % 8 != 0": (1, 8, 12), "rows = 0": (0, 8, 8)}, False),
    "nk_split_channels": (3, (1, 8, 8), {"Ca % 8 != 0": (1, 12, 8), "Cb % 8 != 0": (1, 8, 12), "rows = 0": (0, 8, 8)}, False),
    "nk_upsample2x_fwd": (2, (1, 2, 2, 8), _PIX, False),
    "nk_upsample2x_bwd": (2, (1, 2, 2, 8), _PIX, False),
    "nk_avgpool2x_fwd": (2, (1, 2, 2, 8), {**_PIX, "H = 1": (1, 1, 2, 8), "W = 1": (1, 2, 1, 8)}, False),
    "nk_avgpool2x_bwd": (2, (1, 2, 2, 8), {**_PIX, "H = 1": (1, 1, 2, 8), "W = 1": (1, 2, 1, 8)}, False),
    "nk_maxpool2x2_fwd": (2, (1, 2, 2, 8), {**_PIX, "odd H": (1, 3, 2, 8), "odd W": (1, 2, 3, 8)}, False),
    "nk_maxpool2x2_bwd": (3, (1, 2, 2, 8), {**_PIX, "odd H": (1, 3, 2, 8), "odd W": (1, 2, 3, 8)}, False),
    "nk_maxpool_fwd": (2, (1, 3, 3, 8, 3, 2), {"C % 8 != 0": (1, 3, 3, 12, 3, 2), "H < k": (1, 2, 3, 8, 3, 2), "s = 0": (1, 3, 3, 8, 3, 0)}, False),
    "nk_maxpool_bwd": (3, (1, 3, 3, 8, 3, 2), {"C % 8 != 0": (1, 3, 3, 12, 3, 2), "W < k": (1, 3, 2, 8, 3, 2), "k = 0": (1, 3, 3, 8, 0, 2)}, False),
}
NK_OK, NK_ERR_ARG = 0, 1


def test_argument_refusals(ops):
    """A refused call returns before any launch.  The accepted rows do launch: the good call, and a first pointer off by 2 bytes where the
    entry point has no alignment condition.  Those rows make unaligned 16-byte vector accesses on purpose, because the hand-written entry
    points accepted such a pointer and this table holds every row to what they returned.  Every accepted row runs its tiny shape inside a
    zeroed arena with 4 KiB per pointer."""
    arena = torch.zeros(16 * 4096, dtype=torch.uint8, device="cuda")
    base = arena.data_ptr()
    assert base % 16 == 0
    st = ops._stream()
    seen = []
    for name, (nptr, good, bad, refuses_misaligned) in REFUSALS.items():
        ptrs = [base + 4096 * j for j in range(nptr)]
        rc = lambda p, tail: ops.query(name, *p, *tail, st)
        assert rc(ptrs, good) == NK_OK, name
        for what, tail in bad.items():
            assert rc(ptrs, tail) == NK_ERR_ARG, (name, what)
        for j in range(nptr):
            nulled = ptrs[:j] + [None] + ptrs[j + 1:]
            one_side = name == "nk_split_channels" and j > 0          # either destination of the split may be null, not both
            assert rc(nulled, good) == (NK_OK if one_side else NK_ERR_ARG), (name, f"null pointer {j}")
            if refuses_misaligned:
                assert rc(ptrs[:j] + [ptrs[j] + 2] + ptrs[j + 1:], good) == NK_ERR_ARG, (name, f"misaligned pointer {j}")
        if not refuses_misaligned:
            assert rc([ptrs[0] + 2] + ptrs[1:], good) == NK_OK, (name, "misaligned pointer 0")
        seen.append(name)
    assert ops.query("nk_split_channels", base, None, None, 1, 8, 8, st) == NK_ERR_ARG
    # BatchNorm (the apply and dx passes sit behind these): x gamma beta y mean rstd running_mean running_var ws | dy x y gamma mean rstd dx dgamma dbeta ws
    p = [base + 4096 * j for j in range(10)]
    fwd = lambda q, M=8, C=8, slope=0.2: ops.query("nk_batchnorm_fwd", *q[:6], None, None, q[8], M, C, 1e-5, 0.1, slope, st)
    bwd = lambda q, M=8, C=8, slope=0.2: ops.query("nk_batchnorm_bwd", *q, M, C, slope, 0, st)
    assert fwd(p) == NK_OK and bwd(p) == NK_OK
    assert fwd(p, C=12) == fwd(p, M=0) == fwd(p, slope=0.0) == NK_ERR_ARG and bwd(p, C=12) == bwd(p, M=0) == bwd(p, slope=0.0) == NK_ERR_ARG
    for j in range(10):
        nulled = p[:j] + [None] + p[j + 1:]
        assert bwd(nulled) == NK_ERR_ARG and (j in (6, 7, 9) or fwd(nulled) == NK_ERR_ARG), f"batchnorm null pointer {j}"
    assert ops.query("nk_batchnorm_fwd", *p[:7], None, p[8], 8, 8, 1e-5, 0.1, 0.2, st) == NK_ERR_ARG      # one running statistic without the other
    torch.cuda.synchronize()
    assert len(seen) == len(REFUSALS)
