"""What tests/test_gemm_exact_gpu.py relies on, checked without a GPU: the exactness condition of every row of the case table, that the
integer references exercise the bf16 store's rounding, that the checkers catch each of a list of planted kernel faults (and which of those
faults the tolerance tests let through), and that the table names every launch site of the tile engine."""
import re

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_exact as G
from tests.util import assert_close

TOL_BF16, TOL_F32 = 2e-2, 1e-2       # today's limits of test_kernels_gpu.py / test_gemm_g2_gpu.py / test_conv_*_gpu.py


# ---- the table --------------------------------------------------------------------------------------------------------------------------------
def test_table_names_every_launch_literal_of_the_engine():
    literals = G.launch_literals()
    assert len(literals) >= 20 and "nk_gemm_dma_kernel" in literals and "nk_conv3x3_halo_kernel<128,4,stats=1>" in literals
    missing = set(literals) - {c.expect for c in G.CASES}
    assert not missing, f"launch sites without a case in tests/gemm_exact.py: {sorted(missing)}"
    assert set(literals) <= set(G.TILES), "every launch name needs its tile shape in gemm_exact.TILES"


def test_table_environment_and_guards():
    src = "".join((G.CSRC / f).read_text() for f in G.ENGINE_SOURCES)
    switches = set(re.findall(r'getenv\("(NK_[A-Z0-9_]+)"\)', src))
    for c in G.CASES:
        for k, v in c.env:
            assert k in switches, f"{c.id}: {k} is not read by the engine"
            assert k != "NK_GEMM_XL", "read once per process: reach the kernels behind it by shape"
        assert c.guard == "cols" or c.why_rows, c.id
        if c.guard == "cols":
            assert c.op not in ("conv_fwd", "conv_dgrad", "conv_wgrad")


def test_every_required_path_has_a_real_size_and_a_ragged_case():
    by = {}
    for c in G.CASES:
        if G.op_is_rows_by_k(c) or c.op in ("wgrad", "wgrad_batched"):
            by.setdefault((c.op.replace("_batched", "").replace("_geglu_s", "").replace("_geglu", ""), c.expect.split("<")[0]), set()).add(G.ragged(c))
    for key, kinds in sorted(by.items()):
        assert kinds == {True, False}, f"{key}: needs a real-size and a ragged case, has ragged={sorted(kinds)}"
    # ragged means: a reduction that is a multiple of 8 but not of 64, and once an N that is not a multiple of 8 (the scalar store path)
    assert any(c.op == "fwd" and c.dims[1] % 8 for c in G.CASES)
    assert all(c.dims[2] % 8 == 0 for c in G.CASES if G.op_is_rows_by_k(c))


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_exactness_condition(case):
    """T r_a r_b |alpha| (both passes of a store-then-accumulate check counted) + every epilogue addend < 2^24, from the generators' ranges."""
    t = G.terms(case)
    assert t["ra"] == case.r and all(a <= G.ADD_RANGE for a in t["add"])
    alpha = case.o("alpha", 1.0)
    assert alpha == 1.0 or (abs(alpha) == 2.0 ** round(torch.log2(torch.tensor(abs(alpha))).item())), "alpha is 1 or a power of two"
    assert G.exact_magnitude(case) < G.EXACT_LIMIT, (case.id, G.exact_magnitude(case))
    if case.r == 8:
        assert t["T"] <= 65536
    small = all(d <= 4096 for d in case.dims) and case.op not in ("conv_fwd", "conv_dgrad", "conv_wgrad")
    if small:      # the generators keep to the ranges the condition was computed from
        for k, v in G.make_inputs(case).items():
            for x in (v if isinstance(v, list) else [v]):
                lim = G.ADD_RANGE if k in ("bias", "residual", "add", "rowvec") else case.r
                assert float(x.abs().max()) <= lim and torch.equal(x, x.round()) and torch.equal(x, x.to(torch.bfloat16).float()), (case.id, k)


@pytest.mark.parametrize("cid", ["fwd-g2p160-1280", "wgrad-splitk-ring-320x320", "conv-halo160x4-ragged"])
def test_fp32_product_of_the_generated_operands_is_exact(cid):
    """The claim the GPU test stands on, on the CPU: in fp32, whatever order the BLAS sums in, the result equals float64 bit for bit."""
    c = G.BY_ID[cid]
    inp = G.make_inputs(c)
    ref = G.reference(c, inp)["y"]
    if c.op == "fwd":
        got = inp["x"] @ inp["w"].t() + inp["bias"] + inp["residual"]
    elif c.op == "wgrad":
        got = inp["dy"].t() @ inp["x"]
    else:
        N, H, W, Cin, Cout, k, stride, pad = c.dims
        got = F.conv2d(inp["x"].permute(0, 3, 1, 2), inp["w"].permute(0, 3, 1, 2), inp["bias"], stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
        got = got + inp["rowvec"].repeat_interleave(H * W, 0) + inp["residual"]
    assert got.dtype == torch.float32 and torch.equal(got.double(), ref)


# ---- rounding coverage ------------------------------------------------------------------------------------------------------------------------
def _sample(c: G.Case):
    """The case cut down to at most 512 output rows / one image (same operand distribution, same reduction length): enough to count roundings."""
    if G.op_is_rows_by_k(c):
        return G.Case(c.id, c.op, (min(c.dims[0], 512),) + c.dims[1:], c.expect, c.env, c.opts, c.r, c.guard, c.why_rows)
    return G.Case(c.id, c.op, (1,) + c.dims[1:], c.expect, c.env, c.opts, c.r, c.guard, c.why_rows)


BF16_CASES = [c for c in G.CASES if G.op_is_rows_by_k(c) or c.op in ("conv_fwd", "conv_dgrad")]


@pytest.mark.parametrize("case", BF16_CASES, ids=[c.id for c in BF16_CASES])
def test_reference_exercises_the_bf16_rounding(case):
    """At least 5 % of the exact outputs are not bf16 numbers (the store must round them) and at least 1 % are exact ties (round-to-nearest-EVEN
    is told from round-half-up / truncation there).  From the reference alone.  A row that falls short gets a larger r or a longer K, never a
    lower floor."""
    s = _sample(case)
    y = G.reference(s, G.make_inputs(s))["y"]
    y = torch.cat(y) if isinstance(y, list) else y
    low = y.float().contiguous().view(torch.int32) & 0xFFFF
    needs, ties = float((low != 0).float().mean()), float((low == 0x8000).float().mean())
    print(f"[gemm exact] {case.id}: {100 * needs:.1f} % of outputs need rounding, {100 * ties:.1f} % are exact ties")
    assert needs >= 0.05 and ties >= 0.01, (case.id, needs, ties)


# ---- planted faults ----------------------------------------------------------------------------------------------------------------------------
def _trunc_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def tiled_gemm(a, b, residual=None, fault=None, out=torch.bfloat16):
    """c[M, N] = a[M, K] b[N, K]^T (+ residual) the way a tile kernel does it: fp32 accumulation over 64-deep slabs, one rounding at the store."""
    M, K = a.shape
    slabs = [(k0, min(k0 + 64, K)) for k0 in range(0, K, 64)]
    if fault == "last reduction element dropped":
        slabs[-1] = (slabs[-1][0], slabs[-1][1] - 1)
    if fault == "one slab skipped, another doubled":
        slabs[1] = slabs[2]
    acc = torch.zeros(M, b.shape[0])
    halves = []
    for i, (k0, k1) in enumerate(slabs):
        acc = acc + a[:, k0:k1] @ b[:, k0:k1].t()
        if fault == "split partial rounded to bf16" and i in (len(slabs) // 2 - 1, len(slabs) - 1):
            halves.append(acc.to(torch.bfloat16).float())
            acc = torch.zeros_like(acc)
    if halves:
        acc = halves[0] + halves[1]
    if fault == "accumulator rounded to bf16 before the residual":
        acc = acc.to(torch.bfloat16).float()
    if residual is not None:
        acc = acc + residual
    if out == torch.float32:
        return acc
    return _trunc_bf16(acc) if fault == "truncation instead of round-to-nearest-even" else acc.to(torch.bfloat16)


def tiled_conv3x3(x, w, fault=None):
    """y[N, H, W, Cout] of a 3 x 3 / stride 1 / padding 1 convolution, tap by tap in fp32 (x NHWC, w [Cout][3][3][Cin])."""
    N, H, W, Cin = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros(N, H, W, w.shape[0])
    for kh in range(3):
        for kw in range(3):
            th, tw = kh, kw
            if fault == "two taps of the 3 x 3 weight swapped" and (kh, kw) in ((0, 1), (2, 1)):
                th = 2 - kh
            win = xp[:, kh:kh + H, kw:kw + W, :]
            if fault == "input shifted by one pixel at an image edge" and kw == 2:
                win = win.clone()
                win[:, :, W - 1, :] = xp[:, kh:kh + H, W, :]        # the last output column reads the pixel before the padding instead of the padding
            acc = acc + win @ w[:, th, tw, :].t()
    return acc.reshape(N * H * W, -1).to(torch.bfloat16)


# fault -> does tests/util.assert_close at today's tolerances let it through?  (True: the argument for this module.)
PASSES_TODAY = {
    "last reduction element dropped": True,
    "one slab skipped, another doubled": False,          # (two of 256 slabs: ~3e-2 of max |ref|, seen by the 1e-2 limit)
    "split partial rounded to bf16": True,
    "accumulator rounded to bf16 before the residual": True,
    "truncation instead of round-to-nearest-even": True,
    "two taps of the 3 x 3 weight swapped": False,
    "input shifted by one pixel at an image edge": False,
    "an 8-column chunk written one chunk past N": True,
}


@pytest.mark.parametrize("fault", list(PASSES_TODAY))
def test_planted_fault_is_caught(fault):
    """Each fault, applied in a plain torch emulation of a tiled GEMM / convolution on the table's integer inputs, is flagged by assert_exact or
    by the sentinels.  PASSES_TODAY records which of them assert_close lets through at the tolerance the existing GEMM / conv tests use: the
    dropped tail element, the bf16 split partial, the early bf16 rounding, the truncating store and the out-of-bounds chunk."""
    r = 8
    out_of_bounds = False
    if fault in ("two taps of the 3 x 3 weight swapped", "input shifted by one pixel at an image edge"):
        x, w = G.ints((2, 32, 32, 64), r, 1), G.ints((96, 3, 3, 64), r, 2)
        want64 = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), padding=1).permute(0, 2, 3, 1).reshape(-1, 96)
        good, got, tol = tiled_conv3x3(x, w), tiled_conv3x3(x, w, fault), TOL_BF16
    elif fault in ("last reduction element dropped", "one slab skipped, another doubled", "split partial rounded to bf16"):
        # a weight gradient: 16 384 tokens reduced into an fp32 [320, 328]
        a, b = G.ints((320, 16384), r, 3), G.ints((328, 16384), r, 4)
        want64 = a.double() @ b.double().t()
        good, got, tol = tiled_gemm(a, b, out=torch.float32), tiled_gemm(a, b, fault=fault, out=torch.float32), TOL_F32
    else:
        a, b, res = G.ints((1000, 1096), r, 5), G.ints((328, 1096), r, 6), G.ints((1000, 328), G.ADD_RANGE, 7)
        want64 = a.double() @ b.double().t() + res.double()
        good = tiled_gemm(a, b, res)
        got, tol = tiled_gemm(a, b, res, fault), TOL_BF16
        out_of_bounds = fault == "an 8-column chunk written one chunk past N"
    want = G.expected(want64, good.dtype)
    G.assert_exact(good, want, "emulation without the fault")            # the emulation itself is exact
    dest = G.Guarded(got.shape[0], got.shape[1], got.dtype, col_guard=True, device="cpu")
    dest.arm(G.GARBAGE)
    dest.view.copy_(got)
    if out_of_bounds:
        rows = dest.buf.view(-1, dest.ld)
        rows[G.Guarded.ROWS + 5, got.shape[1] + 8:got.shape[1] + 16] = got[5, -8:]
        G.assert_exact(dest.view, want, fault)                           # the values are right ...
        with pytest.raises(AssertionError, match="STORE OUTSIDE THE OUTPUT"):
            dest.assert_untouched(fault)                                 # ... the neighbour is not
    else:
        dest.assert_untouched(fault)
        with pytest.raises(AssertionError, match="WRONG RESULT") as e:
            G.assert_exact(dest.view, want, fault)
        print(f"[gemm exact] {fault}: {str(e.value).splitlines()[0]}")
    try:
        assert_close(dest.view, want64.float(), tol, fault)
        passes = True
    except AssertionError:
        passes = False
    print(f"[gemm exact] {fault}: assert_close at {tol:g} {'PASSES (the fault goes unseen today)' if passes else 'fails'}")
    assert passes == PASSES_TODAY[fault], (fault, passes)


# ---- the hooks -------------------------------------------------------------------------------------------------------------------------------
def test_launch_log_hooks_are_host_only():
    """On, empty, plan-only, off -- without a device: the hooks touch no GPU state (which is what lets them run during graph capture)."""
    from neurosis_amd import lib

    lib.launch_log(1)
    assert lib.launched() == []
    lib.launch_log(2)
    lib.launch_log(3)
    assert lib.launched() == []
    lib.launch_log(0)
    with pytest.raises(lib.NkError):
        lib.launch_log(4)
