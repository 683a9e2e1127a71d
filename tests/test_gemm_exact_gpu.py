"""Every GEMM and convolution kernel path of the tile engine, bit for bit against float64 on integer inputs (tests/gemm_exact.py has the why,
the helpers and the case table).  Each case first asserts that the library launched the kernel the case means (lib.launched()), then compares
the bits, then the sentinels around the destination.  No tolerance anywhere in the exact tests.

Two value tests on non-integer inputs follow, because integers cannot see range or scaling errors: a scale-and-cancellation test against the
first-order bound of an arbitrary summation tree (gemm_exact.error_bound: derived, not measured; the observed error / bound ratios are printed
and recorded in DESIGN.md), and planted Inf / NaN operands.

Outside this module: the GEGLU-forward and erf-form GEGLU-backward epilogues (not exact: GELU; tolerance tests in test_kernels_gpu.py), the
statistics epilogue's partial sums (fp32 sums of squares; test_fullsize_values_gpu.py), the few-row weight gradient of elementwise.hip."""
import time

import pytest
import torch

from tests import gemm_exact as G

pytestmark = pytest.mark.gpu

REACHED = set()          # launch names seen by the cases of this module (the coverage test at the end reads it)
T0 = time.time()


def _run_logged(run, mode=1):
    """mode 1: launch and log; mode 3: plan-only -- the tile engine logs what it would launch and touches nothing."""
    from neurosis_amd import lib

    lib.launch_log(mode)
    try:
        run.launch()
        names = lib.launched()
    finally:
        lib.launch_log(0)
    REACHED.update(names)
    return names


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_exact(case):
    inp = G.make_inputs(case)
    assert G.exact_magnitude(case) < G.EXACT_LIMIT
    ref = G.reference(case, inp)
    with G.environment(case.env):
        stream = torch.cuda.Stream() if case.graph else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            run = G.Run(case, inp)
            run.arm()
            planned = _run_logged(run, mode=3)
            names = _run_logged(run)
            assert planned == names, f"{case.id}: the plan taken before the launch is not what was launched: planned {planned}, launched {names}"
            stream.synchronize()
            G.check_run(run, ref, names)
            if case.o("splits"):
                S = G.wgrad_halo_splits(case)
                assert (S == 1) == (case.o("splits") == "one"), f"{case.id}: THE DISPATCH MOVED: the cost rule now gives {S} pixel splits; the case means {case.o('splits')}"
            if case.graph:
                # captured and replayed: the zero-fill of a split destination must stay ordered before the atomics (gemm.hip, zero_split_outputs),
                # and the launch log -- host-only -- must work while the stream captures
                run.arm()
                stream.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=stream):
                    captured = _run_logged(run)
                assert case.expect in captured, f"{case.id}: the launch log reported {captured} during capture"
                for _ in range(2):
                    run.arm()
                    g.replay()
                    torch.cuda.synchronize()
                    G.check_run(run, ref, captured, " (graph replay)")


# ---- scale and cancellation ----------------------------------------------------------------------------------------------------------------------
# one shape per kernel family; inputs are bf16-rounded normals times the scale, the first operand offset by 4 sigma: its products with the
# zero-mean second operand are large and of either sign, so sum a b << sum |a||b| and a lost or mis-scaled partial is visible in the error
VALUE_CASES = ["fwd-ring64-ragged-scalar-stores", "fwd-g2p160-1280", "fwd-xl2g-ragged", "fwd-sk-ragged",
               "fwd-ring-ragged-alpha", "fwd-dma-ragged-scalar-stores", "dgrad-g2p128-ragged", "dgrad-sk-ragged", "wgrad-w160-forced-ragged-split3",
               "wgrad-w128-split-by-shape-4096x1280x2048", "wgrad-sk-1280", "wgrad-splitk-ring-320x320", "wgrad-dma-unsplit",
               "conv-halo160x4-ragged", "conv-halo128x4-ragged", "conv-g2p128-gather-ragged", "conv-xl-gather-ragged-stride2",
               "conv-ring-4x4-taps-stride2", "cdgrad-flipped-halo128x4-ragged", "cdgrad-g2p160-stride2", "cdgrad-ring-ragged",
               "cwgrad-halo-forced-ragged", "cwgrad-gather-splitk-atomics", "cwgrad-gather-unsplit-ragged"]
RATIOS = {}


def _normal_inputs(case, scale, seed):
    """bf16-exact normals of the integer inputs' shapes; the first operand carries the 4 sigma offset; addends are plain normals of the scale^2
    of a product."""
    g = torch.Generator().manual_seed(seed)
    first = {"fwd": "x", "dgrad": "dy", "wgrad": "dy", "conv_fwd": "x", "conv_dgrad": "dy", "conv_wgrad": "dy"}[case.op]
    out = {}
    for k, v in G.make_inputs(case).items():
        t = torch.randn(v.shape, generator=g)
        if k == first:
            t = t + 4.0
        t = t * (scale if k in ("x", "w", "dy") else scale * scale)
        out[k] = t if k == "bias" else t.to(torch.bfloat16).float()
        if k == "x" and case.o("cin_real"):
            out[k][..., case.o("cin_real"):] = 0
    return out


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
@pytest.mark.parametrize("cid", VALUE_CASES)
def test_scale_and_cancellation(cid, scale):
    base = G.BY_ID[cid]
    case = G.Case(base.id, base.op, base.dims, base.expect, base.env, tuple(kv for kv in base.opts if kv[0] != "accumulate"), base.r, base.guard,
                  base.why_rows)
    inp = _normal_inputs(case, scale, seed=len(cid))
    ref, mag = G.reference(case, inp), G.reference(case, inp, magnitude=True)
    with G.environment(case.env):
        run = G.Run(case, inp)
        run.arm()
        names = _run_logged(run)
        torch.cuda.synchronize()
    assert case.expect in names, f"{cid}: THE DISPATCH MOVED: expected {case.expect}, the library reports {names}; the case needs a new shape"
    got = run.y[0].view.double().cpu()
    run.y[0].assert_untouched(cid)
    bound = G.error_bound(case, ref, mag, bf16_out=run.y[0].view.dtype == torch.bfloat16)
    assert torch.isfinite(got).all(), f"{cid}: non-finite output at scale {scale}"
    ratio = float(((got - ref["y"]).abs() / bound).max())
    cancel = float((ref["y"] - ref["addends"]).abs().median() / (mag["y"] - mag["addends"]).median())
    RATIOS[(case.expect, scale)] = max(RATIOS.get((case.expect, scale), 0.0), ratio)
    print(f"[gemm exact] scale/cancellation {cid} [{case.expect}] scale {scale:g}: max error / bound {ratio:.4f}; median |sum ab| / sum |a||b| {cancel:.3f}")
    assert ratio <= 1.0, f"{cid} [{case.expect}] scale {scale:g}: error exceeds the derived bound by x{ratio:.3f}"


# ---- non-finite operands ---------------------------------------------------------------------------------------------------------------------------
NONFINITE_CASES = ["fwd-ring64-ragged-scalar-stores", "fwd-g2p160-ragged", "fwd-g2p128-ragged", "fwd-xl2g-ragged", "fwd-sk-ragged", "fwd-ring-ragged-alpha",
                   "fwd-dma-ragged-scalar-stores", "fwd-ring64-context-kv", "dgrad-g2p128-ragged", "dgrad-ring-ragged", "dgrad-dma-ragged",
                   "wgrad-w160-forced-ragged", "wgrad-w128-forced-ragged", "wgrad-ring-unsplit-ragged", "wgrad-splitk-ring-320x320",
                   "conv-halo160x4-ragged", "conv-halo128x4-ragged", "conv-ring-ragged", "conv-g2p160-gather-stride2", "cdgrad-flipped-halo128x4-ragged",
                   "cdgrad-ring-ragged", "cdgrad-g2p160-stride2", "cwgrad-halo-forced-ragged", "cwgrad-gather-unsplit-ragged"]


@pytest.mark.parametrize("cid", NONFINITE_CASES)
def test_planted_inf_and_nan_land_where_the_reference_says(cid):
    """An Inf and a NaN planted in one element each of the first operand: the output is non-finite in exactly the rows / columns / pixels the
    float64 reference is, Inf with the reference's sign, and finite everywhere else."""
    base = G.BY_ID[cid]
    case = G.Case(base.id, base.op, base.dims, base.expect, base.env, tuple(kv for kv in base.opts if kv[0] != "accumulate"), base.r, base.guard,
                  base.why_rows)
    inp = _normal_inputs(case, 1.0, seed=7 + len(cid))
    first = {"fwd": "x", "dgrad": "dy", "wgrad": "dy", "conv_fwd": "x", "conv_dgrad": "dy", "conv_wgrad": "dy"}[case.op]
    a = inp[first]
    flat = a.view(-1, a.shape[-1])
    r_inf, r_nan = flat.shape[0] // 3, flat.shape[0] - 2
    if case.op == "conv_wgrad":
        # interior pixels: at an image edge the planted dy meets the zero padding of x, and whether 0 x Inf is formed (NaN) or the tap is skipped
        # is the kernel's choice, not an error
        _, _, Ho, Wo = G.conv_geometry(case)
        r_inf, r_nan = (Ho // 2) * Wo + Wo // 2, ((case.dims[0] - 1) * Ho + Ho // 2 + 1) * Wo + Wo // 2 - 1
    flat[r_inf, 1] = float("inf")
    flat[r_nan, a.shape[-1] - 3] = float("nan")
    ref = G.reference(case, inp)["y"]
    with G.environment(case.env):
        run = G.Run(case, inp)
        run.arm()
        names = _run_logged(run)
        torch.cuda.synchronize()
    assert case.expect in names, f"{cid}: THE DISPATCH MOVED: expected {case.expect}, the library reports {names}; the case needs a new shape"
    got = run.y[0].view.double().cpu()
    run.y[0].assert_untouched(cid)
    assert 0 < int(ref.isnan().sum()) < ref.numel() and int(ref.isinf().sum()) > 0, "the planted values must reach some outputs and not all"
    for name, gm, rm in [("NaN", got.isnan(), ref.isnan()), ("+Inf", got == float("inf"), ref == float("inf")), ("-Inf", got == float("-inf"), ref == float("-inf"))]:
        bad = (gm != rm).nonzero()
        assert len(bad) == 0, f"{cid} [{case.expect}]: {name} in {int(gm.sum())} outputs, the reference has {int(rm.sum())}; first differing (row, column): {bad[:6].tolist()}"


# ---- coverage (keep last) ------------------------------------------------------------------------------------------------------------------------
def test_every_launch_site_of_the_tile_engine_was_reached():
    """The union of the names logged by the cases above covers every kernel name the planner (gemm_plan.h) can report: a new kernel
    (or instantiation name) without a case fails here."""
    wanted = set(G.launch_literals())
    print(f"[gemm exact] reached: {sorted(REACHED & wanted)}")
    print(f"[gemm exact] worst error / bound per kernel and scale: { {f'{k[0]} @ {k[1]:g}': round(v, 4) for k, v in sorted(RATIOS.items())} }")
    print(f"[gemm exact] module wall time so far: {time.time() - T0:.0f} s")
    assert wanted <= REACHED, f"launch sites never reached by a case: {sorted(wanted - REACHED)}"
