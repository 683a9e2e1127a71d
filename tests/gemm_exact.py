"""Bit-for-bit checks of the MFMA tile engine (csrc/gemm.hip, gemm_plan.h, gemm_g2.h, gemm_w160.h, conv_halo.h, conv_wgrad_halo.h) on integer inputs.

Why exact.  Operands are small integers (exact in bf16), so every product and every partial sum of a GEMM / convolution is an integer below
2^24 and therefore exact in fp32: the result does not depend on the order of summation at all -- not on the k rotation per XCD, the split-K
atomics, the stream-K fix-ups, the 160-row kernel's token splits, nor on how the MFMA's internal adder rounds.  An fp32 output must equal the
float64 reference bit for bit, a bf16 output its one round-to-nearest-even rounding.  One dropped, doubled or misplaced element changes an
integer and fails.

What is here: the integer generators and their exactness condition, the float64 references, guarded destinations (sentinels around the
output), `assert_exact`, the launch-literal scanner, and THE CASE TABLE: entry point, shape, epilogue options, environment and the kernel name
the library must report for it (lib.launched(), fed by nk_check_launch).  tests/test_gemm_exact_cpu.py checks the table and the checkers
without a GPU; tests/test_gemm_exact_gpu.py runs it.

The only numeric constants: 2^24 (fp32 integers), the +-256 range of epilogue addends, the 5 % / 1 % rounding-coverage floors of the CPU
test, and SAFETY = 1.25 with the 2^-23 unit in the one derived bound (`error_bound`).  None is tuned against a kernel's output."""
from __future__ import annotations

import ctypes as C
import os
import re
from contextlib import contextmanager
from dataclasses import dataclass
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "neurosis_amd" / "csrc"
ENGINE_SOURCES = ("gemm.hip", "gemm_plan.h", "gemm_g2.h", "gemm_w160.h", "conv_halo.h", "conv_wgrad_halo.h")
EXACT_LIMIT = 2 ** 24       # integers of smaller magnitude are exact in fp32, and so are their sums while they stay below it
ADD_RANGE = 256             # biases, row vectors, residuals, pre-filled destinations: uniform integers in [-256, 256] (exact in bf16)
SENTINEL = 2.0 ** 100       # exact in bf16 and fp32; no exact result (|.| < 2^24) can equal it
GARBAGE = 12345.0           # what an overwritten destination holds before the launch (a store that adds instead shows up)
SAFETY = 1.25               # as tests/attention_bounds.py
U32 = 2.0 ** -23            # unit of the derived bound: whether the bf16 MFMA's accumulator rounds or truncates is not established


# ---- what the library can launch -----------------------------------------------------------------------------------------------------------
def launch_literals() -> list[str]:
    """Every kernel name a launch of the tile engine reports: the launchers pass the plan's name to nk_check_launch, and the planner
    (gemm_plan.h) is where the names are written -- its kernel-name string literals, plus any literal still inside a nk_check_launch(...)."""
    names = re.findall(r'"(nk_\w+_kernel(?:<[^">]*>)?)"', (CSRC / "gemm_plan.h").read_text())
    for f in ENGINE_SOURCES:
        for call in re.findall(r"nk_check_launch\((.*?)\);", (CSRC / f).read_text(), flags=re.S):
            names += re.findall(r'"([^"]+)"', call)
    return sorted(set(names))


# tile (rows, columns) of the OUTPUT per logged kernel: assert_exact reports the tile a wrong element lies in
TILES = {
    "nk_gemm_ring64_kernel": (64, 64), "nk_gemm_xl_kernel": (256, 256), "nk_gemm_xl2g_kernel<geglu=0>": (256, 256),
    "nk_gemm_xl2g_kernel<geglu=1>": (256, 256), "nk_gemm_ring_kernel": (128, 128), "nk_gemm_dma_kernel": (128, 128),
    "nk_gemm_sk_kernel": (128, 128), "nk_gemm_g2p_kernel<160>": (128, 160), "nk_gemm_g2p_kernel<128>": (128, 128),
    "nk_gemm_w160_kernel<160>": (160, 160),
    "nk_gemm_w160_kernel<128>": (160, 128),
    # halo tiles are patches of 8 / 4 image rows x 32 pixels: in the [pixels][channels] output only the column tile is a contiguous range
    "nk_conv3x3_halo_kernel<160,8,stats=0>": (256, 160), "nk_conv3x3_halo_kernel<160,8,stats=1>": (256, 160),
    "nk_conv3x3_halo_kernel<160,4,stats=0>": (128, 160), "nk_conv3x3_halo_kernel<160,4,stats=1>": (128, 160),
    "nk_conv3x3_halo_kernel<128,8,stats=0>": (256, 128), "nk_conv3x3_halo_kernel<128,8,stats=1>": (256, 128),
    "nk_conv3x3_halo_kernel<128,4,stats=0>": (128, 128), "nk_conv3x3_halo_kernel<128,4,stats=1>": (128, 128),
    # (output channels) x (64 input channels of one tap; a block covers the nine taps of its 64 channels)
    "nk_conv3x3_wgrad_halo_kernel<bias=0>": (128, 64), "nk_conv3x3_wgrad_halo_kernel<bias=1>": (128, 64),
    "colsum_partial": (1, 128),
}


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    op: str                 # fwd | fwd_geglu | fwd_batched | dgrad | dgrad_geglu_s | wgrad | wgrad_batched | colsum | conv_fwd | conv_dgrad | conv_wgrad
    dims: tuple             # Linear: (M, N, K) as the docstring of each op below reads them; conv: (N, H, W, Cin, Cout, k, stride, pad)
    expect: str             # the launch name lib.launched() must contain
    env: tuple = ()         # ((name, value), ...) set around the launch
    opts: tuple = ()        # ((name, value), ...): epilogue and layout options, see `o()`
    r: int = 8              # operands are uniform integers in [-r, r]
    guard: str = "cols"     # "cols": extra columns (ld > N) and rows ahead / behind; "rows": rows ahead / behind only (why: `why_rows`)
    why_rows: str = ""
    graph: bool = False     # also run under a captured and replayed graph

    def o(self, name, default=None):
        return dict(self.opts).get(name, default)


def _c(id, op, dims, expect, env="", r=8, guard="cols", why_rows="", graph=False, **opts):
    envt = tuple(tuple(kv.split("=")) for kv in env.split()) if env else ()
    if guard == "rows":
        assert why_rows, id
    return Case(id, op, tuple(dims), expect, envt, tuple(sorted(opts.items())), r, guard, why_rows, graph)


CONV_LD = "the convolution entry points fix ldc to the channel count"
SPLIT_LD = "split partials meet through atomics on a destination the launcher zeroes: it insists on ldc == N"
G2P160, G2P128 = "nk_gemm_g2p_kernel<160>", "nk_gemm_g2p_kernel<128>"
XL2G, XL, SK, RING, DMA, R64 = "nk_gemm_xl2g_kernel<geglu=0>", "nk_gemm_xl_kernel", "nk_gemm_sk_kernel", "nk_gemm_ring_kernel", "nk_gemm_dma_kernel", "nk_gemm_ring64_kernel"
W160, W128 = "nk_gemm_w160_kernel<160>", "nk_gemm_w160_kernel<128>"
WH0, WH1 = "nk_conv3x3_wgrad_halo_kernel<bias=0>", "nk_conv3x3_wgrad_halo_kernel<bias=1>"


def HALO(bn, rows, stats=0):
    return f"nk_conv3x3_halo_kernel<{bn},{rows},stats={stats}>"


def _table():
    t = []
    # ---- Linear forward: y[M, N] = alpha x[M, K] w[N, K]^T + bias + residual ------------------------------------------------------------
    t += [
        _c("fwd-ring64-context-kv", "fwd", (308, 1280, 2048), R64, bias=1),
        _c("fwd-ring64-ragged-scalar-stores", "fwd", (300, 331, 264), R64, bias=1, residual=1),                 # N % 8 != 0
        _c("fwd-g2p160-1280", "fwd", (4096, 1280, 1280), G2P160, bias=1, residual=1, graph=True),
        _c("fwd-g2p160-1280-krot0", "fwd", (4096, 1280, 1280), G2P160, env="NK_GEMM_KROT=0", bias=1, residual=1),
        _c("fwd-g2p160-ff-out-16384x640x5120", "fwd", (16384, 640, 5120), G2P160, bias=1, residual=1),
        _c("fwd-g2p160-ragged", "fwd", (1000, 160, 136), G2P160, env="NK_GEMM_G2=2", bias=1, ldx_pad=24),
        _c("fwd-g2p128-vae-attn-512", "fwd", (16384, 512, 512), G2P128, bias=1, residual=1),
        _c("fwd-g2p128-ragged", "fwd", (4000, 1000, 328), G2P128, env="NK_GEMM_G2=2", residual=1),
        _c("fwd-g2p128-ragged-scalar-stores", "fwd", (520, 1001, 200), G2P128, env="NK_GEMM_G2=2", bias=1, residual=1),
        _c("fwd-xl2g-ff-proj-4096x10240x1280", "fwd", (4096, 10240, 1280), XL2G, bias=1),
        _c("fwd-xl2g-krot0", "fwd", (4096, 10240, 1280), XL2G, env="NK_GEMM_KROT=0", bias=1),
        # the FeedForward projection with the GEGLU in its epilogue: u = x w^T + bias is exact and checked here; h = a gelu(g) is not (GELU) and
        # keeps its tolerance test (test_kernels_gpu.py), its destination is guarded here all the same.  dims = (M, I, K), u is [M, 2I]
        _c("fwd-xl2g-geglu-ff-proj-u-only", "fwd_geglu", (4096, 5120, 1280), "nk_gemm_xl2g_kernel<geglu=1>", bias=1),
        _c("fwd-xl2g-ragged", "fwd", (4000, 3832, 328), XL2G, bias=1, residual=1),
        _c("fwd-sk-4096x640x2560", "fwd", (4096, 640, 2560), SK, bias=1, residual=1, graph=True),
        _c("fwd-sk-ragged", "fwd", (1000, 328, 200), SK, env="NK_GEMM_SK=1", bias=1, residual=1),
        _c("fwd-ring-4096x640x640", "fwd", (4096, 640, 640), RING, bias=1, residual=1),
        _c("fwd-ring-ragged-alpha", "fwd", (1000, 328, 200), RING, env="NK_GEMM_SK=0", bias=1, alpha=0.125, ldx_pad=8),
        _c("fwd-ring-ragged-scalar-stores", "fwd", (1000, 333, 200), RING, env="NK_GEMM_SK=0", bias=1, residual=1),
        _c("fwd-dma-16384x1280x640", "fwd", (16384, 1280, 640), DMA, bias=1, residual=1),
        _c("fwd-dma-krot0", "fwd", (16384, 1280, 640), DMA, env="NK_GEMM_KROT=0", bias=1),
        _c("fwd-dma-ragged-scalar-stores", "fwd", (4200, 1001, 200), DMA, env="NK_GEMM_G2=0 NK_GEMM_SK=0", bias=1, residual=1, alpha=2.0),
        # eight bias-free projections of one shape in one launch (the context keys / values)
        _c("fwd-batched-context-kv", "fwd_batched", (308, 1280, 2048), SK, batch=8),
        _c("fwd-batched-ragged-dma", "fwd_batched", (300, 328, 200), DMA, env="NK_GEMM_SK=0", batch=3),
    ]
    # ---- Linear dgrad: dx[M, N] = dy[M, K] w[K, N] + dx_add ------------------------------------------------------------------------------
    t += [
        _c("dgrad-g2p160-1280", "dgrad", (4096, 1280, 1280), G2P160, add=1, graph=True),
        _c("dgrad-g2p160-krot0", "dgrad", (4096, 1280, 1280), G2P160, env="NK_GEMM_KROT=0", add=1),
        _c("dgrad-g2p128-ragged", "dgrad", (4000, 1000, 328), G2P128, env="NK_GEMM_G2=2", add=1),
        _c("dgrad-sk-4096x640x2560", "dgrad", (4096, 640, 2560), SK, add=1),
        _c("dgrad-sk-ragged", "dgrad", (1000, 328, 200), SK, env="NK_GEMM_SK=1", add=1),
        _c("dgrad-ring-4096x640x640", "dgrad", (4096, 640, 640), RING, add=1),
        _c("dgrad-ring-ragged", "dgrad", (1000, 328, 200), RING, env="NK_GEMM_SK=0", add=1),
        _c("dgrad-dma-16384x1280x640", "dgrad", (16384, 1280, 640), DMA, add=1),
        _c("dgrad-dma-ragged", "dgrad", (4200, 1000, 200), DMA, env="NK_GEMM_G2=0 NK_GEMM_SK=0"),
        # du[M, 2N] = [d s1 | d s2], d = dy[M, K] w[K, N]: two products per element, exact for integer s
        _c("dgrad-geglu-s-dma-ff-out-4096", "dgrad_geglu_s", (4096, 5120, 1280), DMA),
        _c("dgrad-geglu-s-ring-ragged", "dgrad_geglu_s", (1000, 328, 200), RING),
    ]
    # ---- Linear wgrad: dw[N, K] (+)= dy[M, N]^T x[M, K], dbias[N] (+)= column sums of dy; the reduction runs over the M tokens -----------
    t += [
        _c("wgrad-w160-ff-proj-4096x10240x1280", "wgrad", (4096, 10240, 1280), W160, accumulate=0, dbias=1),
        _c("wgrad-w160-krot0", "wgrad", (4096, 10240, 1280), W160, env="NK_GEMM_KROT=0", accumulate=2),
        _c("wgrad-w160-split-by-shape-16384x5120x640", "wgrad", (16384, 5120, 640), W160, guard="rows", why_rows=SPLIT_LD, accumulate=0, dbias=1,
           graph=True),
        _c("wgrad-w160-split-by-shape-accumulate", "wgrad", (16384, 5120, 640), W160, guard="rows", why_rows=SPLIT_LD, accumulate=1, dbias=1),
        _c("wgrad-w128-split-by-shape-4096x1280x2048", "wgrad", (4096, 1280, 2048), W128, guard="rows", why_rows=SPLIT_LD, accumulate=0),
        _c("wgrad-w160-forced-ragged", "wgrad", (1000, 200, 136), W160, env="NK_GEMM_W160=2", accumulate=0, dbias=1),
        _c("wgrad-w160-forced-ragged-accumulate", "wgrad", (1000, 200, 136), W160, env="NK_GEMM_W160=2", accumulate=1, dbias=1),
        _c("wgrad-w160-forced-ragged-split3", "wgrad", (1000, 200, 136), W160, env="NK_GEMM_W160=2 NK_GEMM_W160_SPLIT=3", guard="rows",
           why_rows=SPLIT_LD, accumulate=0, dbias=1),
        _c("wgrad-w160-forced-ragged-split3-known-zero", "wgrad", (1000, 200, 136), W160, env="NK_GEMM_W160=2 NK_GEMM_W160_SPLIT=3", guard="rows",
           why_rows=SPLIT_LD, accumulate=2),
        _c("wgrad-w128-forced-ragged", "wgrad", (1000, 200, 1024), W128, env="NK_GEMM_W160=2", accumulate=0, dbias=1),
        _c("wgrad-w128-forced-ragged-split2", "wgrad", (1000, 200, 1024), W128, env="NK_GEMM_W160=2 NK_GEMM_W160_SPLIT=2", guard="rows",
           why_rows=SPLIT_LD, accumulate=1),
        # three 1280 x 1280 weight gradients in one launch
        _c("wgrad-batched-g2p160-three-1280", "wgrad_batched", (4096, 1280, 1280), G2P160, env="NK_GEMM_W160=0", batch=3, accumulate=0, dbias=1),
        _c("wgrad-batched-g2p160-krot0-accumulate", "wgrad_batched", (4096, 1280, 1280), G2P160, env="NK_GEMM_W160=0 NK_GEMM_KROT=0", batch=3,
           accumulate=1),
        _c("wgrad-batched-g2p160-ragged", "wgrad_batched", (1000, 200, 160), G2P160, env="NK_GEMM_W160=0 NK_GEMM_G2=2", batch=3, accumulate=0, dbias=1),
        _c("wgrad-batched-g2p128-ragged-accumulate", "wgrad_batched", (1000, 200, 1000), G2P128, env="NK_GEMM_W160=0 NK_GEMM_G2=2", batch=2,
           accumulate=1, dbias=1),
        _c("wgrad-batched-w128-three-1280", "wgrad_batched", (4096, 1280, 1280), W128, batch=3, accumulate=0, dbias=1),
        _c("wgrad-sk-1280", "wgrad", (4096, 1280, 1280), SK, env="NK_GEMM_SK=2 NK_GEMM_W160=0", accumulate=0),
        _c("wgrad-sk-ragged-accumulate", "wgrad", (1000, 200, 136), SK, env="NK_GEMM_SK=2 NK_GEMM_W160=0", accumulate=1),
        # tiny outputs: split-K partials through atomics (8 splits on the ring kernel, 4 on the double-buffer one)
        _c("wgrad-splitk-ring-320x320", "wgrad", (4096, 320, 320), RING, env="NK_GEMM_W160=0", guard="rows", why_rows=SPLIT_LD, accumulate=0,
           dbias=1, graph=True),
        _c("wgrad-splitk-ring-known-zero", "wgrad", (4096, 320, 320), RING, env="NK_GEMM_W160=0", guard="rows", why_rows=SPLIT_LD, accumulate=2),
        _c("wgrad-splitk-ring-4x1280x320-like", "wgrad", (1288, 8, 320), RING, env="NK_GEMM_W160=0", guard="rows", why_rows=SPLIT_LD, accumulate=1,
           dbias=1),
        _c("wgrad-splitk-dma-1280x1152", "wgrad", (4096, 1280, 1152), DMA, env="NK_GEMM_W160=0", guard="rows", why_rows=SPLIT_LD, accumulate=0,
           dbias=1),
        _c("wgrad-ring-unsplit-ragged", "wgrad", (1000, 200, 136), RING, env="NK_GEMM_W160=0", accumulate=0, dbias=1),
        _c("wgrad-ring-unsplit-ragged-accumulate", "wgrad", (1000, 200, 136), RING, env="NK_GEMM_W160=0", accumulate=1, dbias=1),
        _c("wgrad-dma-unsplit", "wgrad", (520, 2048, 2176), DMA, env="NK_GEMM_W160=0", accumulate=0, dbias=1),
        _c("wgrad-dma-unsplit-krot0-known-zero", "wgrad", (520, 2048, 2176), DMA, env="NK_GEMM_W160=0 NK_GEMM_KROT=0", accumulate=2),
        _c("colsum-16384x1280", "colsum", (16384, 1280, 0), "colsum_partial", guard="rows", why_rows="a vector: guards ahead of and behind it",
           accumulate=0),
        _c("colsum-ragged-accumulate", "colsum", (1001, 328, 0), "colsum_partial", guard="rows", why_rows="a vector: guards ahead of and behind it",
           accumulate=1, ldx_pad=8),
    ]
    # ---- Conv forward (N, H, W, Cin, Cout, k, stride, pad): y[pixels, Cout] (+ bias, row vector per image, residual) ----------------------
    all3 = dict(bias=1, rowvec=1, residual=1)
    cv = dict(guard="rows", why_rows=CONV_LD)
    t += [
        _c("conv-halo160x8-2x320x128", "conv_fwd", (2, 128, 128, 320, 320, 3, 1, 1), HALO(160, 8), **cv, **all3),
        _c("conv-halo160x8-stats", "conv_fwd", (2, 128, 128, 320, 320, 3, 1, 1), HALO(160, 8, 1), **cv, **all3, stats=32, graph=True),
        _c("conv-halo160x8-ragged", "conv_fwd", (2, 124, 128, 64, 320, 3, 1, 1), HALO(160, 8), **cv, bias=1),
        _c("conv-halo160x4-4x1280x32", "conv_fwd", (4, 32, 32, 1280, 1280, 3, 1, 1), HALO(160, 4), **cv, **all3),
        _c("conv-halo160x4-krot0", "conv_fwd", (4, 32, 32, 1280, 1280, 3, 1, 1), HALO(160, 4), env="NK_GEMM_KROT=0", **cv, bias=1),
        _c("conv-halo160x4-stats", "conv_fwd", (4, 32, 32, 1280, 1280, 3, 1, 1), HALO(160, 4, 1), **cv, **all3, stats=32),
        _c("conv-halo160x4-ragged", "conv_fwd", (3, 30, 64, 64, 160, 3, 1, 1), HALO(160, 4), **cv, **all3),
        _c("conv-halo128x8-vae-2x128to256x128", "conv_fwd", (2, 128, 128, 128, 256, 3, 1, 1), HALO(128, 8), **cv, bias=1),
        _c("conv-halo128x8-stats", "conv_fwd", (2, 128, 128, 128, 256, 3, 1, 1), HALO(128, 8, 1), **cv, bias=1, stats=32),
        _c("conv-halo128x4-ragged", "conv_fwd", (2, 22, 32, 64, 128, 3, 1, 1), HALO(128, 4), **cv, **all3),
        _c("conv-halo128x4-ragged-stats", "conv_fwd", (2, 22, 32, 64, 128, 3, 1, 1), HALO(128, 4, 1), **cv, bias=1, stats=32),
        _c("conv-g2p160-gather-4x1280x32", "conv_fwd", (4, 32, 32, 1280, 1280, 3, 1, 1), G2P160, env="NK_CONV_HALO=0", **cv, **all3),
        _c("conv-g2p160-gather-stride2", "conv_fwd", (2, 32, 32, 320, 320, 3, 2, 1), G2P160, env="NK_GEMM_G2=2", **cv, bias=1),
        _c("conv-g2p160-gather-upsample", "conv_fwd", (2, 16, 16, 640, 640, 3, 1, 1), G2P160, env="NK_GEMM_G2=2", **cv, bias=1, up=1),
        _c("conv-g2p128-gather-ragged", "conv_fwd", (1, 24, 40, 128, 384, 3, 1, 1), G2P128, env="NK_GEMM_G2=2 NK_CONV_HALO=0", **cv, **all3),
        _c("conv-xl-gather-2x64to1920x64", "conv_fwd", (2, 64, 64, 64, 1920, 3, 1, 1), XL, env="NK_CONV_HALO=0", **cv, **all3),
        _c("conv-xl-gather-ragged-stride2", "conv_fwd", (2, 126, 128, 64, 1912, 3, 2, 1), XL, **cv, bias=1),
        _c("conv-sk-asym-pad-stride2", "conv_fwd", (2, 32, 32, 320, 320, 3, 2, 0), SK, **cv, bias=1, asym=1),
        _c("conv-sk-4x4-taps-stride2", "conv_fwd", (2, 64, 64, 64, 128, 4, 2, 1), SK, env="NK_GEMM_SK=1", **cv, bias=1),
        _c("conv-ring-4x4-taps-stride2", "conv_fwd", (2, 64, 64, 64, 128, 4, 2, 1), RING, **cv, bias=1),
        _c("conv-ring-11x11-taps-stride4", "conv_fwd", (2, 64, 64, 8, 64, 11, 4, 2), RING, **cv, bias=1, cin_real=3),
        _c("conv-ring-channels-4-padded-to-8", "conv_fwd", (2, 64, 64, 8, 320, 3, 1, 1), RING, **cv, bias=1, cin_real=4),
        _c("conv-ring-ragged", "conv_fwd", (3, 19, 13, 40, 72, 3, 1, 1), RING, **cv, **all3),
        _c("conv-dma-2x64to128x256", "conv_fwd", (2, 256, 256, 64, 128, 3, 1, 1), DMA, env="NK_CONV_HALO=0", **cv, **all3),
        _c("conv-dma-1x1-taps-ragged", "conv_fwd", (3, 117, 96, 40, 136, 1, 1, 0), DMA, env="NK_GEMM_SK=0", **cv, bias=1),
    ]
    # ---- Conv dgrad: dx[input pixels, Cin] from dy[pixels, Cout] --------------------------------------------------------------------------
    t += [
        _c("cdgrad-flipped-halo160x4-4x1280x32", "conv_dgrad", (4, 32, 32, 1280, 1280, 3, 1, 1), HALO(160, 4), **cv, flipped=1, graph=True),
        _c("cdgrad-flipped-halo128x4-ragged", "conv_dgrad", (2, 22, 32, 128, 64, 3, 1, 1), HALO(128, 4), **cv, flipped=1),
        _c("cdgrad-flipped-halo160x8-2x320x128", "conv_dgrad", (2, 128, 128, 320, 320, 3, 1, 1), HALO(160, 8), **cv, flipped=1),
        _c("cdgrad-g2p160-transposed-taps-4x1280x32", "conv_dgrad", (4, 32, 32, 1280, 1280, 3, 1, 1), G2P160, **cv),
        _c("cdgrad-g2p160-stride2", "conv_dgrad", (2, 32, 32, 320, 320, 3, 2, 1), G2P160, env="NK_GEMM_G2=2", **cv),
        _c("cdgrad-g2p160-upsample", "conv_dgrad", (2, 16, 16, 640, 640, 3, 1, 1), G2P160, env="NK_GEMM_G2=2", **cv, up=1),
        _c("cdgrad-sk-stride2", "conv_dgrad", (2, 32, 32, 320, 320, 3, 2, 1), SK, env="NK_GEMM_SK=1 NK_GEMM_G2=0", **cv),
        _c("cdgrad-sk-asym-pad-stride2", "conv_dgrad", (2, 32, 32, 320, 320, 3, 2, 0), SK, env="NK_GEMM_SK=1 NK_GEMM_G2=0", **cv, asym=1),
        _c("cdgrad-ring-ragged", "conv_dgrad", (3, 19, 13, 40, 72, 3, 1, 1), RING, **cv),
        _c("cdgrad-ring-4x4-taps-stride2", "conv_dgrad", (2, 32, 32, 64, 128, 4, 2, 1), RING, env="NK_GEMM_SK=0 NK_GEMM_G2=0", **cv),
        _c("cdgrad-dma-upsample", "conv_dgrad", (3, 64, 64, 64, 64, 3, 1, 1), DMA, env="NK_GEMM_SK=0 NK_GEMM_G2=0", **cv, up=1),
    ]
    # ---- Conv wgrad: dw[Cout, taps x Cin] (+)= over N Ho Wo pixels, dbias[Cout] (+)= pixel sums of dy -------------------------------------
    t += [
        _c("cwgrad-halo-one-split-4x1280x32", "conv_wgrad", (4, 32, 32, 1280, 1280, 3, 1, 1), WH1, **cv, accumulate=0, dbias=1, splits="one"),
        _c("cwgrad-halo-one-split-accumulate", "conv_wgrad", (4, 32, 32, 1280, 1280, 3, 1, 1), WH0, **cv, accumulate=1, splits="one"),
        _c("cwgrad-halo-several-splits-2x320x128", "conv_wgrad", (2, 128, 128, 320, 320, 3, 1, 1), WH1, **cv, accumulate=0, dbias=1, splits="several",
           graph=True),
        _c("cwgrad-halo-several-splits-accumulate", "conv_wgrad", (2, 128, 128, 320, 320, 3, 1, 1), WH1, **cv, accumulate=1, dbias=1, splits="several"),
        _c("cwgrad-halo-several-splits-known-zero", "conv_wgrad", (2, 128, 128, 320, 320, 3, 1, 1), WH0, **cv, accumulate=2, splits="several"),
        _c("cwgrad-halo-131072-pixels", "conv_wgrad", (2, 256, 256, 64, 128, 3, 1, 1), WH1, **cv, accumulate=1, dbias=1, r=4, splits="several"),
        _c("cwgrad-halo-forced-ragged", "conv_wgrad", (3, 22, 32, 64, 72, 3, 1, 1), WH1, env="NK_CONV_WGRAD_HALO=2", **cv, accumulate=0, dbias=1),
        _c("cwgrad-gather-sk", "conv_wgrad", (2, 64, 64, 128, 128, 3, 1, 1), SK, env="NK_GEMM_SK=2 NK_CONV_WGRAD_HALO=0", **cv, accumulate=0),
        _c("cwgrad-gather-sk-stride2-accumulate", "conv_wgrad", (2, 64, 64, 64, 128, 4, 2, 1), SK, env="NK_GEMM_SK=2", **cv, accumulate=1),
        _c("cwgrad-gather-splitk-atomics", "conv_wgrad", (2, 32, 32, 64, 64, 3, 1, 1), RING, env="NK_CONV_WGRAD_HALO=0", **cv, accumulate=0, dbias=1),
        _c("cwgrad-gather-splitk-atomics-known-zero", "conv_wgrad", (2, 32, 32, 64, 64, 3, 1, 1), RING, env="NK_CONV_WGRAD_HALO=0", **cv, accumulate=2,
           dbias=1),
        _c("cwgrad-gather-unsplit-ragged", "conv_wgrad", (3, 19, 13, 40, 72, 3, 1, 1), RING, **cv, accumulate=0, dbias=1),
        _c("cwgrad-gather-unsplit-upsample-accumulate", "conv_wgrad", (2, 8, 8, 64, 64, 3, 1, 1), RING, **cv, accumulate=1, dbias=1, up=1),
        _c("cwgrad-gather-dma-1x1-taps", "conv_wgrad", (2, 16, 16, 2304, 2048, 1, 1, 0), DMA, **cv, accumulate=0, dbias=1),
    ]
    ids = [c.id for c in t]
    assert len(ids) == len(set(ids))
    return t


CASES = _table()
BY_ID = {c.id: c for c in CASES}


def op_is_rows_by_k(c: Case) -> bool:
    return c.op in ("fwd", "fwd_geglu", "fwd_batched", "dgrad", "dgrad_geglu_s")


def out_shape(c: Case):
    """(rows, columns) of the output, and the length of the bias gradient (0: none)."""
    op = c.op
    if op in ("fwd", "fwd_batched", "dgrad"):
        return (c.dims[0], c.dims[1]), 0
    if op in ("fwd_geglu", "dgrad_geglu_s"):
        return (c.dims[0], 2 * c.dims[1]), 0
    if op in ("wgrad", "wgrad_batched"):
        return (c.dims[1], c.dims[2]), c.dims[1]
    if op == "colsum":
        return (1, c.dims[1]), 0
    N, H, W, Cin, Cout, k, stride, pad = c.dims
    Hin, Win, Ho, Wo = conv_geometry(c)
    if op == "conv_fwd":
        return (N * Ho * Wo, Cout), 0
    if op == "conv_dgrad":
        return (N * Hin * Win, Cin), 0
    return (Cout, k * k * Cin), Cout


def ragged(c: Case) -> bool:
    """Linear cases: rows not a multiple of the tile height and a reduction that is a multiple of 8 but not of 64."""
    if op_is_rows_by_k(c):
        return c.dims[0] % 64 != 0 and c.dims[2] % 64 != 0
    if c.op in ("wgrad", "wgrad_batched"):
        return c.dims[0] % 64 != 0
    return False


# ---- generators and the exactness condition ------------------------------------------------------------------------------------------------
def ints(shape, r, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-r, r + 1, tuple(shape), generator=g).float()


def _seed(c: Case, k: int) -> int:
    return (sum((i + 1) * d for i, d in enumerate(c.dims)) * 31 + k) % (2 ** 31)


def conv_geometry(c: Case):
    N, H, W, Cin, Cout, k, stride, pad = c.dims
    Hin, Win = (2 * H, 2 * W) if c.o("up") else (H, W)
    if c.o("asym"):
        Ho, Wo = (Hin + 1 - k) // stride + 1, (Win + 1 - k) // stride + 1
    else:
        Ho, Wo = (Hin + 2 * pad - k) // stride + 1, (Win + 2 * pad - k) // stride + 1
    return Hin, Win, Ho, Wo


def terms(c: Case) -> dict:
    """The ranges the exactness condition is computed from (no matmul): T terms of |a| <= ra, |b| <= rb, times `factor` (|alpha|, or the range
    of the saved GEGLU factor), `passes` launches into one destination, and the magnitudes added in the epilogue or sitting in the destination."""
    op, r = c.op, c.r
    add, passes, factor = [], 1, 1.0
    if op in ("fwd", "fwd_batched", "fwd_geglu"):
        T = c.dims[2]
        factor = abs(c.o("alpha", 1.0))
        add = [ADD_RANGE] * (bool(c.o("bias")) + bool(c.o("residual")))
    elif op == "dgrad":
        T, add = c.dims[2], [ADD_RANGE] * bool(c.o("add"))
    elif op == "dgrad_geglu_s":
        T, factor = c.dims[2], float(r)                  # s is drawn from the operands' range
    elif op in ("wgrad", "wgrad_batched", "colsum"):
        T = c.dims[0]
    elif op == "conv_fwd":
        T = c.dims[5] * c.dims[5] * c.dims[3]
        add = [ADD_RANGE] * (bool(c.o("bias")) + bool(c.o("rowvec")) + bool(c.o("residual")))
    elif op == "conv_dgrad":
        T = c.dims[5] * c.dims[5] * c.dims[4]
    elif op == "conv_wgrad":
        _, _, Ho, Wo = conv_geometry(c)
        T = c.dims[0] * Ho * Wo
    else:
        raise ValueError(op)
    if c.o("accumulate") == 1:       # checked as store-then-accumulate: two passes into one destination
        passes = 2
    rb = 1 if op == "colsum" else r
    return dict(T=T, ra=r, rb=rb, factor=factor, passes=passes, add=add)


def exact_magnitude(c: Case) -> float:
    """Upper bound of every intermediate and final value of the case: must stay below 2^24."""
    t = terms(c)
    return t["passes"] * t["T"] * t["ra"] * t["rb"] * t["factor"] + sum(t["add"])


def make_inputs(c: Case) -> dict:
    """Integer-valued fp32 CPU tensors (lists of them for the batched entry points)."""
    op, r = c.op, c.r
    s = lambda k: _seed(c, k)
    nb = c.o("batch", 0)
    if op in ("fwd", "fwd_batched", "fwd_geglu"):
        M, N, K = c.dims
        N = 2 * N if op == "fwd_geglu" else N
        if nb:
            return dict(x=[ints((M, K), r, s(10 + i)) for i in range(nb)], w=[ints((N, K), r, s(30 + i)) for i in range(nb)])
        d = dict(x=ints((M, K), r, s(1)), w=ints((N, K), r, s(2)))
        if c.o("bias"):
            d["bias"] = ints((N,), ADD_RANGE, s(3))
        if c.o("residual"):
            d["residual"] = ints((M, N), ADD_RANGE, s(4))
        return d
    if op == "dgrad":
        M, N, K = c.dims
        d = dict(dy=ints((M, K), r, s(1)), w=ints((K, N), r, s(2)))
        if c.o("add"):
            d["add"] = ints((M, N), ADD_RANGE, s(3))
        return d
    if op == "dgrad_geglu_s":
        M, N, K = c.dims
        return dict(dy=ints((M, K), r, s(1)), w=ints((K, N), r, s(2)), s=ints((M, 2 * N), r, s(3)))
    if op in ("wgrad", "wgrad_batched"):
        M, N, K = c.dims
        if nb:
            return dict(dy=[ints((M, N), r, s(10 + i)) for i in range(nb)], x=[ints((M, K), r, s(30 + i)) for i in range(nb)])
        return dict(dy=ints((M, N), r, s(1)), x=ints((M, K), r, s(2)))
    if op == "colsum":
        return dict(dy=ints((c.dims[0], c.dims[1]), r, s(1)))
    N, H, W, Cin, Cout, k, stride, pad = c.dims
    Hin, Win, Ho, Wo = conv_geometry(c)
    x = ints((N, H, W, Cin), r, s(1))
    if c.o("cin_real"):
        x[..., c.o("cin_real"):] = 0          # 3 or 4 real channels stored padded to 8
    d = dict(x=x, w=ints((Cout, k, k, Cin), r, s(2)))
    if op == "conv_fwd":
        if c.o("bias"):
            d["bias"] = ints((Cout,), ADD_RANGE, s(3))
        if c.o("rowvec"):
            d["rowvec"] = ints((N, Cout), ADD_RANGE, s(4))
        if c.o("residual"):
            d["residual"] = ints((N * Ho * Wo, Cout), ADD_RANGE, s(5))
    else:
        d["dy"] = ints((N * Ho * Wo, Cout), r, s(6))
    return d


# ---- float64 references ---------------------------------------------------------------------------------------------------------------------
def _conv_nchw(c: Case, x):
    N, H, W, Cin = x.shape
    xi = x.permute(0, 3, 1, 2).double()
    if c.o("up"):
        xi = F.interpolate(xi, scale_factor=2, mode="nearest")
    if c.o("asym"):
        xi = F.pad(xi, (0, 1, 0, 1))
    return xi.contiguous()


def reference(c: Case, inp: dict, magnitude: bool = False) -> dict:
    """float64 on the CPU.  Returns {output name: tensor} ("y", and "dbias" for the weight gradients), plus "addends" (the sum of the epilogue
    addends, 0.0 if none) for the derived bound.  magnitude=True: the same with every input replaced by its absolute value (and |alpha|):
    "y" is then |alpha| sum |a||b| + sum |addends|."""
    f = (lambda v: v.double().abs()) if magnitude else (lambda v: v.double())
    op = c.op
    if op in ("fwd", "fwd_geglu"):
        alpha = abs(c.o("alpha", 1.0)) if magnitude else c.o("alpha", 1.0)
        y = alpha * (f(inp["x"]) @ f(inp["w"]).t())
        add = torch.zeros((), dtype=torch.float64)
        if "bias" in inp:
            add = add + f(inp["bias"])
        if "residual" in inp:
            add = add + f(inp["residual"])
        return dict(y=y + add, addends=add)
    if op == "fwd_batched":
        return dict(y=[f(x) @ f(w).t() for x, w in zip(inp["x"], inp["w"])], addends=0.0)
    if op == "dgrad":
        y = f(inp["dy"]) @ f(inp["w"])
        add = f(inp["add"]) if "add" in inp else torch.zeros((), dtype=torch.float64)
        return dict(y=y + add, addends=add)
    if op == "dgrad_geglu_s":
        d = f(inp["dy"]) @ f(inp["w"])
        return dict(y=torch.cat([d, d], 1) * f(inp["s"]), addends=0.0)
    if op == "wgrad":
        return dict(y=f(inp["dy"]).t() @ f(inp["x"]), dbias=f(inp["dy"]).sum(0), addends=0.0)
    if op == "wgrad_batched":
        return dict(y=[f(dy).t() @ f(x) for dy, x in zip(inp["dy"], inp["x"])], dbias=[f(dy).sum(0) for dy in inp["dy"]], addends=0.0)
    if op == "colsum":
        return dict(y=f(inp["dy"]).sum(0)[None, :], addends=0.0)
    N, H, W, Cin, Cout, k, stride, pad = c.dims
    Hin, Win, Ho, Wo = conv_geometry(c)
    p = 0 if c.o("asym") else pad
    x = inp["x"].abs() if magnitude else inp["x"]
    xi = _conv_nchw(c, x)
    wd = f(inp["w"]).permute(0, 3, 1, 2).contiguous()
    if op == "conv_fwd":
        y = F.conv2d(xi, wd, None, stride=stride, padding=p).permute(0, 2, 3, 1).reshape(N * Ho * Wo, Cout)
        add = torch.zeros((), dtype=torch.float64)
        if "bias" in inp:
            add = add + f(inp["bias"])
        if "rowvec" in inp:
            add = add + f(inp["rowvec"]).repeat_interleave(Ho * Wo, 0)
        if "residual" in inp:
            add = add + f(inp["residual"])
        return dict(y=y + add, addends=add)
    dyd = f(inp["dy"]).view(N, Ho, Wo, Cout).permute(0, 3, 1, 2).contiguous()
    if op == "conv_dgrad":
        dx = torch.nn.grad.conv2d_input(xi.shape, wd, dyd, stride=stride, padding=p)
        if c.o("asym"):
            dx = dx[:, :, :-1, :-1]
        return dict(y=dx.permute(0, 2, 3, 1).reshape(N * Hin * Win, Cin), addends=0.0)       # (over the virtual 2x grid under upsample)
    dw = torch.nn.grad.conv2d_weight(xi, wd.shape, dyd, stride=stride, padding=p)
    return dict(y=dw.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin), dbias=f(inp["dy"]).sum(0), addends=0.0)


def expected(ref64: torch.Tensor, dtype) -> torch.Tensor:
    """What the kernel must store: the exact value in fp32 (asserted), rounded once to nearest-even for a bf16 output."""
    e = ref64.float()
    assert torch.equal(e.double(), ref64), "the reference is not exact in fp32: the case breaks the exactness condition"
    return e.to(dtype)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------
def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous() + 0.0          # (-0 + 0 = +0: a signed zero is no arithmetic difference)
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_exact(got: torch.Tensor, want: torch.Tensor, case: str, tile=(128, 128)):
    """Bitwise equality.  On failure: how many elements differ and the first few as (row, column, got, want, got - want) with the tile they lie
    in -- the difference is an integer combination of products, so it usually says which element went missing."""
    assert got.dim() == 2 and got.shape == want.shape and got.dtype == want.dtype, (case, got.shape, want.shape, got.dtype, want.dtype)
    gb, wb = _bits(got), _bits(want)
    if torch.equal(gb, wb):
        return
    bad = (gb != wb).nonzero()
    g, w = got.detach().cpu(), want.detach().cpu()
    lines = []
    for row, col in bad[:8].tolist():
        gv, wv = float(g[row, col]), float(w[row, col])
        lines.append(f"  ({row}, {col}) got {gv!r} want {wv!r} diff {gv - wv!r}  tile ({row // tile[0]}, {col // tile[1]}) at (+{row % tile[0]}, +{col % tile[1]})")
    rows = sorted(set(bad[:, 0].tolist()))
    raise AssertionError(f"{case}: WRONG RESULT: {len(bad)} of {got.numel()} elements differ from the exact value (tile {tile[0]} x {tile[1]}); rows "
                         f"{rows[:6]}{'...' if len(rows) > 6 else ''}\n" + "\n".join(lines))


class Guarded:
    """An output as a view into a larger buffer full of sentinels: ROWS rows ahead of the first element and behind the last, and -- where the
    entry point takes a leading dimension -- extra columns behind every row."""
    ROWS = 8            # (8 rows x any width are a multiple of 16 bytes: the view stays aligned)

    def __init__(self, rows, cols, dtype, col_guard: bool, device="cuda"):
        self.rows, self.cols = rows, cols
        self.ld = (-(-cols // 8) * 8 + 16) if col_guard else cols
        self.buf = torch.full(((rows + 2 * self.ROWS) * self.ld,), SENTINEL, dtype=dtype, device=device)
        self.view = self._view(self.buf)

    def _view(self, buf):
        return buf[self.ROWS * self.ld:(self.ROWS + self.rows) * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def arm(self, fill):
        self.buf.fill_(SENTINEL)
        if torch.is_tensor(fill):
            self.view.copy_(fill)
        else:
            self.view.fill_(fill)

    def assert_untouched(self, case: str):
        c = self.buf.clone()
        self._view(c).fill_(SENTINEL)
        bad = (c != SENTINEL).nonzero().flatten()
        if len(bad):
            where = [((i // self.ld) - self.ROWS, i % self.ld) for i in bad[:8].tolist()]
            raise AssertionError(f"{case}: STORE OUTSIDE THE OUTPUT: {len(bad)} guard elements overwritten around the {self.rows} x {self.cols} "
                                 f"view (ld {self.ld}); first (row, column): {where}")


# ---- running a case on the GPU ---------------------------------------------------------------------------------------------------------------
@contextmanager
def environment(pairs):
    assert all(k != "NK_GEMM_XL" for k, _ in pairs), "NK_GEMM_XL is read once per process: reach the kernels behind it by shape"
    old = {k: os.environ.get(k) for k, _ in pairs}
    os.environ.update(dict(pairs))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def wgrad_halo_splits(c: Case) -> int:
    """Pixel-range splits of the halo-tile weight gradient: the cost rule of gemm_plan.h (wgrad_halo_splits), restated -- the launch name
    does not carry the number, and the cases mean "one" or "several"."""
    N, H, W, Cin, Cout = c.dims[:5]
    T = N * (-(-W // 32)) * (-(-H // 4))
    nblk = (-(-Cout // 128)) * (Cin // 64)
    dw_bytes = Cout * 9 * Cin * 4.0
    best, best_s = 1e30, 1
    for s in range(1, min(64, T) + 1):
        tiles, rounds = -(-T // s), -(-nblk * s // 256)
        cost = rounds * (tiles * 3.0e-6 + 4.0e-6) + (s * dw_bytes / 1.3e12 if s > 1 else dw_bytes / 4.0e12)
        if cost < best * 0.97:
            best, best_s = cost, s
    per = -(-T // best_s)
    return -(-T // per)


class Run:
    """One case on the device: inputs uploaded as bf16, destinations guarded.  arm() resets the destinations, launch() issues the launches
    (host calls only: capturable), outputs() yields (label, Guarded, float64 reference) with the store-then-accumulate factor applied."""

    def __init__(self, c: Case, inp: dict):
        from neurosis_amd import ops

        self.c, self.ops = c, ops
        self.d = {}
        for k, v in inp.items():       # bf16 on the device (the bias stays fp32); ldx_pad: the first operand as a strided view (ld = K + pad)
            pad = c.o("ldx_pad", 0) if k in ("x", "dy") and c.op in ("fwd", "colsum") else 0
            if isinstance(v, list):
                self.d[k] = [t.to("cuda", torch.bfloat16) for t in v]
            else:
                self.d[k] = v.cuda() if k == "bias" else self._pad(v.to("cuda", torch.bfloat16), pad)
        cg = c.guard == "cols"
        nb = c.o("batch", 0)
        op = c.op
        (rows, cols), nbias = out_shape(c)
        out_dtype = torch.float32 if op in ("wgrad", "wgrad_batched", "colsum", "conv_wgrad") else torch.bfloat16
        self.y = [Guarded(rows, cols, out_dtype, cg) for _ in range(nb or 1)]
        self.db = [Guarded(1, nbias, torch.float32, False) for _ in range(nb or 1)] if c.o("dbias") else []
        self.h = Guarded(rows, cols // 2, torch.bfloat16, cg) if op == "fwd_geglu" else None
        self.acc = c.o("accumulate", 0)
        if op in ("conv_fwd", "conv_dgrad", "conv_wgrad"):
            from neurosis_amd.lib import NkConvDesc

            N, H, W, Cin, Cout, k, stride, pad = c.dims
            _, _, Ho, Wo = conv_geometry(c)
            p = 0 if c.o("asym") else pad
            self.desc = NkConvDesc(N, H, W, Cin, Cout, k, k, stride, p, p, Ho, Wo, int(bool(c.o("up"))))
            self.w2d = self.d["w"].reshape(Cout, k * k * Cin)
            if c.o("stats"):
                self.tiles = ops.query("nk_conv2d_stats_tiles", C.byref(self.desc), c.o("stats"))
                assert self.tiles > 0, f"{c.id}: the dispatch moved: the statistics epilogue no longer takes this shape; the case needs a new one"
                self.part = torch.empty(N, self.tiles, 2 * c.o("stats"), dtype=torch.float32, device="cuda")
            if c.o("flipped"):
                assert ops.query("nk_conv2d_dgrad_flipped_ok", C.byref(self.desc)) == 1, f"{c.id}: the dispatch moved: no flipped input gradient here"
                self.wt = torch.empty(Cin * 9 * Cout, dtype=torch.bfloat16, device="cuda")
        if op == "colsum":
            M, N = c.dims[:2]
            self.ws = torch.empty(ops.query("nk_colsum_ws_floats", M, N), dtype=torch.float32, device="cuda")

    @staticmethod
    def _pad(t, pad):
        if not pad:
            return t.contiguous()
        buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]

    def arm(self):
        fill = 0.0 if self.acc == 2 else GARBAGE       # accumulate 1 is checked as a store (over garbage) followed by an accumulate
        for g in self.y + self.db + ([self.h] if self.h else []):
            g.arm(fill)

    def launch(self):
        for acc in ([0, 1] if self.acc == 1 else [self.acc]):
            self._launch(acc)

    def _launch(self, acc):
        c, d, ops, P = self.c, self.d, self.ops, (lambda t: t.data_ptr() if t is not None else None)
        op, st = c.op, self.ops._stream()
        y = self.y[0].view
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        if op == "fwd":
            ops.gemm_nt(d["x"], d["w"], d.get("bias"), d.get("residual"), alpha=c.o("alpha", 1.0), out=y)
        elif op == "fwd_geglu":
            M, I, K = c.dims
            assert ops.query("nk_linear_fwd_geglu_ok", M, I, K), f"{c.id}: the dispatch moved: the fused GEGLU forward no longer takes this shape"
            ops.call("nk_linear_fwd_geglu", P(d["x"]), P(d["w"]), P(d.get("bias")), P(y), P(self.h.view), M, I, K, d["x"].stride(0), d["w"].stride(0),
                     y.stride(0), self.h.view.stride(0), st)
        elif op == "fwd_batched":
            ops.gemm_nt_batched(d["x"], d["w"], [g.view for g in self.y])
        elif op == "dgrad":
            ops.gemm_nn(d["dy"], d["w"], d.get("add"), out=y)
        elif op == "dgrad_geglu_s":
            M, N, K = c.dims
            ops.call("nk_linear_dgrad_geglu_s", P(d["dy"]), P(d["w"]), P(d["s"]), P(y), M, K, N, d["dy"].stride(0), d["w"].stride(0), d["s"].stride(0),
                     y.stride(0), st)
        elif op == "wgrad":
            ops.gemm_tn_f32(d["dy"], d["x"], y, acc, dbias=self.db[0].view[0] if self.db else None)
        elif op == "wgrad_batched":
            M, N, K = c.dims
            dbs = (C.c_void_p * len(self.y))(*[g.view.data_ptr() for g in self.db]) if self.db else None
            ops.call("nk_linear_wgrad_batched", arr(d["dy"]), arr(d["x"]), arr([g.view for g in self.y]), dbs, len(self.y), M, N, K, N, K,
                     self.y[0].ld, acc, st)
        elif op == "colsum":
            M, N = c.dims[:2]
            ops.call("nk_colsum", P(d["dy"]), P(y), P(self.ws), M, N, d["dy"].stride(0), acc, st)
        elif op == "conv_fwd":
            args = (C.byref(self.desc), P(d["x"]), P(self.w2d), P(d.get("bias")), P(d.get("rowvec")), P(d.get("residual")), P(y))
            if c.o("stats"):
                ops.call("nk_conv2d_fwd_stats", *args, P(self.part), c.o("stats"), st)
            else:
                ops.call("nk_conv2d_fwd", *args, st)
        elif op == "conv_dgrad":
            N, H, W, Cin, Cout = c.dims[:5]
            if c.o("flipped"):
                ops.call("nk_conv_weight_flip", P(self.w2d), P(self.wt), Cout, Cin, 9, st)
                ops.call("nk_conv2d_dgrad_flipped", C.byref(self.desc), P(d["dy"]), P(self.wt), P(y), st)
            else:
                ops.call("nk_conv2d_dgrad", C.byref(self.desc), P(d["dy"]), P(self.w2d), P(y), st)
        elif op == "conv_wgrad":
            if self.db:
                ops.call("nk_conv2d_wgrad_bias", C.byref(self.desc), P(d["dy"]), P(d["x"]), P(y), P(self.db[0].view), acc, st)
            else:
                ops.call("nk_conv2d_wgrad", C.byref(self.desc), P(d["dy"]), P(d["x"]), P(y), acc, st)
        else:
            raise ValueError(op)

    def outputs(self, ref: dict):
        k = 2.0 if self.acc == 1 else 1.0
        nb = self.c.o("batch", 0)
        ys = ref["y"] if nb else [ref["y"]]
        for i, (g, r) in enumerate(zip(self.y, ys)):
            yield f"output {i}" if nb else "output", g, k * r
        if self.db:
            dbs = ref["dbias"] if nb else [ref["dbias"]]
            for i, (g, r) in enumerate(zip(self.db, dbs)):
                yield f"bias gradient {i}" if nb else "bias gradient", g, (k * r)[None, :]


def check_run(run: Run, ref: dict, names, where=""):
    """The order the issue asks for: first WHICH kernel ran (a dispatch that moved is not a wrong result), then the values, then the guards."""
    c = run.c
    assert c.expect in names, (f"{c.id}{where}: THE DISPATCH MOVED, the result was not examined: expected a launch of {c.expect}, the library "
                               f"reports {names}.  The case needs a new shape or environment that reaches {c.expect} again.")
    tile = TILES.get(c.expect, (128, 128))
    if run.h is not None:
        run.h.assert_untouched(f"{c.id}{where} GEGLU output [{c.expect}]")
    for label, g, ref64 in run.outputs(ref):
        assert_exact(g.view, expected(ref64, g.view.dtype), f"{c.id}{where} {label} [{c.expect}]", tile if label.startswith("output") else (1, tile[0]))
        g.assert_untouched(f"{c.id}{where} {label} [{c.expect}]")


# ---- the one derived bound (non-integer inputs) ----------------------------------------------------------------------------------------------
def error_bound(c: Case, ref: dict, mag: dict, bf16_out: bool) -> torch.Tensor:
    """Per element, first order, for an ARBITRARY summation tree over T terms of exact bf16 x bf16 products accumulated in fp32:
    SAFETY (T + 8) 2^-23 |alpha| sum |a||b|  +  2^-23 sum |epilogue addends|  (+ half a bf16 ulp of (|ref| + bound) for a bf16 output).
    The + 8 covers alpha, the epilogue additions and the final conversions."""
    T = terms(c)["T"]
    add_mag = mag["addends"] if torch.is_tensor(mag["addends"]) else torch.zeros((), dtype=torch.float64)
    b = SAFETY * (T + 8) * U32 * (mag["y"] - add_mag) + U32 * add_mag
    if bf16_out:
        top = (ref["y"].abs() + b).clamp_min(2.0 ** -126)
        b = b + 0.5 * torch.exp2(torch.floor(torch.log2(top)) - 7)
    return b
