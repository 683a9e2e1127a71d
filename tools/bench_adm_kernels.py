"""Rates of the ADM kernels against the kernels they were derived from, alternating in ONE process: the scale-shift modulated GroupNorm
(apply pass and backward) against the unmodulated one, and the parameter-free resamplers against nk_upsample2x_bwd / nk_cat_channels at the
same byte counts.  GB/s over algorithmic bytes (every tensor read once, written once).

usage: python tools/bench_adm_kernels.py [--rounds 7] [--launches 50] [--parent-lib PATH/libneurosis_hip.so]
--parent-lib: also time the unmodulated GroupNorm entry points of ANOTHER build (the parent commit's library) in the same alternation.

Method: 10 warm-up launches per candidate, then ROUNDS rounds; in a round every candidate is timed once over LAUNCHES back-to-back launches
between two events, and the order of the candidates is reversed every other round.  Reported: median GB/s and the min .. max of the rounds
(the spread)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from neurosis_amd import lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()

parent = None
if a.parent_lib:
    parent = C.CDLL(a.parent_lib)
    for name in ("nk_groupnorm_apply", "nk_groupnorm_bwd"):
        getattr(parent, name).argtypes = lib.SIGNATURES[name]
        getattr(parent, name).restype = C.c_int


def pcall(name, *args):
    rc = getattr(parent, name)(*args)
    assert rc == 0, (name, rc)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / a.launches      # ms


def alternate(cands):
    """cands: [(label, fn, bytes)] -> prints one line each"""
    for _, fn, _ in cands:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _, _ in cands}
    for r in range(a.rounds):
        for label, fn, _ in (cands if r % 2 == 0 else cands[::-1]):
            times[label].append(timed(fn))
    for label, _, nbytes in cands:
        rates = sorted(nbytes / t / 1e6 for t in times[label])
        print(f"  {label:44s} {statistics.median(times[label]) * 1e3:8.1f} us  {statistics.median(rates):7.0f} GB/s   ({rates[0]:.0f} .. {rates[-1]:.0f})", flush=True)


def rb(*shape):
    return torch.randn(*shape, device="cuda").to(torch.bfloat16)


st = ops._stream()
print(f"rounds {a.rounds}, {a.launches} launches per timing, order reversed every other round; GB/s = algorithmic bytes / time, median (min .. max)")
for (N, Cc, H, W) in [(4, 320, 128, 128), (4, 640, 64, 64), (4, 1280, 32, 32)]:
    HW, n = H * W, N * H * W * Cc
    x, dy, y, dx = rb(N * HW, Cc), rb(N * HW, Cc), rb(N * HW, Cc), rb(N * HW, Cc)
    g, b = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    dg, db = torch.zeros(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    mod, dmod = rb(N, 2 * Cc) * 0.5, rb(N, 2 * Cc)
    mean, rstd = torch.empty(N, 32, device="cuda"), torch.empty(N, 32, device="cuda")
    sums = ops.groupnorm_sums(ops.Img(x, N, H, W), 32)
    ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, Cc, 32), "cuda")
    p = lambda t: t.data_ptr()
    apply_args = (p(x), p(sums), p(g), p(b), p(y), p(mean), p(rstd), N, HW, Cc, 32, 1e-5, 1, st)
    bwd_args = (p(dy), p(x), p(g), p(b), p(mean), p(rstd), None, p(dx), p(dg), p(db), p(ws), N, HW, Cc, 32, 1, 0, st)
    ops.call("nk_groupnorm_apply", *apply_args)      # mean / rstd for the backward candidates
    print(f"GroupNorm+SiLU (N, C, H, W) = {(N, Cc, H, W)}")
    cands = [("nk_groupnorm_apply", lambda: ops.call("nk_groupnorm_apply", *apply_args), 4 * n),
             ("nk_groupnorm_mod_apply", lambda: ops.call("nk_groupnorm_mod_apply", p(x), p(sums), p(g), p(b), p(mod), p(y), p(mean), p(rstd), N, HW, Cc, 32, 1e-5, 1, st),
              4 * n + 4 * N * Cc)]
    if parent is not None:
        cands.append(("nk_groupnorm_apply (parent build)", lambda: pcall("nk_groupnorm_apply", *apply_args), 4 * n))
    alternate(cands)
    cands = [("nk_groupnorm_bwd", lambda: ops.call("nk_groupnorm_bwd", *bwd_args), 6 * n),
             ("nk_groupnorm_mod_bwd", lambda: ops.call("nk_groupnorm_mod_bwd", p(dy), p(x), p(g), p(b), p(mod), p(mean), p(rstd), None, p(dx), p(dg), p(db), p(dmod), p(ws),
                                                       N, HW, Cc, 32, 1, 0, st), 6 * n + 8 * N * Cc)]
    if parent is not None:
        cands.append(("nk_groupnorm_bwd (parent build)", lambda: pcall("nk_groupnorm_bwd", *bwd_args), 6 * n))
    alternate(cands)

for (N, Cc, H, W) in [(4, 320, 128, 128), (4, 640, 64, 64), (4, 1280, 32, 32)]:
    n = N * H * W * Cc
    p = lambda t: t.data_ptr()
    x, q, up = rb(N * H * W, Cc), rb(N * (H // 2) * (W // 2), Cc), rb(N * 4 * H * W, Cc)
    print(f"resamplers (N, C, H, W) = {(N, Cc, H, W)}")
    # nearest 2x forward and its adjoint move the same bytes: 2 B per small-grid element on one side, 8 B on the other
    alternate([("nk_upsample2x_fwd", lambda: ops.call("nk_upsample2x_fwd", p(x), p(up), N, H, W, Cc, st), 10 * n),
               ("nk_upsample2x_bwd", lambda: ops.call("nk_upsample2x_bwd", p(up), p(x), N, H, W, Cc, st), 10 * n)])
    # the pool moves 2.5 B per full-grid element; a channel concat of the same byte count: rows x C with 2.5 n = 4 rows C
    rows = (5 * n // 8) // Cc
    ca, cb, cat = rb(rows, Cc // 2), rb(rows, Cc // 2), rb(rows, Cc)
    alternate([("nk_avgpool2x_fwd", lambda: ops.call("nk_avgpool2x_fwd", p(x), p(q), N, H, W, Cc, st), 5 * n // 2),
               ("nk_avgpool2x_bwd", lambda: ops.call("nk_avgpool2x_bwd", p(q), p(x), N, H, W, Cc, st), 5 * n // 2),
               ("nk_cat_channels (same bytes)", lambda: ops.call("nk_cat_channels", p(ca), p(cb), p(cat), rows, Cc // 2, Cc // 2, st), 4 * rows * Cc)])
