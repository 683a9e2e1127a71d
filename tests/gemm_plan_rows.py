"""Rows of tile-engine calls and how to ask the library for the plan of each without a GPU (shared by tests/test_gemm_plan_cpu.py and the
recorder that wrote tests/golden/tile_engine_plans.json).

A row is [op, dims, opts, env]: op and dims as in tests/gemm_exact.py (Linear: (M, N, K) as each op reads them; convolutions:
(N, H, W, Cin, Cout, k, stride, pad)), opts the options that can move a plan (accumulate, dbias, batch, stats, flipped, up, asym, ldx_pad,
ld_guard), env the NK_* switches set around the call.  The call passes dummy 16-byte-aligned pointers: in plan-only mode
(lib.launch_log(3)) nk_gemm_dispatch logs its plan and returns before it touches the GPU.

A plan line reads `name grid=x,y,z block smem splitk ksplit_len acc zero krot gm chunk` (csrc/gemm_plan.h: nk_plan_line)."""
from __future__ import annotations

import ctypes as C

from tests.gemm_exact import Case, conv_geometry, environment

PTR = 0x10000           # dummy operand: non-null and 16-byte aligned, never dereferenced


def case_row(c: Case) -> list:
    """The row of a case of gemm_exact.CASES (its destination's leading dimension as Guarded lays it out)."""
    opts = {k: v for k, v in c.opts if k in ("accumulate", "dbias", "batch", "stats", "flipped", "up", "asym", "ldx_pad", "bias", "residual", "rowvec", "add")}
    if c.guard == "cols":
        opts["ld_guard"] = 1
    return [c.op, list(c.dims), opts, dict(c.env)]


def _desc(dims, o):
    from neurosis_amd.lib import NkConvDesc

    c = Case("row", "conv", tuple(dims), "", opts=tuple(sorted(o.items())))
    N, H, W, Cin, Cout, k, stride, pad = dims
    _, _, Ho, Wo = conv_geometry(c)
    p = 0 if o.get("asym") else pad
    return NkConvDesc(N, H, W, Cin, Cout, k, k, stride, p, p, Ho, Wo, int(bool(o.get("up"))))


def call_row(lib, row) -> int:
    """Issue the row's entry-point call with dummy pointers; returns the status."""
    op, dims, o, _ = row
    f = lambda name, *a: int(getattr(lib.load(), name)(*a))
    ld = lambda cols: (-(-cols // 8) * 8 + 16) if o.get("ld_guard") else cols
    opt = lambda name: PTR if o.get(name) else None
    nb = o.get("batch", 0)
    arr = lambda n: (C.c_void_p * n)(*[PTR + 256 * i for i in range(n)])
    acc = o.get("accumulate", 0)
    if op == "fwd":
        M, N, K = dims
        return f("nk_linear_fwd", PTR, PTR, opt("bias"), opt("residual"), PTR, M, N, K, K + o.get("ldx_pad", 0), K, ld(N), ld(N), 1.0, None)
    if op in ("fwd_geglu", "fwd_geglu_s"):
        M, I, K = dims
        return f("nk_linear_" + op, PTR, PTR, opt("bias"), PTR, PTR, M, I, K, K, K, ld(2 * I), ld(I), None)
    if op == "fwd_batched":
        M, N, K = dims
        return f("nk_linear_fwd_batched", arr(nb), arr(nb), arr(nb), nb, M, N, K, K, K, ld(N), None)
    if op == "dgrad":
        M, N, K = dims          # dx[M, N] = dy[M, K] w[K, N]
        return f("nk_linear_dgrad", PTR, PTR, opt("add"), PTR, M, K, N, K, N, ld(N), ld(N), None)
    if op in ("dgrad_geglu", "dgrad_geglu_s"):
        M, N, K = dims          # du[M, 2N], d = dy[M, K] w[K, N]
        return f("nk_linear_" + op, PTR, PTR, PTR, PTR, M, K, N, K, N, 2 * N, ld(2 * N), None)
    if op == "wgrad":
        M, N, K = dims          # dw[N, K] over M tokens
        if o.get("dbias"):
            return f("nk_linear_wgrad_bias", PTR, PTR, PTR, PTR, M, N, K, N, K, ld(K), acc, None)
        return f("nk_linear_wgrad", PTR, PTR, PTR, M, N, K, N, K, ld(K), acc, None)
    if op == "wgrad_batched":
        M, N, K = dims
        return f("nk_linear_wgrad_batched", arr(nb), arr(nb), arr(nb), arr(nb) if o.get("dbias") else None, nb, M, N, K, N, K, ld(K), acc, None)
    d = C.byref(_desc(dims, o))
    if op == "conv_fwd":
        args = (d, PTR, PTR, opt("bias"), opt("rowvec"), opt("residual"), PTR)
        if o.get("stats"):
            return f("nk_conv2d_fwd_stats", *args, PTR, o["stats"], None)
        return f("nk_conv2d_fwd", *args, None)
    if op == "conv_dgrad":
        return f("nk_conv2d_dgrad_flipped" if o.get("flipped") else "nk_conv2d_dgrad", d, PTR, PTR, PTR, None)
    if op == "conv_wgrad":
        if o.get("dbias"):
            return f("nk_conv2d_wgrad_bias", d, PTR, PTR, PTR, PTR, acc, None)
        return f("nk_conv2d_wgrad", d, PTR, PTR, PTR, acc, None)
    raise ValueError(op)


def plan_lines(lib, row) -> list[str]:
    """The plan lines the library logs for the row in plan-only mode ([] when the call is refused before it is planned)."""
    with environment(tuple(row[3].items())):
        lib.launch_log(3)
        try:
            call_row(lib, row)
            return [s for s in lib.launched() if " grid=" in s]
        finally:
            lib.launch_log(0)


def plan_names(lib, row) -> list[str]:
    return [s.split(" ")[0] for s in plan_lines(lib, row)]


def row_key(row) -> str:
    import json

    return json.dumps(row, sort_keys=True, separators=(",", ":"))
