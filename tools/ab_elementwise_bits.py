"""Bits of the map kernels (csrc/nk_ew.h: the activations, add, concat / split, resamplers and pools of elementwise.hip and gan.hip, and the
BatchNorm apply / dx passes) under two builds of the library: a sha256 of every output of every entry point over a fixed case list, from each
build in a fresh child process of its own (NEUROSIS_HIP_LIB selects the library), and a table with one row per case.  No tolerance: exit
status 0 only if every row is equal.

    python tools/ab_elementwise_bits.py --a PARENT/neurosis_amd/csrc/libneurosis_hip.so --b neurosis_amd/csrc/libneurosis_hip.so --out profiles/elementwise_refactor_bits.txt

Inputs are cut from one pool drawn from a seeded CPU generator: normal values with zeros of both signs among them; the pooling inputs are
half-integers, so that every window holds ties.  Each child runs under its own time limit; if the first one fails or runs out of time the
second is not started."""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FLAT_N = [8, 8 * 257, 8 * (8192 * 256 + 257)]      # the last: past the grid cap, the stride loop runs and ends ragged
ROWS_CASES = [(1, 8), (3, 8), (257, 24), (300, 2560)]
CAT_CASES = [(70, 320, 640), (5, 8, 8)]
PIXEL_CASES = [(2, 8, 7, 10), (1, 320, 16, 16), (2, 64, 5, 5), (1, 8, 2, 2), (2, 8, 6, 10)]      # (N, C, H, W); the first three: RS_SHAPES of tests/test_adm_gpu.py
MAXPOOL32_CASES = [(1, 8, 3, 3), (2, 16, 7, 9)]      # k = 3, s = 2
BN_CASES = [(65, 8), (4096, 64)]


def child() -> None:
    import torch

    from neurosis_amd import ops

    BF16 = torch.bfloat16
    pool = torch.randn(1 << 24, generator=torch.Generator(device="cpu").manual_seed(20241020))
    pool[::5] = 0.0
    pool[3::10] = -0.0
    pool = pool.cuda()
    taken = [0]

    def cut(n):
        start = taken[0] % pool.numel()
        taken[0] += 7919 + n
        return pool[(torch.arange(n, device="cuda") + start) % pool.numel()]

    def rnd(*shape, scale=2.0):
        """bf16 normal values cut from the pool (wrapping around), a different cut per call"""
        n = 1
        for s in shape:
            n *= s
        return (cut(n) * scale).view(*shape).to(BF16)

    def half_ints(*shape):
        n = 1
        for s in shape:
            n *= s
        return ((cut(n) * 2).round().clamp(-4, 4) / 2).view(*shape).to(BF16)

    def emit(case, **outs):
        torch.cuda.synchronize()
        for k, t in outs.items():
            raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
            print(f"ROW {case} {k} {hashlib.sha256(raw).hexdigest()}", flush=True)

    st = ops._stream
    p = lambda t: None if t is None else t.data_ptr()

    def run(name, dst_shape, dst_pos, *args):
        """entry point `name` with a fresh destination as argument `dst_pos`; tensors go in as pointers"""
        dst = torch.full(dst_shape, float("nan"), dtype=BF16, device="cuda")
        a = [p(v) if torch.is_tensor(v) or v is None else v for v in args]
        ops.call(name, *a[:dst_pos], p(dst), *a[dst_pos:], st())
        return dst

    for n in FLAT_N:
        x, dy, b = rnd(n), rnd(n), rnd(n)
        outs = dict(silu_fwd=run("nk_silu_fwd", (n,), 1, x, n), silu_bwd=run("nk_silu_bwd", (n,), 2, dy, x, n), add=run("nk_add", (n,), 2, x, b, n))
        for mode in range(4):
            outs[f"gelu_fwd{mode}"] = run("nk_gelu_fwd", (n,), 1, x, n, mode)
        for mode in range(2):
            outs[f"gelu_bwd{mode}"] = run("nk_gelu_bwd", (n,), 2, dy, x, n, mode)
        for slope in (0.2, 0.25, 0.0):
            y = run("nk_leaky_relu_fwd", (n,), 1, x, n, slope)
            outs[f"leaky_fwd{slope:g}"], outs[f"leaky_bwd{slope:g}"] = y, run("nk_leaky_relu_bwd", (n,), 2, dy, y, n, slope)
        emit(f"flat-{n}", **outs)
        del x, dy, b, outs, y
        torch.cuda.empty_cache()

    for M, I in ROWS_CASES:
        u, dy = rnd(M, 2 * I), rnd(M, I)
        s = torch.empty_like(u)
        y_s = run("nk_geglu_fwd_s", (M, I), 1, u, s, M, I)
        u_in_place = u.clone()
        y_in_place = run("nk_geglu_fwd_s", (M, I), 1, u_in_place, u_in_place, M, I)
        emit(f"rows-{M}x{I}", geglu_fwd=run("nk_geglu_fwd", (M, I), 1, u, M, I), geglu_bwd=run("nk_geglu_bwd", (M, 2 * I), 2, dy, u, M, I),
             geglu_fwd_s_y=y_s, geglu_fwd_s_s=s, geglu_fwd_s_in_place_y=y_in_place, geglu_fwd_s_in_place_s=u_in_place,
             geglu_bwd_s=run("nk_geglu_bwd_s", (M, 2 * I), 2, dy, s, M, I), gated_gelu_tanh=run("nk_gated_gelu_tanh_fwd", (M, I), 1, u, M, I))

    for rows, Ca, Cb in CAT_CASES:
        a, b = rnd(rows, Ca), rnd(rows, Cb)
        out = run("nk_cat_channels", (rows, Ca + Cb), 2, a, b, rows, Ca, Cb)
        sb = torch.empty_like(b)
        emit(f"cat-{rows}x{Ca}+{Cb}", cat=out, split_a=run("nk_split_channels", (rows, Ca), 1, out, sb, rows, Ca, Cb), split_b=sb,
             split_a_alone=run("nk_split_channels", (rows, Ca), 1, out, None, rows, Ca, Cb),
             split_b_alone=run("nk_split_channels", (rows, Cb), 2, out, None, rows, Ca, Cb))

    def maxpool(N, C, H, W, k, s, outs):
        Ho, Wo = (H - k) // s + 1, (W - k) // s + 1
        x, dy = half_ints(N * H * W, C), rnd(N * Ho * Wo, C)
        outs[f"maxpool{k}{s}_fwd"] = run("nk_maxpool_fwd", (N * Ho * Wo, C), 1, x, N, H, W, C, k, s)
        outs[f"maxpool{k}{s}_bwd"] = run("nk_maxpool_bwd", (N * H * W, C), 2, dy, x, N, H, W, C, k, s)
        if k == 2 and H % 2 == 0 and W % 2 == 0:
            outs["maxpool2x2_fwd"] = run("nk_maxpool2x2_fwd", (N * Ho * Wo, C), 1, x, N, H, W, C)
            outs["maxpool2x2_bwd"] = run("nk_maxpool2x2_bwd", (N * H * W, C), 2, dy, x, N, H, W, C)

    for N, C, H, W in PIXEL_CASES:
        x, dy, dup = rnd(N * H * W, C), rnd(N * (H // 2) * (W // 2), C), rnd(N * 4 * H * W, C)
        outs = dict(up_fwd=run("nk_upsample2x_fwd", (N * 4 * H * W, C), 1, x, N, H, W, C), up_bwd=run("nk_upsample2x_bwd", (N * H * W, C), 1, dup, N, H, W, C),
                    avg_fwd=run("nk_avgpool2x_fwd", (N * (H // 2) * (W // 2), C), 1, x, N, H, W, C), avg_bwd=run("nk_avgpool2x_bwd", (N * H * W, C), 1, dy, N, H, W, C))
        maxpool(N, C, H, W, 2, 2, outs)
        if H >= 3 and W >= 3:
            maxpool(N, C, H, W, 3, 2, outs)
        emit(f"pixels-{N}x{C}x{H}x{W}", **outs)
    for N, C, H, W in MAXPOOL32_CASES:
        outs = {}
        maxpool(N, C, H, W, 3, 2, outs)
        emit(f"maxpool32-{N}x{C}x{H}x{W}", **outs)

    for M, C in BN_CASES:
        for slope in (0.2, 1.0):
            x, dy = rnd(M, C, scale=1.0) + 0.25, rnd(M, C, scale=1.0)
            gamma, beta = cut(C) * 0.2 + 1.0, cut(C) * 0.3
            mean, rstd, dgamma, dbeta = (torch.empty(C, device="cuda") for _ in range(4))
            ws = torch.empty(ops.query("nk_batchnorm_ws_floats", M, C), device="cuda")
            y = run("nk_batchnorm_fwd", (M, C), 3, x, gamma, beta, mean, rstd, None, None, ws, M, C, 1e-5, 0.1, slope)
            dx = run("nk_batchnorm_bwd", (M, C), 6, dy, x, y, gamma, mean, rstd, dgamma, dbeta, ws, M, C, slope, 0)
            rstd_eval = torch.empty(C, device="cuda")
            y_eval = run("nk_batchnorm_eval", (M, C), 5, x, gamma, beta, mean, rstd.reciprocal().square(), rstd_eval, M, C, 1e-5, slope)
            emit(f"bn-{M}x{C}-slope{slope:g}", y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta, y_eval=y_eval)
    print("CHILD_DONE", flush=True)


def run_child(lib_path: str, limit: int) -> dict | None:
    env = dict(os.environ, NEUROSIS_HIP_LIB=str(Path(lib_path).resolve()))
    try:
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"{lib_path}: no result within {limit} s", file=sys.stderr)
        return None
    if r.returncode != 0 or "CHILD_DONE" not in r.stdout:
        print(f"{lib_path}: exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}", file=sys.stderr)
        return None
    cases: dict = {}      # case -> {output: sha256}, in the order the child printed them
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            _, case, output, sha = line.split(" ")
            assert output not in cases.setdefault(case, {}), f"two outputs named {case} {output}: case ids must be unique"
            cases[case][output] = sha
    return cases


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--a", help="the library of the parent commit")
    ap.add_argument("--b", help="the library of this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=180, help="seconds per child")
    args = ap.parse_args()
    if args.child:
        child()
        return 0
    a = run_child(args.a, args.limit)
    if a is None:
        return 2      # the second child is not started
    b = run_child(args.b, args.limit)
    if b is None:
        return 2
    digest = lambda outs: hashlib.sha256("".join(f"{k} {v}\n" for k, v in outs.items()).encode()).hexdigest()
    rows = ["# per case: outputs, sha256 over their (name, sha256 of the bytes) list; a = the parent commit's build, b = this tree's", f"# {'case':<30} {'n':>3} {'a':<64} b"]
    differ = [k for k in a if a[k] != b.get(k)]
    for k in a:
        bad = [o for o in a[k] if a[k][o] != b.get(k, {}).get(o)]
        rows.append(f"{k:<32} {len(a[k]):>3} {digest(a[k])} " + ("equal" if a[k] == b.get(k) else f"DIFFERENT {digest(b.get(k, {}))}: " + ", ".join(bad)))
    n = sum(len(v) for v in a.values())
    rows.append(f"# {len(a)} cases, {n} outputs, {len(differ)} cases differ" + (": " + ", ".join(differ[:20]) if differ else "") + ("" if set(a) == set(b) else "; CASE SETS DIFFER"))
    text = "\n".join(rows) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    print(rows[-1])
    return 0 if not differ and set(a) == set(b) else 1


if __name__ == "__main__":
    sys.exit(main())
