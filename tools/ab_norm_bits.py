"""Bits of the normalisation and column-sum kernels under two builds of the library: a sha256 of every output tensor of every case, from
each build in a fresh child process of its own (NEUROSIS_HIP_LIB selects the library), and a table with one row per case: the number of
output tensors, a sha256 over their (name, sha256) list per build, and -- where a case differs -- the outputs that do.

    python tools/ab_norm_bits.py --a PARENT/neurosis_amd/csrc/libneurosis_hip.so --b neurosis_amd/csrc/libneurosis_hip.so --out profiles/norm_refactor_bits.txt

Cases: the real sizes of tests/test_norm_reductions_gpu.py -- GroupNorm (plain, modulated, from sums), LayerNorm (one-pass and three-kernel
backward, with and without dx_add) and BatchNorm -- RMSNorm, the batched column sums, and the small shapes of tests/test_norm_reduce_gpu.py,
all on normal-distributed inputs cut from one pool drawn from a seeded CPU generator.  Each child runs under its own time limit; if the
first one fails or runs out of time the second is not started."""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GN_CASES = [   # tests/test_norm_reductions_gpu.py: (N, H, W, C, G, eps, silu, dx_add, accumulate)
    (4, 128, 128, 320, 32, 1e-5, True, True, False), (4, 64, 64, 640, 32, 1e-5, True, False, True), (4, 32, 32, 1280, 32, 1e-5, True, True, False),
    (4, 32, 32, 2560, 32, 1e-5, True, True, True), (4, 64, 64, 1920, 32, 1e-5, True, True, False), (4, 128, 128, 960, 32, 1e-5, True, False, False),
    (4, 64, 64, 640, 32, 1e-6, False, True, False), (4, 32, 32, 1280, 32, 1e-6, False, False, True), (1, 1024, 1024, 128, 32, 1e-6, True, True, False),
    (4, 512, 512, 256, 32, 1e-6, True, True, False), (4, 256, 256, 512, 32, 1e-6, True, False, False), (4, 104, 152, 320, 32, 1e-5, True, True, False),
    (1, 832, 1216, 128, 32, 1e-6, True, True, False), (32, 256, 256, 128, 32, 1e-6, True, True, True), (2, 32, 32, 2304, 3, 1e-5, True, True, False),
    (4, 64, 64, 320, 1, 1e-5, True, True, False), (2, 32, 32, 4096, 32, 1e-5, False, True, False),
    # tests/test_norm_reduce_gpu.py
    (1, 32, 1, 8, 1, 1e-5, True, True, False), (2, 1056, 1, 72, 3, 1e-5, True, True, True), (3, 64, 1, 2304, 3, 1e-5, False, True, False),
]
LN_CASES = [(16384, 640), (4096, 1280), (308, 768), (308, 1280), (4100, 520), (1000, 1032), (2048, 2048)] + [(m, c) for m in (1, 63, 65, 1093) for c in (8, 72, 136)]
BN_CASES = [(131072, 128), (32768, 256), (30752, 512)]
RMS_CASES = [(1, 64), (3, 1472), (77, 128), (130, 4096), (4096, 1024), (64, 1032), (64, 2056)]
COLSUM_CASES = [(1000, 320, 4), (16384, 320, 4), (5000, 2560, 1), (131073, 128, 1)] + [(m, n, b) for m in (1, 63, 64, 65, 1093) for n in (8, 72, 136) for b in (1, 3)]
PARTS_CASES = [(2, n, g) for n in (1, 7, 8, 9, 128, 129, 300, 4096) for g in (1, 32)]
COLPART_CASES = [(rows, c) for rows in (1, 31, 32, 33, 67, 512) for c in (8, 24, 40, 1280)]


def child() -> None:
    import torch

    from neurosis_amd import ops
    from neurosis_amd.lib import NkColpartBatch

    BF16 = torch.bfloat16
    pool = torch.randn(1 << 24, generator=torch.Generator(device="cpu").manual_seed(20240611)).cuda()
    taken = [0]

    def rnd(*shape, dtype=torch.float32, scale=1.0, shift=0.0):
        """normal values cut from the pool (wrapping around), a different cut per call"""
        n = 1
        for s in shape:
            n *= s
        start = taken[0] % pool.numel()
        taken[0] += 7919 + n
        idx = (torch.arange(n, device="cuda") + start) % pool.numel()
        return (pool[idx] * scale + shift).view(*shape).to(dtype)

    def emit(case, variant, **outs):
        torch.cuda.synchronize()
        for k, t in outs.items():
            raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
            print(f"ROW {case} {variant}.{k} {hashlib.sha256(raw).hexdigest()}", flush=True)

    st = ops._stream
    p = lambda t: None if t is None else t.data_ptr()
    for N, H, W, Cc, G, eps, silu, dx_add, acc in GN_CASES:
        HW = H * W
        case = f"gn-N{N}-{H}x{W}-C{Cc}-G{G}-eps{eps:g}-{'silu' if silu else 'linear'}"      # (two shapes of the list come with both)
        x, dy = rnd(N * HW, Cc, dtype=BF16, shift=0.25), rnd(N * HW, Cc, dtype=BF16)
        add = rnd(N * HW, Cc, dtype=BF16) if dx_add else None
        gamma, beta, mod = rnd(Cc, scale=0.5, shift=1.0), rnd(Cc, scale=0.1), rnd(N, 2 * Cc, dtype=BF16, scale=0.3)
        ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, Cc, G), x.device)
        tail = (N, HW, Cc, G)
        for tag, m in (("plain", None), ("mod", mod)):
            mp = () if m is None else (p(m),)
            y, y2, dx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            mean, rstd, mean2, rstd2 = (torch.empty(N, G, device="cuda") for _ in range(4))
            sums = torch.empty(N, 2 * G, device="cuda")
            dg, db = rnd(Cc), rnd(Cc)
            ops.call("nk_groupnorm_fwd" if m is None else "nk_groupnorm_mod_fwd", p(x), p(gamma), p(beta), *mp, p(y), p(mean), p(rstd), p(ws), *tail, eps, int(silu), st())
            ops.call("nk_groupnorm_sums", p(x), p(sums), p(ws), *tail, st())
            ops.call("nk_groupnorm_apply" if m is None else "nk_groupnorm_mod_apply", p(x), p(sums), p(gamma), p(beta), *mp, p(y2), p(mean2), p(rstd2), *tail, eps, int(silu), st())
            outs = dict(y=y, mean=mean, rstd=rstd, sums=sums, y_from_sums=y2, mean_from_sums=mean2, rstd_from_sums=rstd2)
            if m is None:
                ops.call("nk_groupnorm_bwd", p(dy), p(x), p(gamma), p(beta), p(mean), p(rstd), p(add), p(dx), p(dg), p(db), p(ws), *tail, int(silu), int(acc), st())
            else:
                outs["dmod"] = torch.empty_like(mod)
                ops.call("nk_groupnorm_mod_bwd", p(dy), p(x), p(gamma), p(beta), p(m), p(mean), p(rstd), p(add), p(dx), p(dg), p(db), p(outs["dmod"]), p(ws), *tail,
                         int(silu), int(acc), st())
            emit(case, tag, dx=dx, dgamma=dg, dbeta=db, **outs)
        del x, dy, add
        torch.cuda.empty_cache()

    for M, Cc in LN_CASES:
        x, dy, add = rnd(M, Cc, dtype=BF16, shift=0.25), rnd(M, Cc, dtype=BF16), rnd(M, Cc, dtype=BF16)
        gamma, beta = rnd(Cc, scale=0.5, shift=1.0), rnd(Cc, scale=0.1)
        y, mean, rstd = torch.empty_like(x), torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
        ops.call("nk_layernorm_fwd", p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), M, Cc, 1e-5, st())
        emit(f"ln-{M}x{Cc}", "fwd", y=y, mean=mean, rstd=rstd)
        ws = ops._ws(ops.query("nk_layernorm_ws_floats", M, Cc), x.device)
        rows = ops.query("nk_layernorm_part_rows", M)
        for tag, a in (("add", add), ("noadd", None)):
            for acc in (0, 1):
                # fused "1": dx and partial rows in one pass, the rows reduced by the batched reducer
                dx, dg, db = torch.empty_like(x), rnd(Cc), rnd(Cc)
                part = torch.empty(rows * 2 * Cc, device="cuda")
                ops.call("nk_layernorm_bwd_rows", p(dy), p(x), p(gamma), p(mean), p(rstd), p(a), p(dx), p(part), M, Cc, st())
                b = NkColpartBatch()
                b.n = 1
                b.part[0], b.dgamma[0], b.dbeta[0], b.nrows[0], b.C[0], b.accumulate[0] = p(part), p(dg), p(db), rows, Cc, acc
                ops.call("nk_colpart_reduce_batch", C.byref(b), st())
                emit(f"ln-{M}x{Cc}", f"fused1-{tag}-acc{acc}", dx=dx, dgamma=dg, dbeta=db)
                # fused "0": the three-kernel form
                dx, dg, db = torch.empty_like(x), rnd(Cc), rnd(Cc)
                ops.call("nk_layernorm_bwd_dx", p(dy), p(x), p(gamma), p(mean), p(rstd), p(a), p(dx), M, Cc, st())
                ops.call("nk_layernorm_bwd_params", p(dy), p(x), p(mean), p(rstd), p(dg), p(db), p(ws), M, Cc, acc, st())
                emit(f"ln-{M}x{Cc}", f"fused0-{tag}-acc{acc}", dx=dx, dgamma=dg, dbeta=db)
                # the one-call form
                dx, dg, db = torch.empty_like(x), rnd(Cc), rnd(Cc)
                ops.call("nk_layernorm_bwd", p(dy), p(x), p(gamma), p(mean), p(rstd), p(a), p(dx), p(dg), p(db), p(ws), M, Cc, acc, st())
                emit(f"ln-{M}x{Cc}", f"onecall-{tag}-acc{acc}", dx=dx, dgamma=dg, dbeta=db)

    for M, Cc in BN_CASES:
        for slope in (0.2, 1.0):
            x, dy = rnd(M, Cc, dtype=BF16, shift=0.25), rnd(M, Cc, dtype=BF16)
            w, b = torch.nn.Parameter(rnd(Cc, scale=0.2, shift=1.0)), torch.nn.Parameter(rnd(Cc, scale=0.3))
            rm, rv = rnd(Cc), rnd(Cc).abs() + 0.5
            y, bwd = ops.batchnorm_fwd(x, w, b, rm, rv, 1e-5, 0.1, slope)
            dx = bwd(dy)
            emit(f"bn-{M}x{Cc}", f"slope{slope:g}", y=y, rm=rm, rv=rv, dx=dx, dgamma=w.grad, dbeta=b.grad, y_eval=ops.batchnorm_eval(x, w, b, rm, rv, 1e-5, slope))

    for M, Cc in RMS_CASES:
        x, gamma = rnd(M, Cc, dtype=BF16, scale=3.0), rnd(Cc, scale=0.5, shift=1.0)
        emit(f"rms-{M}x{Cc}", "fwd", y=ops.rmsnorm(x, gamma, 1e-6))

    for M, Nn, nb in COLSUM_CASES:
        dy = rnd(nb * M, Nn, dtype=BF16)
        ws = torch.empty(nb * ops.query("nk_colsum_ws_floats", M, Nn), device="cuda")
        for acc in (0, 1):
            out = rnd(nb, Nn)
            ops.call("nk_colsum_batched", p(dy), p(out), p(ws), M, Nn, Nn, nb, acc, st())
            outs = {"batched": out}
            if nb == 1:
                outs["single"] = rnd(1, Nn)
                ops.call("nk_colsum", p(dy), p(outs["single"]), p(ws), M, Nn, Nn, acc, st())
            emit(f"colsum-{nb}x{M}x{Nn}", f"acc{acc}", **outs)

    for N, nparts, G in PARTS_CASES:
        part, sums = rnd(N, nparts, 2 * G), torch.empty(N, 2 * G, device="cuda")
        ws = ops._ws(ops.query("nk_groupnorm_sums_ws_floats", N, nparts, G), part.device)
        ops.call("nk_groupnorm_sums_from_parts", p(part), p(sums), p(ws), N, nparts, G, st())
        emit(f"parts-N{N}-{nparts}-G{G}", "sums", sums=sums)

    for acc in (0, 1):
        b = NkColpartBatch()
        b.n = len(COLPART_CASES)
        keep = []
        for z, (rows, Cc) in enumerate(COLPART_CASES):
            part, dg, db = rnd(rows, 2, Cc), rnd(Cc), rnd(Cc)
            keep.append((part, dg, db))
            b.part[z], b.dgamma[z], b.dbeta[z], b.nrows[z], b.C[z], b.accumulate[z] = p(part), p(dg), p(db), rows, Cc, acc
        ops.call("nk_colpart_reduce_batch", C.byref(b), st())
        for (rows, Cc), (_, dg, db) in zip(COLPART_CASES, keep):
            emit(f"colpart-{rows}x{Cc}", f"acc{acc}", dgamma=dg, dbeta=db)
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
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
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
    # one row per case: how many output tensors, and a sha256 over the lines "output sha256-of-the-tensor" of each build; a case that differs
    # lists the outputs that do
    digest = lambda outs: hashlib.sha256("".join(f"{k} {v}\n" for k, v in outs.items()).encode()).hexdigest()
    rows = [f"# per case: output tensors, sha256 over their (name, sha256 of the bytes) list; a = {args.a}, b = {args.b}", f"# {'case':<42} {'n':>3} {'a':<64} b"]
    differ = [k for k in a if a[k] != b.get(k)]
    for k in a:
        bad = [o for o in a[k] if a[k][o] != b.get(k, {}).get(o)]
        rows.append(f"{k:<44} {len(a[k]):>3} {digest(a[k])} " + ("equal" if a[k] == b.get(k) else f"DIFFERENT {digest(b.get(k, {}))}: " + ", ".join(bad)))
    n = sum(len(v) for v in a.values())
    rows.append(f"# {len(a)} cases, {n} output tensors, {len(differ)} cases differ" + (": " + ", ".join(differ[:20]) if differ else "") + ("" if set(a) == set(b) else "; CASE SETS DIFFER"))
    text = "\n".join(rows) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    print(rows[-1])
    return 0 if not differ and set(a) == set(b) else 1


if __name__ == "__main__":
    sys.exit(main())
