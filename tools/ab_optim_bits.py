"""Bits of the fused Adafactor and CAME updates (csrc/optim.hip, csrc/came.hip) under two builds of the library: a sha256 of `store.master`,
`store.shadow` and `opt.state` after every step of every case, from each build in a fresh child process of its own (NEUROSIS_HIP_LIB selects
the library), and a table with one row per case: the number of hashed tensors, a sha256 over their (name, sha256) list per build, and -- where
a case differs -- the tensors that do.  There is no tolerance: the exit status is 0 only if every row is equal.

    python tools/ab_optim_bits.py --a PARENT/neurosis_amd/csrc/libneurosis_hip.so --b neurosis_amd/csrc/libneurosis_hip.so --out profiles/optim_refactor_bits.txt

A case is (optimizer options) x (parameter set) x (chunk size); it runs three steps on normal-distributed gradients of magnitude 1, 10 and 0.1
(update clipping engages) drawn, like the parameters, from a seeded CPU generator.  The small set has every code path and every ragged edge
(vectors of one and two items; matrices with a ragged second row strip, nine column tiles the last 8 wide, four full strips; 1x1, 3x3 and
run-time-sized conv taps, one and two items) and runs with 8 KiB chunks and with the default chunk; the taps set is further run-time tap
sizes (2x2, 1x3, 3x2, 2x3); the real-size set is the shapes of
tests/test_came_gpu.py's fp64 comparison.  Adafactor's cases also hash `p2_part` before the first step (af_init_p2_kernel).  Each child runs
under its own time limit; if the first one fails or runs out of time the second is not started."""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SETS = {
    "small": [(7,), (96,), (1500,), (300, 128), (64, 520), (1024, 64), (48, 40, 1, 1), (32, 24, 3, 3), (40, 32, 3, 3), (16, 8, 3, 1)],
    "taps": [(16, 8, 2, 2), (8, 8, 1, 3), (8, 16, 3, 2), (24, 8, 2, 3)],      # run-time-sized conv taps with more than one column
    "real": [(1280, 1280), (10240, 1280), (640, 2048), (320, 320, 3, 3), (4, 320, 3, 3), (1280,), (5,), (1000, 1284)],
}
CHUNKS = {"small": (("8k", 8 << 10), ("default", None)), "taps": (("default", None),), "real": (("default", None),)}
_MANUAL = dict(lr=1e-3, scale_parameter=False, relative_step=False, weight_decay=1e-2)      # the "manual" tag of tests/golden/adafactor_steps
AF_OPTIONS = [     # (name, constructor arguments, grad_scale, NK_AF_STREAMS)
    ("relative", dict(scale_parameter=True, relative_step=True, warmup_init=True), 1.0, "1"),      # the "relative" tag
    ("manual", _MANUAL, 1.0, "1"),
    ("manual-gs0.25-streams1", _MANUAL, 0.25, "1"),
    ("manual-gs0.25-streams2", _MANUAL, 0.25, "2"),
]
_FIXED = dict(lr=1e-3, weight_decay=1e-3, fixed_decay=True, clip_threshold=0.5, betas=(0.8, 0.99, 0.999))      # tags of tests/golden/came_steps
CAME_OPTIONS = [("default", dict(lr=1e-3), 1.0), ("decay", dict(lr=1e-3, weight_decay=1e-2), 1.0), ("fixed", _FIXED, 1.0), ("fixed-gs0.25", _FIXED, 0.25)]
MAGNITUDES = (1.0, 10.0, 0.1)


def child() -> None:
    import torch

    from neurosis_amd.nn import FlatParamStore
    from neurosis_amd.optim import FlatAdafactor, FlatCAME

    def emit(case, name, t):
        raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
        print(f"ROW {case} {name} {hashlib.sha256(raw).hexdigest()}", flush=True)

    def run(case, make_opt, init, grads, grad_scale):
        # conv weights live channels-last (the store's physical layout is [O][KH][KW][I])
        params = [torch.nn.Parameter(t.clone().cuda().contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.clone().cuda()) for t in init]
        store = FlatParamStore(params)
        opt = make_opt(store)
        if isinstance(opt, FlatAdafactor):
            opt.refresh_param_norms()
            torch.cuda.synchronize()
            emit(case, "init.p2_part", opt.p2_part)
        for s, gs in enumerate(grads):
            for p, g in zip(params, gs):
                p.grad.copy_(g.cuda())
            opt.step(grad_scale=grad_scale)
            torch.cuda.synchronize()
            for name, t in (("master", store.master), ("shadow", store.shadow), ("state", opt.state)):
                emit(case, f"step{s + 1}.{name}", t)

    for set_name, shapes in SETS.items():
        g = torch.Generator(device="cpu").manual_seed(20240917)
        init = [torch.randn(*s, generator=g) * 0.05 for s in shapes]
        grads = [[torch.randn(*s, generator=g) * mag for s in shapes] for mag in MAGNITUDES]
        for chunk_name, chunk_bytes in CHUNKS[set_name]:
            for name, kw, grad_scale, streams in AF_OPTIONS:
                os.environ["NK_AF_STREAMS"] = streams      # (read by the constructor)
                run(f"adafactor-{name}-{set_name}-chunk{chunk_name}", lambda st: FlatAdafactor(st, chunk_bytes=chunk_bytes, **kw), init, grads, grad_scale)
            for name, kw, grad_scale in CAME_OPTIONS:
                run(f"came-{name}-{set_name}-chunk{chunk_name}", lambda st: FlatCAME(st, chunk_bytes=chunk_bytes, **kw), init, grads, grad_scale)
        torch.cuda.empty_cache()
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
    cases: dict = {}      # case -> {tensor: sha256}, in the order the child printed them
    for line in r.stdout.splitlines():
        if line.startswith("ROW "):
            _, case, output, sha = line.split(" ")
            assert output not in cases.setdefault(case, {}), f"two tensors named {case} {output}: case ids must be unique"
            cases[case][output] = sha
    return cases


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--a", help="the library of the parent commit")
    ap.add_argument("--b", help="the library of this tree")
    ap.add_argument("--a-name", default=None, help="what the table calls build a (a commit), instead of its path")
    ap.add_argument("--b-name", default=None)
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
    digest = lambda outs: hashlib.sha256("".join(f"{k} {v}\n" for k, v in outs.items()).encode()).hexdigest()
    rows = [f"# per case: hashed tensors (master, shadow, state after each of {len(MAGNITUDES)} steps; Adafactor: and p2_part before the first), sha256 over their",
            f"# (name, sha256 of the bytes) list; a = {args.a_name or args.a}, b = {args.b_name or args.b}", f"# {'case':<46} {'n':>3} {'a':<64} b"]
    differ = [k for k in a if a[k] != b.get(k)]
    for k in a:
        bad = [o for o in a[k] if a[k][o] != b.get(k, {}).get(o)]
        rows.append(f"{k:<48} {len(a[k]):>3} {digest(a[k])} " + ("equal" if a[k] == b.get(k) else f"DIFFERENT {digest(b.get(k, {}))}: " + ", ".join(bad)))
    n = sum(len(v) for v in a.values())
    rows.append(f"# {len(a)} cases, {n} hashed tensors, {len(differ)} cases differ" + (": " + ", ".join(differ[:20]) if differ else "") + ("" if set(a) == set(b) else "; CASE SETS DIFFER"))
    text = "\n".join(rows) + "\n"
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    print(rows[-1])
    return 0 if not differ and set(a) == set(b) else 1


if __name__ == "__main__":
    sys.exit(main())
