"""The frozen T5 encoder tower alone, at T5-v1.1-XL and -XXL shapes with random weights (no files), batch 4, 77 and 256 tokens.

    python tools/bench_t5.py [--models xl,xxl] [--lengths 77,256] [--out FILE.json]
        ms per call: median of RUNS device-event timings after WARM calls, launched from Python (NK_GRAPH=0) and replayed from a hipGraph
        (NK_GRAPH=te), the algorithmic FLOPs of a call and the whole-call rate (an end-to-end figure, not a kernel's).

    rocprofv3 --kernel-trace --stats -d OUT -o t5 -- python tools/bench_t5.py --subject xxl 256
    python tools/bench_t5.py --db OUT/t5_results.db xxl 256
        the per-kernel split of one call from a kernel trace taken in a run of its own (one stream, launched from Python: the kernels run
        one after the other): ms per call by kernel, the GEMMs' achieved TFLOP/s (their FLOPs from the shapes over their kernel time) and
        the share of the three T5 kernels (rms_fwd_kernel, attn_fwd_kernel<relbias>, nk_ew_rows_kernel<GatedGeluTanh>).  The subject runs 1 + CALLS
        calls; the split is taken from the first RMSNorm launch of the second call on (weight preparation happens in the first), so the
        second call's embedding gather and cast, two launches of a few microseconds, are left out.

Memory: the tower keeps fp32 parameters and one bf16 copy of every matrix, 6 bytes per parameter: ~28 GB at XXL."""
import argparse
import json
import os
import sqlite3
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = {
    "xl": dict(vocab_size=32128, d_model=2048, d_kv=64, d_ff=5120, num_layers=24, num_heads=32, feed_forward_proj="gated-gelu"),
    "xxl": dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu"),
}
BATCH, WARM, RUNS, CALLS = 4, 3, 15, 5
NEW_KERNELS = ("rms_fwd_kernel", "attn_fwd_kernel", "GatedGeluTanh")


def flops(cfg: dict, B: int, L: int) -> dict:
    inner, d, ff = cfg["num_heads"] * cfg["d_kv"], cfg["d_model"], cfg["d_ff"]
    gated = cfg["feed_forward_proj"].startswith("gated-")
    gemm = 2 * B * L * (3 * d * inner + inner * d + (2 if gated else 1) * d * ff + ff * d) * cfg["num_layers"]
    attn = 4 * B * cfg["num_heads"] * L * L * cfg["d_kv"] * cfg["num_layers"]
    return {"gemm": gemm, "attention": attn}


def build(name: str):
    import torch

    from neurosis_amd.models.text_encoder import T5EncoderTower

    with torch.device("meta"):
        tower = T5EncoderTower(**SHAPES[name])
    tower = tower.to_empty(device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for key, p in tower.named_parameters():
            if key.endswith("layer_norm.weight"):
                p.fill_(1.0)
            elif key.endswith("relative_attention_bias.weight"):
                p.normal_(0.0, 1.0, generator=g)
            elif key == "shared.weight":
                p.normal_(0.0, 1.0, generator=g)
            else:
                p.normal_(0.0, p.shape[1] ** -0.5, generator=g)
    return tower.eval().requires_grad_(False)


def ids_for(name: str, L: int, seed: int):
    import torch

    return torch.randint(0, SHAPES[name]["vocab_size"], (BATCH, L), generator=torch.Generator().manual_seed(seed)).cuda()


def time_calls(tower, name: str, L: int) -> float:
    import torch

    for i in range(WARM):
        tower(ids_for(name, L, i))
    torch.cuda.synchronize()
    times = []
    for i in range(RUNS):
        ids = ids_for(name, L, 100 + i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        tower(ids)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def run(models, lengths, out):
    import torch

    assert torch.cuda.is_available(), "bench_t5 needs a GPU"
    rows = []
    for name in models:
        tower = build(name)
        params = sum(p.numel() for p in tower.parameters())
        for L in lengths:
            f = flops(SHAPES[name], BATCH, L)
            row = {"model": name, "B": BATCH, "L": L, "parameters": params, "gflop": {k: v / 1e9 for k, v in f.items()}}
            for mode, graph in (("eager", "0"), ("replay", "te")):
                os.environ["NK_GRAPH"] = graph
                ms = time_calls(tower, name, L)
                row[f"{mode}_ms"] = round(ms, 3)
                row[f"{mode}_whole_call_tflops"] = round(sum(f.values()) / ms / 1e9, 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
        print(f"{name}: {params / 1e9:.2f} B parameters, torch allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB at peak", flush=True)
        del tower
        torch.cuda.empty_cache()
    if out:
        Path(out).write_text(json.dumps(rows, indent=1))


def subject(name: str, L: int):
    import torch

    os.environ["NK_GRAPH"] = "0"
    tower = build(name)
    for i in range(1 + CALLS):
        tower(ids_for(name, L, i))
        torch.cuda.synchronize()


def split(db: str, name: str, L: int):
    con = sqlite3.connect(db)
    rows = con.execute("select name, start, end from kernels order by start").fetchall()
    rms = [i for i, r in enumerate(rows) if "rms_fwd_kernel" in r[0]]
    per_call = 2 * SHAPES[name]["num_layers"] + 1
    assert len(rms) == per_call * (1 + CALLS), (len(rms), per_call)
    rows = rows[rms[per_call]:]
    by = {}
    for n, s, e in rows:
        c = by.setdefault(n, [0, 0])
        c[0] += 1
        c[1] += e - s
    total = sum(t for _, t in by.values())
    f = flops(SHAPES[name], BATCH, L)
    gemm = sum(t for n, (_, t) in by.items() if "gemm" in n.lower())
    new = {k: sum(t for n, (_, t) in by.items() if k in n) for k in NEW_KERNELS}
    print(f"T5-v1.1-{name.upper()} encoder, B = {BATCH}, L = {L}: kernel time {total / CALLS / 1e6:.3f} ms per call over {CALLS} calls ({len(rows) // CALLS} launches per call)")
    for n, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1])[:14]:
        print(f"  {n[:88]:88s} {c // CALLS:5d} x {t / c / 1e3:9.1f} us  {t / CALLS / 1e6:8.3f} ms  {100 * t / total:5.1f} %")
    print(f"  GEMMs: {gemm / CALLS / 1e6:.3f} ms per call, {f['gemm'] / 1e9:.0f} GFLOP -> {f['gemm'] * CALLS / gemm / 1e3:.0f} TFLOP/s achieved")
    att = new["attn_fwd_kernel"]
    print(f"  attention (relative bias): {att / CALLS / 1e6:.3f} ms per call, {f['attention'] / 1e9:.1f} GFLOP -> {f['attention'] * CALLS / max(att, 1) / 1e3:.0f} TFLOP/s")
    print("  the three T5 kernels: " + ", ".join(f"{k} {100 * t / total:.1f} %" for k, t in new.items()) + f"; together {100 * sum(new.values()) / total:.1f} % of the tower")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="xl,xxl")
    ap.add_argument("--lengths", default="77,256")
    ap.add_argument("--out")
    ap.add_argument("--subject", nargs=2, metavar=("MODEL", "L"))
    ap.add_argument("--db", nargs=3, metavar=("DB", "MODEL", "L"))
    a = ap.parse_args()
    if a.subject:
        subject(a.subject[0], int(a.subject[1]))
    elif a.db:
        split(a.db[0], a.db[1], int(a.db[2]))
    else:
        run(a.models.split(","), [int(x) for x in a.lengths.split(",")], a.out)


if __name__ == "__main__":
    main()
