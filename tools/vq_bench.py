"""ops.vq_search against the reference's formulation of the code search evaluated by torch in fp32 on the same card:

    d = sum(z^2, 1, keepdim) + sum(E^2, 1) - 2 * einsum("bd,dn->bn", z, E^T);  argmin(d, 1)        (three temporaries plus the argmin)

at VQ-f4 (N = 32768 latent vectors of 256^2 images at batch 8, n_e = 8192, D = 3) and VQ-f16 (N = 2048, n_e = 16384, D = 256).

    python tools/vq_bench.py [--rounds 15] [--reps 20]

Each round times both sides in a freshly shuffled order, `reps` launches between two device events after a warm-up of the shape; the
figures are medians over the rounds.  Peak device memory of a side is torch's allocator peak over one call, above what the inputs hold.
The last line is one JSON object.  At VQ-f4 the fused median must not exceed torch's (the torch side moves a GiB-sized matrix several
times, the fused side none): the tool exits non-zero otherwise.  At VQ-f16 the work is a 17-GFLOP fp32 GEMM and the vendor path a tuned
kernel on the same fp32 MFMA: both medians and the achieved TFLOP/s against the 157 TFLOP/s fp32-matrix peak are reported only."""
import argparse
import json
import random
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

SHAPES = {"vq_f4": (32768, 8192, 3), "vq_f16": (2048, 16384, 256)}
FP32_MATRIX_PEAK_TFLOPS = 157.0


def torch_search(z, E):
    d = torch.sum(z ** 2, dim=1, keepdim=True) + torch.sum(E ** 2, dim=1) - 2 * torch.einsum("bd,dn->bn", z, E.t())
    return torch.argmin(d, dim=1)


def main() -> int:
    from neurosis_amd import ops

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vq_bench: needs a GPU; nothing is measured without one")
    rng = random.Random(0)
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps}
    ok = True
    for name, (N, n_e, D) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(N + D)
        E = torch.randn(n_e, D, device="cuda", generator=g)
        z = E[torch.randint(0, n_e, (N,), device="cuda", generator=g)] + 0.3 * torch.randn(N, D, device="cuda", generator=g)
        sides = {"fused": lambda: ops.vq_search(z, E), "torch": lambda: torch_search(z, E)}
        peak, idx = {}, {}
        for side, fn in sides.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            idx[side] = fn()
            torch.cuda.synchronize()
            peak[side] = torch.cuda.max_memory_allocated() - base
        times = {side: [] for side in sides}
        for _ in range(args.rounds):
            order = list(sides)
            rng.shuffle(order)
            for side in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    sides[side]()
                e1.record()
                torch.cuda.synchronize()
                times[side].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        med = {side: statistics.median(t) for side, t in times.items()}
        flop = 2.0 * N * n_e * D
        res = {"N": N, "n_e": n_e, "D": D, "fused_us": round(med["fused"], 1), "torch_us": round(med["torch"], 1),
               "fused_min_max_us": [round(min(times["fused"]), 1), round(max(times["fused"]), 1)],
               "torch_min_max_us": [round(min(times["torch"]), 1), round(max(times["torch"]), 1)],
               "fused_tflops": round(flop / med["fused"] * 1e-6, 2), "torch_tflops": round(flop / med["torch"] * 1e-6, 2),
               "fused_share_of_fp32_matrix_peak": round(flop / med["fused"] * 1e-6 / FP32_MATRIX_PEAK_TFLOPS, 3),
               "fused_peak_bytes": int(peak["fused"]), "torch_peak_bytes": int(peak["torch"]),
               "rows_where_the_two_sides_differ": int((idx["fused"] != idx["torch"]).sum())}
        print(f"{name}: fused {res['fused_us']} us, torch {res['torch_us']} us (medians of {args.rounds} x {args.reps} launches); peak memory "
              f"fused {peak['fused'] / 2 ** 20:.1f} MiB, torch {peak['torch'] / 2 ** 20:.1f} MiB")
        out[name] = res
    if out["vq_f4"]["fused_us"] > out["vq_f4"]["torch_us"]:
        print("vq_bench: the fused search is SLOWER than the torch formulation at VQ-f4")
        ok = False
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
