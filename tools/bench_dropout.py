"""nk_dropout in place against nk_silu_fwd in place -- the same traffic, 2 B read + 2 B written per element -- at [65536, 320] and
[16384, 5120], in one process.  Kernel times come from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -o dropout -- python tools/bench_dropout.py
    python tools/bench_dropout.py --db OUT/dropout_results.db        # both rates and their ratio, per shape

Without a trace the run prints device-event times of the same launches (they include the launch gaps)."""
import sqlite3
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = [(65536, 320), (16384, 5120)]
WARM, N = 5, 50


def run():
    import torch

    from neurosis_amd import ops
    from neurosis_amd.lib import call

    ops.dropout_seed(1)
    tok = ops.dropout_draw()
    for rows, cols in SHAPES:
        x = torch.randn(rows, cols, device="cuda").to(torch.bfloat16)
        res = {}
        for name, launch in (("dropout", lambda: ops.dropout_mask_like(x, 0.1, 0, tok)),
                             ("silu", lambda: call("nk_silu_fwd", x.data_ptr(), x.data_ptr(), x.numel(), ops._stream()))):
            for _ in range(WARM):
                launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N):
                launch()
            e1.record()
            torch.cuda.synchronize()
            res[name] = e0.elapsed_time(e1) * 1e3 / N
        gb = 4e-3 * rows * cols
        print(f"[{rows}, {cols}] device events: nk_dropout {res['dropout']:.1f} us ({gb / res['dropout']:.0f} GB/s), "
              f"nk_silu_fwd {res['silu']:.1f} us ({gb / res['silu']:.0f} GB/s), ratio {res['dropout'] / res['silu']:.2f}")


def report(db_path: str):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, end - start from kernels order by start").fetchall()
    by = {"dropout": [d for n, d in rows if "dropout_kernel" in n], "silu": [d for n, d in rows if "SiluFwd" in n]}
    for k, v in by.items():
        assert len(v) == len(SHAPES) * (WARM + N), (k, len(v))
    for i, (r, c) in enumerate(SHAPES):
        us = {k: statistics.median(v[i * (WARM + N) + WARM:(i + 1) * (WARM + N)]) / 1e3 for k, v in by.items()}
        gb = 4e-3 * r * c
        print(f"[{r}, {c}] kernel trace (median of {N}): nk_dropout {us['dropout']:.1f} us = {gb / us['dropout']:.0f} GB/s, "
              f"nk_silu_fwd {us['silu']:.1f} us = {gb / us['silu']:.0f} GB/s, ratio {us['dropout'] / us['silu']:.2f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--db":
        report(sys.argv[2])
    else:
        run()
