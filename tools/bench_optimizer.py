"""The fused Adafactor update ALONE on the chip (nothing beside it), against its stream time in the step (beside the next step's frozen VAE
encoder): stream time, launches and effective TB/s over the bytes it touches (22 B/param: g read three times, p read + written, bf16 shadow
written; 14 B/param if the chunk's second and third reads of g come out of the Infinity Cache).  With --beta1 B the update keeps the first moment
(FlatAdafactorMomentum): exp_avg read and written in the apply pass, 30 and 22 B/param.   usage (GPU box): python tools/bench_optimizer.py [--beta1 0.9]"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench

ap = argparse.ArgumentParser()
ap.add_argument("--beta1", type=float, default=None)
beta1 = ap.parse_args().beta1
dev = torch.device("cuda", 0)
eng = bench.build_engine(dev, (1024, 1024), None)
eng.configure_adafactor(scale_parameter=True, relative_step=True, warmup_init=True, beta1=beta1)
touched, hbm = (22, 14) if beta1 is None else (30, 22)
eng.overlap_optimizer = False                      # in line on the current stream: what is timed is the update itself
eng.store.grad.normal_(0, 1e-3)
n = eng.store.grad.numel()
for chunk_mb in (os.environ.get("NK_AF_CHUNK_MB", "default"),):
    for _ in range(2):
        eng.optimizer_step(lr=1e-6, weight_decay=1e-2, grad_scale=1.0, dp=None)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(5):
        eng.optimizer_step(lr=1e-6, weight_decay=1e-2, grad_scale=1.0, dp=None)
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / 5
    print(f"Adafactor{'' if beta1 is None else f' (beta1 {beta1})'} alone, chunk {chunk_mb} MB: {ms:.2f} ms per update of {n / 1e9:.3f} G parameters = "
          f"{touched * n / ms / 1e9:.2f} TB/s over {touched} B/param touched, {hbm * n / ms / 1e9:.2f} TB/s over {hbm} B/param (HBM floor at 8 TB/s: {hbm * n / 8e9:.2f} ms)")
