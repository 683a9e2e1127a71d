"""The banded resampler (csrc/resample.hip) as antialiased bicubic resize against torch-ROCm's own F.interpolate(mode="bicubic", antialias=True)
and its autograd backward, on the same tensors in the same process, alternating: forward, backward and their sum in microseconds (device
events, warm-up, 200 iterations a timing), and the resampler's GB/s over its algorithmic bytes (input + intermediate write and read + output)."""
import sys, torch
import os; sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch.nn.functional as F
from neurosis_amd import ops
from neurosis_amd.lib import query

ITERS = 200

def timeit(fn, iters=ITERS):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3      # us

def moved_bytes(P, H, W, OH, OW):
    return 4 * (P * H * W + 2 * query("nk_resample_ws_floats", P, H, W, OH, OW) + P * OH * OW)

print(f"{'shape':30s} {'round':>5s} | {'hip fwd':>9s} {'hip bwd':>9s} {'hip sum':>9s} | {'torch fwd':>9s} {'torch bwd':>9s} {'torch sum':>9s} | {'fwd GB/s':>8s} {'bwd GB/s':>8s}   (us)")
for (N, C, H, W), (OH, OW) in [((4, 3, 1024, 1024), (512, 512)), ((4, 3, 512, 512), (1024, 1024)), ((8, 3, 512, 512), (224, 224))]:
    torch.manual_seed(0)
    x = torch.rand(N, C, H, W, device="cuda") * 2 - 1
    dy = torch.rand(N, C, OH, OW, device="cuda") * 2 - 1
    _, bwd = ops.resize_bicubic_aa(x, (OH, OW))
    xt = x.clone().requires_grad_(True)
    yt = F.interpolate(xt, size=(OH, OW), mode="bicubic", antialias=True)
    assert float((ops.resize_bicubic_aa(x, (OH, OW))[0] - yt.detach()).abs().max()) < 1e-4       # the same operator
    assert float((bwd(dy) - torch.autograd.grad(yt, xt, dy, retain_graph=True)[0]).abs().max()) < 1e-3
    P = N * C
    for rnd in range(3):          # alternating rounds: a drift of the clocks shows as a drift of both
        hf = timeit(lambda: ops.resize_bicubic_aa(x, (OH, OW)))
        tf = timeit(lambda: F.interpolate(x, size=(OH, OW), mode="bicubic", antialias=True))
        hb = timeit(lambda: bwd(dy))
        tb = timeit(lambda: torch.autograd.grad(yt, xt, dy, retain_graph=True))
        print(f"{str((N, C, H, W)) + ' -> ' + str((OH, OW)):30s} {rnd:5d} | {hf:9.1f} {hb:9.1f} {hf + hb:9.1f} | {tf:9.1f} {tb:9.1f} {tf + tb:9.1f} | "
              f"{moved_bytes(P, H, W, OH, OW) / hf / 1e3:8.0f} {moved_bytes(P, OH, OW, H, W) / hb / 1e3:8.0f}", flush=True)
