"""Per-shape times of conv3x3(nearest_upsample_2x(x)) on the fused-upsample gather (nk_conv2d_fwd(upsample = 1), the flipped input gradient
with nk_upsample2x_bwd behind it, nk_conv2d_wgrad_bias) against the four 2 x 2 phase convolutions (nk_conv2d_up2_*), forward, input gradient
and weight gradient, for the UNet's two Upsample layers at the metric's batch.  One process, the two paths alternating launch by launch,
device events around every call, median over --iters.

    python tools/bench_up2_phases.py [--iters 30] [--plan]      (--plan: print the planned launches only; needs no GPU)
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from neurosis_amd import lib  # noqa: E402

# (N, H, W, Cin, Cout) of x: output_blocks' Upsample layers of the SDXL UNet at 1024 x 1024, batch 4
SHAPES = [(4, 32, 32, 1280, 1280), (4, 64, 64, 640, 640)]


def plan(shape):
    N, H, W, Ci, Co = shape
    d = lib.NkConvDesc(N, H, W, Ci, Co, 3, 3, 1, 1, 1, 2 * H, 2 * W, 1)
    P = 4096
    rows = [("fwd    fused ", "nk_conv2d_fwd", (P, P, P, None, None, P)), ("fwd    phases", "nk_conv2d_up2_fwd", (P, P, P, P, P)),
            ("dgrad  fused ", "nk_conv2d_dgrad_flipped", (P, P, P)), ("dgrad  phases", "nk_conv2d_up2_dgrad", (P, P, P)),
            ("wgrad  fused ", "nk_conv2d_wgrad_bias", (P, P, P, P, 0)), ("wgrad  phases", "nk_conv2d_up2_wgrad_bias", (P, P, P, P, 0, P))]
    for tag, name, args in rows:
        lib.launch_log(3)
        try:
            lib.call(name, C.byref(d), *args, None)
            log = lib.launched()
        finally:
            lib.launch_log(0)
        for line in log[1::2]:
            print(f"  {tag}  {line}")


def measure(shape, iters):
    N, H, W, Ci, Co = shape
    dev = "cuda"
    d = lib.NkConvDesc(N, H, W, Ci, Co, 3, 3, 1, 1, 1, 2 * H, 2 * W, 1)
    g = torch.Generator(device=dev).manual_seed(0)
    bf = lambda *s, scale=1.0: (torch.randn(*s, device=dev, generator=g) * scale).bfloat16()
    x, dy = bf(N * H * W, Ci), bf(N * 4 * H * W, Co)
    w = bf(Co, 9 * Ci, scale=(9 * Ci) ** -0.5)
    bias = torch.randn(Co, device=dev, generator=g)
    y = torch.empty(N * 4 * H * W, Co, dtype=torch.bfloat16, device=dev)
    wp, wd, wt = (torch.empty(16 * Co * Ci, dtype=torch.bfloat16, device=dev) for _ in range(3))
    dx2, dx = torch.empty(N * 4 * H * W, Ci, dtype=torch.bfloat16, device=dev), torch.empty(N * H * W, Ci, dtype=torch.bfloat16, device=dev)
    dw, db = torch.empty(Co, 9 * Ci, device=dev), torch.empty(Co, device=dev)
    ws_f = torch.empty(lib.query("nk_conv2d_up2_ws_bytes", C.byref(d), 0), dtype=torch.uint8, device=dev)
    ws_w = torch.empty(lib.query("nk_conv2d_up2_ws_bytes", C.byref(d), 2), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    if not lib.query("nk_conv2d_dgrad_flipped_ok", C.byref(d)):
        raise SystemExit(f"{shape}: the fused path's input gradient is not the flipped one here")
    steps = {
        "fwd    fused : nk_conv2d_fwd": lambda: lib.call("nk_conv2d_fwd", C.byref(d), p(x), p(w), p(bias), None, None, p(y), st),
        "fwd    phases: nk_up2_phase_weights": lambda: lib.call("nk_up2_phase_weights", p(w), p(wp), p(wd), Co, Ci, st),
        "fwd    phases: nk_conv2d_up2_fwd": lambda: lib.call("nk_conv2d_up2_fwd", C.byref(d), p(x), p(wp), p(bias), p(y), p(ws_f), st),
        "dgrad  fused : nk_conv_weight_flip": lambda: lib.call("nk_conv_weight_flip", p(w), p(wt), Co, Ci, 9, st),
        "dgrad  fused : nk_conv2d_dgrad_flipped": lambda: lib.call("nk_conv2d_dgrad_flipped", C.byref(d), p(dy), p(wt), p(dx2), st),
        "dgrad  fused : nk_upsample2x_bwd": lambda: lib.call("nk_upsample2x_bwd", p(dx2), p(dx), N, H, W, Ci, st),
        "dgrad  phases: nk_conv2d_up2_dgrad": lambda: lib.call("nk_conv2d_up2_dgrad", C.byref(d), p(dy), p(wd), p(dx), st),
        "wgrad  fused : nk_conv2d_wgrad_bias": lambda: lib.call("nk_conv2d_wgrad_bias", C.byref(d), p(dy), p(x), p(dw), p(db), 0, st),
        "wgrad  phases: nk_conv2d_up2_wgrad_bias": lambda: lib.call("nk_conv2d_up2_wgrad_bias", C.byref(d), p(dy), p(x), p(dw), p(db), 0, p(ws_w), st),
    }
    for f in steps.values():       # warm-up: code objects, LDS opt-ins
        f(); f()
    torch.cuda.synchronize()
    ev = {k: [] for k in steps}
    for _ in range(iters):
        for k, f in steps.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); f(); e.record()
            ev[k].append((s, e))
    torch.cuda.synchronize()
    us = {k: statistics.median(s.elapsed_time(e) for s, e in v) * 1e3 for k, v in ev.items()}
    fused_macs = 2.0 * N * 4 * H * W * Co * 9 * Ci
    for k, t in us.items():
        rate = f"  {fused_macs / t / 1e6:7.0f} TF/s of the fused path's 9-tap FLOPs" if "nk_conv2d" in k else ""
        print(f"  {k:42s} {t:8.1f} us{rate}")
    tot = lambda key: sum(t for k, t in us.items() if k.startswith(key))
    for dirn in ("fwd", "dgrad", "wgrad"):
        a, b = tot(f"{dirn:6s} fused"), tot(f"{dirn:6s} phases")
        print(f"  {dirn:6s} fused {a:8.1f} us   phases {b:8.1f} us   saved {a - b:8.1f} us")
    a, b = tot("fwd    fused") + tot("dgrad  fused") + tot("wgrad  fused"), tot("fwd    phases") + tot("dgrad  phases") + tot("wgrad  phases")
    print(f"  layer  fused {a:8.1f} us   phases {b:8.1f} us   saved {a - b:8.1f} us per step")
    return a - b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--plan", action="store_true")
    a = ap.parse_args()
    saved = 0.0
    for shape in SHAPES:
        print("x [N, H, W, Cin] -> y [N, 2H, 2W, Cout]:", shape)
        plan(shape)
        if not a.plan:
            saved += measure(shape, a.iters)
    if not a.plan:
        print(f"both layers: {saved:.1f} us per step saved by the phase path (serialized, event-timed)")


if __name__ == "__main__":
    main()
