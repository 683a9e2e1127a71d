"""Times of the Gumbel-softmax quantizer's four kernels (csrc/gumbel.hip) and of one whole GumbelQuantizer.regularize + bwd, at
N = 4096 latent vectors, num_hiddens h = 256, n_embed n = 8192, embedding_dim d = 256 (a 64 x 64 latent grid against an 8192-code book).

    python tools/gumbel_bench.py [--rounds 15] [--reps 10]

`reps` launches between two device events after a warm-up; the figures are medians over the rounds.  Next to each time: the bytes the
pass must move (its compulsory traffic, each operand once) and the bandwidth that amounts to.  The [N, n] fp32 logits are 134 MB, so the
row passes are memory passes; the logits kernel is a 17-GFLOP fp32 GEMM that writes them.  Nothing is asserted: the tool reports.  The
last line is one JSON object."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

N, H, NE, D = 4096, 256, 8192, 256


def main() -> int:
    from neurosis_amd import ops
    from neurosis_amd.modules.autoencoding.regularizers import GumbelQuantizer

    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gumbel_bench: needs a GPU; nothing is measured without one")
    g = torch.Generator(device="cuda").manual_seed(0)
    q = GumbelQuantizer(H, D, NE, straight_through=True, kl_weight=5e-4).cuda().train()
    z_e = torch.randn(1, H, 64, 64, device="cuda", generator=g)
    dz = torch.randn(1, D, 64, 64, device="cuda", generator=g)
    rows = z_e.permute(0, 2, 3, 1).reshape(N, H).contiguous()
    W, b = q.proj.weight.detach().view(NE, H), q.proj.bias.detach()
    tok = ops.dropout_draw()
    logits = ops.gumbel_logits(rows, W, b)
    noise = ops.gumbel_noise(N, NE, 0, tok)
    y, _, _ = ops.gumbel_softmax_fwd(logits, 1.0, noise=noise)
    G = torch.randn(N, NE, device="cuda", generator=g).to(torch.bfloat16)

    def whole():
        _, _, bwd = q.regularize(z_e)
        bwd(dz, 1.0)

    f32, b16 = 4 * N * NE, 2 * N * NE
    sides = {
        "logits": (lambda: ops.gumbel_logits(rows, W, b), f32 + 4 * (N * H + NE * H)),
        "noise": (lambda: ops.gumbel_noise(N, NE, 0, tok), f32),
        "softmax_fwd_noise_given": (lambda: ops.gumbel_softmax_fwd(logits, 1.0, noise=noise), 2 * f32 + b16),
        "softmax_fwd_token": (lambda: ops.gumbel_softmax_fwd(logits, 1.0, token=tok, site=0), f32 + b16),
        "softmax_bwd": (lambda: ops.gumbel_softmax_bwd(logits, y, G, 1.0, 5e-4), f32 + 3 * b16),
        "regularize_and_bwd": (whole, None),
    }
    out = {"device": torch.cuda.get_device_name(0), "N": N, "h": H, "n": NE, "d": D, "rounds": args.rounds, "reps": args.reps}
    for name, (fn, nbytes) in sides.items():
        for _ in range(3):
            fn()
        times = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / args.reps)
        med = statistics.median(times)
        res = {"us": round(med, 1), "min_max_us": [round(min(times), 1), round(max(times), 1)]}
        line = f"{name}: {res['us']} us (median of {args.rounds} x {args.reps}; {res['min_max_us'][0]} .. {res['min_max_us'][1]})"
        if nbytes is not None:
            res.update(bytes=nbytes, gb_per_s=round(nbytes / med * 1e-3, 1))
            line += f"; {nbytes / 1e6:.1f} MB -> {res['gb_per_s']} GB/s"
        if name == "logits":
            res["tflops"] = round(2.0 * N * NE * H / med * 1e-6, 2)
            line += f"; {res['tflops']} TFLOP/s fp32"
        print(line)
        out[name] = res
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
