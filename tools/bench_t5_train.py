"""Times of the T5 / ByT5 training path on the GPU (device events around repeated calls, after a warm-up; one JSON line per measurement):

  relbias-bwd   nk_attention_relbias_bwd against the generic unbiased backward (nk_attention_bwd under NK_ATTN64=0: the same kernels without
                the bias and without d_rel) at the same shapes, alternating the two inside every repeat -- the difference is the price of
                the bias and of d_rel.  Shapes: ByT5-small-like (B 4, H 6, D 64, L 256) and T5-XL-like (B 4, H 32, D 64, L 77 / 512).
  tower         forward + backward of a ByT5-small-shaped T5EncoderTower (d_model 1472, d_ff 3584, 12 layers, 6 heads, B 4, L 256).

    python tools/bench_t5_train.py [--iters 200] [--repeats 5] [--only relbias|tower] [--profile]

--profile runs each call a few times only and without timing, for a kernel trace taken from outside (rocprofv3 --kernel-trace --stats)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402

from neurosis_amd import ops  # noqa: E402
from neurosis_amd.lib import NkAttnDesc, call, query  # noqa: E402

BF16 = torch.bfloat16
SHAPES = [("byt5-small", 4, 6, 64, 256), ("t5-xl-L77", 4, 32, 64, 77), ("t5-xl-L512", 4, 32, 64, 512)]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters      # us per call


def relbias(args):
    for name, B, H, D, L in SHAPES:
        HD = H * D
        g = torch.Generator(device="cuda").manual_seed(L)
        fused = (torch.randn(B * L, 3 * HD, generator=g, device="cuda") * 0.6).to(BF16)
        q, k, v = fused[:, :HD], fused[:, HD:2 * HD], fused[:, 2 * HD:]
        do = torch.randn(B * L, HD, generator=g, device="cuda").to(BF16)
        rel = torch.randn(H, 2 * L - 1, generator=g, device="cuda") * 2
        d_rel = torch.zeros_like(rel)
        dfused = torch.empty_like(fused)
        dq, dk, dv = dfused[:, :HD], dfused[:, HD:2 * HD], dfused[:, 2 * HD:]
        ob, bwd = ops.attention_relbias_train(q, k, v, B, H, D, rel, 1.0, d_rel)

        d = NkAttnDesc()
        d.B, d.H, d.Lq, d.Lk, d.D, d.scale, d.causal = B, H, L, L, D, 1.0, 0
        d.sq = d.sk = d.sv = d.sdq = d.sdk = d.sdv = 3 * HD
        d.bq = d.bk = d.bv = d.bdq = d.bdk = d.bdv = L * 3 * HD
        d.so = d.sdo = HD
        d.bo = d.bdo = L * HD
        o = torch.empty(B * L, HD, dtype=BF16, device="cuda")
        lse = torch.empty(B, H, L, device="cuda")
        os.environ["NK_ATTN64"] = "0"
        st = ops._stream()
        call("nk_attention_fwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), st)
        ws = torch.empty(query("nk_attention_bwd_ws_floats", C.byref(d)), device="cuda")

        def plain():
            os.environ["NK_ATTN64"] = "0"
            call("nk_attention_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dq.data_ptr(),
                 dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), st)
            os.environ.pop("NK_ATTN64", None)

        os.environ.pop("NK_ATTN64", None)
        wsb = torch.empty(query("nk_attention_relbias_bwd_ws_floats", C.byref(d)), device="cuda")

        def biased():      # (both through the raw entry points: the same host work per call)
            call("nk_attention_relbias_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), ob.data_ptr(), bwd.lse.data_ptr(), do.data_ptr(),
                 dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), rel.data_ptr(), d_rel.data_ptr(), wsb.data_ptr(), 0, st)

        if args.profile:
            for _ in range(3):
                biased()
                plain()
            torch.cuda.synchronize()
            continue
        for _ in range(10):
            biased()
            plain()
        tb, tp = [], []
        for _ in range(args.repeats):
            tb.append(_time(biased, args.iters))
            tp.append(_time(plain, args.iters))
        mb, mp = statistics.median(tb), statistics.median(tp)
        print(json.dumps({"bench": "relbias-bwd", "shape": name, "B": B, "H": H, "D": D, "L": L, "relbias_us": round(mb, 2), "unbiased_us": round(mp, 2),
                          "ratio": round(mb / mp, 3), "relbias_us_min_max": [round(min(tb), 2), round(max(tb), 2)],
                          "unbiased_us_min_max": [round(min(tp), 2), round(max(tp), 2)], "iters": args.iters, "repeats": args.repeats}), flush=True)


def tower(args):
    from neurosis_amd.models.text_encoder.t5 import T5EncoderTower
    from neurosis_amd.nn import FlatParamStore

    torch.manual_seed(0)
    B, L = 4, 256
    cfg = dict(vocab_size=384, d_model=1472, d_kv=64, d_ff=3584, num_layers=12, num_heads=6)
    t = T5EncoderTower(**cfg)
    with torch.no_grad():
        for n, p in t.named_parameters():
            if p.dim() == 2 and "shared" not in n and "relative_attention_bias" not in n:
                p.normal_(std=p.shape[1] ** -0.5)
    t = t.cuda()
    store = FlatParamStore(list(t.parameters()))
    ids = torch.randint(0, 384, (B, L), device="cuda")
    up = torch.randn(B, L, cfg["d_model"], device="cuda")

    def fwd_bwd():
        t.train_outputs(ids).backward(up)

    def fwd():
        with torch.no_grad():
            t._forward_ids(ids)

    if args.profile:
        for _ in range(3):
            fwd_bwd()
        torch.cuda.synchronize()
        return
    for _ in range(5):
        fwd_bwd()
        fwd()
    tt = [_time(fwd_bwd, max(args.iters // 10, 4)) for _ in range(args.repeats)]
    tf = [_time(fwd, max(args.iters // 10, 4)) for _ in range(args.repeats)]
    print(json.dumps({"bench": "tower", "shape": "byt5-small", **cfg, "B": B, "L": L, "parameters": int(store.master.numel()),
                      "fwd_bwd_ms": round(statistics.median(tt) / 1e3, 3), "fwd_bwd_ms_min_max": [round(min(tt) / 1e3, 3), round(max(tt) / 1e3, 3)],
                      "frozen_fwd_eager_ms": round(statistics.median(tf) / 1e3, 3), "repeats": args.repeats}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["relbias", "tower"])
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_t5_train: no GPU (there is no CPU path to time)")
    if a.only != "tower":
        relbias(a)
    if a.only != "relbias":
        tower(a)
