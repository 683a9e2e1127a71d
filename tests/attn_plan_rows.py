"""Rows of attention calls and how to ask the library for the plan of each without a GPU (shared by tests/attention_bounds.py,
tests/test_attn_plan_cpu.py, tests/test_attn_plan_gpu.py and the recorder that wrote tests/golden/attention_plans.json).

A row is [id, [B, H, Lq, Lk, D, causal], env, passes]: env the NK_ATTN* switches set around the call, passes "fwd" and, where a backward
follows, "bwd" (nk_attention_bwd) or "bwd_causal" (nk_attention_bwd_causal).  The call passes null data pointers: in plan-only mode
(lib.launch_log(3)) the entry points log their plan and return before they look at a pointer or touch the GPU.

A plan line reads `name grid=x,y,z block smem gx qsplit part_offset ws_floats` (csrc/attn_plan.h: nk_attn_plan_line), one per launch."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

SWITCHES = ("NK_ATTN_XCD", "NK_ATTN64", "NK_ATTN64_SMALL")


@contextlib.contextmanager
def environment(env):
    """exactly the switches of `env` set, the family's other switches unset; restored afterwards"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def desc(dims):
    """the dense descriptor of [B, H, Lq, Lk, D, causal] (the plan reads no stride)"""
    from neurosis_amd.lib import NkAttnDesc

    B, H, Lq, Lk, D, causal = dims
    d = NkAttnDesc()
    d.B, d.H, d.Lq, d.Lk, d.D, d.causal = B, H, Lq, Lk, D, int(causal)
    d.sq = d.sk = d.sv = d.so = d.sdq = d.sdk = d.sdv = d.sdo = H * D
    d.bq = d.bo = d.bdq = d.bdo = Lq * H * D
    d.bk = d.bv = d.bdk = d.bdv = Lk * H * D
    d.scale = float(D) ** -0.5
    return d


def call(lib, dims, pass_, ptr=None) -> int:
    """issue the entry point of `pass_` with every data pointer = ptr; returns the status"""
    d = C.byref(desc(dims))
    l = lib.load()
    if pass_ == "fwd":
        return int(l.nk_attention_fwd(d, ptr, ptr, ptr, ptr, ptr, None))
    if pass_ == "bwd":
        return int(l.nk_attention_bwd(d, *([ptr] * 10), None))
    return int(l.nk_attention_bwd_causal(d, *([ptr] * 9), None))


def parse(line, dims):
    """a plan line as the fixture's launch record + (qsplit, part, ws_floats)"""
    name, grid, block, smem, gx, qsplit, part, ws = line.split(" ")
    grid = [int(x) for x in grid[len("grid="):].split(",")]
    gx = int(gx)
    extent = [gx, dims[1], dims[0]] if gx else grid          # (x blocks, heads, batch) under the 1-D mapping
    return {"name": name, "extent": extent, "grid": grid, "gx": gx, "block": int(block), "smem": int(smem)}, int(qsplit), int(part), int(ws)


def planned(lib, dims, env, pass_):
    """what the library plans for the call: {"launches": [...], "qsplit", "part", "ws"}; None when the call is refused"""
    with environment(env):
        lib.launch_log(3)
        try:
            if call(lib, dims, pass_) != 0:
                return None
            log = lib.launched()
        finally:
            lib.launch_log(0)
    names, lines = log[0::2], log[1::2]
    assert lines and all(l.startswith(n + " grid=") for n, l in zip(names, lines)), log
    recs = [parse(l, dims) for l in lines]
    assert len({r[1:] for r in recs}) == 1, log
    return {"launches": [r[0] for r in recs], "qsplit": recs[0][1], "part": recs[0][2], "ws": recs[0][3]}


def case_row(case) -> list:
    """the row of a case of attention_bounds.REAL_CASES / EDGE_CASES (the chunked recompute backward is no attention launch)"""
    cid, env, B, H, Lq, Lk, D, causal, _, bwd = case
    return [cid, [B, H, Lq, Lk, D, int(causal)], dict(env), ["fwd", "bwd"] if bwd is True else ["fwd"]]


XCD_OFF = {"NK_ATTN_XCD": "0"}
# every distinct attention call of the training step of the three example configs, at batch 4
STEP_ROWS = [
    # sdxl.example: the UNet's transformer levels (640 channels / 10 heads at 64 x 64, 1280 / 20 at 32 x 32), 77 text tokens
    ["step-sdxl-self-L4096", [4, 10, 4096, 4096, 64, 0], {}, ["fwd", "bwd"]],
    ["step-sdxl-cross-L4096", [4, 10, 4096, 77, 64, 0], {}, ["fwd", "bwd"]],
    ["step-sdxl-self-L1024", [4, 20, 1024, 1024, 64, 0], {}, ["fwd", "bwd"]],
    ["step-sdxl-cross-L1024", [4, 20, 1024, 77, 64, 0], {}, ["fwd", "bwd"]],
    # ... its frozen text towers (CLIP-L 12 heads, bigG 20), and sdxl-te.example's trained ones
    ["step-clip-l-frozen", [4, 12, 77, 77, 64, 1], {}, ["fwd"]],
    ["step-bigg-frozen", [4, 20, 77, 77, 64, 1], {}, ["fwd"]],
    ["step-clip-l-trained", [4, 12, 77, 77, 64, 1], {}, ["fwd", "bwd_causal"]],
    ["step-bigg-trained", [4, 20, 77, 77, 64, 1], {}, ["fwd", "bwd_causal"]],
    # ... the VAE encoder's mid block (one head of 512 channels over 128 x 128 latents; per batch and per sample), and autoencoder training
    ["step-vae-mid-b4", [4, 1, 16384, 16384, 512, 0], {}, ["fwd"]],
    ["step-vae-mid-b1", [1, 1, 16384, 16384, 512, 0], {}, ["fwd"]],
    ["step-vae-train", [4, 1, 1024, 1024, 512, 0], {}, ["fwd", "bwd"]],
    # sd15.example: 8 heads of 40 / 80 / 160 channels at 64 x 64, 32 x 32, 16 x 16 and the 8 x 8 middle block
    ["step-sd15-self-d40", [4, 8, 4096, 4096, 40, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-cross-d40", [4, 8, 4096, 77, 40, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-self-d80", [4, 8, 1024, 1024, 80, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-cross-d80", [4, 8, 1024, 77, 80, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-self-d160", [4, 8, 256, 256, 160, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-cross-d160", [4, 8, 256, 77, 160, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-mid-self-d160", [4, 8, 64, 64, 160, 0], {}, ["fwd", "bwd"]],
    ["step-sd15-mid-cross-d160", [4, 8, 64, 77, 160, 0], {}, ["fwd", "bwd"]],
]
# the 3-D grid (NK_ATTN_XCD=0) of one row per path
XCD_ROWS = [
    ["xcd0-attn64-self", [4, 20, 1024, 1024, 64, 0], XCD_OFF, ["fwd", "bwd"]],
    ["xcd0-attn64-small", [4, 20, 1024, 77, 64, 0], XCD_OFF, ["fwd", "bwd"]],
    ["xcd0-attn64-cross-2k", [4, 20, 1024, 77, 64, 0], dict(XCD_OFF, NK_ATTN64_SMALL="0"), ["fwd", "bwd"]],
    ["xcd0-generic64", [2, 10, 1024, 77, 64, 0], dict(XCD_OFF, NK_ATTN64="0"), ["fwd", "bwd"]],
    ["xcd0-d40", [2, 8, 4096, 77, 40, 0], XCD_OFF, ["fwd", "bwd"]],
    ["xcd0-d80", [2, 8, 1024, 1024, 80, 0], XCD_OFF, ["fwd", "bwd"]],
    ["xcd0-d160", [2, 8, 256, 256, 160, 0], XCD_OFF, ["fwd", "bwd"]],
    ["xcd0-causal", [4, 12, 77, 77, 64, 1], XCD_OFF, ["fwd", "bwd_causal"]],
    ["xcd0-d512", [4, 1, 1024, 1024, 512, 0], XCD_OFF, ["fwd", "bwd"]],
]


def rows() -> list:
    from tests import attention_bounds as ab

    return [case_row(c) for c in ab.REAL_CASES + ab.EDGE_CASES] + STEP_ROWS + XCD_ROWS
