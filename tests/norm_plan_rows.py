"""Rows of normalisation and column-sum calls and how to ask the library for the plan of each without a GPU (shared by
tests/test_norm_plan_cpu.py and the recorder that wrote tests/golden/norm_plans.json).

A row is [entry, dims]: entry names the entry point (ENTRIES below), dims its sizes -- [N, HW, C, G] for the GroupNorm family,
[N, nparts, G] for the sums from partial rows, [M, C] for LayerNorm / RMSNorm, [M, N, nbatch] for the column sums and [[C...], nrows] for
nk_colpart_reduce_batch.  In plan-only mode (lib.launch_log(3)) the entry points log their plan and return before they look at a pointer
or touch the GPU, so the call passes null pointers.

A plan line reads `name grid=x,y,z block smem [region=offset+extent ...] ws=ws_floats` (csrc/norm_plan.h: nk_norm_plan_line), one per
launch: the workspace regions the launch reads or writes, in floats, and what the family's workspace query reports for the call."""
from __future__ import annotations

import ctypes as C

GN_ENTRIES = ("gn_fwd", "gn_sums", "gn_apply", "gn_bwd", "gn_mod_fwd", "gn_mod_apply", "gn_mod_bwd")
LN_ENTRIES = ("ln_fwd", "ln_bwd_dx", "ln_bwd_params", "ln_bwd_rows", "ln_bwd")
ENTRIES = GN_ENTRIES + LN_ENTRIES + ("gn_sums_from_parts", "rms_fwd", "colsum", "colsum_batched", "colpart_batch")


def call_row(lib, row, ptr=None, ws=None) -> int:
    """Issue the row's entry point with every data pointer = ptr and the workspace (or partial-row buffer) = ws; returns the status."""
    entry, d = row
    l = lib.load()
    p = ptr
    if entry in GN_ENTRIES:
        N, HW, Cc, G = d
        tail = (N, HW, Cc, G)
        if entry == "gn_fwd":
            return int(l.nk_groupnorm_fwd(p, p, p, p, p, p, ws, *tail, 1e-5, 1, None))
        if entry == "gn_sums":
            return int(l.nk_groupnorm_sums(p, p, ws, *tail, None))
        if entry == "gn_apply":
            return int(l.nk_groupnorm_apply(p, p, p, p, p, p, p, *tail, 1e-5, 1, None))
        if entry == "gn_bwd":
            return int(l.nk_groupnorm_bwd(p, p, p, p, p, p, p, p, p, p, ws, *tail, 1, 0, None))
        if entry == "gn_mod_fwd":
            return int(l.nk_groupnorm_mod_fwd(p, p, p, p, p, p, p, ws, *tail, 1e-5, 1, None))
        if entry == "gn_mod_apply":
            return int(l.nk_groupnorm_mod_apply(p, p, p, p, p, p, p, p, *tail, 1e-5, 1, None))
        return int(l.nk_groupnorm_mod_bwd(p, p, p, p, p, p, p, p, p, p, p, p, ws, *tail, 1, 0, None))
    if entry == "gn_sums_from_parts":
        return int(l.nk_groupnorm_sums_from_parts(p, p, ws, *d, None))
    if entry == "ln_fwd":
        return int(l.nk_layernorm_fwd(p, p, p, p, p, p, *d, 1e-5, None))
    if entry == "rms_fwd":
        return int(l.nk_rmsnorm_fwd(p, p, p, *d, 1e-6, None))
    if entry == "ln_bwd_dx":
        return int(l.nk_layernorm_bwd_dx(p, p, p, p, p, p, p, *d, None))
    if entry == "ln_bwd_params":
        return int(l.nk_layernorm_bwd_params(p, p, p, p, p, p, ws, *d, 0, None))
    if entry == "ln_bwd_rows":
        return int(l.nk_layernorm_bwd_rows(p, p, p, p, p, p, p, ws, *d, None))
    if entry == "ln_bwd":
        return int(l.nk_layernorm_bwd(p, p, p, p, p, p, p, p, p, ws, *d, 0, None))
    if entry == "colsum":
        M, N, _ = d
        return int(l.nk_colsum(p, p, ws, M, N, N, 0, None))
    if entry == "colsum_batched":
        M, N, nb = d
        return int(l.nk_colsum_batched(p, p, ws, M, N, N, nb, 0, None))
    if entry == "colpart_batch":
        from neurosis_amd.lib import NkColpartBatch

        cs, nrows = d
        b = NkColpartBatch()
        b.n = len(cs)
        for z, c in enumerate(cs[:len(b.C)]):
            b.part[z], b.dgamma[z], b.dbeta[z], b.nrows[z], b.C[z], b.accumulate[z] = p, p, p, nrows, c, z & 1
        return int(l.nk_colpart_reduce_batch(C.byref(b), None))
    raise ValueError(entry)


def queries(lib, row) -> dict:
    """what the family's size queries report for the row"""
    entry, d = row
    if entry in GN_ENTRIES:
        return {"ws": lib.query("nk_groupnorm_ws_floats", *d)}
    if entry == "gn_sums_from_parts":
        return {"ws": lib.query("nk_groupnorm_sums_ws_floats", *d)}
    if entry in LN_ENTRIES:
        return {"ws": lib.query("nk_layernorm_ws_floats", *d), "part_rows": lib.query("nk_layernorm_part_rows", d[0])}
    if entry in ("colsum", "colsum_batched"):
        return {"ws": lib.query("nk_colsum_ws_floats", d[0], d[1])}
    return {}


def plan_lines(lib, row, mode=3, ptr=None, ws=None):
    """the (name, line) pairs the library logs for the row in plan-only mode; None when the call is refused"""
    lib.launch_log(mode)
    try:
        if call_row(lib, row, ptr, ws) != 0:
            return None
        log = lib.launched()
    finally:
        lib.launch_log(0)
    names, lines = log[0::2], log[1::2]
    assert lines and len(names) == len(lines) and all(l.startswith(n + " grid=") for n, l in zip(names, lines)), log
    return lines


def fixture_rows(fx) -> list:
    """the rows of tests/golden/norm_plans.json as ([entry, dims], {queries, "lines": [...]}): the file keeps one shape per line --
    [dims, {queries}, {entry: [ws_floats, "k x,y,z block smem regions|..."]}], k an index into fx["kernels"] -- and this spells each launch
    out again as the plan line the library logs"""
    out = []
    for dims, q, entries in fx["rows"]:
        for entry, (ws, enc) in entries.items():
            lines = []
            for l in enc.split("|"):
                k, grid, *rest = l.split(" ")
                lines.append(" ".join([fx["kernels"][int(k)], "grid=" + grid, *rest, f"ws={ws}"]))
            out.append(([entry, dims], dict(q, lines=lines)))
    return out


def parse(line) -> dict:
    """a plan line as {"name", "grid", "block", "smem", "regions": {name: (offset, extent)}, "ws"}"""
    name, grid, block, smem, *rest = line.split(" ")
    regions = {r.split("=")[0]: tuple(int(v) for v in r.split("=")[1].split("+")) for r in rest[:-1]}
    assert rest[-1].startswith("ws=")
    return {"name": name, "grid": [int(x) for x in grid[len("grid="):].split(",")], "block": int(block), "smem": int(smem),
            "regions": regions, "ws": int(rest[-1][3:])}


# ---- the shapes --------------------------------------------------------------------------------------------------------------------------------
def _gn(N, H, W, Cc, G=32):
    return [N, H * W, Cc, G]


# GroupNorms of the SDXL training step at batch 4 (128 x 128 latents; channel_mult 1, 2, 4 of 320): ResBlock in / out norms on the way down,
# on the concatenations of the way up, the SpatialTransformer norms and the output norm ...
STEP_GN = [_gn(4, s, s, c) for s, c in [(128, 320), (64, 320), (64, 640), (32, 640), (32, 1280), (32, 2560), (32, 1920), (64, 1920), (64, 1280),
                                        (64, 960), (128, 960), (128, 640)]]
# ... the frozen VAE encoder at 1024 x 1024 per batch of four and per sample, and its mid block ...
VAE_GN = [_gn(n, s, s, c) for n in (4, 1) for s, c in [(1024, 128), (512, 128), (512, 256), (256, 256), (256, 512), (128, 512)]]
# ... the tiles of the convolutions whose statistics epilogue feeds those norms (16 x 16 pixels a tile)
VAE_PARTS = [[n, t, 32] for n in (4, 1) for t in (4096, 1024, 256, 64)]
# LayerNorms of the step: the transformer blocks at 64 x 64 and 32 x 32, the text towers' 77 tokens
STEP_LN = [[16384, 640], [4096, 1280], [308, 768], [308, 1280]]
# bias and per-image (time embedding) gradients of the step
STEP_COLSUM = [[16384, 640, 1], [4096, 1280, 1], [16384, 5120, 1], [4096, 10240, 1], [65536, 320, 1], [4, 1280, 1],
               [16384, 320, 4], [4096, 640, 4], [1024, 1280, 4]]
# tests/test_norm_reductions_gpu.py: GN_CASES, the exact-sum shapes, the conv epilogue's tile counts, the LayerNorm sizes
TEST_GN = [_gn(*c) for c in [(4, 128, 128, 320), (4, 64, 64, 640), (4, 32, 32, 1280), (4, 32, 32, 2560), (4, 64, 64, 1920), (4, 128, 128, 960),
                             (1, 1024, 1024, 128), (4, 512, 512, 256), (4, 256, 256, 512), (4, 104, 152, 320), (1, 832, 1216, 128), (32, 256, 256, 128),
                             (2, 32, 32, 2304, 3), (4, 64, 64, 320, 1), (2, 32, 32, 4096), (4, 128, 128, 320, 1), (2, 256, 256, 128), (2, 128, 128, 128),
                             (4, 256, 256, 128)]]
TEST_PARTS = [[2, 256, 32], [2, 64, 32], [1, 4096, 32], [1, 3952, 32], [4, 256, 32]]
TEST_LN = [[16384, 640], [4096, 1280], [308, 768], [308, 1280], [4100, 520], [1000, 1032], [2048, 2048],
           # tests/test_kernels_gpu.py
           [1000, 640], [512, 1280], [77, 320], [4100, 1280], [9000, 640], [8, 2048], [2048, 640]]
# tests/test_adm_gpu.py (GN_SHAPES and the op test) and tests/test_kernels_gpu.py
TEST_GN += [_gn(2, 24, 20, 64), _gn(2, 16, 16, 320), _gn(3, 9, 7, 640), _gn(2, 8, 8, 2560), _gn(1, 32, 32, 128)]
TEST_COLSUM = [[5000, 2560, 1], [4096, 1280, 1], [1000, 320, 4]]
TEST_RMS = [[1, 64], [3, 1472], [77, 128], [130, 4096]]
# tests/test_norm_reduce_gpu.py
EXACT_GN = [[1, 32, 8, 1], [2, 1056, 72, 3], [3, 64, 2304, 3]]
EXACT_PARTS = [[2, n, g] for n in (1, 7, 8, 9, 128, 129, 300) for g in (1, 32)]
EXACT_LN = [[m, c] for m in (1, 63, 65, 1093) for c in (8, 72, 136)]
EXACT_COLSUM = [[m, n, b] for m in (1, 63, 64, 65, 1093) for n in (8, 72, 136) for b in (1, 3)]
EXACT_COLPART = [[[c], r] for r in (1, 31, 32, 33, 67) for c in (8, 24, 40)]
# the edges: one and two channel slabs (C = 2304, 2560 above), rows_per clamped at 32 (few rows) and not, every chunks-per-lane instance,
# column sums around 65 536 rows and at the autoencoder's 2 M, one entry and NK_COLPART_MAX entries of unequal width
EDGE_GN = [[3, 63, 640, 32], [1, 33, 8, 1], [1024, 64, 64, 32], [1, 1048576, 64, 32], [2, 4096, 4096, 64]]
EDGE_LN = [[64, c] for c in (8, 1024, 1032, 1536, 1544, 2048)]
EDGE_RMS = [[64, c] for c in (8, 1024, 1032, 1536, 1544, 2048, 2056, 4096)]
EDGE_COLSUM = [[65536, 320, 1], [65537, 320, 1], [2097152, 128, 1], [131073, 8, 2]]
# widths beyond LN_MAXCH, which only nk_layernorm_bwd_params takes (the workspace query must cover them)
EDGE_LN_PARAMS = [[64, 4096], [1093, 2056]]
# ... and the three LayerNorms of a transformer block in one launch (tests/test_kernels_gpu.py)
EDGE_COLPART = [[[640, 640, 640], 128], [[640], 256], [[8 * (z % 5 + 1) + 64 * (z % 3) for z in range(32)], 257]]


def _uniq(rows):
    seen, out = set(), []
    for r in rows:
        k = repr(r)
        if k not in seen:
            seen.add(k)
            out.append(r)
    return out


def rows() -> list:
    gn = _uniq(STEP_GN + VAE_GN + TEST_GN + EXACT_GN + EDGE_GN)
    ln = _uniq(STEP_LN + TEST_LN + EXACT_LN + EDGE_LN)
    cs = _uniq(STEP_COLSUM + TEST_COLSUM + EXACT_COLSUM + EDGE_COLSUM)
    out = [[e, d] for d in gn for e in GN_ENTRIES]
    out += [["gn_sums_from_parts", d] for d in _uniq(VAE_PARTS + TEST_PARTS + EXACT_PARTS)]
    out += [[e, d] for d in ln for e in LN_ENTRIES]
    out += [["ln_bwd_params", d] for d in EDGE_LN_PARAMS]
    out += [["rms_fwd", d] for d in _uniq(TEST_RMS + EDGE_RMS)]
    out += [["colsum" if d[2] == 1 else "colsum_batched", d] for d in cs]
    out += [["colpart_batch", d] for d in EXACT_COLPART + EDGE_COLPART]
    return out
