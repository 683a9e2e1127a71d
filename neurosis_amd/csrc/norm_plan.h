// Launch planner of the normalisation and column-sum kernels (norm.hip, the bias-gradient section of elementwise.hip): WHICH launches run a
// shape, with what grid and LDS, and WHERE in the caller's workspace each keeps what.
//
// Host-only, in the style of attn_plan.h: no kernel, no HIP call, no getenv, nothing but the constants below, neurosis_hip.h and libc (the macros the entry points run a plan with are in nk_common.h), so a plan can be computed
// (and is tested: tests/test_norm_plan_cpu.py) on a machine without a GPU.  Every entry point of the family checks its sizes through the
// plan (NkNormPlan::err), runs the plan's launches in order, and hands the kernels the plan's offsets; every *_ws_floats / part_rows query
// answers from the same plan, so the size a caller allocates and the offsets the kernels write cannot disagree.  No size or offset of the
// family is computed anywhere else.
#pragma once
#include "../../include/neurosis_hip.h"
#include <stdio.h>

#define GN_THREADS 256
#define GN_MAXC 4096
#define GN_MAXG 64
#define GN_SUMS_MAXG 32              // nk_groupnorm_sums_from_parts: gn_reduce_partials_l1_kernel has 64 columns = 2G
#define GN_SUMS_ONE_LEVEL 128        // ... up to this many partial rows per image go through one level
#define GN_SUMS_CHUNKS 64            // ... more: level 1 leaves this many rows per image in the workspace
#define LN_MAXCH 4                   // LayerNorm: 16-byte chunks per lane, C <= 64*8*4 = 2048
#define RMS_MAXCH 8                  // RMSNorm: C <= 64*8*8 = 4096 (T5-v1.1-XXL)
#define ROWNORM_MAX_BLOCKS 4096      // one-wave-per-row kernels: four rows per 256-thread block, at most this many blocks
#define LNP_ROWS 64                  // ln_bwd_param_kernel: rows per split
#define LNR_WAVES 4                  // ln_bwd_rows_kernel: waves per block (8 waves x 2 rows: 10.2 vs 11.1 us alone at 4096 x 1280, 20.5 vs 18.0 at 16384 x 640, and the smaller A/B gain in the step)
#define LNR_MAX_BLOCKS 512           // ... and its grid limit: one partial row per block
#define LNR_MAX_SMEM (2 * 2 * 2048 * 4)
#define RMSB_MAX_ROWS 512            // rms_bwd_rows_kernel: one partial row of dgamma per wave, at most this many waves
#define CS_ROWS 64                   // colsum_partial_kernel: rows per block up to CS_MAX_SPLIT * 64 rows
#define CS_MAX_SPLIT 1024
#define NORM_WS_PAD 64               // floats every workspace query adds behind the layout

// the kernels the runners can launch
enum NormKernel {
  NK_GN_STATS, NK_GN_REDUCE, NK_GN_REDUCE_L1, NK_GN_APPLY, NK_GN_BWD_STATS, NK_GN_COLPART, NK_GN_COLPART_MOD, NK_GN_DMOD, NK_GN_BWD_APPLY,
  NK_LN_FWD, NK_LN_BWD_DX, NK_LN_BWD_PARAM, NK_LN_BWD_ROWS, NK_LN_COLPART, NK_RMS_FWD, NK_COLPART_BATCH, NK_CS_PARTIAL, NK_CS_REDUCE,
  NK_RMS_BWD_ROWS, NK_RMS_COLPART
};
struct NkNormRegion { const char* name; long off, len; };      // floats of the workspace; len 0: not used
struct NkNormLaunch {
  int kernel;             // NormKernel
  const char* name;       // what nk_check_launch reports (lib.launched())
  unsigned grid[3];
  int block, smem;
  NkNormRegion reg[2];    // the workspace regions this launch reads or writes
};
struct NkNormPlan {       // what every plan of the family starts with
  int n;
  NkNormLaunch launch[5];
  long ws_floats;         // what the family's workspace query reports for the shape
  const char* err;        // the shape is refused: the message of the NK_ERR_ARG
};

static inline NkNormLaunch& norm_launch(NkNormPlan& pl, int kernel, const char* name, unsigned x, unsigned y, unsigned z, int block, int smem,
                                 NkNormRegion r0 = {nullptr, 0, 0}, NkNormRegion r1 = {nullptr, 0, 0}) {
  NkNormLaunch& L = pl.launch[pl.n++];
  L.kernel = kernel; L.name = name; L.block = block; L.smem = smem;
  L.grid[0] = x; L.grid[1] = y; L.grid[2] = z;
  L.reg[0] = r0; L.reg[1] = r1;
  return L;
}

// one line per planned launch, for the launch log and the plan tests: name grid=x,y,z block smem [region=offset+extent ...] ws=ws_floats
static inline void nk_norm_plan_line(const NkNormPlan& pl, int i, char* buf, size_t cap) {
  const NkNormLaunch& L = pl.launch[i];
  int at = snprintf(buf, cap, "%s grid=%u,%u,%u %d %d", L.name, L.grid[0], L.grid[1], L.grid[2], L.block, L.smem);
  for (int r = 0; r < 2 && at > 0 && (size_t)at < cap; ++r)
    if (L.reg[r].len) at += snprintf(buf + at, cap - at, " %s=%ld+%ld", L.reg[r].name, L.reg[r].off, L.reg[r].len);
  if (at > 0 && (size_t)at < cap) snprintf(buf + at, cap - at, " ws=%ld", pl.ws_floats);
}
// plan-only mode (nk_debug_launch_log(3)): name and plan line per launch into the launch log (`add` = nk_launch_log_add)
static inline void nk_norm_plan_log(const NkNormPlan& pl, void (*add)(const char*, const char*)) {
  char line[192];
  for (int i = 0; i < pl.n; ++i) {
    nk_norm_plan_line(pl, i, line, sizeof(line));
    add(pl.launch[i].name, line);
  }
}

// ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------------
// Workspace of one call: part [N][nsplit][nz][2G] (the per-block group partials) | gsum [N][2G] (their sums: the forward's `stats`, the
// backward's s1 / s2) | chan [N][nsplit][2][C] (the backward's channel partials: dgamma, dbeta and dmod come from them).
enum GnPass { GN_FWD, GN_SUMS, GN_APPLY, GN_BWD };
struct NkGnPlan : NkNormPlan {
  int rows_per, nsplit, nz;        // rows per block, blocks per image, channel slabs (one thread owns one 16-byte chunk column: (C/8)/nz <= 256)
  int nparts, chan_rows;           // rows of `part` per image (nsplit * nz) and rows of `chan` in all (N * nsplit)
  NkNormRegion part, gsum, chan;   // the dynamic LDS of each pass is its launch's smem: [C] floats x 2 (apply, backward statistics), x 4 (backward apply)
};
static inline NkGnPlan nk_gn_plan(int N, int HW, int C, int G, int pass, bool mod) {
  NkGnPlan p = {};
  if (!(N > 0 && HW > 0 && C > 0 && G > 0 && G <= GN_MAXG)) { p.err = "N > 0 && HW > 0 && C > 0 && G > 0 && G <= 64"; return p; }
  if (!((C & 7) == 0 && C % G == 0 && C <= GN_MAXC)) { p.err = "(C & 7) == 0 && C % G == 0 && C <= GN_MAXC"; return p; }
  const int cpr = C >> 3;
  p.nz = (cpr + GN_THREADS - 1) / GN_THREADS;
  while (cpr % p.nz) ++p.nz;
  const int want = (1024 + N - 1) / N;      // aim for ~2048 blocks in total
  p.rows_per = (HW + want - 1) / want;
  if (p.rows_per < 32) p.rows_per = 32;
  p.nsplit = (HW + p.rows_per - 1) / p.rows_per;
  p.nparts = p.nsplit * p.nz;
  p.chan_rows = N * p.nsplit;
  p.part = {"part", 0, (long)N * p.nparts * 2 * G};
  p.gsum = {"gsum", p.part.len, (long)N * 2 * G};
  p.chan = {"chan", p.gsum.off + p.gsum.len, (long)p.chan_rows * 2 * C};
  p.ws_floats = p.chan.off + p.chan.len + NORM_WS_PAD;
  const int smem2 = 2 * C * (int)sizeof(float);
  const unsigned ns = (unsigned)p.nsplit, n = (unsigned)N, cb = (unsigned)((C + 63) / 64);
  if (pass == GN_FWD || pass == GN_SUMS) {
    // nk_groupnorm_sums leaves the sums with the caller: its reduce touches the partials alone
    norm_launch(p, NK_GN_STATS, "gn_stats_kernel", ns, n, (unsigned)p.nz, GN_THREADS, 0, p.part);
    norm_launch(p, NK_GN_REDUCE, "gn_reduce_partials_kernel", n, 1, 1, 1024, 0, p.part, pass == GN_FWD ? p.gsum : NkNormRegion{nullptr, 0, 0});
  }
  if (pass == GN_FWD || pass == GN_APPLY)
    norm_launch(p, NK_GN_APPLY, mod ? "gn_apply_kernel<mod>" : "gn_apply_kernel", ns, n, 1, GN_THREADS, smem2,
                pass == GN_FWD ? p.gsum : NkNormRegion{nullptr, 0, 0});
  if (pass == GN_BWD) {
    norm_launch(p, NK_GN_BWD_STATS, mod ? "gn_bwd_stats_kernel<mod>" : "gn_bwd_stats_kernel", ns, n, (unsigned)p.nz, GN_THREADS, smem2, p.part, p.chan);
    norm_launch(p, NK_GN_REDUCE, "gn_reduce_partials_kernel", n, 1, 1, 1024, 0, p.part, p.gsum);
    if (mod) {
      norm_launch(p, NK_GN_COLPART_MOD, "colpart_reduce_mod_kernel", cb, 1, 1, 1024, 0, p.chan);
      norm_launch(p, NK_GN_DMOD, "gn_dmod_kernel", cb, n, 1, 1024, 0, p.chan);
    } else {
      norm_launch(p, NK_GN_COLPART, "colpart_reduce_kernel", cb, 1, 1, 1024, 0, p.chan);
    }
    norm_launch(p, NK_GN_BWD_APPLY, mod ? "gn_bwd_apply_kernel<mod>" : "gn_bwd_apply_kernel", ns, n, 1, GN_THREADS, 2 * smem2, p.gsum);
  }
  return p;
}

// ---- sums[n][2G] from nparts partial rows per image (a convolution's statistics epilogue): one level, or two for many rows -----------------------
struct NkGnSumsPlan : NkNormPlan {
  int levels, nchunks;
  NkNormRegion l1;        // level 1's output [N][nchunks][2G]
};
static inline NkGnSumsPlan nk_gn_sums_plan(int N, int nparts, int G) {
  NkGnSumsPlan p = {};
  if (!(N > 0 && nparts > 0 && G > 0 && G <= GN_SUMS_MAXG)) { p.err = "N > 0 && nparts > 0 && G > 0 && G <= 32"; return p; }
  p.nchunks = GN_SUMS_CHUNKS;
  p.levels = nparts > GN_SUMS_ONE_LEVEL ? 2 : 1;
  p.l1 = {"l1", 0, p.levels == 2 ? (long)N * p.nchunks * 2 * G : 0};
  p.ws_floats = (long)N * p.nchunks * 2 * G + NORM_WS_PAD;      // whatever nparts: callers size the buffer once per layer
  if (p.levels == 2) norm_launch(p, NK_GN_REDUCE_L1, "gn_reduce_partials_l1_kernel", (unsigned)p.nchunks, (unsigned)N, 1, 256, 0, p.l1);
  norm_launch(p, NK_GN_REDUCE, "gn_reduce_partials_kernel", (unsigned)N, 1, 1, 1024, 0, p.l1);
  return p;
}

// ---- LayerNorm and RMSNorm over the last dim of [M][C] -----------------------------------------------------------------------------------------
enum RowNormKind { LN_FWD, LN_BWD_DX, LN_BWD_PARAMS, LN_BWD_ROWS, LN_BWD, RMS_FWD, RMS_FWD_RSTD, RMS_BWD };
struct NkRowNormPlan : NkNormPlan {
  int nch;                // the chunks-per-lane instance: 2, 3 or 4 (LayerNorm), 2, 4 or 8 (RMSNorm); 0: ln_bwd_param_kernel has none
  int part_rows;          // partial rows of ln_bwd_rows_kernel (one per block)
  int param_split;        // partial rows of ln_bwd_param_kernel
  int nrows;              // partial rows this kind writes and reduces: param_split (LN_BWD_PARAMS), part_rows (LN_BWD_ROWS, LN_BWD), else 0
  NkNormRegion part;      // the partial rows [rows][2][C] of this kind (LN_BWD_ROWS: in the caller's `part` buffer)
};
static inline NkRowNormPlan nk_rownorm_plan(int M, int C, int kind) {
  NkRowNormPlan p = {};
  const bool rms = kind == RMS_FWD || kind == RMS_FWD_RSTD || kind == RMS_BWD;
  const int maxch = rms ? RMS_MAXCH : LN_MAXCH;
  if (!(M > 0 && C > 0 && (C & 7) == 0)) { p.err = "M > 0 && C > 0 && (C & 7) == 0"; return p; }
  const int need = ((C >> 3) + 63) / 64;
  if (kind == LN_BWD_PARAMS) p.nch = 0;
  else if (rms) p.nch = need <= 2 ? 2 : (need <= 4 ? 4 : 8);
  else p.nch = need <= 2 ? 2 : need;
  p.param_split = (M + LNP_ROWS - 1) / LNP_ROWS;
  // one block per 16 rows (four per wave), at most 512 blocks (two per CU; 8 rows per wave at M = 16384)
  p.part_rows = (M + 4 * LNR_WAVES - 1) / (4 * LNR_WAVES);
  if (p.part_rows > LNR_MAX_BLOCKS) p.part_rows = LNR_MAX_BLOCKS;
  const unsigned rowgrid = (unsigned)((M + 3) / 4 < ROWNORM_MAX_BLOCKS ? (M + 3) / 4 : ROWNORM_MAX_BLOCKS), cb = (unsigned)((C + 63) / 64);
  // nk_layernorm_ws_floats (LN_BWD_PARAMS and LN_BWD): room for either split, whatever C -- the three-kernel backward and the one-pass backward
  // share the query, and ln_bwd_param_kernel takes any C % 8 == 0.  LN_BWD_ROWS writes the caller's `part` buffer: exactly its partial rows.
  const bool has_ws = kind == LN_BWD_PARAMS || kind == LN_BWD_ROWS || kind == LN_BWD;
  p.nrows = !has_ws ? 0 : (kind == LN_BWD_PARAMS ? p.param_split : p.part_rows);
  p.part = {"part", 0, (long)p.nrows * 2 * C};
  p.ws_floats = !has_ws ? 0 : kind == LN_BWD_ROWS ? p.part.len : (long)(p.param_split > LNR_MAX_BLOCKS ? p.param_split : LNR_MAX_BLOCKS) * 2 * C + NORM_WS_PAD;
  if (kind != LN_BWD_PARAMS && (C >> 3) > 64 * maxch) { p.err = rms ? "(C >> 3) <= 64 * RMS_MAXCH" : "(C >> 3) <= 64 * LN_MAXCH"; return p; }
  if (kind == RMS_BWD) {
    // RMSNorm backward (nk_rmsnorm_bwd): one wave per row, wave w walks rows w, w + nrows, ...; each wave leaves ONE partial row [C] of dgamma
    // in the workspace, and the single-writer reducer sums the rows in ascending order
    p.nrows = M < RMSB_MAX_ROWS ? M : RMSB_MAX_ROWS;
    p.part = {"part", 0, (long)p.nrows * C};
    p.ws_floats = p.part.len + NORM_WS_PAD;
    norm_launch(p, NK_RMS_BWD_ROWS, "rms_bwd_rows_kernel", (unsigned)((p.nrows + 3) / 4), 1, 1, 256, 0, p.part);
    norm_launch(p, NK_RMS_COLPART, "rms_colpart_reduce_kernel", cb, 1, 1, 1024, 0, p.part);
    return p;
  }
  if (kind == LN_FWD) norm_launch(p, NK_LN_FWD, "ln_fwd_kernel", rowgrid, 1, 1, 256, 0);
  if (kind == RMS_FWD || kind == RMS_FWD_RSTD) norm_launch(p, NK_RMS_FWD, "rms_fwd_kernel", rowgrid, 1, 1, 256, 0);
  if (kind == LN_BWD_DX) norm_launch(p, NK_LN_BWD_DX, "ln_bwd_dx_kernel", rowgrid, 1, 1, 256, 0);
  if (kind == LN_BWD_PARAMS) norm_launch(p, NK_LN_BWD_PARAM, "ln_bwd_param_kernel", (unsigned)p.param_split, (unsigned)((C + 127) / 128), 1, 256, 0, p.part);
  if (kind == LN_BWD_ROWS || kind == LN_BWD)
    norm_launch(p, NK_LN_BWD_ROWS, "ln_bwd_rows_kernel", (unsigned)p.part_rows, 1, 1, LNR_WAVES * 64, 2 * 2 * C * (int)sizeof(float), p.part);
  if (kind == LN_BWD_PARAMS || kind == LN_BWD) norm_launch(p, NK_LN_COLPART, "colpart_reduce_kernel", cb, 1, 1, 1024, 0, p.part);
  return p;
}

// ---- several column-partial reductions in one launch (nk_colpart_reduce_batch): 32 channels per block over the widest entry ---------------------
static inline NkNormPlan nk_colpart_batch_plan(const int* C, int n) {
  NkNormPlan p = {};
  if (!(n > 0 && n <= NK_COLPART_MAX)) { p.err = "b->n > 0 && b->n <= NK_COLPART_MAX"; return p; }
  int maxC = 0;
  for (int z = 0; z < n; ++z) {
    if (C[z] <= 0) { p.err = "b->C[z] > 0"; return p; }
    maxC = C[z] > maxC ? C[z] : maxC;
  }
  norm_launch(p, NK_COLPART_BATCH, "colpart_reduce_batch_kernel", (unsigned)((maxC + 31) / 32), (unsigned)n, 1, 1024, 0);
  return p;
}

// ---- bias gradients: out[b][N] (+)= column sums of nbatch row blocks of M rows ---------------------------------------------------------------
struct NkColsumPlan : NkNormPlan {      // ws_floats: nbatch times that of one entry (nk_colsum_ws_floats(M, N) = the plan of nbatch 1)
  int rows_per_block, nsplit;
  NkNormRegion part;      // [nbatch][nsplit][N]
};
static inline NkColsumPlan nk_colsum_plan(long M, int N, int nbatch) {
  NkColsumPlan p = {};
  if (!(M > 0 && N > 0 && (N & 7) == 0 && nbatch >= 1 && nbatch <= 65535)) { p.err = "M > 0 && N > 0 && (N & 7) == 0 && nbatch >= 1 && nbatch <= 65535"; return p; }
  // rows per workgroup: 64 up to 65 536 rows (the UNet's token counts), then as many as keeps the second stage at <= 1 024 partial rows
  // (the autoencoder's 2 M-row feature maps gave it 32 768 rows to walk: 80 us per bias gradient)
  long rows = CS_ROWS;
  while ((M + rows - 1) / rows > CS_MAX_SPLIT) rows *= 2;
  p.rows_per_block = (int)rows;
  p.nsplit = (int)((M + rows - 1) / rows);
  p.part = {"part", 0, (long)nbatch * p.nsplit * N};
  p.ws_floats = (long)nbatch * ((long)p.nsplit * N + NORM_WS_PAD);
  norm_launch(p, NK_CS_PARTIAL, "colsum_partial", (unsigned)p.nsplit, (unsigned)((N + 127) / 128), (unsigned)nbatch, 256, 0, p.part);
  norm_launch(p, NK_CS_REDUCE, "colsum_reduce", (unsigned)((N + 63) / 64), (unsigned)nbatch, 1, 1024, 0, p.part);
  return p;
}
