// Launch planner of the attention kernels: WHICH kernels run a problem, and how -- one pure host function, nk_attn_plan().
//
// Host-only: no kernel, no HIP call, no getenv, nothing but the descriptor (neurosis_hip.h), the constants below and libc, so a plan can be
// computed (and is tested: tests/test_attn_plan_cpu.py) on a machine without a GPU, and a plain C++ program can include this file.  The entry
// points (attention.hip: nk_attention_fwd, nk_attention_relbias_fwd, nk_attention_relbias_fwd_lse, nk_attention_bwd, nk_attention_bwd_causal, nk_attention_relbias_bwd) check the descriptor, ask for the plan, check what the
// plan says about the pointers, fill AttnParams once and walk the plan's launches; nk_attention_bwd_ws_floats answers from the same layout,
// so the workspace a caller sizes and the offsets the kernels are given cannot disagree.  Every selection rule of the family lives here, in
// the order nk_attn_plan applies them, with the measurements behind its thresholds; the switches arrive as an AttnEnv (attention.hip:
// attn_env(), the family's only getenv site).
#pragma once
#include "../../include/neurosis_hip.h"
#include <stdio.h>

#ifdef __HIPCC__
#define ATTN_HD __host__ __device__
#else
#define ATTN_HD
#endif

// ---- LDS images: each size once, for its kernel's launch and for the planner ----------------------------------------------------------------
#define ATTN64_RING_SMEM (3 * 2 * 64 * 128)                               // attn64_fwd_kernel, attn64_bwd_dq_kernel: [3 stages][K, V][64][128 B]
#define ATTN64_DKDV_SMEM (3 * (2 * 32 * 128 + 256))                       // attn64_bwd_dkdv_kernel: three stages of a Q' and a dO tile + 256 B of -delta / -lse2
constexpr int attn_ring_smem(int dp) { return 2 * 2 * 64 * (dp * 2 + 16); }         // attn_fwd_kernel, attn_bwd_dq_kernel: [2 stages][K, V][64][RS]
#define ATTN_RELBIAS_MAX_L 1024                                           // nk_attention_relbias_fwd: tokens of the self-attention (an 8 KiB table at the limit)
constexpr int attn_relbias_smem(int dp, int L) { return attn_ring_smem(dp) + (((2 * L - 1) * 4 + 15) & ~15); }      // attn_fwd_kernel<.., RELBIAS>: the ring + one head's table
constexpr int attn_dkdv_smem(int dp) { return 2 * (2 * 32 * (dp * 2 + 16) + 256); } // attn_bwd_dkdv_kernel
// attn_bwd_dq_kernel<.., RELBIAS>: behind the ring and the table, two strips of d_rel sums per wave (lanes 0-31 / 32-63), indexed by
// key - query_in_wave + 31: attn_drel_width(L) floats each, a multiple of 64 so that every 64-key tile's rows stay inside
constexpr int attn_drel_width(int L) { return ((L + 63) / 64) * 64 + 64; }
constexpr int attn_relbias_dq_smem(int dp, int L) { return attn_relbias_smem(dp, L) + 4 * 2 * attn_drel_width(L) * 4; }
constexpr int attn_relbias_dkdv_smem(int dp, int L) { return attn_dkdv_smem(dp) + (((2 * L - 1) * 4 + 15) & ~15); }
#define SMALL_DSROW 72                               // bytes per row of the dS^T image [96 keys][32 queries] (64 + 8: conflict-free 8-byte writes)
#define ATTN64_SMALL_SMEM (96 * 128 + 3 * (3 * 32 * 128 + 256 + 1024) + 2 * 96 * SMALL_DSROW)      // attn64_bwd_small_kernel: [K image][3 stages][2 dS^T buffers]
#define ATTN512_FWD_SMEM (5 * 32 * 1024)             // attn512.h: K stages 0-2, V stages 0-1: all 160 KiB of the CU's LDS
#define ATTN512_BWD_ROWS 32                          // attn512_bwd.h: A5B_ROWS, A5B_SMEM (attention.hip asserts they agree)
#define ATTN512_BWD_SMEM (4 * ATTN512_BWD_ROWS * 1024 + 2 * ATTN512_BWD_ROWS * 80)

// ---- the backward workspace (floats) ---------------------------------------------------------------------------------------------------------
struct Attn64Ws {       // layout of the backward workspace (floats) for head dim 64
  long ndelta, nlse2, qs, part;
  ATTN_HD static Attn64Ws make(long B, long H, long Lq) {
    Attn64Ws w;
    const long n = (B * H * Lq + 63) & ~63l;
    w.ndelta = 0; w.nlse2 = n; w.qs = 2 * n; w.part = 2 * n + B * H * Lq * 32;
    return w;
  }
};

// ---- the environment and the plan --------------------------------------------------------------------------------------------------------------
struct AttnEnv {
  int xcd;       // NK_ATTN_XCD: 0 keeps the 3-D grid (A/B runs); else the 1-D, XCD-aware launch (attn_wg)
  int attn64;    // NK_ATTN64: 0 = the generic kernels for head dim 64 as well (A/B switch of round 4)
  int small;     // NK_ATTN64_SMALL: 0 = cross-attention backward through the two-kernel path (A/B switch of round 4)
};
enum AttnPass { ATTN_PASS_FWD = 0, ATTN_PASS_BWD = 1, ATTN_PASS_BWD_CAUSAL = 2, ATTN_PASS_FWD_RELBIAS = 3, ATTN_PASS_FWD_RELBIAS_LSE = 4, ATTN_PASS_BWD_RELBIAS = 5 };
// the kernels and template instances the dispatch can select
enum AttnKernel {
  AK_FWD64, AK_FWD_DP64, AK_FWD_DP96, AK_FWD_DP160, AK_FWD512,
  AK_BWD64_SMALL, AK_BWD64_SMALL_CAUSAL, AK_BWD64_DQ, AK_BWD64_DKDV,
  AK_BWD_DQ_DP64, AK_BWD_DQ_DP96, AK_BWD_DQ_DP160, AK_BWD_DKDV_DP64, AK_BWD_DKDV_DP96, AK_BWD_DKDV_DP160,
  AK_DKV_REDUCE, AK_DELTA512, AK_BWD512_DQ, AK_BWD512_DKDV,
  AK_FWD_RELBIAS_DP64, AK_FWD_RELBIAS_DP96, AK_FWD_RELBIAS_DP160,
  AK_FWD_RELBIAS_LSE_DP64, AK_FWD_RELBIAS_LSE_DP96, AK_FWD_RELBIAS_LSE_DP160,
  AK_BWD_RELBIAS_DQ_DP64, AK_BWD_RELBIAS_DQ_DP96, AK_BWD_RELBIAS_DQ_DP160, AK_BWD_RELBIAS_DKDV_DP64, AK_BWD_RELBIAS_DKDV_DP96, AK_BWD_RELBIAS_DKDV_DP160,
  AK_DREL_REDUCE
};
// the caller's pointers, as bits of NkAttnPlan::need / ::align16 and as indices of the array attn_params() takes
enum AttnPtr { AP_Q = 0, AP_K, AP_V, AP_O, AP_LSE, AP_DO, AP_DQ, AP_DK, AP_DV, AP_WS, AP_REL, AP_DREL, AP_N };

struct NkAttnLaunch {
  int kernel;             // AttnKernel
  const char* name;       // what nk_check_launch reports (lib.launched())
  unsigned extent[3];     // (x blocks, heads, batch) as the kernel decodes them
  unsigned grid[3];       // the grid launched: the extent, or its product as a 1-D grid when gx > 0
  int gx;                 // AttnParams::gx of this launch: extent[0] under the XCD-aware 1-D mapping, 0 for a plain grid
  int block, smem;
};
struct NkAttnWs {         // offsets into the caller's workspace (floats; -1: not there), and the size nk_attention_bwd_ws_floats reports
  long ndelta, nlse2, qs; // head dim 64: -delta, -lse2 = -lse log2 e, Q' (Attn64Ws); the other kernels keep delta at ndelta = 0
  long part;              // the query splits' dK / dV partials [qsplit][2][B][Lk][H*D]
  long total;
};
struct NkAttnPlan {
  int n;                  // launches, in order: dQ, dK / dV, reduce -- or delta and the two instances of the head-dim-512 backward
  NkAttnLaunch launch[3];
  int qsplit;             // workgroups per key block along the query range (AttnParams::qsplit); partials at ws.part when > 1
  NkAttnWs ws;
  unsigned need;          // bit AttnPtr: the pointer must not be null
  unsigned align16;       // bit AttnPtr: ... and 16-byte aligned (the kernels of this path load or store it in 16-byte pieces)
  const char* err;        // the path refuses the descriptor's shape: the message of the NK_ERR_ARG
};

// one line per planned launch, for the launch log (nk_debug_launch_names) and the plan tests: name grid=x,y,z block smem gx qsplit part_offset ws_floats
static void nk_attn_plan_line(const NkAttnPlan& pl, int i, char* buf, size_t cap) {
  const NkAttnLaunch& L = pl.launch[i];
  snprintf(buf, cap, "%s grid=%u,%u,%u %d %d %d %d %ld %ld", L.name, L.grid[0], L.grid[1], L.grid[2], L.block, L.smem, L.gx, pl.qsplit,
           pl.qsplit > 1 ? pl.ws.part : -1l, pl.ws.total);
}

// ---- the rules, in the order nk_attn_plan applies them -------------------------------------------------------------------------------------
static int attn_dp(int D) { return D <= 64 ? 64 : (D <= 96 ? 96 : 160); }
// waves per workgroup: 4 x 32 rows.  (A 2-wave variant -- twice the workgroups for SDXL's L = 1024 layers, which give only 640 -- was
// measured SLOWER: forward 72 vs 65 us, backward 200 vs 181 us, twice the K/V tile loads per query row and half the waves sharing a tile.)
static constexpr int ATTN_NW = 4;
static unsigned attn_blocks(int L) { return (unsigned)((L + ATTN_NW * 32 - 1) / (ATTN_NW * 32)); }

// query splits of the one-kernel backward: enough workgroups for the chip (two per CU fit), at least two 32-query tiles each
static int attn_small_qsplit(const NkAttnDesc* d) {
  const int base = d->B * d->H;
  int s = 1;
  while (s < 64 && base * s * 2 <= 512 && d->Lq / (s * 2) >= 64) s *= 2;      // (at most one round of two workgroups per CU)
  return s;
}
static int attn_qsplit(const NkAttnDesc* d) {
  // a single key block (cross-attention, Lk = 77) gives only B*H workgroups that each walk the whole query range:
  // split the query range so the grid has >= ~512 workgroups
  if (d->Lk > 128 || d->Lq < 512) return 1;
  int base = d->B * d->H;
  int s = 1;
  while (s < 16 && base * s < 512 && d->Lq / (s * 2) >= 128) s *= 2;
  return s;
}

// The workspace of nk_attention_bwd: where the kernels of this descriptor keep what, and how much the caller must bring.  The size does not
// depend on the switches (callers size buffers that are captured into hipGraphs, and the switches are read per call): it holds the LARGER
// of the two split counts a head-dim-64 descriptor can run with, and the head-dim-64 layout whichever kernels run.
static NkAttnWs attn_ws(const NkAttnDesc* d, bool layout64) {
  NkAttnWs w = {0, -1, -1, 0, 0};
  const long rows = (long)d->B * d->H * d->Lq;
  const Attn64Ws w64 = Attn64Ws::make(d->B, d->H, d->Lq);
  if (layout64) { w.ndelta = w64.ndelta; w.nlse2 = w64.nlse2; w.qs = w64.qs; w.part = w64.part; }
  else w.part = (rows + 3) & ~3l;
  int s = attn_qsplit(d);
  if (d->D == 64 && d->Lk <= 96 && attn_small_qsplit(d) > s) s = attn_small_qsplit(d);
  const long part = s > 1 ? (long)s * 2 * d->B * d->Lk * d->H * d->D : 0;
  w.total = (d->D == 64 ? w64.part : rows) + part + 64;
  return w;
}

// ---- the plan's pieces -------------------------------------------------------------------------------------------------------------------------
// a launch over the 3-D extent (x, heads, batch); xcd: through the 1-D grid that gives every XCD a contiguous range of the (batch, head, x)
// order (attention.hip: attn_wg), unless NK_ATTN_XCD=0 keeps the 3-D grid
static void attn_launch(NkAttnPlan& pl, int kernel, const char* name, unsigned x, unsigned y, unsigned z, int block, int smem, bool xcd) {
  NkAttnLaunch& L = pl.launch[pl.n++];
  L.kernel = kernel; L.name = name; L.block = block; L.smem = smem;
  L.extent[0] = x; L.extent[1] = y; L.extent[2] = z;
  L.gx = xcd ? (int)x : 0;
  L.grid[0] = xcd ? x * y * z : x; L.grid[1] = xcd ? 1 : y; L.grid[2] = xcd ? 1 : z;
}
// more than one query split: the launch that sums their partials into dK / dV
static void attn_reduce(NkAttnPlan& pl, const NkAttnDesc* d) {
  if (pl.qsplit <= 1) return;
  long total = (long)d->B * d->Lk * ((long)d->H * d->D / 4);
  long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  attn_launch(pl, AK_DKV_REDUCE, "attn_dkv_reduce_kernel", (unsigned)blocks, 1, 1, 256, 0, false);
}
static constexpr unsigned attn_bits(int a, int b = -1, int c = -1, int d = -1, int e = -1) {
  return (1u << a) | (b < 0 ? 0 : 1u << b) | (c < 0 ? 0 : 1u << c) | (d < 0 ? 0 : 1u << d) | (e < 0 ? 0 : 1u << e);
}
static const unsigned ATTN_BITS_QKVO = attn_bits(AP_Q, AP_K, AP_V, AP_O), ATTN_BITS_GRADS = attn_bits(AP_DQ, AP_DK, AP_DV);

// The launches of one pass over descriptor `d`: a pure function of the descriptor and the environment.  attn_check (attention.hip) has
// checked what the rules rely on (positive sizes, D % 8 == 0, D <= 160 or D == 512).
static NkAttnPlan nk_attn_plan(const NkAttnDesc* d, int pass, const AttnEnv& env) {
  NkAttnPlan pl = {};
  const bool xcd = env.xcd != 0, a64 = d->D == 64 && env.attn64;
  const int dp = attn_dp(d->D);
  const unsigned H = (unsigned)d->H, B = (unsigned)d->B;
  pl.ws = attn_ws(d, a64);
  if (pass != ATTN_PASS_BWD) pl.ws = NkAttnWs{-1, -1, -1, -1, 0};      // no workspace

  if (pass == ATTN_PASS_FWD) {
    pl.need = ATTN_BITS_QKVO | (d->D == 512 ? 0 : attn_bits(AP_LSE));
    if (d->causal && d->Lq != d->Lk) { pl.err = "!d->causal || d->Lq == d->Lk"; return pl; }
    if (d->D == 512 || a64) pl.align16 = attn_bits(AP_O);      // 16-byte output stores
    if (d->D == 512) {
      // the VAE mid block's single head: one workgroup per CU, 512 registers per lane, all 160 KiB of LDS (attn512.h); lse may be null
      if (d->causal) { pl.err = "!d->causal"; return pl; }
      attn_launch(pl, AK_FWD512, "attn512_fwd_kernel", attn_blocks(d->Lq), H, B, 256, ATTN512_FWD_SMEM, xcd);
    } else if (a64) {
      attn_launch(pl, AK_FWD64, "attn64_fwd_kernel", attn_blocks(d->Lq), H, B, ATTN_NW * 64, ATTN64_RING_SMEM, xcd);
    } else {
      attn_launch(pl, dp == 64 ? AK_FWD_DP64 : dp == 96 ? AK_FWD_DP96 : AK_FWD_DP160, "attn_fwd_kernel", attn_blocks(d->Lq), H, B, ATTN_NW * 64,
                  attn_ring_smem(dp), xcd);
    }
    return pl;
  }

  if (pass == ATTN_PASS_FWD_RELBIAS) {
    // The T5 encoders' self-attention: the generic forward in its RELBIAS instantiation, whatever the head dim (the head-dim-64 kernel of
    // round 4 has no bias variant), with one head's table [Lq + Lk - 1] behind the K / V ring in LDS.  The output leaves in 8-byte stores.
    pl.need = ATTN_BITS_QKVO | attn_bits(AP_REL);
    if (d->causal) { pl.err = "!d->causal"; return pl; }
    if (d->D > 160) { pl.err = "d->D <= 160"; return pl; }
    if (!(d->Lq == d->Lk && d->Lk <= ATTN_RELBIAS_MAX_L)) { pl.err = "d->Lq == d->Lk && d->Lk <= ATTN_RELBIAS_MAX_L (relative-bias attention: self-attention over at most 1024 tokens)"; return pl; }
    attn_launch(pl, dp == 64 ? AK_FWD_RELBIAS_DP64 : dp == 96 ? AK_FWD_RELBIAS_DP96 : AK_FWD_RELBIAS_DP160, "attn_fwd_kernel<relbias>", attn_blocks(d->Lq), H, B,
                ATTN_NW * 64, attn_relbias_smem(dp, d->Lk), xcd);
    return pl;
  }

  if (pass == ATTN_PASS_FWD_RELBIAS_LSE || pass == ATTN_PASS_BWD_RELBIAS) {
    // The T5 encoders under training.  Forward: the RELBIAS instance that also writes the log-sum-exp of the biased scores (same launch shape
    // as ATTN_PASS_FWD_RELBIAS, same output bits).  Backward: the RELBIAS instances of the generic dQ and dK / dV kernels at every head dim
    // (64 as well), then the fixed-order sum of the dQ kernel's d_rel partial rows.  Self-attention over at most 1024 tokens, so
    // attn_qsplit() is 1: dK / dV leave directly.  Workspace: delta [B H L] | d_rel partials [B][H][query waves][attn_drel_width(L)].
    const bool fwd = pass == ATTN_PASS_FWD_RELBIAS_LSE;
    pl.need = ATTN_BITS_QKVO | attn_bits(AP_REL, AP_LSE) | (fwd ? 0 : ATTN_BITS_GRADS | attn_bits(AP_DO, AP_WS, AP_DREL));
    if (d->causal) { pl.err = "!d->causal"; return pl; }
    if (d->D > 160) { pl.err = "d->D <= 160"; return pl; }
    if (!(d->Lq == d->Lk && d->Lk <= ATTN_RELBIAS_MAX_L)) { pl.err = "d->Lq == d->Lk && d->Lk <= ATTN_RELBIAS_MAX_L (relative-bias attention: self-attention over at most 1024 tokens)"; return pl; }
    if (fwd) {
      attn_launch(pl, dp == 64 ? AK_FWD_RELBIAS_LSE_DP64 : dp == 96 ? AK_FWD_RELBIAS_LSE_DP96 : AK_FWD_RELBIAS_LSE_DP160, "attn_fwd_kernel<relbias,lse>",
                  attn_blocks(d->Lq), H, B, ATTN_NW * 64, attn_relbias_smem(dp, d->Lk), xcd);
      return pl;
    }
    const long rows = (long)d->B * d->H * d->Lq;
    pl.qsplit = 1;
    pl.ws = NkAttnWs{0, -1, -1, (rows + 3) & ~3l, 0};
    pl.ws.total = pl.ws.part + (long)d->B * d->H * attn_blocks(d->Lq) * ATTN_NW * attn_drel_width(d->Lk) + 64;
    attn_launch(pl, dp == 64 ? AK_BWD_RELBIAS_DQ_DP64 : dp == 96 ? AK_BWD_RELBIAS_DQ_DP96 : AK_BWD_RELBIAS_DQ_DP160, "attn_bwd_dq_kernel<relbias>",
                attn_blocks(d->Lq), H, B, ATTN_NW * 64, attn_relbias_dq_smem(dp, d->Lk), xcd);
    attn_launch(pl, dp == 64 ? AK_BWD_RELBIAS_DKDV_DP64 : dp == 96 ? AK_BWD_RELBIAS_DKDV_DP96 : AK_BWD_RELBIAS_DKDV_DP160, "attn_bwd_dkdv_kernel<relbias>",
                attn_blocks(d->Lk), H, B, ATTN_NW * 64, attn_relbias_dkdv_smem(dp, d->Lk), xcd);
    attn_launch(pl, AK_DREL_REDUCE, "attn_drel_reduce_kernel", (unsigned)((2 * d->Lk - 1 + 63) / 64), H, 1, 1024, 0, false);
    return pl;
  }

  if (pass == ATTN_PASS_BWD_CAUSAL) {
    // Backward of the CAUSAL forward: head dim 64, Lq == Lk <= 96 (77 tokens): the one-kernel backward in its causal instantiation, one query
    // split, so dK / dV leave directly and no workspace is needed
    pl.need = ATTN_BITS_QKVO | ATTN_BITS_GRADS | attn_bits(AP_LSE, AP_DO);
    pl.align16 = ATTN_BITS_QKVO | ATTN_BITS_GRADS | attn_bits(AP_DO);
    if (!(d->causal && d->D == 64 && d->Lq == d->Lk && d->Lk <= 96)) { pl.err = "d->causal && d->D == 64 && d->Lq == d->Lk && d->Lk <= 96"; return pl; }
    pl.qsplit = 1;
    attn_launch(pl, AK_BWD64_SMALL_CAUSAL, "attn64_bwd_small_kernel<causal>", 1, H, B, 256, ATTN64_SMALL_SMEM, xcd);
    return pl;
  }

  pl.need = ATTN_BITS_QKVO | ATTN_BITS_GRADS | attn_bits(AP_LSE, AP_DO, AP_WS);
  if (d->causal) { pl.err = "!d->causal"; return pl; }   // the causal variant has an entry point of its own (nk_attention_bwd_causal)
  if (d->D == 512) {
    // head dim 512 (the VAE mid block under autoencoder training): delta = rowsum(dO o O), then the same kernel template twice --
    // dQ per 32-query block, dK / dV per 32-key block -- recomputing the scores tile by tile from the forward's log-sum-exp (attn512_bwd.h)
    pl.align16 = ATTN_BITS_QKVO | attn_bits(AP_DO);
    const long rows = (long)d->B * d->H * d->Lq;
    attn_launch(pl, AK_DELTA512, "attn512_delta_kernel", (unsigned)((rows + 3) / 4), 1, 1, 256, 0, false);
    attn_launch(pl, AK_BWD512_DQ, "attn512_bwd_kernel<0>", (unsigned)((d->Lq + ATTN512_BWD_ROWS - 1) / ATTN512_BWD_ROWS), H, B, 256, ATTN512_BWD_SMEM, false);
    attn_launch(pl, AK_BWD512_DKDV, "attn512_bwd_kernel<1>", (unsigned)((d->Lk + ATTN512_BWD_ROWS - 1) / ATTN512_BWD_ROWS), H, B, 256, ATTN512_BWD_SMEM, false);
    return pl;
  }
  if (a64) pl.align16 = ATTN_BITS_GRADS | attn_bits(AP_WS);      // 16-byte gradient stores; -delta, -lse2 and Q' by DMA
  if (a64 && d->Lk <= 96 && env.small) {
    // head dim 64, at most 96 keys (cross-attention): everything in one kernel (+ the sum of the query splits' dK / dV partials)
    pl.qsplit = attn_small_qsplit(d);
    attn_launch(pl, AK_BWD64_SMALL, "attn64_bwd_small_kernel", (unsigned)pl.qsplit, H, B, 256, ATTN64_SMALL_SMEM, xcd);
  } else if (a64) {
    // head dim 64: the dQ kernel (which also writes -delta, -lse2 and Q' into the workspace), then dK / dV
    pl.qsplit = attn_qsplit(d);
    attn_launch(pl, AK_BWD64_DQ, "attn64_bwd_dq_kernel", attn_blocks(d->Lq), H, B, ATTN_NW * 64, ATTN64_RING_SMEM, xcd);
    attn_launch(pl, AK_BWD64_DKDV, "attn64_bwd_dkdv_kernel", attn_blocks(d->Lk) * pl.qsplit, H, B, ATTN_NW * 64, ATTN64_DKDV_SMEM, xcd);
  } else {
    // order: dQ kernel first (it also produces delta = rowsum(dO * O) for the dK / dV kernel), then dK / dV
    pl.qsplit = attn_qsplit(d);
    attn_launch(pl, dp == 64 ? AK_BWD_DQ_DP64 : dp == 96 ? AK_BWD_DQ_DP96 : AK_BWD_DQ_DP160, "attn_bwd_dq_kernel", attn_blocks(d->Lq), H, B, ATTN_NW * 64,
                attn_ring_smem(dp), xcd);
    attn_launch(pl, dp == 64 ? AK_BWD_DKDV_DP64 : dp == 96 ? AK_BWD_DKDV_DP96 : AK_BWD_DKDV_DP160, "attn_bwd_dkdv_kernel", attn_blocks(d->Lk) * pl.qsplit, H, B,
                ATTN_NW * 64, attn_dkdv_smem(dp), xcd);
  }
  attn_reduce(pl, d);
  return pl;
}
