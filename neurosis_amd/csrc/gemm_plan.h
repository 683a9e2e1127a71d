// Launch planner of the MFMA tile engine: WHICH kernel runs a problem, and how -- one pure host function, nk_gemm_plan().
//
// Host-only: no kernel, no HIP call, nothing but nk_gemm.h, the tile-shape constants below and libc, so a plan can be computed (and is
// tested: tests/test_gemm_plan_cpu.py) on a machine without a GPU.  nk_gemm_dispatch (gemm.hip) checks its arguments, asks for the plan,
// prepares what the plan says the launch needs (zero-filled destinations, the stream-K workspace) and launches the plan's kernel; the side
// queries (nk_halo_tiles_per_image, nk_geglu_fwd_fusable) answer from the same plan, so they cannot disagree with the dispatch.
// Every selection rule of the engine lives here, in the order nk_gemm_plan applies them, with the measurements that justify its thresholds;
// every environment switch of the engine is read in tile_env() and nowhere else.
#pragma once
#include "nk_gemm.h"
#include <stdio.h>
#include <stdlib.h>

enum { OP_KC = 0, OP_KCG = 1, OP_MC = 2, OP_MCT = 3, OP_MCG = 4 };

// ---- tile shapes: each constant once, for its kernel and for the planner ------------------------------------------------------------------
// 128 x 128 x 64 kernels (gemm.hip: nk_gemm_dma_kernel, nk_gemm_ring_kernel, nk_gemm_sk_kernel)
#define BM 128
#define BN 128
#define BK 64
#define GROUP_M 8
#define CS_LD 132                            // fp32 epilogue staging row stride (floats)
#define V2_OPND_BYTES 16384
#define V2_STAGE_BYTES (2 * V2_OPND_BYTES)
#define V2_SMEM_BYTES (BM * CS_LD * 4)   // 67584: epilogue staging is the larger need (2 stages = 65536)
#define RING_NS 4
#define RING_SMEM_BYTES (RING_NS * V2_STAGE_BYTES)    // 131072 >= 67584 (epilogue staging)
#define SK_NT 512
#define SK_SMEM_BYTES (2 * V2_STAGE_BYTES)
#define SK_MAX_GRID 512
// 64 x 64 ring (nk_gemm_ring64_kernel)
#define R64_NS 8
#define R64_OPND 8192
#define R64_STAGE (2 * R64_OPND)
#define R64_SMEM (R64_NS * R64_STAGE)      // 131072
// 256 x 256 kernels (nk_gemm_xl_kernel, nk_gemm_xl2g_kernel)
#define XL_BM 256
#define XL_BN 256
#define XL_STAGE_BYTES 65536
#define XL_SMEM_BYTES (2 * XL_STAGE_BYTES)
// two-group staggered ring with producer waves (gemm_g2.h)
#define G2_BM 128
#define G2_STAGE_BYTES 36864                     // A image 16 KiB + B image up to 20 KiB
#define G2_NS 4
#define G2_SMEM_BYTES (G2_NS * G2_STAGE_BYTES)   // 147456
// 160-row weight-gradient kernel (gemm_w160.h): a stage is [64 tokens][160 + BN rows] bf16
#define W160_BM 160
#define W160_NS 3
constexpr int w160_smem(int bn) { return W160_NS * (W160_BM + bn) * 128; }      // 122880 / 110592
// halo-tile convolution (conv_halo.h has the why of the two rings): 32-pixel tile rows; the 128-column tile runs a four-stage weight ring and
// four producer waves, the 160-column tile three stages and eight waves
#define CH_TW 32
#define CH_HW (CH_TW + 2)
#define CH_BSTAGE 20480                         // weights of one k-step: up to 160 rows x 128 B
#define CH_NS 3
#define CH_BSTAGE_DEEP 16384
#define CH_NS_DEEP 4
constexpr int halo_threads(int bn) { return bn == 128 ? 768 : 512; }
constexpr int halo_hpieces(int th) { return ((((th + 2) * CH_HW + 7) / 8) + 1) & ~1; }      // 1 KiB pieces (8 pixels each) of a halo, even: 26 / 44
constexpr int halo_smem(int bn, int th) { return 2 * halo_hpieces(th) * 1024 + (bn == 128 ? CH_NS_DEEP * CH_BSTAGE_DEEP : CH_NS * CH_BSTAGE); }
// halo-tile convolution weight gradient (conv_wgrad_halo.h)
#define WH_TH 4
#define WH_TW 32
#define WH_HS 48                                   // halo slots per row (34 used)
#define WH_X_BYTES ((WH_TH + 2) * WH_HS * 128)     // 36864
#define WH_DY_BYTES (WH_TH * WH_TW * 256)          // 32768
#define WH_STAGE (WH_X_BYTES + WH_DY_BYTES)        // 69632
#define WH_SMEM (2 * WH_STAGE)                     // 139264
#define WH_BCO 128
#define WH_BCI 64

// ---- the environment: every switch of the tile engine, read here and nowhere else ---------------------------------------------------------
struct TileEnv {
  int xl;            // NK_GEMM_XL: 0 = never the 256 x 256 kernels.  Read ONCE per process (the others per call: tools and tests flip them in-process)
  int g2;            // NK_GEMM_G2: 0 = never; 1 (default) = by shape; 2 = every eligible launch (A/B runs)
  int sk;            // NK_GEMM_SK: see use_sk
  int sk_debug;      // NK_SK_DEBUG=2 (fault injection for tests/test_health_gpu.py): every stream-K fix-up wait gives up at once
  int w160;          // NK_GEMM_W160: 0 = never; 1 (default) = by shape; 2 = every eligible launch (tests: ragged shapes, K splits)
  int w160_split;    // NK_GEMM_W160_SPLIT: the token split of NK_GEMM_W160=2
  int krot;          // NK_GEMM_KROT: 1 (default) = rotated k order per XCD (OpG2::rotate; the two-group, 128 x 128 double-buffer and 256 x 256 two-group kernels) in launches of at least eight slabs; 0 = every XCD starts at k = 0 (A/B runs)
  int r64;           // NK_GEMM_R64: 0 = never (A/B runs)
  int halo;          // NK_CONV_HALO=0 keeps every convolution on the gather kernels (A/B runs)
  int wgrad_halo;    // NK_CONV_WGRAD_HALO: 0 = never (A/B runs, tests), 2 = every eligible shape, unset / 1 = by shape
};
static int env_int(const char* e, int unset) { return e ? atoi(e) : unset; }
static int env_not0(const char* e) { return !(e && e[0] == '0'); }
static TileEnv tile_env() {
  static const int xl = env_not0(getenv("NK_GEMM_XL"));
  TileEnv t;
  t.xl = xl;
  t.g2 = env_int(getenv("NK_GEMM_G2"), 1);
  t.sk = env_int(getenv("NK_GEMM_SK"), 4);
  t.sk_debug = env_int(getenv("NK_SK_DEBUG"), 0) & 2;
  t.w160 = env_int(getenv("NK_GEMM_W160"), 1);
  t.w160_split = env_int(getenv("NK_GEMM_W160_SPLIT"), 1);
  t.krot = env_int(getenv("NK_GEMM_KROT"), 1) != 0;
  t.r64 = env_not0(getenv("NK_GEMM_R64"));
  t.halo = env_not0(getenv("NK_CONV_HALO"));
  t.wgrad_halo = env_int(getenv("NK_CONV_WGRAD_HALO"), 1);
  return t;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------
enum NkFamily { NK_FAM_NONE = 0, NK_FAM_RING64, NK_FAM_G2P, NK_FAM_XL, NK_FAM_XL2G, NK_FAM_SK, NK_FAM_RING, NK_FAM_DMA, NK_FAM_W160, NK_FAM_HALO, NK_FAM_WGRAD_HALO };
struct NkGemmPlan {
  int family;             // NkFamily
  int bn;                 // variant: column-tile width (two-group, 160-row and halo kernels: 160 or 128)
  int halo_rows;          //          halo kernel: image rows of a tile (8 or 4)
  int flag;               //          halo: statistics epilogue; halo weight gradient: bias gradient; 256 x 256 two-group: fused GEGLU forward
  const char* name;       // what nk_check_launch reports (lib.launched()): the kernel with its template arguments
  unsigned grid[3];
  int block, smem;
  int splitk;             // workgroups sharing one output tile through atomics (blockIdx.y; the halo weight gradient's pixel ranges)
  int ksplit_len, accumulate, k_rotate, group_m, sk_chunked;      // the launcher's fields of NkGemmParams, as the kernel will see them
  bool zero_c, zero_dbias;      // zero-fill the destination / the bias gradient(s) first (split partials meet through atomics)
  int tiles_per_image;    // halo kernel: pixel tiles per image (= rows per image of the statistics epilogue's partials)
  const char* err;        // the problem cannot be launched as asked: the message of the NK_ERR_ARG
};

// one line per plan, for the launch log (nk_debug_launch_names) and the plan tests: name grid=x,y,z block smem splitk ksplit_len acc zero krot gm chunk
static void nk_plan_line(const NkGemmPlan& pl, char* buf, size_t cap) {
  snprintf(buf, cap, "%s grid=%u,%u,%u %d %d %d %d %d %d %d %d %d", pl.name, pl.grid[0], pl.grid[1], pl.grid[2], pl.block, pl.smem, pl.splitk,
           pl.ksplit_len, pl.accumulate, (pl.zero_c ? 1 : 0) | (pl.zero_dbias ? 2 : 0), pl.k_rotate, pl.group_m, pl.sk_chunked);
}

// ---- the rules, in the order nk_gemm_plan applies them --------------------------------------------------------------------------------------
static int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static int nbatch1(const NkGemmParams& p) { return p.nbatch ? p.nbatch : 1; }
static bool has_dbias(const NkGemmParams& p) {
  bool any = p.dbias != nullptr;
  for (int z = 0; z < p.nbatch && z < NK_MAX_BATCH; ++z) any = any || p.dbias_b[z] != nullptr;
  return any;
}

// rotated k order per XCD, in launches of at least eight slabs
static bool k_rotate_on(const TileEnv& env, int k_len) { return env.krot && (k_len + BK - 1) / BK >= 8; }

static bool use_xl(const TileEnv& env, const NkGemmParams& p, int amode, int bmode, int out_f32, int splitk) {
  if (!env.xl || p.nbatch || out_f32 || splitk != 1 || bmode != OP_KC || !(amode == OP_KC || amode == OP_KCG)) return false;
  const long ntn = (p.N + XL_BN - 1) / XL_BN;
  const long tiles = (long)((p.M + XL_BM - 1) / XL_BM) * ntn;
  // at least ~one workgroup per CU, and no more than 12 % of the last column tile wasted (N = 320 / 640 would idle 37 % / 17 %)
  // ... and rounds of 256 workgroups that are at least 80 % full (320 tiles would run as two rounds at 62 %: measured 775 vs 847 TFLOP/s
  // against the 128 x 128 kernel's finer rounds)
  const long rounds = (tiles + 255) / 256;
  return tiles >= 224 && tiles * 10 >= rounds * 256 * 8 && ntn * XL_BN * 100 <= (long)p.N * 112 && p.K >= 4 * BK;
}

static bool halo_shape_ok(const NkGemmParams& p) {
  const NkGather& g = p.ga;
  if (!p.halo_nb || g.KW != 3 || p.K != 9 * g.C || g.rs != 1 || g.ks != 1 || g.div != 1 || g.off_h != -1 || g.off_w != -1) return false;
  if (g.Ho != g.H || g.Wo != g.W || (g.C & 63) || p.alpha != 1.0f || p.nbatch) return false;
  if (p.N % 160 && p.N % 128) return false;
  if ((p.N & 7) || (p.ldc & 7) || (p.residual && (p.ldr & 7))) return false;
  return true;
}
// column-tile width of the halo-tile launch for N output channels: THE rule (the statistics epilogue's partial layout depends on it)
static int halo_bn(int N) { return N % 160 == 0 ? 160 : 128; }
// tile height for this problem: 8-row tiles where they still give about one workgroup per CU, else 4-row tiles; 0 = the patches
// would cover the image with too much waste (ragged small images keep the gather kernels)
static int halo_tile_rows(const NkGemmParams& p) {
  const NkGather& g = p.ga;
  const int bn = halo_bn(p.N);
  const long txn = (g.W + CH_TW - 1) / CH_TW;
  for (int th = 8; th >= 4; th -= 4) {
    const long tyn = (g.H + th - 1) / th;
    const long cover = txn * CH_TW * tyn * th;
    if (cover * 100 > (long)g.H * g.W * 115) continue;
    const long tiles = (long)p.halo_nb * txn * tyn * (p.N / bn);
    if (th == 8 && tiles < 224) continue;
    return th;
  }
  return 0;
}
static bool use_halo(const TileEnv& env, const NkGemmParams& p, int amode, int bmode, int out_f32) {
  if (amode != OP_KCG || bmode != OP_KC || out_f32) return false;
  if (!env.halo) return false;
  return halo_shape_ok(p) && halo_tile_rows(p) != 0;
}

static bool wgrad_halo_shape_ok(const NkGemmParams& p) {
  const NkGather& g = p.gb;
  if (!p.halo_nb || g.KW != 3 || p.N != 9 * g.C || g.rs != 1 || g.ks != 1 || g.div != 1 || g.off_h != -1 || g.off_w != -1) return false;
  if (g.Ho != g.H || g.Wo != g.W || (g.C % WH_BCI) || (p.M & 7) || p.nbatch || p.ldc != p.N || p.lda != p.M) return false;
  if (p.K != (long)p.halo_nb * g.H * g.W) return false;
  // ragged small images (the 26-wide level of a 1216 x 832 bucket) would spend the tile on padding: they keep the gather kernel
  const long cover = (long)((g.W + WH_TW - 1) / WH_TW) * WH_TW * ((g.H + WH_TH - 1) / WH_TH) * WH_TH;
  return cover * 100 <= (long)g.H * g.W * 125;
}
// pixel-range splits per (co, ci) block: rounds of 256 workgroups at ~3 us per pixel tile against the atomics the splits cost (1.3 TB/s)
static int wgrad_halo_splits(const NkGemmParams& p, int& per) {
  const NkGather& g = p.gb;
  const long T = (long)p.halo_nb * ((g.W + WH_TW - 1) / WH_TW) * ((g.H + WH_TH - 1) / WH_TH);
  const long nblk = (long)((p.M + WH_BCO - 1) / WH_BCO) * (g.C / WH_BCI);
  const double dw_bytes = (double)p.M * p.N * 4.0;
  double best = 1e30;
  int best_s = 1;
  for (int s = 1; s <= 64 && s <= T; ++s) {
    const long tiles = (T + s - 1) / s;
    const long rounds = (nblk * s + 255) / 256;
    const double cost = (double)rounds * (tiles * 3.0e-6 + 4.0e-6) + (s > 1 ? s * dw_bytes / 1.3e12 : dw_bytes / 4.0e12);
    if (cost < best * 0.97) { best = cost; best_s = s; }     // (a larger S must win by 3 %: fewer atomics at a tie)
  }
  per = (int)((T + best_s - 1) / best_s);
  return (int)((T + per - 1) / per);
}
// By shape (tools/bench_conv_wgrad.py, profiles/r04_conv_wgrad.txt, one box, alternating): the kernel wins where the reduction is long -- the
// 64^2 and 128^2 levels, x1.0-1.8 -- and where the (co, ci) blocks fill the chip without splitting the pixel range (1280 -> 1280 at 32^2: 200
// blocks, x1.12); few pixels into a half-empty grid (640 -> 1280 at 32^2: 100 blocks, two splits, as many atomics as products: x0.69) stay
// with the gather kernel.
static bool use_wgrad_halo(const TileEnv& env, const NkGemmParams& p, int amode, int bmode, int out_f32) {
  if (amode != OP_MC || bmode != OP_MCG || !out_f32) return false;
  const int mode = env.wgrad_halo;
  if (!mode || !wgrad_halo_shape_ok(p)) return false;
  if (mode == 2) return true;
  if (p.M < 64) return false;
  const long nblk = (long)((p.M + WH_BCO - 1) / WH_BCO) * (p.gb.C / WH_BCI);
  return p.K >= 16384 || nblk >= 180;
}

struct W160Plan { int bn, splitk; };
// tile width and token split for this weight gradient, {0, 0} when the kernel does not take it
static W160Plan w160_plan(const TileEnv& env, const NkGemmParams& p, int amode, int bmode, int out_f32, int allow_splitk) {
  const int mode = env.w160;
  if (!mode || amode != OP_MC || bmode != OP_MC || !out_f32) return {0, 0};
  if (p.nbatch > NK_MAX_BATCH) return {0, 0};
  const int nb = p.nbatch ? p.nbatch : 1;
  const long nk = (p.K + BK - 1) / BK;
  if (mode == 2) {      // tests: everything, split when asked to by a second variable
    int sk = env.w160_split;
    if (sk < 1 || !allow_splitk || nk < 2 * sk) sk = 1;
    return {p.N % 160 == 0 || p.N % 128 != 0 ? 160 : 128, sk};
  }
  if (p.M % W160_BM) return {0, 0};                        // rows of the weight in whole 160-row tiles (every 640 / 1280-level Linear)
  if (nk < 32) return {0, 0};                              // (the 308-token context projections stay where they are)
  W160Plan best = {0, 0};
  double best_us = 1e30;
  for (int bn = 160; bn >= 128; bn -= 32) {
    const long ntn = (p.N + bn - 1) / bn;
    if (ntn * bn * 100 > (long)p.N * 104) continue;        // at most 4 % of a column tile wasted
    const long tiles = (long)(p.M / W160_BM) * ntn * nb;
    for (int sk = 1; sk <= 8; ++sk) {
      if (sk > 1 && (!allow_splitk || nk / sk < 32)) break;
      const long wgs = tiles * sk, rounds = (wgs + 255) / 256;
      if ((double)wgs < 0.85 * (double)(rounds * 256)) continue;
      // calibrated on tools/bench_w160.py (round 6): a 160 x 160 tile takes ~0.66 us per 64-token slab at the clock the chip holds under this
      // load; the atomics of a split launch all arrive at its end (one round: nothing left to hide them behind) at ~0.6 TB/s
      const double us = (double)rounds * (double)((nk + sk - 1) / sk) * 0.66 * bn / 160.0 + (sk > 1 ? sk * (double)p.M * p.N * nb * 4.0 / 0.6e6 : 0.0);
      if (us < best_us) { best_us = us; best = {bn, sk}; }
    }
  }
  return best;
}

// Dense k-contiguous bf16-output launches of at most 512 rows whose 128 x 128 grid would leave most CUs idle.
static bool use_ring64(const TileEnv& env, const NkGemmParams& p, int amode, int bmode, int out_f32) {
  if (amode != OP_KC || bmode != OP_KC || out_f32 || p.nbatch || p.geglu_u || p.geglu_h || p.stats_part) return false;
  if (!env.r64) return false;
  if (p.M > 512 || p.K < 4 * BK) return false;
  // one round at one workgroup per CU (the ring takes 128 KiB of LDS): 308 x 1280 -> 100 tiles, x 3072 -> 240; at 308 x 3840 / 5120 (300 / 400
  // tiles: two rounds) the 128 x 128 kernels are faster again (16.8 / 17.1 against 19.2 / 19.9 us, tools/bench_skinny.py)
  const long t64 = (long)((p.M + 63) / 64) * ((p.N + 63) / 64);
  return t64 <= 256;
}

// two-group tile width for this N: 160 when it divides N (1280, 640, 1920, 3840, 5120, 10240 ...), else 128 when that wastes little
static int g2_bn(int N) {
  if (N % 160 == 0) return 160;
  const int ntn = (N + 127) / 128;
  return (long)ntn * 128 * 100 <= (long)N * 112 ? 128 : 0;
}
static bool use_g2(const TileEnv& env, const NkGemmParams& p, int amode, int bmode, int out_f32, int splitk) {
  const int mode = env.g2;
  if (!mode || splitk != 1) return false;
  const bool conv = amode == OP_KCG;
  if (conv) {   // the gather modes decode the tap once per slab: channels in whole 64-deep slabs, full slabs only
    if (p.ga.C % 64 || p.K % 64) return false;
    if (bmode == OP_MCT && p.tw.fCout.d % 64) return false;
  }
  if (!((amode == OP_KC && bmode == OP_KC) || (amode == OP_KC && bmode == OP_MC) || (amode == OP_MC && bmode == OP_MC) ||
        (conv && (bmode == OP_KC || bmode == OP_MCT))))
    return false;
  if (p.K < 2 * BK) return false;
  // not the SINGLE weight gradients: in the two-stream step they do better with the co-resident 128 x 128 kernels (187.6 vs 189.0 ms);
  // the batched ones (three 1280 x 1280 per launch = 240 tiles, one round) do better here: 49.7 vs 65.4 us alone, 177.2 vs 177.6 ms/step
  if (amode == OP_MC && bmode == OP_MC && !p.nbatch) return false;      // (round 4, with the producer-wave kernel: 158.0 / 157.9 vs 158.0 / 158.9 ms per step -- still nothing)
  const int bn = g2_bn(p.N);
  if (!bn) return false;
  if (mode == 2) return true;
  // By shape (tools/bench_g2.py, interleaved A/B on the SDXL Linear shapes).  The kernel wins where its tiles come out in ONE or
  // TWO whole rounds of 256 (one workgroup per CU: 4096 x 1280 -> 256 tiles, 16384 x 640 -> 512, 3840 x 1280 -> 240, three batched
  // 1280 x 1280 weight gradients -> 240) -- forward +12..29 %, dgrad +5..27 %, wgrad +32..35 % -- and where K is long enough (>= 40
  // slabs) to amortise a tile's prologue and epilogue over up to four rounds.  It loses where many short rounds follow each other
  // (at one workgroup per CU nothing overlaps a tile's epilogue: 16384 x 1280 x 640 forward 0.87x, 65536 x 1280 x 1280 0.67x) and
  // against the 256 x 256 two-group kernel on the shapes that one takes (4096 x 3840 / 10240 x 1280 forward 0.76-0.80x).
  const long tiles = (long)((p.M + G2_BM - 1) / G2_BM) * ((p.N + bn - 1) / bn) * (p.nbatch ? p.nbatch : 1);
  const long rounds = (tiles + 255) / 256;
  const double fill = (double)tiles / (double)(rounds * 256);
  const long nk = (p.K + BK - 1) / BK;
  if (fill < 0.85) return false;
  return rounds <= 2 || (rounds <= 4 && nk >= 40);
}

// NK_GEMM_SK: 0 = never, 1 = always, 2 = fp32 outputs (weight gradients) only, 3 = by shape, 4 (default) = by shape and
// bf16 outputs only (weight gradients run on the side stream, where non-persistent grids back-fill the main stream's
// kernels: measured 203.7 ms/step vs 206.3 without stream-K, 211 with it on every kernel).  By shape:
// stream-K where the data-parallel grid fills the chip badly or would need split-K, the plain kernel for big grids
// (measured 5-19 % faster there: its workgroups drift out of phase, the persistent ones load and store in lock-step).
static bool use_sk(const TileEnv& env, const NkGemmParams& p, int out_f32) {
  const int mode = env.sk;
  if (mode == 0) return false;
  if (mode == 1) return true;
  if (mode == 2) return out_f32 != 0;
  if (mode == 4 && out_f32) return false;     // by shape, bf16 outputs (main-stream forward / dgrad) only
  const long tiles = (long)((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN) * (p.nbatch ? p.nbatch : 1);
  const long nk = (p.K + BK - 1) / BK;
  const long rounds = (tiles + 511) / 512;
  const double fill = (double)tiles / (double)(rounds * 512);
  if (tiles >= 1024 && fill >= 0.8) return false;
  if (tiles >= 512 && fill >= 0.95) return false;
  return nk >= 24;    // a fix-up costs about as much as 6-8 k-steps
}

static int pick_splitk(int M, int N, int K, int max_split) {
  // Split K only for grids far below one workgroup per CU.  Each extra split costs M*N*4 bytes of fp32 atomics at the
  // chip-wide ~1.3 TB/s atomic rate (MI355X_MICROARCH.md), which is 923/K_red of the GEMM's own time per split -- 22 %
  // per split at a 4096-row reduction -- while under-filled grids are back-filled by the kernels running concurrently
  // on the other stream (dgrad chain vs weight-gradient stream).
  int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int nk = (K + BK - 1) / BK;
  const int lo = 96, hi = 192;
  // ... except long reductions into grids that leave half the 512 slots empty (the 128^2- and 64^2-level convolution weight gradients:
  // 65 536 / 16 384 pixels = 1 024 / 256 k-steps into 135-225 tiles; the 64^2-level Linear ones): the atomics of one extra split are a few
  // per cent of such a launch and two splits fill the slots -- 65536 x 320 x 5760: 938 -> 587 us, x 8640: 972 -> 617; step -1 ms (round 3)
  if (tiles >= lo && tiles * 2 <= 512 && nk >= 256 && max_split >= 2) return 2;
  if (tiles >= lo) return 1;
  int s = 1;
  while (s < max_split && tiles * s < hi && nk / (s * 2) >= 8) s *= 2;
  return s;
}

// ---- the plan's pieces ------------------------------------------------------------------------------------------------------------------------
static void plan_kernel(NkGemmPlan& pl, int family, const char* name, long gx, int gy, int gz, int block, int smem) {
  pl.family = family; pl.name = name;
  pl.grid[0] = (unsigned)gx; pl.grid[1] = (unsigned)gy; pl.grid[2] = (unsigned)gz;
  pl.block = block; pl.smem = smem;
}
// K split over `splits` workgroups per tile: k range of one (whole slabs), and THE accumulate policy -- 0 = overwrite, 1 = add, 2 = the
// destination is known to be zero (flat gradient buffer right after zero_grad).  Split partials are summed with fp32 atomics, which need a
// zeroed destination (weight gradient and fused bias gradient): zero-filled first unless it is being added to or known zero; a single
// split stores (or adds) plainly, and "known zero" never costs a zero-fill
static void plan_split(NkGemmPlan& pl, const NkGemmParams& p, int splits) {
  pl.splitk = splits;
  pl.ksplit_len = cdiv(cdiv(p.K, BK), splits) * BK;
  if (splits > 1 && pl.accumulate == 0) {
    pl.zero_c = true; pl.zero_dbias = has_dbias(p);
    pl.accumulate = 1;
  } else if (pl.accumulate == 2) {
    pl.accumulate = splits > 1 ? 1 : 0;
  }
}
// the 256 x 256 kernels by operand mode: dense k-contiguous A -> the two-group phased kernel (+3..6 % on the Linear shapes); gathered A -> the
// 16-wave kernel (the gather's address arithmetic would sit in the phased kernel's read phases, where only one wave per SIMD is there to
// absorb it: conv forward 781-785 vs 835-840 TFLOP/s)
static void plan_xl(NkGemmPlan& pl, const TileEnv& env, const NkGemmParams& p, int amode) {
  const long tiles = (long)cdiv(p.M, XL_BM) * cdiv(p.N, XL_BN);
  if (amode == OP_KC) {
    pl.flag = p.geglu_h != nullptr;
    plan_kernel(pl, NK_FAM_XL2G, pl.flag ? "nk_gemm_xl2g_kernel<geglu=1>" : "nk_gemm_xl2g_kernel<geglu=0>", tiles, 1, 1, 512, XL_SMEM_BYTES);
    pl.k_rotate = k_rotate_on(env, p.K);
  } else {
    plan_kernel(pl, NK_FAM_XL, "nk_gemm_xl_kernel", tiles, 1, 1, 1024, XL_SMEM_BYTES);
  }
}
// the 128 x 128 data-parallel kernels
static void plan_ring_or_dma(NkGemmPlan& pl, const TileEnv& env, const NkGemmParams& p) {
  const int ntm = cdiv(p.M, BM), ntn = cdiv(p.N, BN);
  {  // patch height: with T tiles over 8 XCDs an XCD runs ~T/8 tiles at a time; a gm x (T/8/gm) patch touches gm + T/8/gm operand
     // panels, least at gm = sqrt(T/8).  (A fixed 8 gave a 100-tile weight gradient 8 x 1.5 patches: 10 panels per XCD where 7 do.)
    int per_xcd = (ntm * ntn + 7) / 8, g = 1;
    while ((g + 1) * (g + 1) <= per_xcd) ++g;
    pl.group_m = g > GROUP_M ? GROUP_M : g;
  }
  pl.k_rotate = k_rotate_on(env, pl.splitk > 1 ? pl.ksplit_len : p.K);      // (nk_gemm_dma_kernel; the ring kernel walks k in order)
  // under-filled grids (at most one workgroup per CU): the four-stage ring.  (The ring on LARGE grids was measured too: 723 vs 830 TFLOP/s
  // at 65536 x 1280 x 1280 -- three slabs in flight do not make up for two waves per SIMD meeting at a barrier every k-step.)
  if (!p.nbatch && (long)ntm * ntn * pl.splitk <= 256) plan_kernel(pl, NK_FAM_RING, "nk_gemm_ring_kernel", ntm * ntn, pl.splitk, 1, 512, RING_SMEM_BYTES);
  else plan_kernel(pl, NK_FAM_DMA, "nk_gemm_dma_kernel", ntm * ntn, pl.splitk, nbatch1(p), 512, V2_SMEM_BYTES);      // 8 waves per 128 x 128 tile: +4..14 % over 4 waves on every SDXL shape
}
static const char* halo_name(int bn, int rows, int stats) {
  // <column-tile width, tile rows, statistics epilogue>
  static const char* const names[2][2][2] = {
      {{"nk_conv3x3_halo_kernel<128,4,stats=0>", "nk_conv3x3_halo_kernel<128,4,stats=1>"}, {"nk_conv3x3_halo_kernel<128,8,stats=0>", "nk_conv3x3_halo_kernel<128,8,stats=1>"}},
      {{"nk_conv3x3_halo_kernel<160,4,stats=0>", "nk_conv3x3_halo_kernel<160,4,stats=1>"}, {"nk_conv3x3_halo_kernel<160,8,stats=0>", "nk_conv3x3_halo_kernel<160,8,stats=1>"}}};
  return names[bn == 160][rows == 8][stats != 0];
}

// The launch of C = A B^T (+ epilogue) for operand modes (amode, bmode): a pure function of the problem, the caller's options and the
// environment.  The pointers of `p` are only tested for presence.  nk_gemm_dispatch has checked the arguments the rules rely on.
static NkGemmPlan nk_gemm_plan(const NkGemmParams& p, int amode, int bmode, int out_f32, int allow_splitk, const TileEnv& env) {
  NkGemmPlan pl = {};
  pl.splitk = 1;
  // the launcher's fields start as the caller left them: a kernel that does not use one sees what it always saw
  pl.ksplit_len = p.ksplit_len; pl.accumulate = p.accumulate; pl.k_rotate = p.k_rotate; pl.group_m = p.group_m; pl.sk_chunked = p.sk_chunked;

  if (p.geglu_h) {   // the fused GEGLU forward lives in the 256 x 256 two-group kernel only: the caller asks nk_linear_fwd_geglu_ok first
    if (amode != OP_KC || !use_xl(env, p, amode, bmode, out_f32, 1)) {
      pl.err = "fused GEGLU forward on a shape the 256 x 256 kernel does not take (ask nk_linear_fwd_geglu_ok first)";
      return pl;
    }
    plan_split(pl, p, 1);
    plan_xl(pl, env, p, OP_KC);
    return pl;
  }
  if (p.geglu_u) {   // the fused GEGLU backward lives in the LDS-staged epilogue of the 128 x 128 data-parallel / ring kernels only
    plan_split(pl, p, 1);
    plan_ring_or_dma(pl, env, p);
    return pl;
  }
  // 3 x 3 / stride 1 / padding 1 convolutions over whole 64-channel slabs: the halo-tile kernel (conv_halo.h)
  if (use_halo(env, p, amode, bmode, out_f32)) {
    const NkGather& g = p.ga;
    pl.bn = halo_bn(p.N); pl.halo_rows = halo_tile_rows(p); pl.flag = p.stats_part != nullptr;
    pl.tiles_per_image = cdiv(g.W, CH_TW) * cdiv(g.H, pl.halo_rows);
    plan_kernel(pl, NK_FAM_HALO, halo_name(pl.bn, pl.halo_rows, pl.flag), (long)p.halo_nb * pl.tiles_per_image * (p.N / pl.bn), 1, 1,
                halo_threads(pl.bn), halo_smem(pl.bn, pl.halo_rows));
    pl.k_rotate = k_rotate_on(env, g.C);          // (channel slabs, not k-steps: 512 input channels and up)
    return pl;
  }
  // ... and their weight gradients: nine taps from one staged halo per pixel tile (conv_wgrad_halo.h)
  if (use_wgrad_halo(env, p, amode, bmode, out_f32)) {
    int per = 0;
    const int S = wgrad_halo_splits(p, per);
    const long nblk = (long)((p.M + WH_BCO - 1) / WH_BCO) * (p.gb.C / WH_BCI);
    pl.flag = p.dbias != nullptr;
    plan_kernel(pl, NK_FAM_WGRAD_HALO, pl.flag ? "nk_conv3x3_wgrad_halo_kernel<bias=1>" : "nk_conv3x3_wgrad_halo_kernel<bias=0>", nblk * S, 1, 1, 512, WH_SMEM);
    // Split pixel ranges meet through atomics and need a zeroed destination; one range per block stores (or atomically adds to what is
    // there: nobody else touches those elements).  This kernel reads accumulate as "1 = add to what is there": with S > 1 it adds anyway
    pl.splitk = S;
    pl.ksplit_len = per;          // (pixel tiles per range)
    pl.zero_c = S > 1 && p.accumulate == 0; pl.zero_dbias = pl.zero_c && p.dbias;
    pl.accumulate = p.accumulate == 1 ? 1 : 0;
    return pl;
  }
  if (p.stats_part) {      // the GroupNorm statistics epilogue exists in the halo-tile kernel only
    pl.err = "statistics epilogue on a convolution the halo-tile kernel does not take (ask nk_conv2d_stats_tiles first)";
    return pl;
  }

  // Linear weight gradients whose 160-row tiles come out in whole rounds of 256 workgroups (gemm_w160.h), the token range split where the
  // weight alone is too small a grid (fp32 atomics: zeroed destination)
  {
    const W160Plan wp = w160_plan(env, p, amode, bmode, out_f32, allow_splitk);
    if (wp.bn) {
      pl.bn = wp.bn;
      plan_split(pl, p, wp.splitk);
      pl.k_rotate = k_rotate_on(env, wp.splitk > 1 ? pl.ksplit_len : p.K);
      plan_kernel(pl, NK_FAM_W160, wp.bn == 160 ? "nk_gemm_w160_kernel<160>" : "nk_gemm_w160_kernel<128>", (long)cdiv(p.M, W160_BM) * cdiv(p.N, wp.bn),
                  wp.splitk, nbatch1(p), 512, w160_smem(wp.bn));
      return pl;
    }
  }
  if (use_ring64(env, p, amode, bmode, out_f32)) {
    plan_kernel(pl, NK_FAM_RING64, "nk_gemm_ring64_kernel", (long)((p.M + 63) >> 6) * ((p.N + 63) >> 6), 1, 1, 512, R64_SMEM);
    return pl;
  }
  // two-group staggered ring at one workgroup per CU (gemm_g2.h): Linear forward / dgrad / wgrad shapes whose 128 x 160 (or
  // 128 x 128) tiles come out in whole rounds of 256
  if ((!p.nbatch || p.nbatch <= NK_MAX_BATCH) && use_g2(env, p, amode, bmode, out_f32, 1) && (env.g2 == 2 || !use_xl(env, p, amode, bmode, out_f32, 1))) {
    pl.bn = g2_bn(p.N);
    if (pl.accumulate == 2) pl.accumulate = 0;       // no K split here: "destination known zero" means plain stores
    pl.k_rotate = k_rotate_on(env, p.K);
    plan_kernel(pl, NK_FAM_G2P, pl.bn == 160 ? "nk_gemm_g2p_kernel<160>" : "nk_gemm_g2p_kernel<128>", (long)cdiv(p.M, G2_BM) * cdiv(p.N, pl.bn), 1, nbatch1(p), 768,
                G2_SMEM_BYTES);
    return pl;
  }

  // (a launch that carries a fused bias gradient never goes to stream-K, whatever NK_GEMM_SK says: that kernel has no ones-MFMA row sum,
  // and the gradient would silently stay unwritten)
  if (!has_dbias(p) && use_sk(env, p, out_f32)) {
    const long T = (long)cdiv(p.M, BM) * cdiv(p.N, BN) * nbatch1(p), W = T * cdiv(p.K, BK);
    if (W < (1l << 22)) {   // share arithmetic is 32-bit: W * grid < 2^31
      if (pl.accumulate == 2) pl.accumulate = 0;     // "destination known zero" only matters to the atomic split-K path
      // persistent grid: two workgroups per CU, at least ~4 k-steps each
      const int max_grid = SK_MAX_GRID & ~7, min_iters = 4;
      long grid = (W / min_iters) & ~7l;
      if (grid > max_grid) grid = max_grid;
      if (grid < 8) grid = 8;
      pl.sk_chunked = T >= 64;
      plan_kernel(pl, NK_FAM_SK, "nk_gemm_sk_kernel", grid, 1, 1, SK_NT, SK_SMEM_BYTES);
      return pl;
    }
  }
  if (p.nbatch > NK_MAX_BATCH) { pl.err = "p.nbatch <= NK_MAX_BATCH"; return pl; }
  plan_split(pl, p, out_f32 && allow_splitk ? pick_splitk(p.M * nbatch1(p), p.N, p.K, 32) : 1);
  if (use_xl(env, p, amode, bmode, out_f32, pl.splitk)) {
    plan_xl(pl, env, p, amode);
    return pl;
  }
  const bool known = (amode == OP_KC && (bmode == OP_KC || bmode == OP_MC)) || (amode == OP_MC && (bmode == OP_MC || bmode == OP_MCG)) ||
                     (amode == OP_KCG && (bmode == OP_KC || bmode == OP_MCT));
  if (!known) { pl.err = "unsupported operand mode combination"; return pl; }
  plan_ring_or_dma(pl, env, p);
  return pl;
}
