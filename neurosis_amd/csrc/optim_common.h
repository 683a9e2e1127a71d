// What the fused multi-tensor optimizers share (optim.hip: Adafactor, came.hip: CAME, adamw8bit.hip: the host part and the health gate).
//   - the work item of a chunk, the tile sizes, the backward-health gate, the fixed-order block reduction and the "last block done" hand-off;
//   - the factored-statistics core, written once: the 256 x 64 matrix tile (FacTile), a tile's row / column sums and the strip finish that
//     turns them into the row / column EMAs (fac_tile_add_row, fac_strip_finish), the matrix pass that sums u^2 (fac_matrix_u2), conv weights
//     walked one thread per (o, i) pair (FacConv, fac_conv_dispatch, fac_for_pairs, fac_conv_ema, fac_conv_factor) and the vector loop
//     (fac_for_elems).  These are templates over the optimizer's argument block `a` and tensor-table entry `t`: NkAfArgs / NkAfTensor and
//     NkCmArgs / NkCameTensor name their common fields alike (grad, state, ws, mean_row, counters, u2_part, item_lo; off, d0, d1, ws_row,
//     ws_col, mr0, cnt0, nitems).  What an optimizer keeps for itself is its arithmetic.  Adafactor uses all of it; CAME uses the tile, the
//     strip finish, the u^2 pass and fac_mean_slots, and keeps the row loop of its two statistics passes and its conv and vector passes
//     as they were written: on the shared loops they kept their bits but ran 1-3 % slower (came.hip has the figures);
//   - the host prologue and epilogue of an update's entry point (nk_opt_begin, nk_opt_end, NK_OPT_LAUNCH).
#pragma once
#include "nk_common.h"

struct NkAfItem { int tensor, tr, tc, pad; };   // one block's work: tensor index, tile row (or pair / element block), tile column

// (wave-uniform scalar load; `volatile` so it is not hoisted or cached across the check)
#define AF_HEALTH_GATE(a) do { if (*(const volatile unsigned*)(a).health) return; } while (0)

#define AF_TR 256   // matrix tile rows
#define AF_TC 64    // matrix tile cols
#define AF_CONV_PAIRS 1024
#define AF_VEC 1024

// number of elements of a tensor-table entry, as the float the RMS divisions use (vector: d0; matrix: d0 x d1; conv: O x I x KH x KW)
__device__ __forceinline__ float af_tensor_numel(int kind, int d0, int d1, int kh, int kw) {
  return kind == 0 ? (float)d0 : (float)d0 * (float)d1 * (float)(kind == 2 ? kh * kw : 1);
}

__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// "last block done": count this block in; true (for every thread of the block) in the block that completes `total`.
// No fences: an agent-scope release / acquire writes back and invalidates the XCD's WHOLE L2 -- with every block of a 1 000-block launch
// doing that beside the next step's VAE encoder the step went from 165 to 238 ms (round 4, first version).  Instead every handed-off
// value is STORED with an agent-scope atomic store (sc1: written through to the coherence point) and drained (vmcnt(0)) before the
// block is counted, and the finishing block LOADS them with agent-scope atomic loads (sc1: past its own non-coherent L2 lines) --
// the second valid form of MI355X_MICROARCH.md "Correctness boundaries".
#define AF_PUBLISH(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define AF_FETCH(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ bool af_last_block(unsigned* counter, unsigned total, int tid, unsigned* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this thread's published values have been acknowledged
  __syncthreads();
  if (tid == 0) {
    const unsigned old = atomicAdd(counter, 1u);
    *flag = old + 1u == total;
    if (old + 1u == total) AF_PUBLISH(counter, 0u);   // back to zero for the next step (nobody else touches it any more)
  }
  __syncthreads();
  return *flag != 0u;
}

// ema = old * beta + x * omb
__device__ __forceinline__ float fac_ema(float old, float beta, float x, float omb) { return old * beta + x * omb; }
// The same with the new value's product fused, fma(x, omb, old * beta).  The compiler pairs lanes of such sums into packed operations and
// fuses a different product from place to place; for run-time-sized conv taps the shipped kernels' choice is not the one the shared loop
// gets by itself, so it is written down and states keep their bits (tools/ab_optim_bits.py).
__device__ __forceinline__ float fac_ema_new_fused(float old, float beta, float x, float omb) { return __builtin_fmaf(x, omb, old * beta); }

// ---- matrices [d0][d1]: the 256 x 64 tile of one block ---------------------------------------------------------------------------------
// Thread (ry, cx) holds the four columns col..col+3 of the rows ry + 16 i, i = 0..15.  A pass walks them four rows at a time
// (`#pragma unroll 1` over i0 = 0, 4, 8, 12; loads of rows i0..i0+3 first, then the arithmetic), so four float4 loads per stream are in flight.
struct FacTile {
  int ry, cx, col, row0, d0, d1;
  bool cok;                                   // this lane's columns exist (d1 is a multiple of 4: all four or none)
  __device__ __forceinline__ FacTile(const NkAfItem& it, int d0_, int d1_, int tid)
      : ry(tid >> 4), cx(tid & 15), col(it.tc * AF_TC + cx * 4), row0(it.tr * AF_TR), d0(d0_), d1(d1_), cok(col < d1_) {}
  __device__ __forceinline__ int row(int i) const { return row0 + ry + 16 * i; }
  __device__ __forceinline__ bool ok(int r) const { return cok && r < d0; }
  __device__ __forceinline__ long at(int r) const { return (long)r * d1 + col; }      // element offset inside the tensor
  // four elements of row r of a tensor that starts at `base`; zeros outside it
  __device__ __forceinline__ float4_t load(const float* base, int r) const { return load(ok(r), base + at(r)); }
  static __device__ __forceinline__ float4_t load(bool ok, const float* p) { return ok ? *(const float4_t*)p : (float4_t){0.f, 0.f, 0.f, 0.f}; }
  // fp32 master and packed bf16 shadow of row r (the caller checks ok(r)); `off` is the tensor's offset in both
  __device__ __forceinline__ void store(float* master, bf16_t* shadow, long off, int r, const float4_t& pn) const {
    const long o = off + at(r);
    *(float4_t*)(master + o) = pn;
    uint2_t sh;
    sh.x = pack2bf(pn[0], pn[1]);
    sh.y = pack2bf(pn[2], pn[3]);
    *(uint2_t*)(shadow + o) = sh;
  }
  // rsqrt of this lane's four column EMAs (zeros where the columns do not exist)
  __device__ __forceinline__ void col_factors(const float* col_ema, float (&ci)[4]) const {
#pragma unroll
    for (int e = 0; e < 4; ++e) ci[e] = 0.f;
    if (cok) {
      const float4_t c4 = *(const float4_t*)(col_ema + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) ci[e] = rsqrtf(c4[e]);
    }
  }
  // rsqrt(row EMA / mean of the row EMA) of row r (zero outside the tensor)
  __device__ __forceinline__ float row_factor(const float* row_ema, int r, float mean) const { return ok(r) ? rsqrtf(row_ema[r] / mean) : 0.f; }
};

// mean of a row EMA from the partial sums its strips left behind (one slot per 256-row strip, from `first_slot`)
__device__ __forceinline__ float fac_mean_slots(const float* mean_row, int first_slot, int d0) {
  float s = 0.f;
  const int n = (d0 + AF_TR - 1) / AF_TR;
  for (int i = 0; i < n; ++i) s += mean_row[first_slot + i];
  return s / (float)d0;
}

// LDS of a statistics pass: the block reduction's, a tile's row / column sums, the two "last block" flags
struct FacStatsLds {
  float red[4];
  float colsh[16][AF_TC + 4];
  float rowsh[AF_TR];
  unsigned flag[2];
};

// the four values v of this lane in row ry + 16 i (zeros outside the tensor) go into the lane's column sums and the tile's row sums
__device__ __forceinline__ void fac_tile_add_row(const FacTile& T, FacStatsLds& L, float (&cs)[4], int i, const float (&v)[4]) {
  float rs = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cs[e] += v[e];
    rs += v[e];
  }
  // sum over the 16 column lanes of this row (lanes cx = 0..15 are adjacent within the wave)
  rs += __shfl_xor(rs, 8); rs += __shfl_xor(rs, 4); rs += __shfl_xor(rs, 2); rs += __shfl_xor(rs, 1);
  // (through LDS, published in one piece by fac_strip_finish: one coalesced 1 KiB store per block instead of 64 masked 16-byte write-through
  // stores on the same vmcnt as the next batch of loads; Adafactor's pass 51.9 -> 50.3 us per 128 MB chunk.  What holds that pass at 2.4 TB/s
  // against the 4.5 of af_u2_kernel's identical reads is its tail -- two counter round trips and the finishing blocks' reductions, with one
  // generation of blocks per chunk and nothing to overlap them; bigger chunks run the update faster alone (13.6 -> 11.1 ms) and the
  // step slower beside the frozen VAE encoder (146.2 -> 147.2 ms): profiles/r06_adafactor_chunks.txt)
  if (T.cx == 0) L.rowsh[T.ry + 16 * i] = rs;
}

// The end of a statistics pass over a matrix tile: publish the tile's row / column sums; the last tile of its 256-row strip folds the strip's
// row sums into the row EMA at state + row_off (ema = ema * beta + mean * omb) and leaves the strip's sum of that EMA in mean_row[mean_slot0 + tr]
// (mean of the row EMA = sum of the slots / d0); the last tile of its 64-column strip does the column EMA at state + col_off.
template <class A, class T_>
__device__ __forceinline__ void fac_strip_finish(const A& a, const T_& t, const NkAfItem& it, const FacTile& T, FacStatsLds& L, const float (&cs)[4],
                                                 int tid, float beta, float omb, long row_off, long col_off, int mean_slot0) {
  const int ntc = (t.d1 + AF_TC - 1) / AF_TC, ntr = (t.d0 + AF_TR - 1) / AF_TR;
#pragma unroll
  for (int e = 0; e < 4; ++e) L.colsh[T.ry][T.cx * 4 + e] = cs[e];
  __syncthreads();
  float* rowpart = a.ws + t.ws_row + (long)it.tc * t.d0;
  if (it.tr * AF_TR + tid < t.d0) AF_PUBLISH(rowpart + it.tr * AF_TR + tid, L.rowsh[tid]);      // 256 consecutive floats
  if (tid < AF_TC) {
    const int c = it.tc * AF_TC + tid;
    if (c < t.d1) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += L.colsh[r][tid];
      AF_PUBLISH(a.ws + t.ws_col + (long)it.tr * t.d1 + c, s);
    }
  }
  if (af_last_block(a.counters + t.cnt0 + 1 + it.tr, (unsigned)ntc, tid, &L.flag[0])) {
    const int r = it.tr * AF_TR + tid;
    float v = 0.f;
    if (r < t.d0) {
      float s = 0.f;
#pragma unroll 8
      for (int c = 0; c < ntc; ++c) s += AF_FETCH(a.ws + t.ws_row + (long)c * t.d0 + r);   // (independent loads: keep 8 in flight)
      float* st = a.state + row_off + r;
      v = fac_ema(*st, beta, s / (float)t.d1, omb);
      *st = v;
    }
    v = block_sum_256(v, L.red);
    if (tid == 0) a.mean_row[mean_slot0 + it.tr] = v;
  }
  if (af_last_block(a.counters + t.cnt0 + 1 + ntr + it.tc, (unsigned)ntr, tid, &L.flag[1])) {
    const int c = it.tc * AF_TC + tid;
    if (tid < AF_TC && c < t.d1) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < ntr; ++r) s += AF_FETCH(a.ws + t.ws_col + (long)r * t.d1 + c);
      float* st = a.state + col_off + c;
      *st = fac_ema(*st, beta, s / (float)t.d0, omb);
    }
  }
}

// The matrix pass between the statistics and the update: this tile's partial sum of u^2, u = g * rsqrt(row / mean row) * rsqrt(col), from the
// EMAs at state + row_off / col_off; the tensor's last block then calls finish(tid, red) on the published sums.
template <class A, class T_, class Finish>
__device__ __forceinline__ void fac_matrix_u2(const A& a, const T_& t, const NkAfItem& it, long row_off, long col_off, Finish finish) {
  __shared__ float red[4];
  __shared__ unsigned flag;
  const int tid = threadIdx.x;
  const FacTile T(it, t.d0, t.d1, tid);
  const float mr = fac_mean_slots(a.mean_row, t.mr0, t.d0);
  const float gs = a.grad_scale;
  float ci[4];
  T.col_factors(a.state + col_off, ci);
  float acc = 0.f;
#pragma unroll 1
  for (int i0 = 0; i0 < AF_TR / 16; i0 += 4) {
    float4_t g[4];
    float rf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = T.row(i0 + u);
      const bool ok = T.ok(r);
      g[u] = T.load(ok, a.grad + t.off + T.at(r));
      rf[u] = ok ? rsqrtf(a.state[row_off + r] / mr) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float uu = rf[u] * ci[e] * (g[u][e] * gs);
        acc += uu * uu;
      }
  }
  acc = block_sum_256(acc, red);
  if (tid == 0) AF_PUBLISH(a.u2_part + a.item_lo + blockIdx.x, acc);
  if (af_last_block(a.counters + t.cnt0, (unsigned)t.nitems, tid, &flag)) finish(tid, red);
}

// ---- conv weights stored [O][KH][KW][I]: one thread per (o, i) pair, all of that pair's KH x KW taps and statistics stay in registers -----
// KH_/KW_ = 0: runtime sizes (<= 3), otherwise compile-time (no scratch-resident arrays).  The statistics are laid out [O][KH][I], [O][KW][I].
template <int KH_, int KW_>
struct FacConv {
  static constexpr bool runtime = KH_ == 0;
  int rkh, rkw, I;
  __device__ __forceinline__ int KH() const { return KH_ ? KH_ : rkh; }
  __device__ __forceinline__ int KW() const { return KW_ ? KW_ : rkw; }
  __device__ __forceinline__ long tap(int o, int i, int x, int y) const { return (((long)o * KH() + x) * KW() + y) * I + i; }
  __device__ __forceinline__ long row(int o, int i, int x) const { return ((long)o * KH() + x) * I + i; }
  __device__ __forceinline__ long col(int o, int i, int y) const { return ((long)o * KW() + y) * I + i; }
  template <class F> __device__ __forceinline__ void rows(F f) const {
#pragma unroll
    for (int x = 0; x < 3; ++x)
      if (x < KH()) f(x);
  }
  template <class F> __device__ __forceinline__ void cols(F f) const {
#pragma unroll
    for (int y = 0; y < 3; ++y)
      if (y < KW()) f(y);
  }
  template <class F> __device__ __forceinline__ void taps(F f) const {
    rows([&](int x) { cols([&](int y) { f(x, y); }); });
  }
};

// f(FacConv) with the tap counts of a tensor-table entry: 3 x 3 and 1 x 1 at compile time, anything else at run time
template <class T_, class F>
__device__ __forceinline__ void fac_conv_dispatch(const T_& t, F f) {
  if (t.kh == 3 && t.kw == 3) f(FacConv<3, 3>{3, 3, t.d1});
  else if (t.kh == 1 && t.kw == 1) f(FacConv<1, 1>{1, 1, t.d1});
  else f(FacConv<0, 0>{t.kh, t.kw, t.d1});
}

// f(o, i) for the pairs of work item `tr` (AF_CONV_PAIRS consecutive pairs, I fastest) of a conv weight with d0 output channels
template <class F>
__device__ __forceinline__ void fac_for_pairs(int tr, int tid, int d0, int I, F f) {
  const long npairs = (long)d0 * I;
  for (int q = 0; q < AF_CONV_PAIRS / 256; ++q) {
    const long pr = (long)tr * AF_CONV_PAIRS + q * 256 + tid;
    if (pr < npairs) {
      const int o = (int)(pr / I);
      f(o, (int)(pr - (long)o * I));
    }
  }
}

// EMAs of the row / column means of q[KH][KW] into the pair's statistics at row_off / col_off; returns them in row / col
template <class CV>
__device__ __forceinline__ void fac_conv_ema(const CV& cv, float* state, long row_off, long col_off, int o, int i, const float (&q)[3][3],
                                             float beta, float omb, float (&row)[3], float (&col)[3]) {
  cv.rows([&](int x) {
    float m = 0.f;
    cv.cols([&](int y) { m += q[x][y]; });
    float* st = state + row_off + cv.row(o, i, x);
    row[x] = CV::runtime ? fac_ema_new_fused(*st, beta, m / (float)cv.KW(), omb) : fac_ema(*st, beta, m / (float)cv.KW(), omb);
    *st = row[x];
  });
  cv.cols([&](int y) {
    float m = 0.f;
    cv.rows([&](int x) { m += q[x][y]; });
    float* st = state + col_off + cv.col(o, i, y);
    col[y] = CV::runtime ? fac_ema_new_fused(*st, beta, m / (float)cv.KH(), omb) : fac_ema(*st, beta, m / (float)cv.KH(), omb);
    *st = col[y];
  });
}

// the pair's statistics as they stand in `state`
template <class CV>
__device__ __forceinline__ void fac_conv_load(const CV& cv, const float* state, long row_off, long col_off, int o, int i, float (&row)[3], float (&col)[3]) {
  cv.rows([&](int x) { row[x] = state[row_off + cv.row(o, i, x)]; });
  cv.cols([&](int y) { col[y] = state[col_off + cv.col(o, i, y)]; });
}

// f[x][y] = rsqrt(row[x] / mean(row)) * rsqrt(col[y]), the factored preconditioner of one pair (the mean is over KH); u = f * g, in that order
template <class CV>
__device__ __forceinline__ void fac_conv_factor(const CV& cv, const float (&row)[3], const float (&col)[3], float (&f)[3][3]) {
  float mr = 0.f;
  cv.rows([&](int x) { mr += row[x]; });
  mr /= (float)cv.KH();
  cv.rows([&](int x) {
    const float rf = rsqrtf(row[x] / mr);
    cv.cols([&](int y) { f[x][y] = rf * rsqrtf(col[y]); });
  });
}

// The statistics pass over conv weights: the EMAs at row_off / col_off from q = g^2 + eps1 of this step's gradients, and this item's partial
// sum of u^2, u = f * g with the new EMAs
template <class A, class T_, class CV>
__device__ __forceinline__ float fac_conv_stats(const A& a, const T_& t, const CV& cv, int tr, int tid, long row_off, long col_off, float beta, float omb) {
  const float gs = a.grad_scale;
  float acc = 0.f;
  fac_for_pairs(tr, tid, t.d0, t.d1, [&](int o, int i) {
    float g[3][3], sq[3][3], row[3], col[3], f[3][3];
    cv.taps([&](int x, int y) {
      g[x][y] = a.grad[t.off + cv.tap(o, i, x, y)] * gs;
      sq[x][y] = g[x][y] * g[x][y] + a.eps1;
    });
    fac_conv_ema(cv, a.state, row_off, col_off, o, i, sq, beta, omb, row, col);
    fac_conv_factor(cv, row, col, f);
    cv.taps([&](int x, int y) {
      const float u = f[x][y] * g[x][y];
      acc += u * u;
    });
  });
  return acc;
}

// ---- vectors: f(e) for the elements of work item `tr` (AF_VEC consecutive ones) of a vector of n ---------------------------------------
template <class F>
__device__ __forceinline__ void fac_for_elems(int tr, int tid, long n, F f) {
  for (int q = 0; q < AF_VEC / 256; ++q) {
    const long e = (long)tr * AF_VEC + q * 256 + tid;
    if (e < n) f(e);
  }
}

// ---- host: what every update's entry point does around its launches -------------------------------------------------------------------
// Before: on the first chunk of a step, refuse to go on silently when an EARLIER step's backward was flagged (later chunks of the same step
// must not trip over this step's own snapshot); the health word the kernels gate on.
static inline int nk_opt_begin(bool first_chunk, const unsigned** health) {
  if (first_chunk)
    if (int e = nk_health_poll()) return e;
  *health = nk_health_word();
  if (!*health) { nk_set_error(__FILE__, __LINE__, "health word allocation failed"); return NK_ERR_LAUNCH; }
  return NK_OK;
}
// After: a snapshot of what the backward in front of this update left in the word
static inline int nk_opt_end(hipStream_t stream) {
  nk_health_snapshot(stream);
  return NK_OK;
}
// one block of 256 threads per work item; returns from the entry point when the launch fails
#define NK_OPT_LAUNCH(kernel, nblocks, stream, a)                                       \
  do {                                                                                  \
    hipLaunchKernelGGL(kernel, dim3(nblocks), dim3(256), 0, stream, a);                 \
    if (int e_ = nk_check_launch(#kernel)) return e_;                                   \
  } while (0)
