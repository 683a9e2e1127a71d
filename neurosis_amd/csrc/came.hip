// Fused multi-tensor CAME (Confidence-guided Adaptive Memory Efficient optimization) over the flat parameter / gradient buffers.
// Replaces the reference's per-tensor Python loop (`optimizers/came.py:115-224`, `approximate_sq_grad` :107-113, `get_rms` :101-104).
// CAME is Adafactor's factored second moment (same rule: factored over the LAST TWO dims of every tensor with >= 2 dims; OIHW conv
// weights factor over the KH x KW taps of every (o,i) pair) plus a first moment m and a second factored statistic of the
// "instability" residual (u_hat - m)^2.  Four launches per CHUNK of tensors:
//
//   A  statistics   matrices: row / column partials of g^2+eps1 per 256x64 tile; the last tile of a strip turns them into the R / C EMAs
//                   and a partial sum of R (F1).  Conv pairs and vectors: R / C (or v) EMAs, u, partial sum of u^2; the last block of the
//                   tensor turns the sums into the clip denominator (F2)
//   B  matrices     u = g * rsqrt(R / mean R) * rsqrt(C), partial sum of u^2; the tensor's last block: clip denominator (F2)
//   C1 momentum     u again, u_hat = u / denom, m = b1 m + (1-b1) u_hat written back; matrices: row / column partials of
//                   res = (u_hat - m)^2 + eps2 and, in the last tile of a strip, the Rr / Cr EMAs and a partial sum of Rr (F3).
//                   Conv pairs own their residual statistics (the taps of one pair are one thread's), and vectors have none: both
//                   finish here (p and the bf16 shadow)
//   C2 matrices     p = p * decay - lr * rsqrt(Rr / mean Rr) * rsqrt(Cr) * m; bf16 shadow rewritten
//
// Per matrix parameter: g read three times, m read twice and written once, p read and written, the shadow written: 34 B against
// Adafactor's 22 and AdamW's 30.  State: m (full size) and the four factored vectors, or m and v for a vector (4 B/param + a little,
// against AdamW's 8).  Every reduction goes through per-tile partials combined in a fixed order: no atomics on values, bitwise
// reproducible step to step.  Every kernel returns at once while the backward-health word is raised.
//
// The tile geometry, the strip finish, pass B and the mean slots are optim_common.h's, shared with Adafactor.  The row loop of
// cm_matrix_stats and the conv / vector passes are NOT written on the shared loops, deliberately: both statistics kernels sit at the edge of
// what the compiler pairs into packed operations, and on the shared loops (same bits) CAME's update of 2.57 G parameters went from 19.77 to
// 20.14 ms: matrices +1.4 %, 3x3 convs +1.2 %; with only the KH/KW ladder shared the 3x3 convs still ran +2 %, with the pair EMA / factor
// helpers shared the 1x1 convs +5 % (profiles/optim_refactor_ab.txt).
#include "../../include/neurosis_hip.h"
#include "nk_common.h"
#include "optim_common.h"

struct NkCameTensor {    // mirrored by neurosis_amd/optim.py (CAME_TENSOR_DTYPE); 104 bytes
  long off;              // element offset of the tensor in master / grad / shadow
  long m_off;            // first moment, same physical layout as the parameter                  (offsets in `state`)
  long r_off, c_off;     // matrix: R [d0], C [d1]; conv: [O][KH][I], [O][KW][I]; vector: v [numel] at r_off
  long rr_off, cr_off;   // residual statistics, laid out as R / C (matrices and convs)
  long ws_row;           // matrix: row partials [ntc][d0], offset in the chunk workspace
  long ws_col;           // matrix: col partials [ntr][d1]
  int kind;              // 0 vector, 1 matrix [d0][d1], 2 conv stored [O=d0][KH][KW][I=d1]
  int d0, d1;
  int kh, kw;
  int item0, nitems;     // this tensor's range in the item table
  int mr0;               // matrix: slots of the partial sums of R (one per 256-row strip) at mr0, of Rr at mr0 + ntr, in `mean_row`
  int cnt0;              // "blocks done" counters: [0] the tensor's, matrices: [1 + tr] row strips, [1 + ntr + tc] column strips
  int pad;
};
static_assert(sizeof(NkCameTensor) == 104, "mirrored by neurosis_amd/optim.py");

struct NkCmArgs {
  float* master; const float* grad; bf16_t* shadow; float* state; float* ws;
  const NkCameTensor* tensors; const NkAfItem* items;
  float* u2_part;      // [nitems] partial sums of u^2
  float* mean_row;     // per matrix: partial sums of R, then of Rr, one per 256-row strip
  float* denom;        // [ntensors] max(1, rms(u) / clip)
  unsigned* counters;
  int item_lo, item_hi, tensor_lo, tensor_hi;
  float beta1, beta2, beta3, omb1, omb2, omb3, eps1, eps2, clip, lr, decay, grad_scale;   // omb = 1 - beta, from the host
  const unsigned* health;
};

// the clip denominator of one tensor from its items' partial sums of u^2 (came.py:187)
__device__ __forceinline__ void cm_tensor_denom(const NkCmArgs& a, const NkCameTensor& t, int ti, int tid, float* red) {
  float su = 0.f;
  for (int i = tid; i < t.nitems; i += 256) su += AF_FETCH(a.u2_part + t.item0 + i);
  su = block_sum_256(su, red);
  if (tid == 0) {
    const float numel = af_tensor_numel(t.kind, t.d0, t.d1, t.kh, t.kw);
    const float rms = sqrtf(su) / sqrtf(numel);
    a.denom[ti] = fmaxf(1.0f, rms / a.clip);
  }
}

// ---- matrices: the two row / column statistics passes (A: q = g^2 + eps1 -> R, C;  C1: m update, res -> Rr, Cr) -------------------------
template <bool RES>
__device__ __forceinline__ void cm_matrix_stats(const NkCmArgs& a, const NkAfItem& it, const NkCameTensor& t, int tid) {
  __shared__ FacStatsLds L;
  const FacTile T(it, t.d0, t.d1, tid);
  const int ry = T.ry, cx = T.cx, col = T.col;
  const bool cok = T.cok;
  const float gs = a.grad_scale;
  float ci[4] = {0.f, 0.f, 0.f, 0.f}, mr = 1.f, den = 1.f;
  if (RES) {
    mr = fac_mean_slots(a.mean_row, t.mr0, t.d0);
    if (cok) {
      const float4_t c4 = *(const float4_t*)(a.state + t.c_off + col);
#pragma unroll
      for (int e = 0; e < 4; ++e) ci[e] = rsqrtf(c4[e]);
    }
    den = a.denom[it.tensor];
  }
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int i0 = 0; i0 < AF_TR / 16; i0 += 4) {
    float4_t g[4], m[4];
    float rf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = it.tr * AF_TR + ry + 16 * (i0 + u);
      const bool ok = cok && r < t.d0;
      const long o = (long)r * t.d1 + col;
      g[u] = ok ? *(const float4_t*)(a.grad + t.off + o) : (float4_t){0.f, 0.f, 0.f, 0.f};
      if (RES) {
        m[u] = ok ? *(const float4_t*)(a.state + t.m_off + o) : (float4_t){0.f, 0.f, 0.f, 0.f};
        rf[u] = ok ? rsqrtf(a.state[t.r_off + r] / mr) : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = it.tr * AF_TR + ry + 16 * (i0 + u);
      const bool ok = cok && r < t.d0;
      float rs = 0.f;
      float4_t mn;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = g[u][e] * gs;
        float v;
        if (RES) {
          const float uh = (rf[u] * ci[e] * gg) / den;
          mn[e] = m[u][e] * a.beta1 + uh * a.omb1;
          const float d = uh - mn[e];
          v = d * d + a.eps2;
        } else {
          v = gg * gg + a.eps1;
        }
        v = ok ? v : 0.f;
        cs[e] += v;
        rs += v;
      }
      if (RES && ok) *(float4_t*)(a.state + t.m_off + (long)r * t.d1 + col) = mn;
      // sum over the 16 column lanes of this row (lanes cx = 0..15 are adjacent within the wave)
      rs += __shfl_xor(rs, 8); rs += __shfl_xor(rs, 4); rs += __shfl_xor(rs, 2); rs += __shfl_xor(rs, 1);
      if (cx == 0) L.rowsh[ry + 16 * (i0 + u)] = rs;
    }
  }
  const int ntr = (t.d0 + AF_TR - 1) / AF_TR;
  fac_strip_finish(a, t, it, T, L, cs, tid, RES ? a.beta3 : a.beta2, RES ? a.omb3 : a.omb2, RES ? t.rr_off : t.r_off, RES ? t.cr_off : t.c_off,
                   t.mr0 + (RES ? ntr : 0));
}

// ---- conv weights: one thread per (o, i) pair; all of that pair's KH x KW taps and factored statistics stay in registers ---------------
// KH_/KW_ = 0: runtime sizes (<= 3), otherwise compile-time (no scratch-resident arrays)

// rsqrt(row[x] / mean(row)) * rsqrt(col[y]), the factored preconditioner of one pair (came.py:107-113 with the mean over KH)
template <int KH_, int KW_>
__device__ __forceinline__ void cm_conv_factor(const float (&row)[3], const float (&col)[3], int KH, int KW, float (&f)[3][3]) {
  float mr = 0.f;
#pragma unroll
  for (int x = 0; x < 3; ++x)
    if (x < KH) mr += row[x];
  mr /= (float)KH;
#pragma unroll
  for (int x = 0; x < 3; ++x)
    if (x < KH) {
      const float rf = rsqrtf(row[x] / mr);
#pragma unroll
      for (int y = 0; y < 3; ++y)
        if (y < KW) f[x][y] = rf * rsqrtf(col[y]);
    }
}

// EMAs of the row / column means of q[KH][KW] into the pair's statistics at row_off / col_off; returns them in row / col
template <int KH_, int KW_>
__device__ __forceinline__ void cm_conv_ema(float* state, long row_off, long col_off, int o, int i, int I, const float (&q)[3][3], int KH, int KW,
                                            float beta, float omb, float (&row)[3], float (&col)[3]) {
#pragma unroll
  for (int x = 0; x < 3; ++x)
    if (x < KH) {
      float m = 0.f;
#pragma unroll
      for (int y = 0; y < 3; ++y)
        if (y < KW) m += q[x][y];
      float* st = state + row_off + ((long)o * KH + x) * I + i;
      row[x] = *st * beta + (m / (float)KW) * omb;
      *st = row[x];
    }
#pragma unroll
  for (int y = 0; y < 3; ++y)
    if (y < KW) {
      float m = 0.f;
#pragma unroll
      for (int x = 0; x < 3; ++x)
        if (x < KH) m += q[x][y];
      float* st = state + col_off + ((long)o * KW + y) * I + i;
      col[y] = *st * beta + (m / (float)KH) * omb;
      *st = col[y];
    }
}

template <int KH_, int KW_>
__device__ __forceinline__ float cm_conv_stats(const NkCmArgs& a, const NkCameTensor& t, int tr, int tid) {
  const int KH = KH_ ? KH_ : t.kh, KW = KW_ ? KW_ : t.kw, I = t.d1;
  const long npairs = (long)t.d0 * I;
  const float gs = a.grad_scale;
  float acc = 0.f;
  for (int q = 0; q < AF_CONV_PAIRS / 256; ++q) {
    const long pr = (long)tr * AF_CONV_PAIRS + q * 256 + tid;
    if (pr < npairs) {
      const int o = (int)(pr / I), i = (int)(pr - (long)o * I);
      float g[3][3], sq[3][3], row[3], col[3], f[3][3];
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y)
          if (x < KH && y < KW) {
            g[x][y] = a.grad[t.off + (((long)o * KH + x) * KW + y) * I + i] * gs;
            sq[x][y] = g[x][y] * g[x][y] + a.eps1;
          }
      cm_conv_ema<KH_, KW_>(a.state, t.r_off, t.c_off, o, i, I, sq, KH, KW, a.beta2, a.omb2, row, col);
      cm_conv_factor<KH_, KW_>(row, col, KH, KW, f);
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y)
          if (x < KH && y < KW) {
            const float u = f[x][y] * g[x][y];
            acc += u * u;
          }
    }
  }
  return acc;
}

template <int KH_, int KW_>
__device__ __forceinline__ void cm_conv_finish(const NkCmArgs& a, const NkCameTensor& t, int tr, int tid, float den) {
  const int KH = KH_ ? KH_ : t.kh, KW = KW_ ? KW_ : t.kw, I = t.d1;
  const long npairs = (long)t.d0 * I;
  const float gs = a.grad_scale;
  for (int q = 0; q < AF_CONV_PAIRS / 256; ++q) {
    const long pr = (long)tr * AF_CONV_PAIRS + q * 256 + tid;
    if (pr < npairs) {
      const int o = (int)(pr / I), i = (int)(pr - (long)o * I);
      float row[3], col[3], f[3][3], m[3][3], res[3][3];
#pragma unroll
      for (int x = 0; x < 3; ++x)
        if (x < KH) row[x] = a.state[t.r_off + ((long)o * KH + x) * I + i];
#pragma unroll
      for (int y = 0; y < 3; ++y)
        if (y < KW) col[y] = a.state[t.c_off + ((long)o * KW + y) * I + i];
      cm_conv_factor<KH_, KW_>(row, col, KH, KW, f);
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y)
          if (x < KH && y < KW) {
            const long e = (((long)o * KH + x) * KW + y) * I + i;
            const float uh = (f[x][y] * (a.grad[t.off + e] * gs)) / den;
            const float mn = a.state[t.m_off + e] * a.beta1 + uh * a.omb1;
            a.state[t.m_off + e] = mn;
            m[x][y] = mn;
            const float d = uh - mn;
            res[x][y] = d * d + a.eps2;
          }
      cm_conv_ema<KH_, KW_>(a.state, t.rr_off, t.cr_off, o, i, I, res, KH, KW, a.beta3, a.omb3, row, col);
      cm_conv_factor<KH_, KW_>(row, col, KH, KW, f);
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y)
          if (x < KH && y < KW) {
            const long e = t.off + (((long)o * KH + x) * KW + y) * I + i;
            const float pn = a.master[e] * a.decay - (f[x][y] * m[x][y]) * a.lr;
            a.master[e] = pn;
            a.shadow[e] = f2bf(pn);
          }
    }
  }
}

// ---- pass A -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void came_stats_kernel(const NkCmArgs a) {
  AF_HEALTH_GATE(a);
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkCameTensor t = a.tensors[it.tensor];
  const int tid = threadIdx.x;
  if (t.kind == 1) {
    cm_matrix_stats<false>(a, it, t, tid);
    return;
  }
  __shared__ float red[4];
  __shared__ unsigned flag;
  float acc = 0.f;
  if (t.kind == 2) {
    if (t.kh == 3 && t.kw == 3) acc = cm_conv_stats<3, 3>(a, t, it.tr, tid);
    else if (t.kh == 1 && t.kw == 1) acc = cm_conv_stats<1, 1>(a, t, it.tr, tid);
    else acc = cm_conv_stats<0, 0>(a, t, it.tr, tid);
  } else {
    const long n = (long)t.d0;
    for (int q = 0; q < AF_VEC / 256; ++q) {
      const long e = (long)it.tr * AF_VEC + q * 256 + tid;
      if (e < n) {
        const float g = a.grad[t.off + e] * a.grad_scale;
        float* st = a.state + t.r_off + e;
        const float v = *st * a.beta2 + (g * g + a.eps1) * a.omb2;
        *st = v;
        const float u = rsqrtf(v) * g;
        acc += u * u;
      }
    }
  }
  acc = block_sum_256(acc, red);
  if (tid == 0) AF_PUBLISH(a.u2_part + a.item_lo + blockIdx.x, acc);
  if (af_last_block(a.counters + t.cnt0, (unsigned)t.nitems, tid, &flag)) cm_tensor_denom(a, t, it.tensor, tid, red);
}

// ---- pass B (matrices): partial sums of u^2, the clip denominator ------------------------------------------------------------------
__global__ __launch_bounds__(256) void came_u2_kernel(const NkCmArgs a) {
  AF_HEALTH_GATE(a);
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkCameTensor t = a.tensors[it.tensor];
  if (t.kind != 1) return;
  fac_matrix_u2(a, t, it, t.r_off, t.c_off, [&](int tid, float* red) { cm_tensor_denom(a, t, it.tensor, tid, red); });
}

// ---- pass C1: first moment; matrices: residual statistics; conv weights and vectors: the whole rest of the update ----------------------
__global__ __launch_bounds__(256) void came_moment_kernel(const NkCmArgs a) {
  AF_HEALTH_GATE(a);
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkCameTensor t = a.tensors[it.tensor];
  const int tid = threadIdx.x;
  if (t.kind == 1) {
    cm_matrix_stats<true>(a, it, t, tid);
  } else if (t.kind == 2) {
    const float den = a.denom[it.tensor];
    if (t.kh == 3 && t.kw == 3) cm_conv_finish<3, 3>(a, t, it.tr, tid, den);
    else if (t.kh == 1 && t.kw == 1) cm_conv_finish<1, 1>(a, t, it.tr, tid, den);
    else cm_conv_finish<0, 0>(a, t, it.tr, tid, den);
  } else {
    const long n = (long)t.d0;
    const float den = a.denom[it.tensor];
    for (int q = 0; q < AF_VEC / 256; ++q) {
      const long e = (long)it.tr * AF_VEC + q * 256 + tid;
      if (e < n) {
        const float g = a.grad[t.off + e] * a.grad_scale;
        const float uh = (rsqrtf(a.state[t.r_off + e]) * g) / den;
        const float mn = a.state[t.m_off + e] * a.beta1 + uh * a.omb1;
        a.state[t.m_off + e] = mn;
        const float pn = a.master[t.off + e] * a.decay - mn * a.lr;
        a.master[t.off + e] = pn;
        a.shadow[t.off + e] = f2bf(pn);
      }
    }
  }
}

// ---- pass C2 (matrices): apply -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void came_apply_kernel(const NkCmArgs a) {
  AF_HEALTH_GATE(a);
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkCameTensor t = a.tensors[it.tensor];
  if (t.kind != 1) return;
  const FacTile T(it, t.d0, t.d1, threadIdx.x);
  if (!T.cok) return;                               // (no block-wide synchronisation below)
  const float mr = fac_mean_slots(a.mean_row, t.mr0 + (t.d0 + AF_TR - 1) / AF_TR, t.d0);
  float ci[4];
  T.col_factors(a.state + t.cr_off, ci);
#pragma unroll 1
  for (int i0 = 0; i0 < AF_TR / 16; i0 += 4) {
    float4_t m[4], p[4];
    float rf[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = T.row(i0 + u);
      const bool ok = T.ok(r);
      const long o = T.at(r);
      m[u] = T.load(ok, a.state + t.m_off + o);
      p[u] = T.load(ok, a.master + t.off + o);
      rf[u] = ok ? rsqrtf(a.state[t.rr_off + r] / mr) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = T.row(i0 + u);
      if (!T.ok(r)) continue;
      float4_t pn;
#pragma unroll
      for (int e = 0; e < 4; ++e) pn[e] = p[u][e] * a.decay - (rf[u] * ci[e] * m[u][e]) * a.lr;
      T.store(a.master, a.shadow, t.off, r, pn);
    }
  }
}

static int cm_check(const NkCameArgs* h) {
  NK_CHECK_ARG(h && h->master && h->grad && h->shadow && h->state && h->ws && h->tensors && h->items);
  NK_CHECK_ARG(h->u2_part && h->mean_row && h->denom && h->counters);
  NK_CHECK_ARG(h->item_hi > h->item_lo && h->tensor_hi > h->tensor_lo);
  return NK_OK;
}

extern "C" long nk_came_tensor_bytes(void) { return (long)sizeof(NkCameTensor); }

extern "C" int nk_came_chunk(const NkCameArgs* h, void* stream_) {
  if (int e = cm_check(h)) return e;
  hipStream_t stream = (hipStream_t)stream_;
  NkCmArgs a;
  a.master = h->master; a.grad = h->grad; a.shadow = (bf16_t*)h->shadow; a.state = h->state; a.ws = h->ws;
  a.tensors = (const NkCameTensor*)h->tensors; a.items = (const NkAfItem*)h->items;
  a.u2_part = h->u2_part; a.mean_row = h->mean_row; a.denom = h->denom; a.counters = h->counters;
  a.item_lo = h->item_lo; a.item_hi = h->item_hi; a.tensor_lo = h->tensor_lo; a.tensor_hi = h->tensor_hi;
  a.beta1 = h->beta1; a.beta2 = h->beta2; a.beta3 = h->beta3;
  a.omb1 = h->one_minus_beta1; a.omb2 = h->one_minus_beta2; a.omb3 = h->one_minus_beta3; a.eps1 = h->eps1; a.eps2 = h->eps2; a.clip = h->clip_threshold;
  a.lr = h->lr; a.decay = h->decay; a.grad_scale = h->grad_scale;
  if (int e = nk_opt_begin(h->tensor_lo == 0, &a.health)) return e;
  const int nitems = a.item_hi - a.item_lo;
  NK_OPT_LAUNCH(came_stats_kernel, nitems, stream, a);
  if (h->has_matrix) NK_OPT_LAUNCH(came_u2_kernel, nitems, stream, a);
  NK_OPT_LAUNCH(came_moment_kernel, nitems, stream, a);
  if (h->has_matrix) NK_OPT_LAUNCH(came_apply_kernel, nitems, stream, a);
  return nk_opt_end(stream);
}
