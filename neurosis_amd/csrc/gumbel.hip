// Gumbel-softmax quantizer bottleneck (reference modules/autoencoding/regularizers/quantize.py:59-160, GumbelQuantizer):
// the projection logits on the exact fp32 MFMA, the Gumbel noise from the counter-based generator of dropout.hip, the Gumbel-softmax
// with its KL term and their backward.  Plain HIP and compiler builtins; no float atomics anywhere: every result is bit-identical from
// run to run.
//
// Row passes (softmax forward / backward): one workgroup of 256 threads per row, thread t owns the 4-element groups t, t + 256, ...
// (elements 4 * group .. 4 * group + 3).  Widths:
//     n <= 1024           one group per thread, the row held in registers
//     n <= 8192           eight groups per thread, the row held in registers
//     n <= 65536          nothing is held: every pass reads the row again (a 65536-wide fp32 row is 256 KiB, more than the LDS; it stays in
//                         L2 between the passes) and, on the token route, draws the noise again
// Every sum is fp32 in a fixed order: the thread adds its elements in rising order, the 64 lanes of a wave merge by an xor butterfly, thread
// 0..255 then adds the four wave results in wave order.
//
// inv_tau and w_kl are LAUNCH ARGUMENTS: the temperature is a Python attribute that a training loop anneals between steps, and a captured
// hipGraph would freeze it at capture.  Nothing captures the autoencoder step today; the noise, which must change on every replay, is read
// from the device token as in nk_dropout.
#include "../../include/neurosis_hip.h"
#include "nk_common.h"
#include "nk_reduce.h"

#define GB_ROWS 32          // rows of z per workgroup of the logits kernel: two 16-row MFMA groups, held in registers
#define GB_WAVES 4
#define GB_THREADS 256
#define GB_NONE 0x7fffffff
#define GB_KEY_XOR 0x47554D42u      // "GUMB": separates this stream from the dropout masks drawn under the same token

static int gb_refuse(int line, const char* what) {
  nk_set_error(__FILE__, line, what);
  return NK_ERR_ARG;
}

// ---- logits[i][j] = b_j + sum_k z_ik w_jk ---------------------------------------------------------------------------------------
// The tile loop and operand layout of vq_search_kernel (vq.hip): A operand lane l holds z[row (l & 15)][k = 4 s + (l >> 4)], B operand
// w[code (l & 15)][same k], K = 4 * KS >= h with a zero tail; the result has the code on lane (l & 15) and rows 4 * (l >> 4) + r in its four
// registers, and is bit for bit the chain fmaf(z_k, w_jk, acc) in rising k from 0.  The bias is one __fadd_rn on top.  The epilogue here
// stores the tile instead of reducing it.  blockIdx.y cuts the code tiles when there are too few rows to fill the machine.
template <int KS>
__global__ __launch_bounds__(64 * GB_WAVES) void gumbel_logits_kernel(const float* __restrict__ z, long ldz, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, float* __restrict__ logits, long ldl, int N,
                                                                       int h, int n, int tiles_per_split) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const long row0 = (long)blockIdx.x * GB_ROWS;
  float a[2][KS];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const long row = row0 + 16 * g + c;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + q;
      a[g][s] = (row < N && k < h) ? z[row * ldz + k] : 0.f;
    }
  }
  const int ntiles = (n + 15) >> 4;
  const int t1 = min(ntiles, ((int)blockIdx.y + 1) * tiles_per_split);
  for (int t = blockIdx.y * tiles_per_split + wave; t < t1; t += GB_WAVES) {
    const int j = t * 16 + c;
    const bool live = j < n;
    const float* e = w + (long)(live ? j : 0) * h;
    float4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + q;
      const float b = (live && k < h) ? e[k] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][s], b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][s], b, acc1, 0, 0, 0);
    }
    if (!live) continue;
    const float bj = bias[j];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long r0 = row0 + 4 * q + r, r1 = r0 + 16;
      if (r0 < N) logits[r0 * ldl + j] = __fadd_rn(acc0[r], bj);
      if (r1 < N) logits[r1 * ldl + j] = __fadd_rn(acc1[r], bj);
    }
  }
}

#define GB_TARGET_BLOCKS 1024
static int gb_splits(long N, int n) {       // as vq_splits: about four waves per SIMD, at least 16 tiles to a cut
  const long blocks = (N + GB_ROWS - 1) / GB_ROWS;
  const int ntiles = (n + 15) >> 4;
  long s = blocks > 0 ? GB_TARGET_BLOCKS / blocks : 1;
  if (s > ntiles / 16) s = ntiles / 16;
  return s < 1 ? 1 : (int)s;
}

extern "C" int nk_gumbel_logits(const float* z, long ldz, const float* w, const float* bias, float* logits, long ldl, long N, int h, int n,
                                void* stream_) {
  if (h < 1 || h > NK_VQ_MAX_D) return gb_refuse(__LINE__, "gumbel_logits: 1 <= num_hiddens <= 256 (NK_VQ_MAX_D)");
  if (n < 1 || n > NK_VQ_MAX_CODES) return gb_refuse(__LINE__, "gumbel_logits: 1 <= n_embed <= 65536 (NK_VQ_MAX_CODES)");
  if (N < 0 || N >= (1L << 31)) return gb_refuse(__LINE__, "gumbel_logits: N < 2^31");
  NK_CHECK_ARG(z && w && bias && logits && ldz >= h && ldl >= n);
  if (N == 0) return NK_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const int splits = gb_splits(N, n), ntiles = (n + 15) >> 4;
  const int tiles_per_split = (ntiles + splits - 1) / splits;
  const dim3 grid((unsigned)((N + GB_ROWS - 1) / GB_ROWS), splits), block(64 * GB_WAVES);
#define GB_LAUNCH(KS) hipLaunchKernelGGL(gumbel_logits_kernel<KS>, grid, block, 0, stream, z, ldz, w, bias, logits, ldl, (int)N, h, n, tiles_per_split)
  if (h <= 4) GB_LAUNCH(1);
  else if (h <= 8) GB_LAUNCH(2);
  else if (h <= 16) GB_LAUNCH(4);
  else if (h <= 32) GB_LAUNCH(8);
  else if (h <= 64) GB_LAUNCH(16);
  else if (h <= 128) GB_LAUNCH(32);
  else GB_LAUNCH(64);
#undef GB_LAUNCH
  return nk_check_launch("gumbel_logits");
}

// ---- the noise ----------------------------------------------------------------------------------------------------------------------
// g is a pure function of (token, site, logical element e = i * n + j): Philox4x32-10, one call per 4 consecutive elements, v = e / 4,
// counter (v lo, v hi, site, step lo), key (seed lo, seed hi ^ GB_KEY_XOR); element e % 4 takes word w:
//     u = (2 * (w >> 9) + 1) * 2^-24      an odd 24-bit integer, scaled: exact in fp32, never 0 or 1
//     g = -logf(-logf(u))                 the library logf, not the fast intrinsic
__device__ __forceinline__ uint4_t gb_philox(uint4_t c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    uint4_t nx;
    nx.x = hi1 ^ c.y ^ k0;
    nx.y = lo1;
    nx.z = hi0 ^ c.w ^ k1;
    nx.w = lo0;
    c = nx;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
struct GbKey {
  unsigned k0, k1, site, step;
};
__device__ __forceinline__ GbKey gb_key(const unsigned long long* __restrict__ token, unsigned site) {
  const unsigned long long seed = token[0], step = token[1];
  GbKey k;
  k.k0 = (unsigned)seed;
  k.k1 = (unsigned)(seed >> 32) ^ GB_KEY_XOR;
  k.site = site;
  k.step = (unsigned)step;
  return k;
}
__device__ __forceinline__ uint4_t gb_words(const GbKey& k, unsigned long long v) {
  uint4_t c;
  c.x = (unsigned)v;
  c.y = (unsigned)(v >> 32);
  c.z = k.site;
  c.w = k.step;
  return gb_philox(c, k.k0, k.k1);
}
__device__ __forceinline__ float gb_from_word(unsigned w) {
  const float u = __fmul_rn((float)(2u * (w >> 9) + 1u), 5.9604644775390625e-08f);      // 2^-24
  return -logf(-logf(u));
}
__device__ __forceinline__ unsigned gb_pick(const uint4_t& w, unsigned m) { return m == 0 ? w.x : m == 1 ? w.y : m == 2 ? w.z : w.w; }
// the noise of elements e0 .. e0 + 3 (those below `end`): one Philox call when e0 is a multiple of 4, else one per 4-aligned run it touches
__device__ __forceinline__ void gb_noise4(const GbKey& k, unsigned long long e0, unsigned long long end, float* g) {
  if ((e0 & 3) == 0) {
    const uint4_t w = gb_words(k, e0 >> 2);
#pragma unroll
    for (int m = 0; m < 4; ++m) g[m] = e0 + m < end ? gb_from_word(gb_pick(w, m)) : 0.f;
    return;
  }
  const uint4_t w0 = gb_words(k, e0 >> 2), w1 = gb_words(k, (e0 >> 2) + 1);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const unsigned long long e = e0 + m;
    g[m] = e < end ? gb_from_word(gb_pick((e >> 2) == (e0 >> 2) ? w0 : w1, (unsigned)(e & 3))) : 0.f;
  }
}

__global__ __launch_bounds__(GB_THREADS) void gumbel_noise_kernel(float* __restrict__ g, unsigned long long total,
                                                                  const unsigned long long* __restrict__ token, unsigned site) {
  const GbKey k = gb_key(token, site);
  const unsigned long long nvec = (total + 3) >> 2;
  for (unsigned long long v = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; v < nvec; v += (unsigned long long)gridDim.x * blockDim.x) {
    float o[4];
    gb_noise4(k, 4 * v, total, o);
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (4 * v + m < total) g[4 * v + m] = o[m];
  }
}

extern "C" int nk_gumbel_noise(float* g, long rows, int cols, const void* token, int site, void* stream) {
  NK_CHECK_ARG(g && token && rows >= 0 && cols >= 1 && site >= 0 && ((uintptr_t)token & 7) == 0);
  const unsigned long long total = (unsigned long long)rows * cols;
  if (total == 0) return NK_OK;
  unsigned long long blocks = ((total + 3) / 4 + GB_THREADS - 1) / GB_THREADS;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gumbel_noise_kernel, dim3((unsigned)blocks), dim3(GB_THREADS), 0, (hipStream_t)stream, g, total,
                     (const unsigned long long*)token, (unsigned)site);
  return nk_check_launch("gumbel_noise");
}

// ---- workgroup reductions in a fixed order ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float gb_block_sum(float v, float* sm) {
  v = wave_sum(v);
  __syncthreads();                         // the previous reduction's readers are done with sm
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = sm[0];
#pragma unroll
  for (int w = 1; w < GB_WAVES; ++w) s += sm[w];
  return s;
}
__device__ __forceinline__ float gb_block_max(float v, float* sm) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = sm[0];
#pragma unroll
  for (int w = 1; w < GB_WAVES; ++w) s = fmaxf(s, sm[w]);
  return s;
}
// (a2, i2) beats (a, i): larger score, or the same score at a lower index.  A NaN compares false both ways and is never taken.
__device__ __forceinline__ bool gb_better(float a2, int i2, float a, int i) { return a2 > a || (a2 == a && i2 < i); }

// four fp32 values of a row from column j0 (a multiple of 4); columns >= n give `fill`
__device__ __forceinline__ void gb_load4(const float* __restrict__ p, int j0, int n, bool vec, float fill, float* o) {
  if (vec && j0 + 4 <= n) {
    const float4_t v = *(const float4_t*)(p + j0);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    return;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) o[m] = j0 + m < n ? p[j0 + m] : fill;
}

// ---- forward: y = softmax((l + g) / tau) (bf16), idx = argmax, kl_row = sum_j q_j log(q_j n + 1e-10), q = softmax(l) -----------------------------
// G = groups of 4 per thread held in registers (1 or 8); G = 0 reads (and draws) the row again in every pass.
template <int G>
__global__ __launch_bounds__(GB_THREADS) void gumbel_softmax_fwd_kernel(const float* __restrict__ logits, long ldl, const float* __restrict__ noise,
                                                                        const unsigned long long* __restrict__ token, unsigned site, float inv_tau,
                                                                        bf16_t* __restrict__ y, long long* __restrict__ idx,
                                                                        float* __restrict__ kl_row, int n) {
  __shared__ float sm[GB_WAVES];
  __shared__ float sa[GB_WAVES];
  __shared__ int si[GB_WAVES];
  const int t = threadIdx.x;
  const long row = blockIdx.x;
  const float* lrow = logits + row * ldl;
  const float* nrow = noise ? noise + row * (long)n : nullptr;
  const bool lvec = (ldl & 3) == 0 && ((uintptr_t)logits & 15) == 0, nvec = (n & 3) == 0 && ((uintptr_t)noise & 15) == 0;
  const unsigned long long e_row = (unsigned long long)row * (unsigned long long)n;
  GbKey key = {0u, 0u, 0u, 0u};
  if (!nrow) key = gb_key(token, site);
  const float ninf = -__builtin_inff();
  const int groups = G ? G : (n + 4 * GB_THREADS - 1) / (4 * GB_THREADS);

  auto fetch = [&](int gi, float* l, float* a) {        // l and a = (l + g) * inv_tau of group gi; -inf past the end of the row
    const int j0 = 4 * (t + GB_THREADS * gi);
    float g[4];
    gb_load4(lrow, j0, n, lvec, ninf, l);
    if (nrow) gb_load4(nrow, j0, n, nvec, 0.f, g);
    else gb_noise4(key, e_row + j0, e_row + n, g);
#pragma unroll
    for (int m = 0; m < 4; ++m) a[m] = j0 + m < n ? __fmul_rn(__fadd_rn(l[m], g[m]), inv_tau) : ninf;
  };

  float L[G ? G : 1][4], A[G ? G : 1][4];
  if constexpr (G > 0) {
#pragma unroll
    for (int gi = 0; gi < G; ++gi) fetch(gi, L[gi], A[gi]);
  }
  auto get = [&](int gi, float* l, float* a) {
    if constexpr (G > 0) {
#pragma unroll
      for (int m = 0; m < 4; ++m) { l[m] = L[gi][m]; a[m] = A[gi][m]; }
    } else {
      fetch(gi, l, a);
    }
  };

  // pass 1: the two maxima and the argmax of a
  float ma = ninf, ml = ninf;
  int bi = GB_NONE;
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], a[4];
    get(gi, l, a);
    const int j0 = 4 * (t + GB_THREADS * gi);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      ml = fmaxf(ml, l[m]);
      if (a[m] > ma) { ma = a[m]; bi = j0 + m; }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float a2 = __shfl_xor(ma, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (gb_better(a2, i2, ma, bi)) { ma = a2; bi = i2; }
  }
  if ((t & 63) == 0) { sa[t >> 6] = ma; si[t >> 6] = bi; }
  ml = gb_block_max(ml, sm);               // its barriers publish sa / si as well
  ma = sa[0];
  bi = si[0];
#pragma unroll
  for (int w = 1; w < GB_WAVES; ++w)
    if (gb_better(sa[w], si[w], ma, bi)) { ma = sa[w]; bi = si[w]; }
  if (t == 0) idx[row] = bi == GB_NONE ? 0 : bi;        // a row of NaN / -inf scores takes 0

  // pass 2: the two normalisers
  float sum_a = 0.f, sum_l = 0.f;
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], a[4];
    get(gi, l, a);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      sum_a += expf(a[m] - ma);
      sum_l += expf(l[m] - ml);
    }
  }
  sum_a = gb_block_sum(sum_a, sm);
  sum_l = gb_block_sum(sum_l, sm);

  // pass 3: y and the KL terms
  const float fn = (float)n;
  float kl = 0.f;
  bf16_t* yrow = y + row * (long)n;
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], a[4];
    get(gi, l, a);
    const int j0 = 4 * (t + GB_THREADS * gi);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (j0 + m >= n) continue;
      yrow[j0 + m] = f2bf(expf(a[m] - ma) / sum_a);
      const float q = expf(l[m] - ml) / sum_l;
      kl = __fadd_rn(kl, __fmul_rn(q, logf(__fadd_rn(__fmul_rn(q, fn), 1e-10f))));
    }
  }
  kl = gb_block_sum(kl, sm);
  if (t == 0) kl_row[row] = kl;
}

// kl[0] = (1 / N) sum_i kl_row[i] through the fixed-order reducer: thread ty adds rows ty, ty + 256, ... in order, thread 0 the 256 slots in order
__global__ __launch_bounds__(GB_THREADS) void gumbel_kl_mean_kernel(const float* __restrict__ kl_row, int N, float* __restrict__ out) {
  nk_reduce_rows<GB_THREADS, 1, 1, 0, 0>(
      true, N, [&](int r, float* acc) { acc[0] += kl_row[r]; }, [&](const float* acc) { out[0] = acc[0] / (float)N; });
}

extern "C" long nk_gumbel_softmax_ws_floats(long N) { return N <= 0 ? 1 : N; }

extern "C" int nk_gumbel_softmax_fwd(const float* logits, long ldl, const float* noise, const void* token, int site, float inv_tau, void* y,
                                     long long* idx, float* kl, float* ws, long N, int n, void* stream_) {
  if (n < 1 || n > NK_VQ_MAX_CODES) return gb_refuse(__LINE__, "gumbel_softmax_fwd: 1 <= n_embed <= 65536 (NK_VQ_MAX_CODES)");
  if (N < 1 || N >= (1L << 31)) return gb_refuse(__LINE__, "gumbel_softmax_fwd: 1 <= N < 2^31");
  if (!noise && !token) return gb_refuse(__LINE__, "gumbel_softmax_fwd: a noise matrix or a token");
  NK_CHECK_ARG(logits && y && idx && kl && ws && ldl >= n && site >= 0 && inv_tau > 0.f && ((uintptr_t)token & 7) == 0);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)N), block(GB_THREADS);
#define GB_LAUNCH(G)                                                                                                                          \
  hipLaunchKernelGGL(gumbel_softmax_fwd_kernel<G>, grid, block, 0, stream, logits, ldl, noise, (const unsigned long long*)token, (unsigned)site, \
                     inv_tau, (bf16_t*)y, idx, ws, n)
  if (n <= 4 * GB_THREADS) GB_LAUNCH(1);
  else if (n <= 32 * GB_THREADS) GB_LAUNCH(8);
  else GB_LAUNCH(0);
#undef GB_LAUNCH
  hipLaunchKernelGGL(gumbel_kl_mean_kernel, dim3(1), dim3(GB_THREADS), 0, stream, (const float*)ws, (int)N, kl);
  return nk_check_launch("gumbel_softmax_fwd");
}

// ---- backward, in place on bf16 G = d<dz_q, z_q>/dS ------------------------------------------------------------------------------------
//     d_j = inv_tau y_j (G_j - sum_k G_k y_k) + (w_kl / N) q_j (h_j - sum_k q_k h_k),   h_j = log(q_j n + 1e-10) + q_j n / (q_j n + 1e-10)
// q = softmax(l) is recomputed from the fp32 logits.  A thread reads its own elements of G before it writes them, and the row's sums are
// complete (behind barriers) before the first write.
template <int G>
__global__ __launch_bounds__(GB_THREADS) void gumbel_softmax_bwd_kernel(const float* __restrict__ logits, long ldl, const bf16_t* __restrict__ y,
                                                                        bf16_t* gmat, float inv_tau, float c_kl, int n) {
  __shared__ float sm[GB_WAVES];
  const int t = threadIdx.x;
  const long row = blockIdx.x;
  const float* lrow = logits + row * ldl;
  const bf16_t* yrow = y + row * (long)n;
  bf16_t* grow = gmat + row * (long)n;
  const bool lvec = (ldl & 3) == 0 && ((uintptr_t)logits & 15) == 0;
  const float ninf = -__builtin_inff();
  const int groups = G ? G : (n + 4 * GB_THREADS - 1) / (4 * GB_THREADS);

  auto fetch = [&](int gi, float* l, float* yy, float* gg) {
    const int j0 = 4 * (t + GB_THREADS * gi);
    gb_load4(lrow, j0, n, lvec, ninf, l);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const bool in = j0 + m < n;
      yy[m] = in ? bf2f(yrow[j0 + m]) : 0.f;
      gg[m] = in ? bf2f(grow[j0 + m]) : 0.f;
    }
  };
  float L[G ? G : 1][4], Y[G ? G : 1][4], D[G ? G : 1][4];
  if constexpr (G > 0) {
#pragma unroll
    for (int gi = 0; gi < G; ++gi) fetch(gi, L[gi], Y[gi], D[gi]);
  }
  auto get = [&](int gi, float* l, float* yy, float* gg) {
    if constexpr (G > 0) {
#pragma unroll
      for (int m = 0; m < 4; ++m) { l[m] = L[gi][m]; yy[m] = Y[gi][m]; gg[m] = D[gi][m]; }
    } else {
      fetch(gi, l, yy, gg);
    }
  };

  float ml = ninf, gy = 0.f;
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], yy[4], gg[4];
    get(gi, l, yy, gg);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      ml = fmaxf(ml, l[m]);
      gy = __builtin_fmaf(gg[m], yy[m], gy);
    }
  }
  ml = gb_block_max(ml, sm);
  gy = gb_block_sum(gy, sm);
  float sum_l = 0.f;
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], yy[4], gg[4];
    get(gi, l, yy, gg);
#pragma unroll
    for (int m = 0; m < 4; ++m) sum_l += expf(l[m] - ml);
  }
  sum_l = gb_block_sum(sum_l, sm);
  const float fn = (float)n;
  float qh = 0.f;
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], yy[4], gg[4];
    get(gi, l, yy, gg);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float q = expf(l[m] - ml) / sum_l;
      const float x = __fmul_rn(q, fn), xe = __fadd_rn(x, 1e-10f);
      qh = __builtin_fmaf(q, logf(xe) + x / xe, qh);
    }
  }
  qh = gb_block_sum(qh, sm);              // its barriers also put every read of G in front of the writes below
#pragma unroll
  for (int gi = 0; gi < groups; ++gi) {
    float l[4], yy[4], gg[4];
    get(gi, l, yy, gg);
    const int j0 = 4 * (t + GB_THREADS * gi);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      if (j0 + m >= n) continue;
      const float q = expf(l[m] - ml) / sum_l;
      const float x = __fmul_rn(q, fn), xe = __fadd_rn(x, 1e-10f);
      const float hj = logf(xe) + x / xe;
      grow[j0 + m] = f2bf(inv_tau * yy[m] * (gg[m] - gy) + c_kl * q * (hj - qh));
    }
  }
}

extern "C" int nk_gumbel_softmax_bwd(const float* logits, long ldl, const void* y, void* G, float inv_tau, float w_kl, long N, int n,
                                     void* stream_) {
  if (n < 1 || n > NK_VQ_MAX_CODES) return gb_refuse(__LINE__, "gumbel_softmax_bwd: 1 <= n_embed <= 65536 (NK_VQ_MAX_CODES)");
  if (N < 1 || N >= (1L << 31)) return gb_refuse(__LINE__, "gumbel_softmax_bwd: 1 <= N < 2^31");
  NK_CHECK_ARG(logits && y && G && ldl >= n && inv_tau > 0.f);
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid((unsigned)N), block(GB_THREADS);
  const float c_kl = w_kl / (float)N;
#define GB_LAUNCH(GR) \
  hipLaunchKernelGGL(gumbel_softmax_bwd_kernel<GR>, grid, block, 0, stream, logits, ldl, (const bf16_t*)y, (bf16_t*)G, inv_tau, c_kl, n)
  if (n <= 4 * GB_THREADS) GB_LAUNCH(1);
  else if (n <= 32 * GB_THREADS) GB_LAUNCH(8);
  else GB_LAUNCH(0);
#undef GB_LAUNCH
  return nk_check_launch("gumbel_softmax_bwd");
}
