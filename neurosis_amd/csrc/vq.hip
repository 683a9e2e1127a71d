// Vector-quantizer bottleneck (VQGAN / VQ-f4 / f8 / f16 first stages; reference modules/autoencoding/regularizers/quantize.py):
// nearest-code search on the exact fp32 MFMA, per-code statistics, codebook gather with the squared-error sum.
// Plain HIP and compiler builtins; no float atomics anywhere: every result is bit-reproducible from run to run.
#include "../../include/neurosis_hip.h"
#include "nk_common.h"

#define VQ_ROWS 32          // rows of z per workgroup: two 16-row MFMA groups, held in registers for the whole launch
#define VQ_WAVES 4          // the waves of a workgroup split the code tiles: wave w takes tiles w, w + 4, ...
#define VQ_NONE 0x7fffffff  // "no code yet"

static int vq_refuse(int line, const char* what) {
  nk_set_error(__FILE__, line, what);
  return NK_ERR_ARG;
}

// ---- n_j = sum_k e_jk^2: an fp32 fma chain in k order, once per launch -----------------------------------------------
__global__ void vq_norms_kernel(const float* __restrict__ cb, float* __restrict__ norms, int n_e, int D) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_e) return;
  const float* e = cb + (long)j * D;
  float n = 0.f;
  for (int k = 0; k < D; ++k) n = __builtin_fmaf(e[k], e[k], n);
  norms[j] = n;
}

// (d2, i2) beats (d, i): smaller score, or the same score at a lower index.  Scores that reach a merge are never NaN.
__device__ __forceinline__ bool vq_better(float d2, int i2, float d, int i) { return d2 < d || (d2 == d && i2 < i); }

// ---- code search --------------------------------------------------------------------------------------------------------
// score d_j = fma(-2, z . e_j, n_j); the dot product comes from v_mfma_f32_16x16x4_f32, whose result is bit for bit the fmaf chain
// fma(z_k, e_jk, acc) in k order from acc = 0.  K = 4 * KS >= D, the tail multiplies zeros by zeros, which adds exactly.
// A operand: lane l holds z[row (l & 15)][k = l >> 4], B operand e[code (l & 15)][k = l >> 4]; the result has the code on the lane
// (l & 15) and z rows 4 * (l >> 4) + r in its four registers.  The [N, n_e] matrix exists only as those registers: every lane keeps a
// running (min, index) per row over the codes it sees in rising order (strict <, so the lowest index of equal scores stays; a NaN
// score compares false and is never taken), then the 16 lanes of a row merge by shuffles, then the waves through LDS, both under
// vq_better.  A row whose scores are all NaN or +inf reaches the end with no index: it takes the first +inf score, or 0.
// When there are too few rows to fill the machine, blockIdx.y splits the code tiles as well (vq_splits): each split leaves its
// (min, index) per row in `part`, and vq_merge_kernel merges them in split order under the same vq_better -- min with the lowest index
// is associative, so the index does not depend on how the codes were cut.
__device__ __forceinline__ int vq_rescue(const float* __restrict__ z, const float* __restrict__ cb, const float* __restrict__ norms, int D,
                                         int n_e) {
  for (int j = 0; j < n_e; ++j) {       // every score NaN or +inf (rare): the same arithmetic one code at a time
    float dot = 0.f;
    for (int k = 0; k < D; ++k) dot = __builtin_fmaf(z[k], cb[(long)j * D + k], dot);
    if (__builtin_fmaf(-2.f, dot, norms[j]) == __builtin_inff()) return j;
  }
  return 0;
}

template <int KS>
__global__ __launch_bounds__(64 * VQ_WAVES) void vq_search_kernel(const float* __restrict__ z, long ldz, const float* __restrict__ cb,
                                                                   const float* __restrict__ norms, long long* __restrict__ idx,
                                                                   float* __restrict__ part_d, int* __restrict__ part_i, int N, int D,
                                                                   int n_e, int tiles_per_split) {
  __shared__ float sd[VQ_WAVES][VQ_ROWS];
  __shared__ int si[VQ_WAVES][VQ_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const long row0 = (long)blockIdx.x * VQ_ROWS;
  float a[2][KS];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const long row = row0 + 16 * g + c;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + q;
      a[g][s] = (row < N && k < D) ? z[row * ldz + k] : 0.f;
    }
  }
  float best[2][4];
  int bi[2][4];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      best[g][r] = __builtin_inff();
      bi[g][r] = VQ_NONE;
    }
  const int ntiles = (n_e + 15) >> 4;
  const int t1 = min(ntiles, ((int)blockIdx.y + 1) * tiles_per_split);
  for (int t = blockIdx.y * tiles_per_split + wave; t < t1; t += VQ_WAVES) {
    const int j = t * 16 + c;
    const bool live = j < n_e;
    const float* e = cb + (long)(live ? j : 0) * D;
    float4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};      // two independent chains cover the MFMA's latency
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 4 * s + q;
      const float b = (live && k < D) ? e[k] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][s], b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][s], b, acc1, 0, 0, 0);
    }
    const float nj = live ? norms[j] : __builtin_nanf("");       // a code past the end scores NaN: never taken
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d0 = __builtin_fmaf(-2.f, acc0[r], nj), d1 = __builtin_fmaf(-2.f, acc1[r], nj);
      if (d0 < best[0][r]) { best[0][r] = d0; bi[0][r] = j; }
      if (d1 < best[1][r]) { best[1][r] = d1; bi[1][r] = j; }
    }
  }
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float d2 = __shfl_xor(best[g][r], o, 64);
        const int i2 = __shfl_xor(bi[g][r], o, 64);
        if (vq_better(d2, i2, best[g][r], bi[g][r])) { best[g][r] = d2; bi[g][r] = i2; }
      }
      if (c == 0) {
        sd[wave][16 * g + 4 * q + r] = best[g][r];
        si[wave][16 * g + 4 * q + r] = bi[g][r];
      }
    }
  __syncthreads();
  const int t = threadIdx.x;
  const long row = row0 + t;
  if (t >= VQ_ROWS || row >= N) return;
  float d = sd[0][t];
  int i = si[0][t];
#pragma unroll
  for (int w = 1; w < VQ_WAVES; ++w)
    if (vq_better(sd[w][t], si[w][t], d, i)) { d = sd[w][t]; i = si[w][t]; }
  if (gridDim.y > 1) {
    part_d[(long)blockIdx.y * N + row] = d;
    part_i[(long)blockIdx.y * N + row] = i;
    return;
  }
  idx[row] = i == VQ_NONE ? vq_rescue(z + row * ldz, cb, norms, D, n_e) : i;
}

__global__ void vq_merge_kernel(const float* __restrict__ part_d, const int* __restrict__ part_i, int splits, const float* __restrict__ z,
                                long ldz, const float* __restrict__ cb, const float* __restrict__ norms, long long* __restrict__ idx, int N,
                                int D, int n_e) {
  const long row = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (row >= N) return;
  float d = part_d[row];
  int i = part_i[row];
  for (int s = 1; s < splits; ++s) {
    const float d2 = part_d[(long)s * N + row];
    const int i2 = part_i[(long)s * N + row];
    if (vq_better(d2, i2, d, i)) { d = d2; i = i2; }
  }
  idx[row] = i == VQ_NONE ? vq_rescue(z + row * ldz, cb, norms, D, n_e) : i;
}

// How many ways the code tiles are cut: enough workgroups for about four waves per SIMD of the 256 CUs, at least 16 tiles (four per
// wave) to a cut.  One cut (the direct path) from N = 32768 rows on, and always for small codebooks.
#define VQ_TARGET_BLOCKS 1024
static int vq_splits(long N, int n_e) {
  const long blocks = (N + VQ_ROWS - 1) / VQ_ROWS;
  const int ntiles = (n_e + 15) >> 4;
  long s = blocks > 0 ? VQ_TARGET_BLOCKS / blocks : 1;
  if (s > ntiles / 16) s = ntiles / 16;
  return s < 1 ? 1 : (int)s;
}
extern "C" long nk_vq_search_ws_floats(long N, int n_e) {
  if (N < 0 || n_e < 1) return 0;
  const int s = vq_splits(N, n_e);
  return n_e + (s > 1 ? 2L * s * N : 0);
}

extern "C" int nk_vq_search(const float* z, long ldz, const float* codebook, float* ws, long long* idx, long N, int D, int n_e,
                            void* stream_) {
  if (D < 1 || D > NK_VQ_MAX_D) return vq_refuse(__LINE__, "vq_search: 1 <= D <= 256 (NK_VQ_MAX_D)");
  if (n_e < 1 || n_e > NK_VQ_MAX_CODES) return vq_refuse(__LINE__, "vq_search: 1 <= n_e <= 65536 (NK_VQ_MAX_CODES)");
  if (N < 0 || N >= (1L << 31)) return vq_refuse(__LINE__, "vq_search: N < 2^31");
  NK_CHECK_ARG(z && codebook && ws && idx && ldz >= D);
  if (N == 0) return NK_OK;
  hipStream_t stream = (hipStream_t)stream_;
  float* norms = ws;                                  // ws: [n_e] norms, then [splits][N] scores and [splits][N] indices
  const int splits = vq_splits(N, n_e), ntiles = (n_e + 15) >> 4;
  const int tiles_per_split = (ntiles + splits - 1) / splits;
  float* part_d = ws + n_e;
  int* part_i = (int*)(part_d + (long)splits * N);
  hipLaunchKernelGGL(vq_norms_kernel, dim3((n_e + 255) / 256), dim3(256), 0, stream, codebook, norms, n_e, D);
  const dim3 grid((unsigned)((N + VQ_ROWS - 1) / VQ_ROWS), splits), block(64 * VQ_WAVES);
#define VQ_LAUNCH(KS)                                                                                                                  \
  hipLaunchKernelGGL(vq_search_kernel<KS>, grid, block, 0, stream, z, ldz, codebook, (const float*)norms, idx, part_d, part_i, (int)N, D, n_e, \
                     tiles_per_split)
  if (D <= 4) VQ_LAUNCH(1);
  else if (D <= 8) VQ_LAUNCH(2);
  else if (D <= 16) VQ_LAUNCH(4);
  else if (D <= 32) VQ_LAUNCH(8);
  else if (D <= 64) VQ_LAUNCH(16);
  else if (D <= 128) VQ_LAUNCH(32);
  else VQ_LAUNCH(64);
#undef VQ_LAUNCH
  if (splits > 1)
    hipLaunchKernelGGL(vq_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, (const float*)part_d, (const int*)part_i, splits,
                       z, ldz, codebook, (const float*)norms, idx, (int)N, D, n_e);
  return nk_check_launch("vq_search");
}

// ---- per-code count and sum of the rows that chose it ---------------------------------------------------------------------
// A wave owns VQ_STATS_CPW consecutive codes and walks ALL row ids, 64 at a time; a ballot per code gives the rows of that chunk that
// chose it, and the wave adds those rows of z in rising row order (lane = column, up to four columns a lane).  So sum[j] is one
// addition chain over the rows of code j in row order -- count[j] additions, the longest chain of the result -- whatever the
// schedule; count[j] is a sum of popcounts.  No sort, no atomics; codes nobody chose come out as the zeros they started from.
// The walk is serial in the rows of one code: a codebook collapsed onto one code is summed by one wave.
#define VQ_STATS_CPW 8
__global__ __launch_bounds__(256) void vq_code_stats_kernel(const long long* __restrict__ idx, const float* __restrict__ z, long ldz,
                                                            long long* __restrict__ count, float* __restrict__ sum, int N, int D, int n_e) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = (blockIdx.x * 4 + wave) * VQ_STATS_CPW;
  if (j0 >= n_e) return;
  float acc[VQ_STATS_CPW][4];
  int cnt[VQ_STATS_CPW];
#pragma unroll
  for (int c = 0; c < VQ_STATS_CPW; ++c) {
    cnt[c] = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[c][u] = 0.f;
  }
  for (long base = 0; base < N; base += 64) {
    const long i = base + lane;
    const long long v = i < N ? idx[i] : -1;
    const int rel = (v >= j0 && v < j0 + VQ_STATS_CPW) ? (int)(v - j0) : -1;
    if (__ballot(rel >= 0) == 0) continue;
#pragma unroll
    for (int c = 0; c < VQ_STATS_CPW; ++c) {
      unsigned long long m = __ballot(rel == c);
      cnt[c] += __popcll(m);
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const float* zr = z + (base + b) * ldz;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int col = lane + 64 * u;
          if (col < D) acc[c][u] += zr[col];
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < VQ_STATS_CPW; ++c) {
    const int j = j0 + c;
    if (j >= n_e) break;
    if (lane == 0) count[j] = cnt[c];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int col = lane + 64 * u;
      if (col < D) sum[(long)j * D + col] = acc[c][u];
    }
  }
}

extern "C" int nk_vq_code_stats(const long long* idx, const float* z, long ldz, long long* count, float* sum, long N, int D, int n_e,
                                void* stream_) {
  if (D < 1 || D > NK_VQ_MAX_D) return vq_refuse(__LINE__, "vq_code_stats: 1 <= D <= 256 (NK_VQ_MAX_D)");
  if (n_e < 1 || n_e > NK_VQ_MAX_CODES) return vq_refuse(__LINE__, "vq_code_stats: 1 <= n_e <= 65536 (NK_VQ_MAX_CODES)");
  if (N < 0 || N >= (1L << 31)) return vq_refuse(__LINE__, "vq_code_stats: N < 2^31");
  NK_CHECK_ARG(idx && z && count && sum && ldz >= D);
  const int per_block = 4 * VQ_STATS_CPW;
  hipLaunchKernelGGL(vq_code_stats_kernel, dim3((n_e + per_block - 1) / per_block), dim3(256), 0, (hipStream_t)stream_, idx, z, ldz, count, sum,
                     (int)N, D, n_e);
  return nk_check_launch("vq_code_stats");
}

// ---- z_q = codebook[idx] and sum (z_q - z)^2 --------------------------------------------------------------------------------
// Row i = b * HW + p of z goes to zq[b][k][p] (fp32 NCHW; HW = 1 is the plain [N, D] matrix).  One thread per row: its squared
// error is an fma chain over k (D links); a workgroup's 256 rows are summed by a halving tree in LDS (8 links) into partial[block];
// the second kernel's thread t adds partials t, t + 256, ... in order (ceil(blocks / 256) links) and a second tree (8 links) gives the
// scalar.  Longest addition chain: D + ceil(ceil(N / 256) / 256) + 16, every term non-negative.  An index outside the codebook reads
// nothing and writes NaN.
__global__ __launch_bounds__(256) void vq_quantize_kernel(const long long* __restrict__ idx, const float* __restrict__ cb,
                                                          const float* __restrict__ z, long ldz, float* __restrict__ zq,
                                                          float* __restrict__ partial, int N, int D, int n_e, int HW) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  const long i = blockIdx.x * 256L + t;
  float s = 0.f;
  if (i < N) {
    const long long j = idx[i];
    const bool ok = j >= 0 && j < n_e;
    const float* e = cb + (ok ? j : 0) * D;
    const long b = i / HW, p = i - b * HW;
    float* o = zq + b * D * HW + p;
    const float* zr = z + i * ldz;
    for (int k = 0; k < D; ++k) {
      const float v = ok ? e[k] : __builtin_nanf("");
      o[(long)k * HW] = v;
      const float df = v - zr[k];
      s = __builtin_fmaf(df, df, s);
    }
  }
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void vq_sumsq_kernel(const float* __restrict__ partial, int n, float* __restrict__ out) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  float s = 0.f;
  for (int i = t; i < n; i += 256) s += partial[i];
  red[t] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  if (t == 0) out[0] = red[0];
}

extern "C" long nk_vq_quantize_ws_floats(long N) { return N <= 0 ? 1 : (N + 255) / 256; }

extern "C" int nk_vq_quantize(const long long* idx, const float* codebook, const float* z, long ldz, float* zq, float* sumsq, float* ws,
                              long N, int D, int n_e, int HW, void* stream_) {
  if (D < 1 || D > NK_VQ_MAX_D) return vq_refuse(__LINE__, "vq_quantize: 1 <= D <= 256 (NK_VQ_MAX_D)");
  if (n_e < 1 || n_e > NK_VQ_MAX_CODES) return vq_refuse(__LINE__, "vq_quantize: 1 <= n_e <= 65536 (NK_VQ_MAX_CODES)");
  if (N < 1 || N >= (1L << 31)) return vq_refuse(__LINE__, "vq_quantize: 1 <= N < 2^31");
  NK_CHECK_ARG(idx && codebook && z && zq && sumsq && ws && ldz >= D && HW >= 1 && N % HW == 0);
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = (int)((N + 255) / 256);
  hipLaunchKernelGGL(vq_quantize_kernel, dim3(blocks), dim3(256), 0, stream, idx, codebook, z, ldz, zq, ws, (int)N, D, n_e, HW);
  hipLaunchKernelGGL(vq_sumsq_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws, blocks, sumsq);
  return nk_check_launch("vq_quantize");
}
