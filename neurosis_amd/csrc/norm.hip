// HBM-bound normalisation kernels on channels-last bf16 data: GroupNorm(+SiLU) and LayerNorm,
// forward and backward.  Statistics are fp32; reductions are staged per thread -> LDS -> one fp32
// atomic per (block, statistic); loads and stores are 16 B per lane and row-contiguous.
//
// Reference: nn.GroupNorm(32, C)+nn.SiLU (modules/diffusion/openaimodel.py:247-250,281-283,797-799),
// SpatialTransformer.norm (modules/attention.py:612, eps 1e-6), Normalize (modules/layers.py:5-7),
// nn.LayerNorm (modules/attention.py:468-470).
#include "../../include/neurosis_hip.h"
#include "nk_common.h"
#include "nk_reduce.h"
#include "norm_plan.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// GroupNorm forward, pass 1: per-(n, group) sum and sum of squares
// grid (nsplit, N); block handles rows [split*rows_per, ...) of image n
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const bf16_t* __restrict__ x, float* __restrict__ stats,
                                                              int HW, int C, int G, int rows_per) {
  // thread (rsub, chunk) accumulates 8 channels over its rows; partials are combined in a FIXED order
  // (LDS staging, no atomics) so the statistics -- and therefore the forward -- are bitwise reproducible
  __shared__ float ps[GN_THREADS * 8], pss[GN_THREADS * 8];
  const int n = blockIdx.y;
  const int cpr = (C >> 3) / gridDim.z;        // 16-byte chunks per row in this block's channel slab
  const int ch0 = blockIdx.z * cpr;            // first chunk of the slab
  const int rows_par = GN_THREADS / cpr;       // rows processed in parallel by the block
  const int tid = threadIdx.x;
  const int cpg = C / G;
  const int row_lo = blockIdx.x * rows_per;
  const int row_hi = min(HW, row_lo + rows_per);
  float s[8], ss[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; ss[e] = 0.f; }
  const int chunk = tid % cpr, rsub = tid / cpr;
  if (rsub < rows_par) {
    const bf16_t* base = x + ((long)n * HW) * C + (ch0 + chunk) * 8;
    int r = row_lo + rsub;
    for (; r + 3 * rows_par < row_hi; r += 4 * rows_par) {   // four rows' loads in flight per thread
      uint4_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const uint4_t*)(base + (long)(r + u * rows_par) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float f[8];
        unpack8(v[u], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] += f[e]; ss[e] += f[e] * f[e]; }
      }
    }
    for (; r < row_hi; r += rows_par) {
      float f[8];
      unpack8(*(const uint4_t*)(base + (long)r * C), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += f[e]; ss[e] += f[e] * f[e]; }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ps[(rsub * cpr + chunk) * 8 + e] = s[e];
      pss[(rsub * cpr + chunk) * 8 + e] = ss[e];
    }
  }
  __syncthreads();
  // per-block partial: part[n][blockIdx.x * gridDim.z + blockIdx.z][2G]; groups outside this slab get 0
  float* part = stats + (((long)n * gridDim.x + blockIdx.x) * gridDim.z + blockIdx.z) * 2 * G;
  for (int i = tid; i < 2 * G; i += GN_THREADS) {
    const int g = i >> 1;
    const float* src = (i & 1) ? pss : ps;
    const int c_lo = max(g * cpg, ch0 * 8), c_hi = min((g + 1) * cpg, (ch0 + cpr) * 8);
    float a = 0.f;
    for (int c = c_lo; c < c_hi; ++c)
      for (int r = 0; r < rows_par; ++r) a += src[r * cpr * 8 + (c - ch0 * 8)];
    part[i] = a;
  }
}

// sums the per-block partials of one image in a fixed order: out[n][2G] = sum_p part[n][p][2G]
// block = G2 (<= 128) columns x (1024 / 128) row groups, in the order of nk_reduce_rows
__global__ __launch_bounds__(1024) void gn_reduce_partials_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                 int nparts, int G2) {
  const int n = blockIdx.x, tx = threadIdx.x & 127;
  nk_reduce_rows<8, 128, 1, 0, 0>(
      tx < G2, nparts, [&](int p, float* a) { a[0] += part[((long)n * nparts + p) * G2 + tx]; },
      [&](const float* a) { out[(long)n * G2 + tx] = a[0]; });
}

// ------------------------------------------------------------------------------------------------
// GroupNorm forward, pass 2: y = silu?((x - mean) * rstd * gamma + beta); also emits mean / rstd
// The variance is formed in one pass, E[x^2] - E[x]^2 from fp32 sums, so its error grows as (|mean| / sigma)^2.  Measured at 163 840
// elements per group (tools/norm_one_pass_limit.py): relative rstd error 1.5e-4 at |mean| / sigma = 32, 6.9e-4 at 64, 3.0e-3 at 128.
// Half a bf16 ulp is 1.95e-3: beyond |mean| / sigma ~ 64 the statistics are no longer bf16-accurate.  The network's activations stay
// far below that; tests/test_norm_reductions_gpu.py holds the statistics to their derived bounds up to 32.
// ------------------------------------------------------------------------------------------------
// Scale-shift modulation (ResBlock use_scale_shift_norm, openaimodel.py:332-336): GN(x) * (1 + s_nc) + t_nc is a GroupNorm whose affine
// differs per image, gamma'_nc = gamma_c (1 + s_nc), beta'_nc = beta_c (1 + s_nc) + t_nc.  mod: bf16 [N][2C], scale | shift; all in fp32.
// With s = t = 0 both come out as gamma_c and beta_c exactly, so the MOD kernels then compute what the plain ones do, bit for bit.
__device__ __forceinline__ void gn_modulate(const bf16_t* __restrict__ mod, int n, int c, int C, float& ga, float& be) {
  const float s1 = 1.0f + bf2f(mod[(long)n * 2 * C + c]);
  const float t = bf2f(mod[(long)n * 2 * C + C + c]);
  ga = ga * s1;
  be = be * s1 + t;
}

template <bool MOD>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const bf16_t* __restrict__ mod,
                                                              bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                              float* __restrict__ rstd_out, int HW, int C, int G,
                                                              float eps, int silu, int rows_per) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* sc = (float*)smem_raw;   // [C]
  float* sh = sc + C;             // [C]
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int cpg = C / G;
  const float inv_cnt = 1.0f / ((float)HW * (float)cpg);
  for (int c = tid; c < C; c += GN_THREADS) {
    int g = c / cpg;
    float m = stats[(long)n * 2 * G + 2 * g] * inv_cnt;
    float var = fmaxf(stats[(long)n * 2 * G + 2 * g + 1] * inv_cnt - m * m, 0.f);
    float rs = rsqrtf(var + eps);
    float ga = gamma[c], be = beta[c];
    if constexpr (MOD) gn_modulate(mod, n, c, C, ga, be);
    float a = rs * ga;
    sc[c] = a;
    sh[c] = be - m * a;
    if (blockIdx.x == 0 && (c % cpg) == 0) { mean_out[n * G + g] = m; rstd_out[n * G + g] = rs; }
  }
  __syncthreads();
  const int cpr = C >> 3;
  const int row_lo = blockIdx.x * rows_per;
  const int row_hi = min(HW, row_lo + rows_per);
  const unsigned total = (unsigned)(row_hi - row_lo) * (unsigned)cpr;
  const bf16_t* xb = x + ((long)n * HW + row_lo) * C;
  bf16_t* yb = y + ((long)n * HW + row_lo) * C;
  auto one = [&](unsigned i, const uint4_t& raw) {
    const unsigned chunk = i % (unsigned)cpr;
    float f[8];
    unpack8(raw, f);
    const float4_t a0 = *(const float4_t*)(sc + chunk * 8), a1 = *(const float4_t*)(sc + chunk * 8 + 4);
    const float4_t b0 = *(const float4_t*)(sh + chunk * 8), b1 = *(const float4_t*)(sh + chunk * 8 + 4);
    f[0] = f[0] * a0[0] + b0[0]; f[1] = f[1] * a0[1] + b0[1]; f[2] = f[2] * a0[2] + b0[2]; f[3] = f[3] * a0[3] + b0[3];
    f[4] = f[4] * a1[0] + b1[0]; f[5] = f[5] * a1[1] + b1[1]; f[6] = f[6] * a1[2] + b1[2]; f[7] = f[7] * a1[3] + b1[3];
    if (silu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = silu_f(f[e]);
    }
    *(uint4_t*)(yb + (size_t)i * 8) = pack8(f);
  };
  unsigned i = tid;
  for (; i + 3 * GN_THREADS < total; i += 4 * GN_THREADS) {   // four 16-byte loads in flight per thread
    uint4_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const uint4_t*)(xb + (size_t)(i + u * GN_THREADS) * 8);
#pragma unroll
    for (int u = 0; u < 4; ++u) one(i + u * GN_THREADS, v[u]);
  }
  for (; i < total; i += GN_THREADS) one(i, *(const uint4_t*)(xb + (size_t)i * 8));
}

// ------------------------------------------------------------------------------------------------
// GroupNorm backward, pass 1.
//   dz = dy * silu'(z) (z = xhat*gamma+beta) or dy
//   per channel: a_c = sum dz, b_c = sum dz*xhat           -> dbeta += a, dgamma += b
//   per (n,g):   s1 = sum_c gamma_c a_c, s2 = sum_c gamma_c b_c -> gsum[n][g][2]
// ------------------------------------------------------------------------------------------------
//   MOD: gamma, beta are the image's gamma'_nc, beta'_nc; the channel partials stay per image (a_nc, b_nc) for the folds below
template <bool MOD>
__global__ __launch_bounds__(GN_THREADS, 4) void gn_bwd_stats_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const bf16_t* __restrict__ mod,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  float* __restrict__ gsum, float* __restrict__ chan_part,
                                                                  int HW, int C, int G, int silu, int rows_per) {
  __shared__ float pa[GN_THREADS * 8], pb[GN_THREADS * 8];   // per-thread partials, combined in a fixed order
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* ca = (float*)smem_raw;   // [slab channels] sum dz
  float* cb = ca + C;             // [slab channels] sum dz*xhat
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int cpg = C / G;
  const int cpr = (C >> 3) / gridDim.z;
  const int ch0 = blockIdx.z * cpr;
  const int rows_par = GN_THREADS / cpr;
  const int row_lo = blockIdx.x * rows_per;
  const int row_hi = min(HW, row_lo + rows_per);
  const int chunk = tid % cpr, rsub = tid / cpr;
  if (rsub < rows_par) {
    float a[8], b[8], mu[8], rs[8], ga[8], be[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int c = (ch0 + chunk) * 8 + e;
      int g = c / cpg;
      a[e] = 0.f; b[e] = 0.f;
      mu[e] = mean[n * G + g]; rs[e] = rstd[n * G + g];
      ga[e] = gamma[c]; be[e] = beta[c];
      if constexpr (MOD) gn_modulate(mod, n, c, C, ga[e], be[e]);
    }
    const long base = ((long)n * HW) * C + (ch0 + chunk) * 8;
    auto one = [&](const uint4_t& rx, const uint4_t& rd) {
      float fx[8], fd[8];
      unpack8(rx, fx);
      unpack8(rd, fd);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float xh = (fx[e] - mu[e]) * rs[e];
        float dz = fd[e];
        if (silu) dz *= dsilu_f(xh * ga[e] + be[e]);
        a[e] += dz;
        b[e] += dz * xh;
      }
    };
    int r = row_lo + rsub;
    for (; r + 3 * rows_par < row_hi; r += 4 * rows_par) {   // eight 16-byte loads in flight per thread
      uint4_t vx[4], vd[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        vx[u] = *(const uint4_t*)(x + base + (long)(r + u * rows_par) * C);
        vd[u] = *(const uint4_t*)(dy + base + (long)(r + u * rows_par) * C);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) one(vx[u], vd[u]);
    }
    for (; r < row_hi; r += rows_par) one(*(const uint4_t*)(x + base + (long)r * C), *(const uint4_t*)(dy + base + (long)r * C));
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pa[(rsub * cpr + chunk) * 8 + e] = a[e];
      pb[(rsub * cpr + chunk) * 8 + e] = b[e];
    }
  }
  __syncthreads();
  // per channel of the slab: combine the rows_par partials; write channel partials for dgamma / dbeta
  float* cp = chan_part + ((long)n * gridDim.x + blockIdx.x) * 2 * C;
  for (int cl = tid; cl < cpr * 8; cl += GN_THREADS) {
    float av = 0.f, bv = 0.f;
    for (int r = 0; r < rows_par; ++r) { av += pa[r * cpr * 8 + cl]; bv += pb[r * cpr * 8 + cl]; }
    const int c = ch0 * 8 + cl;
    ca[cl] = av;
    cb[cl] = bv;
    cp[c] = bv;        // dgamma partial
    cp[C + c] = av;    // dbeta partial
  }
  __syncthreads();
  float* part = gsum + (((long)n * gridDim.x + blockIdx.x) * gridDim.z + blockIdx.z) * 2 * G;
  for (int i = tid; i < 2 * G; i += GN_THREADS) {
    const int g = i >> 1;
    const float* src = (i & 1) ? cb : ca;
    const int c_lo = max(g * cpg, ch0 * 8), c_hi = min((g + 1) * cpg, (ch0 + cpr) * 8);
    float acc = 0.f;
    for (int c = c_lo; c < c_hi; ++c) {
      float gc = gamma[c];
      if constexpr (MOD) { float bc = 0.f; gn_modulate(mod, n, c, C, gc, bc); }
      acc += gc * src[c - ch0 * 8];
    }
    part[i] = acc;
  }
}

// dgamma[c] += sum_rows part[row][0][c] ; dbeta[c] += sum_rows part[row][1][c]
// block = 64 channels x 16 row groups (1024 threads); single writer per channel, so no atomics (nk_reduce_rows has the order)
__global__ __launch_bounds__(1024) void colpart_reduce_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int nrows, int C, int accumulate) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  nk_reduce_rows<16, 64, 2, 0, 4>(
      c < C, nrows,
      [&](int r, float* a) {
        a[0] += part[(long)r * 2 * C + c];
        a[1] += part[(long)r * 2 * C + C + c];
      },
      [&](const float* a) {
        dgamma[c] = accumulate ? dgamma[c] + a[0] : a[0];
        dbeta[c] = accumulate ? dbeta[c] + a[1] : a[1];
      });
}

// The modulated GroupNorm's parameter gradients from the same per-(image, split) channel partials (row r belongs to image r / nsplit):
//   dgamma[c] += sum_n (1 + s_nc) b_nc ; dbeta[c] += sum_n (1 + s_nc) a_nc.  Same block shape and summation order as colpart_reduce_kernel.
__global__ __launch_bounds__(1024) void colpart_reduce_mod_kernel(const float* __restrict__ part, const bf16_t* __restrict__ mod,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta, int nrows, int nsplit,
                                                                  int C, int accumulate) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  nk_reduce_rows<16, 64, 2, 0, 4>(
      c < C, nrows,
      [&](int r, float* a) {
        const float s1 = 1.0f + bf2f(mod[(long)(r / nsplit) * 2 * C + c]);
        a[0] += s1 * part[(long)r * 2 * C + c];
        a[1] += s1 * part[(long)r * 2 * C + C + c];
      },
      [&](const float* a) {
        dgamma[c] = accumulate ? dgamma[c] + a[0] : a[0];
        dbeta[c] = accumulate ? dbeta[c] + a[1] : a[1];
      });
}

// ... and the gradient of the modulation itself, dmod[n] = [d_scale | d_shift]: with a_nc = sum_hw dz, b_nc = sum_hw dz*xhat (the image's
// nsplit partial rows, summed in a fixed order)  d_shift = a_nc,  d_scale = gamma_c b_nc + beta_c a_nc.  grid (C / 64, N).
__global__ __launch_bounds__(1024) void gn_dmod_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, bf16_t* __restrict__ dmod, int nsplit, int C) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), n = blockIdx.y;
  nk_reduce_rows<16, 64, 2, 0, 0>(
      c < C, nsplit,
      [&](int r, float* ab) {      // ab[0] = a (the dbeta half of the row), ab[1] = b
        ab[1] += part[((long)n * nsplit + r) * 2 * C + c];
        ab[0] += part[((long)n * nsplit + r) * 2 * C + C + c];
      },
      [&](const float* ab) {
        dmod[(long)n * 2 * C + c] = f2bf(gamma[c] * ab[1] + beta[c] * ab[0]);
        dmod[(long)n * 2 * C + C + c] = f2bf(ab[0]);
      });
}

// GroupNorm backward, pass 2: dx = rstd * (dz*gamma - (s1 + xhat*s2)/cnt) (+ dx_add)
template <bool MOD>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_apply_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const bf16_t* __restrict__ mod,
                                                                  const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                  const float* __restrict__ gsum, const bf16_t* __restrict__ dx_add,
                                                                  bf16_t* __restrict__ dx, int HW, int C, int G, int silu,
                                                                  int rows_per) {
  // With z = x*A + B the pre-activation (A = rstd*gamma, B = beta - mean*A) and dz = dy * silu'(z):
  //   dx = rstd*(dz*gamma - (s1 + xhat*s2)/cnt) = A*dz + x*Cc + Dd,  Cc = -rstd^2*s2/cnt,  Dd = -rstd*s1/cnt + mean*rstd^2*s2/cnt
  // four per-channel coefficients in LDS, read as float4 pairs (the first version kept six and read them one float at a time: 48 LDS reads
  // per 16-byte chunk -- the kernel ran at 1.7 TB/s where the forward apply pass runs at 4.8)
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* p_a = (float*)smem_raw;
  float* p_b = p_a + C;
  float* p_c = p_b + C;
  float* p_d = p_c + C;
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int cpg = C / G;
  const float inv_cnt = 1.0f / ((float)HW * (float)cpg);
  for (int c = tid; c < C; c += GN_THREADS) {
    const int g = c / cpg;
    const float mu = mean[n * G + g], rs = rstd[n * G + g];
    const float s1 = gsum[(long)n * 2 * G + 2 * g] * inv_cnt, s2 = gsum[(long)n * 2 * G + 2 * g + 1] * inv_cnt;
    float ga = gamma[c], be = beta[c];
    if constexpr (MOD) gn_modulate(mod, n, c, C, ga, be);
    const float a = rs * ga;
    p_a[c] = a;
    p_b[c] = be - mu * a;
    p_c[c] = -rs * rs * s2;
    p_d[c] = -rs * s1 + mu * rs * rs * s2;
  }
  __syncthreads();
  const int cpr = C >> 3;
  const int row_lo = blockIdx.x * rows_per;
  const int row_hi = min(HW, row_lo + rows_per);
  const unsigned total = (unsigned)(row_hi - row_lo) * (unsigned)cpr;
  const long off0 = ((long)n * HW + row_lo) * C;
  auto one = [&](unsigned i, const uint4_t& rx, const uint4_t& rd, const uint4_t& ra) {
    const int c0 = (int)(i % (unsigned)cpr) * 8;
    float fx[8], fd[8], fa[8], ca[8], cb[8], cc[8], cd[8];
    unpack8(rx, fx);
    unpack8(rd, fd);
    unpack8(ra, fa);
    *(float4_t*)ca = *(const float4_t*)(p_a + c0); *(float4_t*)(ca + 4) = *(const float4_t*)(p_a + c0 + 4);
    *(float4_t*)cc = *(const float4_t*)(p_c + c0); *(float4_t*)(cc + 4) = *(const float4_t*)(p_c + c0 + 4);
    *(float4_t*)cd = *(const float4_t*)(p_d + c0); *(float4_t*)(cd + 4) = *(const float4_t*)(p_d + c0 + 4);
    if (silu) {
      *(float4_t*)cb = *(const float4_t*)(p_b + c0); *(float4_t*)(cb + 4) = *(const float4_t*)(p_b + c0 + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) fd[e] *= dsilu_f(fx[e] * ca[e] + cb[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) fx[e] = ca[e] * fd[e] + (fx[e] * cc[e] + cd[e]) + fa[e];
    *(uint4_t*)(dx + off0 + (size_t)i * 8) = pack8(fx);
  };
  const uint4_t zero4 = {0u, 0u, 0u, 0u};
  unsigned i = tid;
  for (; i + GN_THREADS < total; i += 2 * GN_THREADS) {   // two chunks (4-6 loads of 16 bytes) in flight per thread
    uint4_t vx[2], vd[2], va[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const size_t o = off0 + (size_t)(i + u * GN_THREADS) * 8;
      vx[u] = *(const uint4_t*)(x + o);
      vd[u] = *(const uint4_t*)(dy + o);
      va[u] = dx_add ? *(const uint4_t*)(dx_add + o) : zero4;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) one(i + u * GN_THREADS, vx[u], vd[u], va[u]);
  }
  for (; i < total; i += GN_THREADS) {
    const size_t o = off0 + (size_t)i * 8;
    one(i, *(const uint4_t*)(x + o), *(const uint4_t*)(dy + o), dx_add ? *(const uint4_t*)(dx_add + o) : zero4);
  }
}

// ---- GroupNorm, host side: one forward and one backward runner -- plan (norm_plan.h: nk_gn_plan has the sizes, the workspace layout and the
// launches), check the pointers, run the plan's launches in order.  The plain and the modulated entry points differ in what they pass. ----
static int gn_forward(int pass, bool modulated, const void* x, float* sums, const float* gamma, const float* beta, const void* mod, void* y, float* mean,
                      float* rstd, float* ws, int N, int HW, int C, int G, float eps, int silu, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const NkGnPlan p = nk_gn_plan(N, HW, C, G, pass, modulated);
  NORM_PLAN_OR_RETURN(p);
  NK_CHECK_ARG(x && (pass == GN_APPLY || ws) && (pass == GN_FWD || sums) && (pass == GN_SUMS || (gamma && beta && y && mean && rstd)) && (!modulated || mod));
  if (pass == GN_FWD) sums = ws + p.gsum.off;      // the one-call form keeps the sums in its workspace
  for (int i = 0; i < p.n; ++i) {
    const NkNormLaunch& L = p.launch[i];
    if (L.kernel == NK_GN_STATS) NORM_LAUNCH(L, gn_stats_kernel, (const bf16_t*)x, ws + p.part.off, HW, C, G, p.rows_per);
    else if (L.kernel == NK_GN_REDUCE) NORM_LAUNCH(L, gn_reduce_partials_kernel, ws + p.part.off, sums, p.nparts, 2 * G);
    else if (modulated) NORM_LAUNCH(L, gn_apply_kernel<true>, (const bf16_t*)x, sums, gamma, beta, (const bf16_t*)mod, (bf16_t*)y, mean, rstd, HW, C, G, eps, silu, p.rows_per);
    else NORM_LAUNCH(L, gn_apply_kernel<false>, (const bf16_t*)x, sums, gamma, beta, (const bf16_t*)nullptr, (bf16_t*)y, mean, rstd, HW, C, G, eps, silu, p.rows_per);
    if (int e = nk_check_launch(L.name)) return e;
  }
  return NK_OK;
}

static int gn_backward(bool modulated, const void* dy_, const void* x_, const float* gamma, const float* beta, const void* mod_, const float* mean, const float* rstd,
                       const void* dx_add, void* dx, float* dgamma, float* dbeta, void* dmod, float* ws, int N, int HW, int C, int G, int silu, int accumulate,
                       void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const NkGnPlan p = nk_gn_plan(N, HW, C, G, GN_BWD, modulated);
  NORM_PLAN_OR_RETURN(p);
  NK_CHECK_ARG(dy_ && x_ && gamma && beta && mean && rstd && dx && dgamma && dbeta && ws && (!modulated || (mod_ && dmod)));
  const bf16_t *dy = (const bf16_t*)dy_, *x = (const bf16_t*)x_, *mod = (const bf16_t*)mod_;
  float *part = ws + p.part.off, *gsum = ws + p.gsum.off, *chan = ws + p.chan.off;
  for (int i = 0; i < p.n; ++i) {
    const NkNormLaunch& L = p.launch[i];
    switch (L.kernel) {
      case NK_GN_BWD_STATS:
        if (modulated) NORM_LAUNCH(L, gn_bwd_stats_kernel<true>, dy, x, gamma, beta, mod, mean, rstd, part, chan, HW, C, G, silu, p.rows_per);
        else NORM_LAUNCH(L, gn_bwd_stats_kernel<false>, dy, x, gamma, beta, mod, mean, rstd, part, chan, HW, C, G, silu, p.rows_per);
        break;
      case NK_GN_REDUCE: NORM_LAUNCH(L, gn_reduce_partials_kernel, part, gsum, p.nparts, 2 * G); break;
      case NK_GN_COLPART: NORM_LAUNCH(L, colpart_reduce_kernel, chan, dgamma, dbeta, p.chan_rows, C, accumulate); break;
      case NK_GN_COLPART_MOD: NORM_LAUNCH(L, colpart_reduce_mod_kernel, chan, mod, dgamma, dbeta, p.chan_rows, p.nsplit, C, accumulate); break;
      case NK_GN_DMOD: NORM_LAUNCH(L, gn_dmod_kernel, chan, gamma, beta, (bf16_t*)dmod, p.nsplit, C); break;
      case NK_GN_BWD_APPLY:
        if (modulated) NORM_LAUNCH(L, gn_bwd_apply_kernel<true>, dy, x, gamma, beta, mod, mean, rstd, gsum, (const bf16_t*)dx_add, (bf16_t*)dx, HW, C, G, silu, p.rows_per);
        else NORM_LAUNCH(L, gn_bwd_apply_kernel<false>, dy, x, gamma, beta, mod, mean, rstd, gsum, (const bf16_t*)dx_add, (bf16_t*)dx, HW, C, G, silu, p.rows_per);
        break;
    }
    if (int e = nk_check_launch(L.name)) return e;
  }
  return NK_OK;
}

// fp32 elements of workspace nk_groupnorm_fwd / _sums / _bwd and their modulated forms need; 0 for a shape they refuse
extern "C" long nk_groupnorm_ws_floats(int N, int HW, int C, int G) { return nk_gn_plan(N, HW, C, G, GN_BWD, false).ws_floats; }

extern "C" int nk_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, float* ws, int N, int HW, int C, int G, float eps,
                                int silu, void* stream) {
  return gn_forward(GN_FWD, false, x, nullptr, gamma, beta, nullptr, y, mean, rstd, ws, N, HW, C, G, eps, silu, stream);
}
// ---- GroupNorm in separable passes: the sums, and the normalisation given the sums.  A convolution's statistics epilogue
// (conv_halo.h) produces the sums' per-tile partials itself, and its GroupNorm prologue consumes the sums: the passes below are
// what remains for tensors that come from elsewhere.  sums[n][2g] = sum, sums[n][2g+1] = sum of squares over H*W*(C/G) elements. ----
extern "C" int nk_groupnorm_sums(const void* x, float* sums, float* ws, int N, int HW, int C, int G, void* stream) {
  return gn_forward(GN_SUMS, false, x, sums, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ws, N, HW, C, G, 0.f, 0, stream);
}
extern "C" int nk_groupnorm_apply(const void* x, const float* sums, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int N, int HW, int C, int G,
                                  float eps, int silu, void* stream) {
  return gn_forward(GN_APPLY, false, x, (float*)sums, gamma, beta, nullptr, y, mean, rstd, nullptr, N, HW, C, G, eps, silu, stream);
}
extern "C" int nk_groupnorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean, const float* rstd, const void* dx_add, void* dx,
                                float* dgamma, float* dbeta, float* ws, int N, int HW, int C, int G, int silu, int accumulate, void* stream) {
  return gn_backward(false, dy, x, gamma, beta, nullptr, mean, rstd, dx_add, dx, dgamma, dbeta, nullptr, ws, N, HW, C, G, silu, accumulate, stream);
}
// ---- the modulated forms (scale-shift norm): same passes, same workspace (nk_groupnorm_ws_floats), mod = bf16 [N][2C] scale | shift ----
extern "C" int nk_groupnorm_mod_fwd(const void* x, const float* gamma, const float* beta, const void* mod, void* y, float* mean, float* rstd, float* ws, int N, int HW,
                                    int C, int G, float eps, int silu, void* stream) {
  return gn_forward(GN_FWD, true, x, nullptr, gamma, beta, mod, y, mean, rstd, ws, N, HW, C, G, eps, silu, stream);
}
extern "C" int nk_groupnorm_mod_apply(const void* x, const float* sums, const float* gamma, const float* beta, const void* mod, void* y, float* mean, float* rstd, int N,
                                      int HW, int C, int G, float eps, int silu, void* stream) {
  return gn_forward(GN_APPLY, true, x, (float*)sums, gamma, beta, mod, y, mean, rstd, nullptr, N, HW, C, G, eps, silu, stream);
}
extern "C" int nk_groupnorm_mod_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const void* mod, const float* mean, const float* rstd,
                                    const void* dx_add, void* dx, float* dgamma, float* dbeta, void* dmod, float* ws, int N, int HW, int C, int G, int silu,
                                    int accumulate, void* stream) {
  return gn_backward(true, dy, x, gamma, beta, mod, mean, rstd, dx_add, dx, dgamma, dbeta, dmod, ws, N, HW, C, G, silu, accumulate, stream);
}

// ---- sums from a producer's partial rows: one fixed-order level, or two for many rows ----
__global__ __launch_bounds__(256) void gn_reduce_partials_l1_kernel(const float* __restrict__ part, float* __restrict__ out, int nparts, int G2, int nchunks) {
  // level 1 of a two-level fixed-order sum for many partial rows: block (chunk, n) sums rows chunk, chunk + nchunks, ... of image n.
  // Its four row groups combine PAIRWISE, (a + s1) + (s2 + s3): not the ascending fold of nk_reduce_rows, so it keeps its own body.
  __shared__ float sm[4][64];
  const int n = blockIdx.y, chunk = blockIdx.x;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  float a = 0.f;
  if (tx < G2)
    for (int p = chunk + ty * nchunks; p < nparts; p += 4 * nchunks) a += part[((long)n * nparts + p) * G2 + tx];
  sm[ty][tx] = a;
  __syncthreads();
  if (ty == 0 && tx < G2) out[((long)n * nchunks + chunk) * G2 + tx] = (a + sm[1][tx]) + (sm[2][tx] + sm[3][tx]);
}

extern "C" long nk_groupnorm_sums_ws_floats(int N, int nparts, int G) { return nk_gn_sums_plan(N, nparts, G).ws_floats; }
extern "C" int nk_groupnorm_sums_from_parts(const float* part, float* sums, float* ws, int N, int nparts, int G, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const NkGnSumsPlan p = nk_gn_sums_plan(N, nparts, G);
  NORM_PLAN_OR_RETURN(p);
  NK_CHECK_ARG(part && sums && (p.levels == 1 || ws));
  for (int i = 0; i < p.n; ++i) {
    const NkNormLaunch& L = p.launch[i];
    if (L.kernel == NK_GN_REDUCE_L1) {
      NORM_LAUNCH(L, gn_reduce_partials_l1_kernel, part, ws + p.l1.off, nparts, 2 * G, p.nchunks);
      part = ws + p.l1.off;
      nparts = p.nchunks;
    } else {
      NORM_LAUNCH(L, gn_reduce_partials_kernel, part, sums, nparts, 2 * G);
    }
    if (int e = nk_check_launch(L.name)) return e;
  }
  return NK_OK;
}

// ------------------------------------------------------------------------------------------------
// LayerNorm over the last dim of [M][C]; one wavefront per row, rows strided over the grid.
// ------------------------------------------------------------------------------------------------
// NCH = 16-byte chunks per lane actually needed (2: C <= 1024, 3: <= 1536, 4: <= 2048): the per-lane arrays are sized by
// it, which is what decides the register count and with it how many rows a CU keeps in flight.
template <int NCH>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int M, int C,
                                                     float eps) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int cpr = C >> 3;
  const float invC = 1.0f / (float)C;
  for (int row = wave; row < M; row += nwaves) {
    float f[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int ch = lane + 64 * j;
      if (ch < cpr) {
        unpack8(*(const uint4_t*)(x + (long)row * C + ch * 8), f[j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f[j][e];
      }
    }
    const float mu = wave_sum(s) * invC;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int ch = lane + 64 * j;
      if (ch < cpr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { float d = f[j][e] - mu; v += d * d; }
      }
    }
    const float rs = rsqrtf(wave_sum(v) * invC + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int ch = lane + 64 * j;
      if (ch < cpr) {
        const float4_t g0 = *(const float4_t*)(gamma + ch * 8), g1 = *(const float4_t*)(gamma + ch * 8 + 4);
        const float4_t b0 = *(const float4_t*)(beta + ch * 8), b1 = *(const float4_t*)(beta + ch * 8 + 4);
        float o[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = (f[j][e] - mu) * rs * g0[e] + b0[e];
          o[4 + e] = (f[j][4 + e] - mu) * rs * g1[e] + b1[e];
        }
        *(uint4_t*)(y + (long)row * C + ch * 8) = pack8(o);
      }
    }
  }
}

// LayerNorm backward, input gradient:
// dx = rstd * (dy*gamma - mean_c(dy*gamma) - xhat * mean_c(dy*gamma*xhat)) (+ dx_add).  One wavefront per row; x and dy stay
// in registers as packed bf16 between the statistics pass and the output pass.
template <int NCH>
__global__ __launch_bounds__(256, 4) void ln_bwd_dx_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                        const float* __restrict__ gamma, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const bf16_t* __restrict__ dx_add,
                                                        bf16_t* __restrict__ dx, int M, int C) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int cpr = C >> 3;
  const float invC = 1.0f / (float)C;
  float gm[NCH][8];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int ch = lane + 64 * j;
#pragma unroll
    for (int e = 0; e < 8; ++e) gm[j][e] = 0.f;
    if (ch < cpr) {
      const float4_t g0 = *(const float4_t*)(gamma + ch * 8), g1 = *(const float4_t*)(gamma + ch * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { gm[j][e] = g0[e]; gm[j][4 + e] = g1[e]; }
    }
  }
  for (int row = wave; row < M; row += nwaves) {
    const float mu = mean[row], rs = rstd[row];
    uint4_t rx[NCH], rd[NCH], ra[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int ch = lane + 64 * j;
      rx[j] = rd[j] = ra[j] = (uint4_t){0u, 0u, 0u, 0u};
      if (ch < cpr) {
        rx[j] = *(const uint4_t*)(x + (long)row * C + ch * 8);
        rd[j] = *(const uint4_t*)(dy + (long)row * C + ch * 8);
        if (dx_add) ra[j] = *(const uint4_t*)(dx_add + (long)row * C + ch * 8);
      }
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float fx[8], fd[8];
      unpack8(rx[j], fx);
      unpack8(rd[j], fd);
#pragma unroll
      for (int e = 0; e < 8; ++e) {   // lanes past the row hold zeros (dy = 0), so they add nothing
        float d = fd[e] * gm[j][e];
        s1 += d;
        s2 += d * ((fx[e] - mu) * rs);
      }
    }
    s1 = wave_sum(s1) * invC;
    s2 = wave_sum(s2) * invC;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int ch = lane + 64 * j;
      if (ch < cpr) {
        float fx[8], fd[8], o[8];
        unpack8(rx[j], fx);
        unpack8(rd[j], fd);
        unpack8(ra[j], o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += rs * (fd[e] * gm[j][e] - s1 - (fx[e] - mu) * rs * s2);
        *(uint4_t*)(dx + (long)row * C + ch * 8) = pack8(o);
      }
    }
  }
}

// LayerNorm backward, parameter gradients: part[split][0][c] = sum_rows dy*xhat, part[split][1][c] = sum_rows dy over the
// split's 64 rows.  Block = 16 row lanes x 16 chunk lanes (256 contiguous bytes per row lane, four rows in flight per
// thread); splits are combined by colpart_reduce_kernel (single writer per channel, deterministic).
__global__ __launch_bounds__(256) void ln_bwd_param_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           float* __restrict__ part, int M, int C) {
  __shared__ float pg[16][16 * 8 + 4], pb[16][16 * 8 + 4];
  const int tid = threadIdx.x;
  const int cx = tid & 15, ry = tid >> 4;
  const int chunk = blockIdx.y * 16 + cx;
  const bool cok = chunk < (C >> 3);
  const int row_lo = blockIdx.x * LNP_ROWS;
  float sg[8], sb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sg[e] = 0.f; sb[e] = 0.f; }
  if (cok) {
    uint4_t vx[4], vd[4];
    float mu[4], rs[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = row_lo + ry + 16 * i;
      const bool ok = r < M;
      vx[i] = ok ? *(const uint4_t*)(x + (long)r * C + chunk * 8) : (uint4_t){0u, 0u, 0u, 0u};
      vd[i] = ok ? *(const uint4_t*)(dy + (long)r * C + chunk * 8) : (uint4_t){0u, 0u, 0u, 0u};
      mu[i] = ok ? mean[r] : 0.f;
      rs[i] = ok ? rstd[r] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float fx[8], fd[8];
      unpack8(vx[i], fx);
      unpack8(vd[i], fd);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sb[e] += fd[e];
        sg[e] += fd[e] * ((fx[e] - mu[i]) * rs[i]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { pg[ry][cx * 8 + e] = sg[e]; pb[ry][cx * 8 + e] = sb[e]; }
  __syncthreads();
  if (tid < 128) {
    const int c = blockIdx.y * 128 + tid;
    if (c < C) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { a += pg[r][tid]; b += pb[r][tid]; }
      float* out = part + (long)blockIdx.x * 2 * C;
      out[c] = a;
      out[C + c] = b;
    }
  }
}

// LayerNorm backward in ONE pass over x and dy (round 5; replaces the round-2 one-row-per-wave fused kernel, whose per-wave LDS fold cost
// more than the row it had processed).  A wave walks SEVERAL rows (row = wave, wave + nwaves, ...: 4 at M = 4096, 8 at M = 16384), the next
// row's x / dy / residual-gradient loads are issued before the current row's reductions (two rows in flight per wave: these 10-40 MB
// tensors are latency-bound), dx is produced as in ln_bwd_dx_kernel, and -- from the same registers -- the wave keeps column partials of
// dgamma (sum dy * xhat) and dbeta (sum dy) over ITS rows.  At the end the block's four waves fold through two LDS slots in a fixed order
// ((w0 + w2) + (w1 + w3): bit-reproducible) into ONE partial row per block: <= 512 rows, 1.3-2.6 MB, against the 21 MB the separate
// parameter kernel re-read.  colpart_reduce_kernel / colpart_reduce_batch_kernel sum the partial rows (single writer per channel).
// Algorithmic traffic 6 B/elem (+2 with dx_add); the three-kernel form moved 10 (+2) and took three launches.
template <int NCH>
__global__ __launch_bounds__(LNR_WAVES * 64) void ln_bwd_rows_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                       const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                       const float* __restrict__ rstd, const bf16_t* __restrict__ dx_add,
                                                                       bf16_t* __restrict__ dx, float* __restrict__ part, int M, int C) {
  extern __shared__ __attribute__((aligned(16))) char ln_smem[];
  float* red = (float*)ln_smem;                     // [2 slots][2][C]: 20 KB at C = 1280
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wave = blockIdx.x * LNR_WAVES + wv;
  const int nwaves = gridDim.x * LNR_WAVES;
  const int cpr = C >> 3;
  const float invC = 1.0f / (float)C;
  float gm[NCH][8], sg[NCH][8], sb[NCH][8];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    int ch = lane + 64 * j;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gm[j][e] = 0.f; sg[j][e] = 0.f; sb[j][e] = 0.f; }
    if (ch < cpr) {
      const float4_t g0 = *(const float4_t*)(gamma + ch * 8), g1 = *(const float4_t*)(gamma + ch * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { gm[j][e] = g0[e]; gm[j][4 + e] = g1[e]; }
    }
  }
  uint4_t rx[NCH], rd[NCH], ra[NCH];
  float mu = 0.f, rs = 0.f;
  auto fetch = [&](int row, uint4_t (&fx)[NCH], uint4_t (&fd)[NCH], uint4_t (&fa)[NCH], float& fmu, float& frs) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int ch = lane + 64 * j;
      fx[j] = fd[j] = fa[j] = (uint4_t){0u, 0u, 0u, 0u};
      if (row < M && ch < cpr) {
        fx[j] = *(const uint4_t*)(x + (long)row * C + ch * 8);
        fd[j] = *(const uint4_t*)(dy + (long)row * C + ch * 8);
        if (dx_add) fa[j] = *(const uint4_t*)(dx_add + (long)row * C + ch * 8);
      }
    }
    fmu = row < M ? mean[row] : 0.f;
    frs = row < M ? rstd[row] : 0.f;
  };
  constexpr bool AHEAD = NCH < 4;      // (C > 1536 -- no SDXL / SD1.5 LayerNorm -- would spill with two rows in registers: one row at a time)
  if (AHEAD) fetch(wave, rx, rd, ra, mu, rs);
  for (int row = wave; row < M; row += nwaves) {
    uint4_t nx[NCH], nd[NCH], na[NCH];
    float nmu = 0.f, nrs = 0.f;
    if (AHEAD) fetch(row + nwaves, nx, nd, na, nmu, nrs);        // the next row's loads are in flight under this row's arithmetic
    else fetch(row, rx, rd, ra, mu, rs);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      float fx[8], fd[8];
      unpack8(rx[j], fx);
      unpack8(rd[j], fd);
#pragma unroll
      for (int e = 0; e < 8; ++e) {   // lanes past the row hold zeros (dy = 0), so they add nothing
        const float xh = (fx[e] - mu) * rs;
        const float d = fd[e] * gm[j][e];
        s1 += d;
        s2 += d * xh;
        sb[j][e] += fd[e];
        sg[j][e] += fd[e] * xh;
      }
    }
    s1 = wave_sum(s1) * invC;
    s2 = wave_sum(s2) * invC;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      int ch = lane + 64 * j;
      if (ch < cpr) {
        float fx[8], fd[8], o[8];
        unpack8(rx[j], fx);
        unpack8(rd[j], fd);
        unpack8(ra[j], o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += rs * (fd[e] * gm[j][e] - s1 - (fx[e] - mu) * rs * s2);
        *(uint4_t*)(dx + (long)row * C + ch * 8) = pack8(o);
      }
    }
    if (AHEAD) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) { rx[j] = nx[j]; rd[j] = nd[j]; ra[j] = na[j]; }
      mu = nmu;
      rs = nrs;
    }
  }
  // this wave's column partials -> LDS -> one row per block.  Waves 0, 1 write slots 0, 1; waves 2, 3 add into them; then slot 0 + slot 1.
#pragma unroll
  for (int round = 0; round < LNR_WAVES / 2; ++round) {
    if ((wv >> 1) == round) {
      float* gbase = red + ((long)(wv & 1) * 2) * C;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        int ch = lane + 64 * j;
        if (ch < cpr) {
          float* g = gbase + ch * 8;
          float4_t g0 = {sg[j][0], sg[j][1], sg[j][2], sg[j][3]}, g1 = {sg[j][4], sg[j][5], sg[j][6], sg[j][7]};
          float4_t b0 = {sb[j][0], sb[j][1], sb[j][2], sb[j][3]}, b1 = {sb[j][4], sb[j][5], sb[j][6], sb[j][7]};
          if (round) { g0 += *(const float4_t*)g; g1 += *(const float4_t*)(g + 4); b0 += *(const float4_t*)(g + C); b1 += *(const float4_t*)(g + C + 4); }
          *(float4_t*)g = g0;
          *(float4_t*)(g + 4) = g1;
          *(float4_t*)(g + C) = b0;
          *(float4_t*)(g + C + 4) = b1;
        }
      }
    }
    __syncthreads();
  }
  float* out = part + (long)blockIdx.x * 2 * C;
  for (int c = threadIdx.x; c < 2 * C; c += LNR_WAVES * 64) out[c] = red[c] + red[2 * C + c];
}
// Several column-partial reductions in ONE launch (blockIdx.y = entry): the three LayerNorms of a transformer block hand their partial
// rows to the weight-gradient queue, which reduces them behind the block's batched weight gradients (ops.WgradQueue).
__global__ __launch_bounds__(1024) void colpart_reduce_batch_kernel(const NkColpartBatch b) {
  // block = 32 channels x 32 row groups: 120 workgroups for three 1280-wide LayerNorms, eight rows per thread at 256 partial rows, all of them
  // in flight at once (the 64 x 16 layout of colpart_reduce_kernel measured 10.4 us per launch in the step: 60 workgroups, 16 dependent rounds)
  const int z = blockIdx.y;
  const int C = b.C[z];
  if ((int)blockIdx.x * 32 >= C) return;
  const float* __restrict__ part = b.part[z];
  const int c = blockIdx.x * 32 + (threadIdx.x & 31);
  nk_reduce_rows<32, 32, 2, 1, 8>(
      c < C, b.nrows[z],
      [&](int r, float* a) {
        a[0] += part[(long)r * 2 * C + c];
        a[1] += part[(long)r * 2 * C + C + c];
      },
      [&](const float* a) {
        float* dgamma = b.dgamma[z];
        float* dbeta = b.dbeta[z];
        dgamma[c] = b.accumulate[z] ? dgamma[c] + a[0] : a[0];
        dbeta[c] = b.accumulate[z] ? dbeta[c] + a[1] : a[1];
      });
}

// ------------------------------------------------------------------------------------------------
// RMSNorm (T5LayerNorm: no mean subtraction, no bias) over the last dim of [M][C], forward only: y = x * rsqrt(mean(x^2) + eps) * gamma.
// One wavefront per row as in ln_fwd_kernel.  The sum of squares is a per-lane sum over the lane's chunks in chunk order, then the xor
// butterfly: a fixed order that depends on C alone, so a row's bits do not depend on M or on which wave got the row.
// ------------------------------------------------------------------------------------------------
// STAT (nk_rmsnorm_fwd_rstd: the T5 encoders under training) also keeps the row's rstd for the backward; y has the same bits.
template <int NCH, bool STAT = false>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma, bf16_t* __restrict__ y, int M, int C,
                                                      float eps, float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int cpr = C >> 3;
  const float invC = 1.0f / (float)C;
  for (int row = wave; row < M; row += nwaves) {
    uint4_t raw[NCH];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int ch = lane + 64 * j;
      if (ch < cpr) {
        float f[8];
        raw[j] = *(const uint4_t*)(x + (long)row * C + ch * 8);
        unpack8(raw[j], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(f[e], f[e], s);
      }
    }
    const float rs = rsqrtf(wave_sum(s) * invC + eps);
    if constexpr (STAT) {
      if (lane == 0) rstd[row] = rs;
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int ch = lane + 64 * j;
      if (ch < cpr) {
        const float4_t g0 = *(const float4_t*)(gamma + ch * 8), g1 = *(const float4_t*)(gamma + ch * 8 + 4);
        float f[8], o[8];
        unpack8(raw[j], f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = f[e] * rs * g0[e];
          o[4 + e] = f[4 + e] * rs * g1[e];
        }
        *(uint4_t*)(y + (long)row * C + ch * 8) = pack8(o);
      }
    }
  }
}

// RMSNorm backward: dx = rstd (g o dy - xhat mean_c(g o dy o xhat)) (+ dx_add), xhat = x rstd, in fp32 with ONE rounding to bf16 at the store
// (dx_add is added in fp32 before it), and dgamma[c] = sum_m dy xhat.  One wavefront per row; wave w of `nw` walks rows w, w + nw, ... and
// keeps its column sums of dy xhat in registers (rows ascending), then writes them as partial row w: rms_colpart_reduce_kernel sums the rows
// in a fixed order.  The row mean is a per-lane sum in chunk order then the xor butterfly, as in the forward: a row's dx does not depend on M.
template <int NCH>
__global__ __launch_bounds__(256) void rms_bwd_rows_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ rstd, const bf16_t* __restrict__ dx_add, bf16_t* __restrict__ dx,
                                                           float* __restrict__ part, int M, int C, int nw) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave >= nw) return;
  const int cpr = C >> 3;
  const float invC = 1.0f / (float)C;
  float gm[NCH][8], sg[NCH][8];
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int ch = lane + 64 * j;
#pragma unroll
    for (int e = 0; e < 8; ++e) { gm[j][e] = 0.f; sg[j][e] = 0.f; }
    if (ch < cpr) {
      const float4_t g0 = *(const float4_t*)(gamma + ch * 8), g1 = *(const float4_t*)(gamma + ch * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { gm[j][e] = g0[e]; gm[j][4 + e] = g1[e]; }
    }
  }
  for (int row = wave; row < M; row += nw) {
    uint4_t rx[NCH], rd[NCH];
    const float rs = rstd[row];
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int ch = lane + 64 * j;
      rx[j] = rd[j] = (uint4_t){0u, 0u, 0u, 0u};
      if (ch < cpr) {
        rx[j] = *(const uint4_t*)(x + (long)row * C + ch * 8);
        rd[j] = *(const uint4_t*)(dy + (long)row * C + ch * 8);
      }
      float fx[8], fd[8];
      unpack8(rx[j], fx);
      unpack8(rd[j], fd);
#pragma unroll
      for (int e = 0; e < 8; ++e) {      // lanes past the row hold zeros, so they add nothing
        const float xh = fx[e] * rs;
        s2 += fd[e] * gm[j][e] * xh;
        sg[j][e] += fd[e] * xh;
      }
    }
    s2 = wave_sum(s2) * invC;
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const int ch = lane + 64 * j;
      if (ch < cpr) {
        float fx[8], fd[8], o[8];
        unpack8(rx[j], fx);
        unpack8(rd[j], fd);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
        if (dx_add) unpack8(*(const uint4_t*)(dx_add + (long)row * C + ch * 8), o);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += rs * (fd[e] * gm[j][e] - fx[e] * rs * s2);
        *(uint4_t*)(dx + (long)row * C + ch * 8) = pack8(o);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NCH; ++j) {
    const int ch = lane + 64 * j;
    if (ch < cpr) {
      float* out = part + (long)wave * C + ch * 8;
      *(float4_t*)out = (float4_t){sg[j][0], sg[j][1], sg[j][2], sg[j][3]};
      *(float4_t*)(out + 4) = (float4_t){sg[j][4], sg[j][5], sg[j][6], sg[j][7]};
    }
  }
}
// dgamma[c] (+)= sum_rows part[row][c]: colpart_reduce_kernel's block shape and order (nk_reduce_rows) for one value per column
__global__ __launch_bounds__(1024) void rms_colpart_reduce_kernel(const float* __restrict__ part, float* __restrict__ dgamma, int nrows, int C, int accumulate) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  nk_reduce_rows<16, 64, 1, 0, 4>(
      c < C, nrows, [&](int r, float* a) { a[0] += part[(long)r * C + c]; },
      [&](const float* a) { dgamma[c] = accumulate ? dgamma[c] + a[0] : a[0]; });
}

// ---- LayerNorm / RMSNorm / column partials, host side: one runner -- plan (norm_plan.h: nk_rownorm_plan), check the pointers the kind needs,
// run the plan's launches in order.  nch_dispatch: f(integral_constant<NCH>) for the chunks-per-lane instance the plan chose. ----
template <int... NCH, class F>
static void nch_dispatch(int nch, F f) {
  ((nch == NCH ? f(std::integral_constant<int, NCH>{}) : void()), ...);
}

struct RowNormArgs {
  const void *dy, *x, *dx_add;
  const float *gamma, *beta, *mean, *rstd;      // mean / rstd: written by the forward, read by the backward
  void* out;                                    // y or dx
  float *dgamma, *dbeta, *part;
};
// ptrs: the entry point's own "every pointer it needs is there" (evaluated by the caller, examined only behind plan-only mode)
static int rownorm_run(int kind, bool ptrs, const RowNormArgs& a, int M, int C, float eps, int accumulate, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const NkRowNormPlan p = nk_rownorm_plan(M, C, kind);
  NORM_PLAN_OR_RETURN(p);
  NK_CHECK_ARG(ptrs && "a required pointer argument is null");
  if (kind == RMS_FWD || kind == RMS_FWD_RSTD || kind == RMS_BWD)
    NK_CHECK_ARG(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.out & 15) == 0 && ((uintptr_t)a.gamma & 15) == 0 && ((uintptr_t)a.dy & 15) == 0 &&
                 ((uintptr_t)a.dx_add & 15) == 0 && ((uintptr_t)a.part & 15) == 0);     // 16-byte accesses
  const bf16_t *dy = (const bf16_t*)a.dy, *x = (const bf16_t*)a.x, *dx_add = (const bf16_t*)a.dx_add;
  bf16_t* out = (bf16_t*)a.out;
  float* part = a.part + p.part.off;
  for (int i = 0; i < p.n; ++i) {
    const NkNormLaunch& L = p.launch[i];
    switch (L.kernel) {
      case NK_LN_FWD:
        nch_dispatch<2, 3, 4>(p.nch, [&](auto n) { NORM_LAUNCH(L, ln_fwd_kernel<decltype(n)::value>, x, a.gamma, a.beta, out, (float*)a.mean, (float*)a.rstd, M, C, eps); });
        break;
      case NK_RMS_FWD:
        if (kind == RMS_FWD_RSTD) nch_dispatch<2, 4, 8>(p.nch, [&](auto n) {
          auto kern = rms_fwd_kernel<decltype(n)::value, true>;
          NORM_LAUNCH(L, kern, x, a.gamma, out, M, C, eps, (float*)a.rstd);
        });
        else nch_dispatch<2, 4, 8>(p.nch, [&](auto n) { NORM_LAUNCH(L, rms_fwd_kernel<decltype(n)::value>, x, a.gamma, out, M, C, eps, (float*)nullptr); });
        break;
      case NK_RMS_BWD_ROWS:
        nch_dispatch<2, 4, 8>(p.nch, [&](auto n) { NORM_LAUNCH(L, rms_bwd_rows_kernel<decltype(n)::value>, dy, x, a.gamma, a.rstd, dx_add, out, part, M, C, p.nrows); });
        break;
      case NK_RMS_COLPART: NORM_LAUNCH(L, rms_colpart_reduce_kernel, part, a.dgamma, p.nrows, C, accumulate); break;
      case NK_LN_BWD_DX:
        // input gradient: one wavefront per row.  (Fewer, longer-lived workgroups -- a grid capped at 256 / 512 / 1024 blocks with the rows
        // strided over them -- make no difference beside the weight-gradient stream: 180.4 / 180.3 / 180.2 vs 180.1 ms per step.)
        nch_dispatch<2, 3, 4>(p.nch, [&](auto n) { NORM_LAUNCH(L, ln_bwd_dx_kernel<decltype(n)::value>, dy, x, a.gamma, a.mean, a.rstd, dx_add, out, M, C); });
        break;
      case NK_LN_BWD_PARAM: NORM_LAUNCH(L, ln_bwd_param_kernel, dy, x, a.mean, a.rstd, part, M, C); break;      // column partials over row splits
      case NK_LN_BWD_ROWS:
        nch_dispatch<2, 3, 4>(p.nch, [&](auto n) {
          nk_optin_lds((const void*)ln_bwd_rows_kernel<decltype(n)::value>, LNR_MAX_SMEM);
          NORM_LAUNCH(L, ln_bwd_rows_kernel<decltype(n)::value>, dy, x, a.gamma, a.mean, a.rstd, dx_add, out, part, M, C);
        });
        break;
      case NK_LN_COLPART: NORM_LAUNCH(L, colpart_reduce_kernel, part, a.dgamma, a.dbeta, p.nrows, C, accumulate); break;      // the single-writer reduce
    }
    if (int e = nk_check_launch(L.name)) return e;
  }
  return NK_OK;
}

// the size for every C that any entry point using it accepts: nk_layernorm_bwd_params takes widths beyond LN_MAXCH
extern "C" long nk_layernorm_ws_floats(int M, int C) { return nk_rownorm_plan(M, C, LN_BWD_PARAMS).ws_floats; }
extern "C" long nk_layernorm_part_rows(int M) { return nk_rownorm_plan(M, 8, LN_BWD_ROWS).part_rows; }

extern "C" int nk_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int M, int C, float eps, void* stream) {
  return rownorm_run(LN_FWD, x && gamma && beta && y && mean && rstd, {nullptr, x, nullptr, gamma, beta, mean, rstd, y}, M, C, eps, 0, stream);
}
extern "C" int nk_rmsnorm_fwd(const void* x, const float* gamma, void* y, int M, int C, float eps, void* stream) {
  return rownorm_run(RMS_FWD, x && gamma && y, {nullptr, x, nullptr, gamma, nullptr, nullptr, nullptr, y}, M, C, eps, 0, stream);
}
// ... keeping rstd [M] for nk_rmsnorm_bwd (y: nk_rmsnorm_fwd's bits)
extern "C" int nk_rmsnorm_fwd_rstd(const void* x, const float* gamma, void* y, float* rstd, int M, int C, float eps, void* stream) {
  return rownorm_run(RMS_FWD_RSTD, x && gamma && y && rstd, {nullptr, x, nullptr, gamma, nullptr, nullptr, rstd, y}, M, C, eps, 0, stream);
}
extern "C" long nk_rmsnorm_bwd_ws_floats(int M, int C) { return nk_rownorm_plan(M, C, RMS_BWD).ws_floats; }
extern "C" int nk_rmsnorm_bwd(const void* dy, const void* x, const float* gamma, const float* rstd, const void* dx_add, void* dx, float* dgamma, float* ws, int M,
                              int C, int accumulate, void* stream) {
  return rownorm_run(RMS_BWD, dy && x && gamma && rstd && dx && dgamma && ws, {dy, x, dx_add, gamma, nullptr, nullptr, rstd, dx, dgamma, nullptr, ws}, M, C, 0.f,
                     accumulate, stream);
}
/* The backward in two parts, so the caller can run the parameter gradients (off the critical path) on another stream ... */
extern "C" int nk_layernorm_bwd_dx(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dx_add, void* dx, int M, int C,
                                   void* stream) {
  return rownorm_run(LN_BWD_DX, dy && x && gamma && mean && rstd && dx, {dy, x, dx_add, gamma, nullptr, mean, rstd, dx}, M, C, 0.f, 0, stream);
}
extern "C" int nk_layernorm_bwd_params(const void* dy, const void* x, const float* mean, const float* rstd, float* dgamma, float* dbeta, float* ws, int M, int C,
                                       int accumulate, void* stream) {
  return rownorm_run(LN_BWD_PARAMS, dy && x && mean && rstd && dgamma && dbeta && ws, {dy, x, nullptr, nullptr, nullptr, mean, rstd, nullptr, dgamma, dbeta, ws}, M, C, 0.f, accumulate, stream);
}
/* ... dx and nk_layernorm_part_rows(M) partial rows [rows][2][C] (dgamma partials, dbeta partials) in one pass; the caller reduces the rows with
 * nk_colpart_reduce_batch (any stream, any later time: `part` is the only state) ... */
extern "C" int nk_layernorm_bwd_rows(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dx_add, void* dx, float* part,
                                     int M, int C, void* stream) {
  return rownorm_run(LN_BWD_ROWS, dy && x && gamma && mean && rstd && dx && part, {dy, x, dx_add, gamma, nullptr, mean, rstd, dx, nullptr, nullptr, part}, M, C, 0.f, 0, stream);
}
/* ... or one pass over x and dy for the input gradient AND the per-block parameter partials, then the single-writer column reduce */
extern "C" int nk_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dx_add, void* dx, float* dgamma,
                                float* dbeta, float* ws, int M, int C, int accumulate, void* stream) {
  return rownorm_run(LN_BWD, dy && x && gamma && mean && rstd && dx && dgamma && dbeta && ws, {dy, x, dx_add, gamma, nullptr, mean, rstd, dx, dgamma, dbeta, ws}, M, C, 0.f, accumulate, stream);
}

extern "C" int nk_colpart_reduce_batch(const NkColpartBatch* b, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  NK_CHECK_ARG(b != nullptr);
  const NkNormPlan p = nk_colpart_batch_plan(b->C, b->n);
  NORM_PLAN_OR_RETURN(p);
  for (int z = 0; z < b->n; ++z) NK_CHECK_ARG(b->part[z] && b->dgamma[z] && b->dbeta[z] && b->nrows[z] > 0);
  NORM_LAUNCH(p.launch[0], colpart_reduce_batch_kernel, *b);
  return nk_check_launch(p.launch[0].name);
}
