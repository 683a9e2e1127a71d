// The parts of a frozen DreamSim ViT tower that are not a transformer layer (neurosis_amd/modules/losses/dreamsim): the patch gather in front of
// the patch-embedding GEMM and its adjoint, the token assembly (cls token, position table) and its adjoint, and the embedding head
// d = 1 - cos(z0, z1), z = f / |f| - mean(f / |f|), with its gradient w.r.t. the second image's features.  The layers themselves run on the
// kernels the CLIP text towers use.  Nothing here uses an atomic: every output element has one writer and every sum a fixed order.
#include "../../include/neurosis_hip.h"
#include "nk_ew.h"
#include "nk_reduce.h"

// ---- patchify -------------------------------------------------------------------------------------------------------------------------------
// x fp32 NCHW [N, 3, H, W] -> rows bf16 [N * Hp * Wp, 3 p p], row = (n, py, px), column = (c, ky, kx): nn.Conv2d's weight order, so the
// patch embedding is rows @ proj.weight.view(E, 3 p p)^T.  The load applies  a_c * clamp(x, lo, hi) + b_c  (Normalize(mean, std), and under
// rescale_input the x / 2 + 0.5 with its clamp to [0, 1], which is a clamp of x to [-1, 1]); product and sum are rounded separately, so
// the value is the one two fp32 torch ops give.  A work item is 8 consecutive kx of one patch row (p % 8 == 0).
struct VitAffine {
  float a[3], b[3], lo, hi;
};
struct VitGeom {
  int Hp, Wp, p, H, W, cpp;      // cpp = chunks per patch row = p / 8
  __device__ __forceinline__ long pixel(long row, int ch, int& c) const {
    const int per_c = p * cpp;                 // chunks per channel of one patch
    c = ch / per_c;
    const int r = ch - c * per_c, ky = r / cpp, kx = (r - ky * cpp) * 8;
    const long n = row / ((long)Hp * Wp);
    const int t = (int)(row - n * Hp * Wp), py = t / Wp, px = t - py * Wp;
    return ((n * 3 + c) * H + (long)py * p + ky) * W + (long)px * p + kx;
  }
};
struct VitPatchify {
  const float* x; bf16_t* out; VitAffine af; VitGeom g;
  __device__ __forceinline__ void operator()(long i, long row, int ch) const {
#pragma clang fp contract(off)      // a * v + b as a product and a sum, each rounded: not one fused multiply-add
    int c;
    const float* src = x + g.pixel(row, ch, c);
    const float4_t v0 = *(const float4_t*)src, v1 = *(const float4_t*)(src + 4);
    const float in[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = af.a[c] * fminf(fmaxf(in[k], af.lo), af.hi) + af.b[c];
    ew_store(out + i * 8, f);
  }
};
// the adjoint: dx[pixel] (+)= a_c * dy[row][col] where lo <= x <= hi, 0 where the forward clamped.  Patches do not overlap: each pixel is
// written once, by the item that read it in the forward.
template <int ACC>
struct VitPatchifyBwd {
  const bf16_t* dy; const float* x; float* dx; VitAffine af; VitGeom g;
  __device__ __forceinline__ void operator()(long i, long row, int ch) const {
    int c;
    const long at = g.pixel(row, ch, c);
    float d[8];
    ew_load(dy + i * 8, d);
    const float4_t x0 = *(const float4_t*)(x + at), x1 = *(const float4_t*)(x + at + 4);
    const float in[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
    float4_t o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0;
    if (ACC) { o0 = *(const float4_t*)(dx + at); o1 = *(const float4_t*)(dx + at + 4); }
    float o[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] += (in[k] >= af.lo && in[k] <= af.hi) ? af.a[c] * d[k] : 0.f;
    *(float4_t*)(dx + at) = float4_t{o[0], o[1], o[2], o[3]};
    *(float4_t*)(dx + at + 4) = float4_t{o[4], o[5], o[6], o[7]};
  }
};

static int vit_geom(VitGeom& g, int N, int H, int W, int p) {
  if (!(N > 0 && H > 0 && W > 0 && p > 0 && p % 8 == 0 && H % p == 0 && W % p == 0)) return 0;
  g.Hp = H / p; g.Wp = W / p; g.p = p; g.H = H; g.W = W; g.cpp = p / 8;
  return 1;
}
static VitAffine vit_affine(const float* affine) {
  VitAffine af;
  for (int c = 0; c < 3; ++c) { af.a[c] = affine[c]; af.b[c] = affine[3 + c]; }
  af.lo = affine[6]; af.hi = affine[7];
  return af;
}

extern "C" int nk_vit_patchify(const float* x, void* rows, const float* affine, int N, int H, int W, int p, void* stream) {
  VitGeom g;
  NK_CHECK_ARG(x && rows && affine && vit_geom(g, N, H, W, p));
  NK_CHECK_ARG(nk_aligned16(x) && nk_aligned16(rows));
  return nk_ew_rows("vit_patchify", stream, (long)N * g.Hp * g.Wp, 3 * p * g.cpp, VitPatchify{x, (bf16_t*)rows, vit_affine(affine), g});
}
extern "C" int nk_vit_patchify_bwd(const void* drows, const float* x, float* dx, const float* affine, int N, int H, int W, int p, int accumulate,
                                   void* stream) {
  VitGeom g;
  NK_CHECK_ARG(drows && x && dx && affine && vit_geom(g, N, H, W, p) && (accumulate == 0 || accumulate == 1));
  NK_CHECK_ARG(nk_aligned16(x) && nk_aligned16(drows) && nk_aligned16(dx));
  const long rows = (long)N * g.Hp * g.Wp;
  const int cpr = 3 * p * g.cpp;
  const VitAffine af = vit_affine(affine);
  return nk_ew_mode<0, 1>(accumulate, [&](auto m) {
    return nk_ew_rows("vit_patchify_bwd", stream, rows, cpr, VitPatchifyBwd<decltype(m)::value>{(const bf16_t*)drows, x, dx, af, g});
  });
}

// ---- token assembly -------------------------------------------------------------------------------------------------------------------------
// tokens [N (Np + 1), E] fp32 (the towers' residual stream is fp32, below): row 0 of a sample = cls + pos[0], row 1 + i = patch row i (the GEMM's output, bias included) + pos[1 + i];
// cls [E] and pos [Np + 1, E] fp32, the sum in fp32.  The adjoint (bf16 gradients) w.r.t. the patch rows drops the cls rows.
struct VitTokens {
  const bf16_t* patches; const float* cls; const float* pos; float* out; int L, E;      // L = Np + 1
  __device__ __forceinline__ void operator()(long i, long row, int ch) const {
    const long n = row / L;
    const int t = (int)(row - n * L);
    const float* ps = pos + (long)t * E + ch * 8;
    float f[8];
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = cls[ch * 8 + k];
    } else {
      ew_load(patches + ((n * (L - 1) + t - 1) * E + ch * 8), f);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] += ps[k];
    *(float4_t*)(out + i * 8) = float4_t{f[0], f[1], f[2], f[3]};
    *(float4_t*)(out + i * 8 + 4) = float4_t{f[4], f[5], f[6], f[7]};
  }
};
// the adjoint is a strided copy: patch row n * Np + j <- token row n * (Np + 1) + 1 + j; rows of cpr 16-byte chunks
struct VitDropCls {
  const uint4_t* dtok; uint4_t* dpatch; int Np, cpr;
  __device__ __forceinline__ void operator()(long i, long row, int ch) const { dpatch[i] = dtok[i + (row / Np + 1) * cpr]; }
};

extern "C" int nk_vit_tokens(const void* patches, const float* cls, const float* pos, void* tokens, int N, int Np, int E, void* stream) {
  NK_CHECK_ARG(patches && cls && pos && tokens && N > 0 && Np > 0 && E > 0 && E % 8 == 0);
  NK_CHECK_ARG(nk_aligned16(patches) && nk_aligned16(tokens));
  return nk_ew_rows("vit_tokens", stream, (long)N * (Np + 1), E / 8, VitTokens{(const bf16_t*)patches, cls, pos, (float*)tokens, Np + 1, E});
}
extern "C" int nk_vit_tokens_bwd(const void* dtokens, void* dpatches, int N, int Np, int E, void* stream) {
  NK_CHECK_ARG(dtokens && dpatches && N > 0 && Np > 0 && E > 0 && E % 8 == 0);
  NK_CHECK_ARG(nk_aligned16(dtokens) && nk_aligned16(dpatches));
  return nk_ew_rows("vit_tokens_bwd", stream, (long)N * Np, E / 8, VitDropCls{(const uint4_t*)dtokens, (uint4_t*)dpatches, Np, E / 8});
}

// ---- embedding head -------------------------------------------------------------------------------------------------------------------------
// f [2, B, Dz] fp32 (image 0 the input's features, image 1 the reconstruction's).  Per sample b, with u_j = f_j / |f_j|, z_j = u_j - mean(u_j)
// and zn_j = z_j / max(|z_j|, eps):    d_b = 1 - zn_0 . zn_1 = 0.5 |zn_0 - zn_1|^2    (the second form has no cancellation at small d).
// One workgroup of 256 threads per sample; every sum over Dz goes through nk_reduce_rows with one column: thread t adds elements t, t + 256, ...
// in ascending order, thread 0 then adds the 256 partial sums in ascending order.
#define HEAD_THREADS 256
template <int NACC, class Term>
__device__ __forceinline__ void head_sums(int Dz, float* bc, float* out, Term term) {
  nk_reduce_rows<HEAD_THREADS, 1, NACC, 0, 0>(true, Dz, term, [&](const float* acc) {
#pragma unroll
    for (int k = 0; k < NACC; ++k) bc[k] = acc[k];
  });
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NACC; ++k) out[k] = bc[k];
  __syncthreads();
}
struct HeadStats {
  float rn0, rn1, m0, m1;      // 1 / |f_j|, mean(u_j)
  float rz0, rz1;              // 1 / max(|z_j|, eps)
};
__device__ __forceinline__ HeadStats head_stats(const float* f0, const float* f1, int Dz, float eps, float* bc) {
  HeadStats s;
  float a[4];
  head_sums<4>(Dz, bc, a, [&](int r, float* acc) {
    const float x = f0[r], y = f1[r];
    acc[0] += x * x; acc[1] += y * y; acc[2] += x; acc[3] += y;
  });
  s.rn0 = 1.f / sqrtf(a[0]); s.rn1 = 1.f / sqrtf(a[1]);
  s.m0 = a[2] * s.rn0 / (float)Dz; s.m1 = a[3] * s.rn1 / (float)Dz;
  float q[2];
  head_sums<2>(Dz, bc, q, [&](int r, float* acc) {
    const float z0 = f0[r] * s.rn0 - s.m0, z1 = f1[r] * s.rn1 - s.m1;
    acc[0] += z0 * z0; acc[1] += z1 * z1;
  });
  s.rz0 = 1.f / fmaxf(sqrtf(q[0]), eps); s.rz1 = 1.f / fmaxf(sqrtf(q[1]), eps);
  return s;
}
__global__ __launch_bounds__(HEAD_THREADS) void dreamsim_head_fwd_kernel(const float* __restrict__ f, float* __restrict__ d, int B, int Dz, float eps) {
  __shared__ float bc[4];
  const float* f0 = f + (long)blockIdx.x * Dz;
  const float* f1 = f0 + (long)B * Dz;
  const HeadStats s = head_stats(f0, f1, Dz, eps, bc);
  float h[1];
  head_sums<1>(Dz, bc, h, [&](int r, float* acc) {
    const float e = (f0[r] * s.rn0 - s.m0) * s.rz0 - (f1[r] * s.rn1 - s.m1) * s.rz1;
    acc[0] += e * e;
  });
  if (threadIdx.x == 0) d[blockIdx.x] = 0.5f * h[0];
}
// df1 = up_b * d d_b / d f_1:   gz = -(zn_0 - c zn_1) * rz1 (c = zn_0 . zn_1);  gu = gz - mean(gz);  df1 = (gu - u_1 (u_1 . gu)) / |f_1|
__global__ __launch_bounds__(HEAD_THREADS) void dreamsim_head_bwd_kernel(const float* __restrict__ f, const float* __restrict__ up, float* __restrict__ df1,
                                                                         int B, int Dz, float eps) {
  __shared__ float bc[4];
  const float* f0 = f + (long)blockIdx.x * Dz;
  const float* f1 = f0 + (long)B * Dz;
  const HeadStats s = head_stats(f0, f1, Dz, eps, bc);
  float h[1];
  head_sums<1>(Dz, bc, h, [&](int r, float* acc) { acc[0] += ((f0[r] * s.rn0 - s.m0) * s.rz0) * ((f1[r] * s.rn1 - s.m1) * s.rz1); });
  const float c = h[0], g = -up[blockIdx.x] * s.rz1;
  auto gz = [&](int r) { return g * ((f0[r] * s.rn0 - s.m0) * s.rz0 - c * ((f1[r] * s.rn1 - s.m1) * s.rz1)); };
  float t[2];
  head_sums<2>(Dz, bc, t, [&](int r, float* acc) {
    const float v = gz(r);
    acc[0] += v; acc[1] += v * (f1[r] * s.rn1);
  });
  const float gmean = t[0] / (float)Dz;
  const float udot = t[1] - gmean * (s.m1 * (float)Dz);      // u_1 . gu = u_1 . gz - mean(gz) sum(u_1)
  float* out = df1 + (long)blockIdx.x * Dz;
  for (int r = threadIdx.x; r < Dz; r += HEAD_THREADS) out[r] = (gz(r) - gmean - (f1[r] * s.rn1) * udot) * s.rn1;
}

extern "C" int nk_dreamsim_head_fwd(const float* f, float* d, int B, int Dz, float eps, void* stream) {
  NK_CHECK_ARG(f && d && B > 0 && Dz > 0 && eps > 0.f);
  hipLaunchKernelGGL(dreamsim_head_fwd_kernel, dim3(B), dim3(HEAD_THREADS), 0, (hipStream_t)stream, f, d, B, Dz, eps);
  return nk_check_launch("dreamsim_head_fwd");
}
extern "C" int nk_dreamsim_head_bwd(const float* f, const float* upstream, float* df1, int B, int Dz, float eps, void* stream) {
  NK_CHECK_ARG(f && upstream && df1 && B > 0 && Dz > 0 && eps > 0.f);
  hipLaunchKernelGGL(dreamsim_head_bwd_kernel, dim3(B), dim3(HEAD_THREADS), 0, (hipStream_t)stream, f, upstream, df1, B, Dz, eps);
  return nk_check_launch("dreamsim_head_bwd");
}

// ---- the cls row's final LayerNorm and head, in fp32 ----------------------------------------------------------------------------------------
// Only the cls row of each sample reaches the embedding, and 1 - cos amplifies what its last two layers round away, so they run in fp32 on
// the fp32 parameters: row n * L of the fp32 token matrix -> (LayerNorm when gamma != NULL) -> (x W^T + bias when W != NULL) -> out fp32
// [N, nc] (nc = E without a head).  One workgroup per sample: the row sits in LDS, the statistics go through head_sums, and each output is
// one wave's dot product (lanes stride the row, xor butterfly: a fixed order).  mean / rstd [N] are kept for the backward.
#define CLS_MAX_E 2048
__global__ __launch_bounds__(HEAD_THREADS) void vit_cls_head_fwd_kernel(const float* __restrict__ tokens, long sample_stride, const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta, const float* __restrict__ W,
                                                                        const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ mean,
                                                                        float* __restrict__ rstd, int E, int nc, float eps) {
  __shared__ float row[CLS_MAX_E];
  __shared__ float bc[4];
  const float* src = tokens + (long)blockIdx.x * sample_stride;
  for (int k = threadIdx.x; k < E; k += HEAD_THREADS) row[k] = src[k];
  __syncthreads();
  if (gamma) {
    float s[1], q[1];
    head_sums<1>(E, bc, s, [&](int r, float* acc) { acc[0] += row[r]; });
    const float mu = s[0] / (float)E;
    head_sums<1>(E, bc, q, [&](int r, float* acc) { const float c = row[r] - mu; acc[0] += c * c; });
    const float rs = rsqrtf(q[0] / (float)E + eps);
    for (int k = threadIdx.x; k < E; k += HEAD_THREADS) row[k] = (row[k] - mu) * rs * gamma[k] + beta[k];
    if (threadIdx.x == 0) { mean[blockIdx.x] = mu; rstd[blockIdx.x] = rs; }
    __syncthreads();
  }
  float* dst = out + (long)blockIdx.x * nc;
  if (!W) {
    for (int k = threadIdx.x; k < E; k += HEAD_THREADS) dst[k] = row[k];
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < nc; j += HEAD_THREADS / 64) {
    const float* w = W + (long)j * E;
    float acc = 0.f;
    for (int k = lane; k < E; k += 64) acc += row[k] * w[k];
    acc = wave_sum(acc);
    if (lane == 0) dst[j] = acc + (bias ? bias[j] : 0.f);
  }
}
// dcls bf16 [N, E] = d out / d (cls row): dn_k = sum_j dout_j W_jk (dout itself without a head), then the LayerNorm's input gradient
// rstd (g dn - mean(g dn) - xhat mean(g dn xhat)) when there is one.  `tokens` points at the first sample's cls row.
__global__ __launch_bounds__(HEAD_THREADS) void vit_cls_head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ tokens, long sample_stride,
                                                                        const float* __restrict__ gamma, const float* __restrict__ W,
                                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                        bf16_t* __restrict__ dcls, int E, int nc) {
  __shared__ float dn[CLS_MAX_E];
  __shared__ float xh[CLS_MAX_E];
  __shared__ float bc[4];
  const float* g = dout + (long)blockIdx.x * nc;
  for (int k = threadIdx.x; k < E; k += HEAD_THREADS) {
    float acc = 0.f;
    if (W) {
      for (int j = 0; j < nc; ++j) acc += g[j] * W[(long)j * E + k];
    } else {
      acc = g[k];
    }
    dn[k] = acc;
  }
  bf16_t* dst = dcls + (long)blockIdx.x * E;
  if (!gamma) {
    for (int k = threadIdx.x; k < E; k += HEAD_THREADS) dst[k] = f2bf(dn[k]);
    return;
  }
  const float* src = tokens + (long)blockIdx.x * sample_stride;
  const float mu = mean[blockIdx.x], rs = rstd[blockIdx.x];
  for (int k = threadIdx.x; k < E; k += HEAD_THREADS) {
    xh[k] = (src[k] - mu) * rs;
    dn[k] *= gamma[k];
  }
  __syncthreads();
  float t[2];
  head_sums<2>(E, bc, t, [&](int r, float* acc) { acc[0] += dn[r]; acc[1] += dn[r] * xh[r]; });
  const float m1 = t[0] / (float)E, m2 = t[1] / (float)E;
  for (int k = threadIdx.x; k < E; k += HEAD_THREADS) dst[k] = f2bf(rs * (dn[k] - m1 - xh[k] * m2));
}

extern "C" int nk_vit_cls_head_fwd(const void* tokens, long sample_stride, const float* gamma, const float* beta, const float* W, const float* bias,
                                   float* out, float* mean, float* rstd, int N, int E, int nc, float eps, void* stream) {
  NK_CHECK_ARG(tokens && out && N > 0 && E > 0 && E <= CLS_MAX_E && nc > 0 && sample_stride >= E);
  NK_CHECK_ARG((gamma == nullptr) == (beta == nullptr) && (!gamma || (mean && rstd && eps > 0.f)) && (W || nc == E));
  hipLaunchKernelGGL(vit_cls_head_fwd_kernel, dim3(N), dim3(HEAD_THREADS), 0, (hipStream_t)stream, (const float*)tokens, sample_stride, gamma, beta, W,
                     bias, out, mean, rstd, E, nc, eps);
  return nk_check_launch("vit_cls_head_fwd");
}
extern "C" int nk_vit_cls_head_bwd(const float* dout, const void* tokens, long sample_stride, const float* gamma, const float* W, const float* mean,
                                   const float* rstd, void* dcls, int N, int E, int nc, void* stream) {
  NK_CHECK_ARG(dout && dcls && N > 0 && E > 0 && E <= CLS_MAX_E && nc > 0 && (W || nc == E));
  NK_CHECK_ARG(!gamma || (tokens && mean && rstd && sample_stride >= E));
  hipLaunchKernelGGL(vit_cls_head_bwd_kernel, dim3(N), dim3(HEAD_THREADS), 0, (hipStream_t)stream, dout, (const float*)tokens, sample_stride, gamma, W, mean,
                     rstd, (bf16_t*)dcls, E, nc);
  return nk_check_launch("vit_cls_head_bwd");
}

// ---- the fp32 residual stream ---------------------------------------------------------------------------------------------------------------
// A frozen tower keeps its residual stream x [M, E] in fp32: 1 - cos of two nearby embeddings amplifies what a bf16 stream rounds away at every
// add.  The GEMMs and the attention still read and write bf16, so one kernel sits at each seam:  x += branch (the bf16 output of the out
// projection or of fc2; skipped when NULL), in place, and then y = LayerNorm(x) * gamma + beta for the next GEMM (bf16), or for the stream
// itself (fp32: norm_pre), or no norm at all (gamma NULL: the add alone).  xb, when given, receives x rounded to bf16: what
// nk_layernorm_bwd_dx reads in the backward, with the mean / rstd [M] written here.  One wave per row, the row in registers (E <= 2048,
// E % 64 == 0 not required), sums by xor butterfly: a fixed order.
#define ADDLN_MAX_PER_LANE 32
__global__ __launch_bounds__(256) void vit_add_ln_kernel(float* __restrict__ x, const bf16_t* __restrict__ branch, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, void* __restrict__ y, int y_f32, bf16_t* __restrict__ xb,
                                                         float* __restrict__ mean, float* __restrict__ rstd, int M, int E, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                    // whole waves leave together: no barrier below
  float* xr = x + row * E;
  float v[ADDLN_MAX_PER_LANE];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < ADDLN_MAX_PER_LANE; ++j) {
    const int k = lane + 64 * j;
    v[j] = 0.f;
    if (k < E) {
      v[j] = xr[k] + (branch ? bf2f(branch[row * E + k]) : 0.f);
      if (branch) xr[k] = v[j];
      if (xb) xb[row * E + k] = f2bf(v[j]);
      sum += v[j];
    }
  }
  if (!gamma) return;
  const float mu = wave_sum(sum) / (float)E;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < ADDLN_MAX_PER_LANE; ++j) {
    const float c = v[j] - mu;
    if (lane + 64 * j < E) sq += c * c;
  }
  const float rs = rsqrtf(wave_sum(sq) / (float)E + eps);
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
  for (int j = 0; j < ADDLN_MAX_PER_LANE; ++j) {
    const int k = lane + 64 * j;
    if (k < E) {
      const float o = (v[j] - mu) * rs * gamma[k] + beta[k];
      if (y_f32) ((float*)y)[row * E + k] = o;
      else ((bf16_t*)y)[row * E + k] = f2bf(o);
    }
  }
}
extern "C" int nk_vit_add_ln(float* x, const void* branch, const float* gamma, const float* beta, void* y, int y_f32, void* xb, float* mean, float* rstd,
                             int M, int E, float eps, void* stream) {
  NK_CHECK_ARG(x && M > 0 && E > 0 && E <= 64 * ADDLN_MAX_PER_LANE && (y_f32 == 0 || y_f32 == 1));
  NK_CHECK_ARG((gamma == nullptr) == (beta == nullptr) && (!gamma || (y && mean && rstd && eps > 0.f)) && (gamma || branch || xb));
  hipLaunchKernelGGL(vit_add_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)branch, gamma, beta, y, y_f32, (bf16_t*)xb,
                     mean, rstd, M, E, eps);
  return nk_check_launch("vit_add_ln");
}
