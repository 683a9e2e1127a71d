// HBM-bound elementwise / data-movement kernels of the SDXL training step (gfx950).
// All bf16 traffic is 16 B per lane; fp32 traffic 16 B per lane where the layout allows.
#include "../../include/neurosis_hip.h"
#include "nk_common.h"
#include "nk_ew.h"
#include "nk_reduce.h"
#include "norm_plan.h"

// ---- the map kernels: functors on the core of nk_ew.h -------------------------------------------------------------------------------------
// ---- GEGLU (modules/attention.py:55-57): y = u[:, :I] * gelu(u[:, I:]) ------------------------
struct GegluFwd {
  const bf16_t* u; bf16_t* y; int I;
  __device__ void operator()(long, long row, int ch) const {
    float a[8], g[8];
    ew_load(u + row * 2 * I + ch * 8, a);
    ew_load(u + row * 2 * I + I + ch * 8, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] *= gelu_erf(g[e]);
    ew_store(y + row * I + ch * 8, a);
  }
};
struct GegluBwd {
  const bf16_t *dy, *u; bf16_t* du; int I;
  __device__ void operator()(long, long row, int ch) const {
    float a[8], g[8], d[8], da[8], dg[8];
    ew_load(u + row * 2 * I + ch * 8, a);
    ew_load(u + row * 2 * I + I + ch * 8, g);
    ew_load(dy + row * I + ch * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float cdf, pdf;
      normal_cdf_pdf(g[e], cdf, pdf);
      da[e] = d[e] * (g[e] * cdf);
      dg[e] = d[e] * a[e] * (cdf + g[e] * pdf);
    }
    ew_store(du + row * 2 * I + ch * 8, da);
    ew_store(du + row * 2 * I + I + ch * 8, dg);
  }
};
// saved-derivative form (round 6): y = a gelu(g) and s = [gelu(g) | a gelu'(g)] from u = [a | g] (s may BE u: every thread rewrites the two
// chunks it read, after it has read both); the backward is then two products per element
struct GegluFwdS {
  const bf16_t* u; bf16_t *y, *s; int I;
  __device__ void operator()(long, long row, int ch) const {
    float a[8], g[8], h[8], s1[8], s2[8];
    ew_load(u + row * 2 * I + ch * 8, a);
    ew_load(u + row * 2 * I + I + ch * 8, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float cdf, pdf;
      normal_cdf_pdf(g[e], cdf, pdf);
      s1[e] = g[e] * cdf;
      h[e] = a[e] * s1[e];
      s2[e] = a[e] * (cdf + g[e] * pdf);
    }
    ew_store(y + row * I + ch * 8, h);
    ew_store(s + row * 2 * I + ch * 8, s1);
    ew_store(s + row * 2 * I + I + ch * 8, s2);
  }
};
struct GegluBwdS {
  const bf16_t *dy, *s; bf16_t* du; int I;
  __device__ void operator()(long, long row, int ch) const {
    float s1[8], s2[8], d[8];
    ew_load(s + row * 2 * I + ch * 8, s1);
    ew_load(s + row * 2 * I + I + ch * 8, s2);
    ew_load(dy + row * I + ch * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] *= d[e]; s2[e] *= d[e]; }
    ew_store(du + row * 2 * I + ch * 8, s1);
    ew_store(du + row * 2 * I + I + ch * 8, s2);
  }
};
extern "C" int nk_geglu_fwd_s(const void* u, void* y, void* s, long M, int I, void* stream) {
  NK_CHECK_ARG(u && y && s && M > 0 && I > 0 && (I & 7) == 0);
  return nk_ew_rows("geglu_fwd_s", stream, M, I >> 3, GegluFwdS{(const bf16_t*)u, (bf16_t*)y, (bf16_t*)s, I});
}
extern "C" int nk_geglu_bwd_s(const void* dy, const void* s, void* du, long M, int I, void* stream) {
  NK_CHECK_ARG(dy && s && du && M > 0 && I > 0 && (I & 7) == 0);
  return nk_ew_rows("geglu_bwd_s", stream, M, I >> 3, GegluBwdS{(const bf16_t*)dy, (const bf16_t*)s, (bf16_t*)du, I});
}
extern "C" int nk_geglu_fwd(const void* u, void* y, long M, int I, void* stream) {
  NK_CHECK_ARG(u && y && M > 0 && I > 0 && (I & 7) == 0);
  return nk_ew_rows("geglu_fwd", stream, M, I >> 3, GegluFwd{(const bf16_t*)u, (bf16_t*)y, I});
}
extern "C" int nk_geglu_bwd(const void* dy, const void* u, void* du, long M, int I, void* stream) {
  NK_CHECK_ARG(dy && u && du && M > 0 && I > 0 && (I & 7) == 0);
  return nk_ew_rows("geglu_bwd", stream, M, I >> 3, GegluBwd{(const bf16_t*)dy, (const bf16_t*)u, (bf16_t*)du, I});
}

// ---- SiLU on a flat bf16 array (openaimodel.py:274, 588, 615) ----------------------------------
struct SiluFwd {
  const bf16_t* x; bf16_t* y;
  __device__ void operator()(long i) const {
    float f[8];
    ew_load(x + i * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = silu_f(f[e]);
    ew_store(y + i * 8, f);
  }
};
struct SiluBwd {
  const bf16_t *dy, *x; bf16_t* dx;
  __device__ void operator()(long i) const {
    float f[8], d[8];
    ew_load(x + i * 8, f);
    ew_load(dy + i * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] *= dsilu_f(f[e]);
    ew_store(dx + i * 8, d);
  }
};
extern "C" int nk_silu_fwd(const void* x, void* y, long n, void* stream) {
  NK_CHECK_ARG(x && y && n > 0 && (n & 7) == 0);
  return nk_ew_flat("silu_fwd", stream, n >> 3, SiluFwd{(const bf16_t*)x, (bf16_t*)y});
}
extern "C" int nk_silu_bwd(const void* dy, const void* x, void* dx, long n, void* stream) {
  NK_CHECK_ARG(dy && x && dx && n > 0 && (n & 7) == 0);
  return nk_ew_flat("silu_bwd", stream, n >> 3, SiluBwd{(const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx});
}

// ---- GELU of the CLIP text transformers ---------------------------------------------------------
// mode 0: exact erf form (open_clip's nn.GELU); mode 1: quick_gelu x * sigmoid(1.702 x) (openai/clip-vit-large-patch14);
// mode 2: "gelu_new", the tanh form of T5 v1.1 / ByT5 (gelu_tanh, nk_common.h); mode 3: ReLU (T5 v1.0)
template <int MODE>
struct GeluFwd {
  const bf16_t* x; bf16_t* y;
  __device__ void operator()(long i) const {
    float f[8];
    ew_load(x + i * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      f[e] = MODE == 0 ? 0.5f * f[e] * (1.0f + erff(f[e] * 0.70710678118654752f)) : MODE == 1 ? f[e] / (1.0f + __expf(-1.702f * f[e]))
           : MODE == 2 ? gelu_tanh(f[e]) : fmaxf(f[e], 0.f);
    ew_store(y + i * 8, f);
  }
};
extern "C" int nk_gelu_fwd(const void* x, void* y, long n, int mode, void* stream) {
  NK_CHECK_ARG(x && y && n > 0 && (n & 7) == 0 && mode >= 0 && mode <= 3);
  return nk_ew_mode<0, 3>(mode, [&](auto m) { return nk_ew_flat("gelu_fwd", stream, n >> 3, GeluFwd<decltype(m)::value>{(const bf16_t*)x, (bf16_t*)y}); });
}

// ---- gated activation of the T5 v1.1 / ByT5 FeedForward: y = gelu_new(u[:, :I]) * u[:, I:] ----------------------------------------------
// u [M][2 I] = one stacked projection [wi_0; wi_1] of the normed tokens, so the FeedForward is two GEMMs and this pass.  (The GEGLU of the
// UNet, GegluFwd above, gates the other way round and with the erf form.)
struct GatedGeluTanh {
  const bf16_t* u; bf16_t* y; int I;
  __device__ void operator()(long, long row, int ch) const {
    float a[8], g[8];
    ew_load(u + row * 2 * I + ch * 8, a);
    ew_load(u + row * 2 * I + I + ch * 8, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = gelu_tanh(a[e]) * g[e];
    ew_store(y + row * I + ch * 8, a);
  }
};
extern "C" int nk_gated_gelu_tanh_fwd(const void* u, void* y, long M, int I, void* stream) {
  NK_CHECK_ARG(u && y && M > 0 && I > 0 && (I & 7) == 0);
  NK_CHECK_ARG(nk_aligned16(u) && nk_aligned16(y));     // 16-byte accesses
  return nk_ew_rows("gated_gelu_tanh_kernel", stream, M, I >> 3, GatedGeluTanh{(const bf16_t*)u, (bf16_t*)y, I});
}

// GELU backward (trainable text towers): dx = dy * gelu'(x), fp32 arithmetic on bf16 data, the same modes as the forward
//   mode 0: gelu'(x) = Phi(x) + x phi(x);  mode 1: s + 1.702 x s (1 - s), s = sigmoid(1.702 x)
template <int MODE>
struct GeluBwd {
  const bf16_t *dy, *x; bf16_t* dx;
  __device__ void operator()(long i) const {
    float g[8], f[8];
    ew_load(dy + i * 8, g);
    ew_load(x + i * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float d;
      if (MODE == 0) {
        d = 0.5f * (1.0f + erff(f[e] * 0.70710678118654752f)) + f[e] * 0.39894228040143268f * __expf(-0.5f * f[e] * f[e]);
      } else if (MODE == 1) {
        const float sg = 1.0f / (1.0f + __expf(-1.702f * f[e]));
        d = sg + 1.702f * f[e] * sg * (1.0f - sg);
      } else if (MODE == 2) {
        d = dgelu_tanh(f[e]);
      } else {
        d = f[e] > 0.f ? 1.0f : 0.f;      // ReLU: dx = dy where x > 0, exactly
      }
      g[e] *= d;
    }
    ew_store(dx + i * 8, g);
  }
};
extern "C" int nk_gelu_bwd(const void* dy, const void* x, void* dx, long n, int mode, void* stream) {
  NK_CHECK_ARG(dy && x && dx && n > 0 && (n & 7) == 0 && (mode == 0 || mode == 1));
  NK_CHECK_ARG(nk_aligned16(dy) && nk_aligned16(x) && nk_aligned16(dx));     // 16-byte accesses
  return nk_ew_mode<0, 1>(mode, [&](auto m) {
    return nk_ew_flat("gelu_bwd", stream, n >> 3, GeluBwd<decltype(m)::value>{(const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx});
  });
}

// The activations of the T5 FeedForwards under training: the same functor in all four modes of nk_gelu_fwd (2: "gelu_new", 3: ReLU).
// (nk_gelu_bwd keeps its two modes: the CLIP towers' contract.)
extern "C" int nk_act_bwd(const void* dy, const void* x, void* dx, long n, int mode, void* stream) {
  NK_CHECK_ARG(dy && x && dx && n > 0 && (n & 7) == 0 && mode >= 0 && mode <= 3);
  NK_CHECK_ARG(nk_aligned16(dy) && nk_aligned16(x) && nk_aligned16(dx));     // 16-byte accesses
  return nk_ew_mode<0, 3>(mode, [&](auto m) {
    return nk_ew_flat("act_bwd", stream, n >> 3, GeluBwd<decltype(m)::value>{(const bf16_t*)dy, (const bf16_t*)x, (bf16_t*)dx});
  });
}
// backward of nk_gated_gelu_tanh_fwd: du [M][2 I] = [dy b gelu_new'(a) | dy gelu_new(a)] from dy [M][I] and u = [a | b]; fp32 arithmetic, one
// rounding to bf16 per element
struct GatedGeluTanhBwd {
  const bf16_t *dy, *u; bf16_t* du; int I;
  __device__ void operator()(long, long row, int ch) const {
    float g[8], a[8], b[8], da[8];
    ew_load(dy + row * I + ch * 8, g);
    ew_load(u + row * 2 * I + ch * 8, a);
    ew_load(u + row * 2 * I + I + ch * 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      da[e] = g[e] * b[e] * dgelu_tanh(a[e]);
      b[e] = g[e] * gelu_tanh(a[e]);
    }
    ew_store(du + row * 2 * I + ch * 8, da);
    ew_store(du + row * 2 * I + I + ch * 8, b);
  }
};
extern "C" int nk_gated_gelu_tanh_bwd(const void* dy, const void* u, void* du, long M, int I, void* stream) {
  NK_CHECK_ARG(dy && u && du && M > 0 && I > 0 && (I & 7) == 0);
  NK_CHECK_ARG(nk_aligned16(dy) && nk_aligned16(u) && nk_aligned16(du));     // 16-byte accesses
  return nk_ew_rows("gated_gelu_tanh_bwd_kernel", stream, M, I >> 3, GatedGeluTanhBwd{(const bf16_t*)dy, (const bf16_t*)u, (bf16_t*)du, I});
}

// ---- token + position embedding backward (trainable text towers) --------------------------------
// Workgroup w < N = B * L owns token w: if w is the FIRST token with its id v, it sums the gradient rows of every token with id v in token
// order and writes (or adds) table row v; later tokens with the same id do nothing.  Workgroup N + l sums position l over the batch, b = 0 .. B-1.
// Fixed-order sums, no atomics: the result does not depend on scheduling (a padded prompt repeats one id some 60 times).  Each lane owns
// 8 columns.  The ids are wave-uniform loads; the O(N^2) id scan is nothing at N = 308.
template <class T>
__global__ void embedding_bwd_kernel(const long long* __restrict__ ids, const T* __restrict__ dx, long ldx, float* __restrict__ dtab,
                                     float* __restrict__ dpos, int N, int L, int V, int C, int accumulate) {
  const int w = blockIdx.x;
  const int c8 = C >> 3;
  if (w < N) {
    const long long v = ids[w];
    if (v < 0 || v >= V) return;      // (the forward's lookup rejects such ids; never write outside the table)
    int seen = 0;
    for (int j = threadIdx.x; j < w; j += blockDim.x) seen |= ids[j] == v;
    if (__syncthreads_or(seen)) return;
    for (int ch = threadIdx.x; ch < c8; ch += blockDim.x) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int t = w; t < N; ++t) {
        if (ids[t] != v) continue;
        float f[8];
        ew_load(dx + (long)t * ldx + ch * 8, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += f[e];
      }
      float4_t* out = (float4_t*)(dtab + v * (long)C + ch * 8);
      float4_t lo = {acc[0], acc[1], acc[2], acc[3]}, hi = {acc[4], acc[5], acc[6], acc[7]};
      if (accumulate) { lo += out[0]; hi += out[1]; }
      out[0] = lo;
      out[1] = hi;
    }
  } else {
    const int l = w - N, B = N / L;
    for (int ch = threadIdx.x; ch < c8; ch += blockDim.x) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < B; ++b) {
        float f[8];
        ew_load(dx + ((long)b * L + l) * ldx + ch * 8, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += f[e];
      }
      float4_t* out = (float4_t*)(dpos + (long)l * C + ch * 8);
      float4_t lo = {acc[0], acc[1], acc[2], acc[3]}, hi = {acc[4], acc[5], acc[6], acc[7]};
      if (accumulate) { lo += out[0]; hi += out[1]; }
      out[0] = lo;
      out[1] = hi;
    }
  }
}
// the clearing pass and the launch, for the text towers' entry and for the label embedding's (T = float: fp32 gradient rows)
template <class T>
static int embedding_bwd_launch(const char* name, const long long* ids, const T* dx, long ldx, float* dtable, float* dpos, int B, int L, int V, int P, int C,
                                int accumulate, hipStream_t stream) {
  if (accumulate == 0) {     // overwrite: rows no token (no position) hit are zero; (2: the caller's buffers are zero already)
    if (hipMemsetAsync(dtable, 0, (size_t)V * C * sizeof(float), stream) != hipSuccess) return nk_check_launch("embedding_bwd memset");
    if (dpos && hipMemsetAsync(dpos, 0, (size_t)P * C * sizeof(float), stream) != hipSuccess) return nk_check_launch("embedding_bwd memset");
  }
  hipLaunchKernelGGL(embedding_bwd_kernel<T>, dim3(B * L + (dpos ? L : 0)), dim3(128), 0, stream, ids, dx, ldx, dtable, dpos, B * L, L, V, C, accumulate == 1);
  return nk_check_launch(name);
}
extern "C" int nk_embedding_bwd(const long long* ids, const void* dx, long ldx, float* dtable, float* dpos, int B, int L, int V, int P, int C,
                                int accumulate, void* stream_) {
  // (dpos == NULL with P == 0: an embedding without a position table -- the T5 encoders -- so no position workgroups are launched)
  NK_CHECK_ARG(ids && dx && dtable && B > 0 && L > 0 && V > 0 && C > 0 && (C & 7) == 0 && (ldx & 7) == 0 && ldx >= C);
  NK_CHECK_ARG(dpos ? L <= P : P == 0);
  NK_CHECK_ARG(nk_aligned16(dx) && nk_aligned16(dtable) && nk_aligned16(dpos));
  NK_CHECK_ARG((long)B * L <= NK_EMBEDDING_BWD_MAX_TOKENS && accumulate >= 0 && accumulate <= 2);     // (the id scans are quadratic in B * L)
  return embedding_bwd_launch("embedding_bwd", ids, (const bf16_t*)dx, ldx, dtable, dpos, B, L, V, P, C, accumulate, (hipStream_t)stream_);
}

// ---- label embeddings of a class-conditional UNet (openaimodel.py:574-590) and ClassEmbedder (encoders/classed.py) ------------------------------
// lookup: out[b, :] = table[ids[b], :] (+ add[b, :]), fp32 arithmetic, one rounding when out is bf16.  An id outside [0, V) is never an
// address: its row comes out NaN (nn.Embedding raises; a kernel cannot, and a clamped id would train the wrong class in silence)
template <bool F32OUT>
struct LabelRows {
  const float* table; const long long* ids; const bf16_t* add; void* out; int V, D;
  __device__ void operator()(long i, long row, int ch) const {
    const long long v = ids[row];
    float f[8];
    if (v < 0 || v >= V) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = __builtin_nanf("");
    } else {
      ew_load(table + v * (long)D + ch * 8, f);
      if (add) {
        float a[8];
        ew_load(add + row * D + ch * 8, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += a[e];
      }
    }
    if constexpr (F32OUT) ew_store((float*)out + i * 8, f);
    else ew_store((bf16_t*)out + i * 8, f);
  }
};
extern "C" int nk_label_rows_fwd(const float* table, const long long* ids, const void* add, void* out, int out_is_f32, int B, int V, int D, void* stream) {
  NK_CHECK_ARG(table && ids && out && B > 0 && V > 0 && D > 0 && (D & 7) == 0);
  NK_CHECK_ARG(nk_aligned16(table) && nk_aligned16(add) && nk_aligned16(out));     // 16-byte accesses
  if (out_is_f32) return nk_ew_rows("label_rows_fwd", stream, B, D >> 3, LabelRows<true>{table, ids, (const bf16_t*)add, out, V, D});
  return nk_ew_rows("label_rows_fwd", stream, B, D >> 3, LabelRows<false>{table, ids, (const bf16_t*)add, out, V, D});
}
// gradient: dtable[v, :] = sum of d[b, :] over the samples with ids[b] = v in ascending b -- nk_embedding_bwd's kernel with one token per
// sample and no position table, on bf16 or fp32 rows
extern "C" int nk_label_rows_bwd(const long long* ids, const void* d, long ldd, int d_is_f32, float* dtable, int B, int V, int D, int accumulate,
                                 void* stream) {
  NK_CHECK_ARG(ids && d && dtable && B > 0 && V > 0 && D > 0 && (D & 7) == 0 && (ldd & 7) == 0 && ldd >= D);
  NK_CHECK_ARG(nk_aligned16(d) && nk_aligned16(dtable));
  NK_CHECK_ARG(B <= NK_EMBEDDING_BWD_MAX_TOKENS && accumulate >= 0 && accumulate <= 2);     // (the id scans are quadratic in B)
  if (d_is_f32) return embedding_bwd_launch("label_rows_bwd", ids, (const float*)d, ldd, dtable, nullptr, B, 1, V, 0, D, accumulate, (hipStream_t)stream);
  return embedding_bwd_launch("label_rows_bwd", ids, (const bf16_t*)d, ldd, dtable, nullptr, B, 1, V, 0, D, accumulate, (hipStream_t)stream);
}

// nn.Linear(1, D), the "continuous" label embedding: K = 1 is an outer product, not a shape for the matrix pipe.
// forward: out[b, j] = bf16(y[b] w[j] + bias[j] (+ add[b, j]))
struct Linear1Fwd {
  const float *y, *w, *bias; const bf16_t* add; bf16_t* out; int D;
  __device__ void operator()(long i, long row, int ch) const {
    const float yb = y[row];
    float f[8], b[8];
    ew_load(w + ch * 8, f);
    ew_load(bias + ch * 8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = yb * f[e] + b[e];
    if (add) {
      ew_load(add + i * 8, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += b[e];
    }
    ew_store(out + i * 8, f);
  }
};
extern "C" int nk_linear1_fwd(const float* y, const float* w, const float* bias, const void* add, void* out, int B, int D, void* stream) {
  NK_CHECK_ARG(y && w && bias && out && B > 0 && D > 0 && (D & 7) == 0);
  NK_CHECK_ARG(nk_aligned16(w) && nk_aligned16(bias) && nk_aligned16(add) && nk_aligned16(out));     // 16-byte accesses
  return nk_ew_rows("linear1_fwd", stream, B, D >> 3, Linear1Fwd{y, w, bias, (const bf16_t*)add, (bf16_t*)out, D});
}
// backward: dw[j] = sum_b y[b] d[b, j] and db[j] = sum_b d[b, j], one thread per column adding b = 0 .. B - 1 in order (nk_reduce_rows with one
// row group); dy[b] = sum_j d[b, j] w[j], one thread column per sample, 16 row groups over j in the reducer's order
__global__ void __launch_bounds__(256) linear1_bwd_params_kernel(const bf16_t* __restrict__ d, const float* __restrict__ y, float* __restrict__ dw,
                                                                 float* __restrict__ db, int B, int D, int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  nk_reduce_rows<1, 256, 2, 0, 4>(
      j < D, B,
      [&](int b, float* acc) {
        const float g = bf2f(d[(long)b * D + j]);
        acc[0] += y[b] * g;
        acc[1] += g;
      },
      [&](const float* acc) {
        dw[j] = accumulate ? dw[j] + acc[0] : acc[0];
        db[j] = accumulate ? db[j] + acc[1] : acc[1];
      });
}
__global__ void __launch_bounds__(256) linear1_bwd_dy_kernel(const bf16_t* __restrict__ d, const float* __restrict__ w, float* __restrict__ dy, int B, int D) {
  const int b = blockIdx.x * 16 + threadIdx.x % 16;
  nk_reduce_rows<16, 16, 1, 1, 4>(
      b < B, D, [&](int j, float* acc) { acc[0] += bf2f(d[(long)b * D + j]) * w[j]; }, [&](const float* acc) { dy[b] = acc[0]; });
}
extern "C" int nk_linear1_bwd(const void* d, const float* y, const float* w, float* dw, float* db, float* dy, int B, int D, int accumulate, void* stream_) {
  NK_CHECK_ARG(d && y && w && dw && db && B > 0 && D > 0 && (D & 7) == 0 && accumulate >= 0 && accumulate <= 2);
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(linear1_bwd_params_kernel, dim3((D + 255) / 256), dim3(256), 0, stream, (const bf16_t*)d, y, dw, db, B, D, accumulate == 1);
  if (dy) hipLaunchKernelGGL(linear1_bwd_dy_kernel, dim3((B + 15) / 16), dim3(256), 0, stream, (const bf16_t*)d, w, dy, B, D);
  return nk_check_launch("linear1_bwd");
}

// ---- backward of a row gather: dx[B * L][C] = 0 except row b * L + idx[b] = dsel[b] (idx read on the device; 0 <= idx[b] < L) ----
__global__ void gather_rows_bwd_kernel(const bf16_t* __restrict__ dsel, long ldsel, const long long* __restrict__ idx, bf16_t* __restrict__ dx,
                                       int L, int c8, long n8) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const long r = i / c8;
    const int ch = (int)(i - r * c8);
    const int b = (int)(r / L), l = (int)(r - (long)b * L);
    uint4_t z = {0u, 0u, 0u, 0u};
    if (idx[b] == l) z = *(const uint4_t*)(dsel + (long)b * ldsel + ch * 8);
    *(uint4_t*)(dx + i * 8) = z;
  }
}
extern "C" int nk_gather_rows_bwd(const void* dsel, long ldsel, const long long* idx, void* dx, int B, int L, int C, void* stream) {
  NK_CHECK_ARG(dsel && idx && dx && B > 0 && L > 0 && C > 0 && (C & 7) == 0 && (ldsel & 7) == 0 && ldsel >= C);
  NK_CHECK_ARG(nk_aligned16(dsel) && nk_aligned16(dx));                                 // 16-byte accesses
  const long n8 = (long)B * L * (C >> 3);
  hipLaunchKernelGGL(gather_rows_bwd_kernel, dim3(nk_ew_grid(n8)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, (const bf16_t*)dsel, ldsel, idx,
                     (bf16_t*)dx, L, C >> 3, n8);
  return nk_check_launch("gather_rows_bwd");
}

// ---- weight gradient contracted over a few rows: dw[K][N] (+)= sum_m x[m][k] dy[m][n], m = 0 .. M-1 in order (M <= 256) ----------
// bigG's text_projection [width, embed_dim] (read transposed by the forward) sees only the B end-of-text rows.  One lane per output.
__global__ void wgrad_few_rows_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ dy, long lddy, float* __restrict__ dw,
                                      long lddw, int M, int K, int N, int accumulate) {
  const long total = (long)K * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int k = (int)(i / N), n = (int)(i - (long)k * N);
    float acc = 0.f;
    for (int m = 0; m < M; ++m) acc += bf2f(x[(long)m * ldx + k]) * bf2f(dy[(long)m * lddy + n]);
    float* o = dw + (long)k * lddw + n;
    *o = accumulate ? *o + acc : acc;
  }
}
extern "C" int nk_wgrad_few_rows(const void* x, long ldx, const void* dy, long lddy, float* dw, long lddw, int M, int K, int N, int accumulate,
                                 void* stream) {
  NK_CHECK_ARG(x && dy && dw && M > 0 && M <= 256 && K > 0 && N > 0 && ldx >= K && lddy >= N && lddw >= N);
  const long total = (long)K * N;
  hipLaunchKernelGGL(wgrad_few_rows_kernel, dim3(nk_ew_grid(total)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, ldx,
                     (const bf16_t*)dy, lddy, dw, lddw, M, K, N, accumulate);
  return nk_check_launch("wgrad_few_rows");
}

// ---- out = a + b (gradient join where a tensor feeds two consumers) ----------------------------
struct Add {
  const bf16_t *a, *b; bf16_t* o;
  __device__ void operator()(long i) const {
    float f[8], g[8];
    ew_load(a + i * 8, f);
    ew_load(b + i * 8, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += g[e];
    ew_store(o + i * 8, f);
  }
};
extern "C" int nk_add(const void* a, const void* b, void* out, long n, void* stream) {
  NK_CHECK_ARG(a && b && out && n > 0 && (n & 7) == 0);
  return nk_ew_flat("add", stream, n >> 3, Add{(const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out});
}

// ---- channel concat / split on channels-last rows (torch.cat(dim=1), openaimodel.py:836) -------
// dir 0: out[row] = [a[row] | b[row]] ; dir 1: a[row], b[row] = split(out[row]) (either may be NULL)
struct Cat {
  bf16_t *a, *b, *o; int Ca, Cb, dir;
  __device__ void operator()(long i, long row, int ch) const {
    const int ca8 = Ca >> 3;
    bf16_t* side = ch < ca8 ? (a ? a + row * Ca + ch * 8 : nullptr) : (b ? b + row * Cb + (ch - ca8) * 8 : nullptr);
    if (!side) return;
    uint4_t* op = (uint4_t*)(o + i * 8);
    if (dir == 0) *op = *(const uint4_t*)side;
    else *(uint4_t*)side = *op;
  }
};
extern "C" int nk_cat_channels(const void* a, const void* b, void* out, long rows, int Ca, int Cb, void* stream) {
  NK_CHECK_ARG(a && b && out && rows > 0 && Ca > 0 && Cb > 0 && (Ca & 7) == 0 && (Cb & 7) == 0);
  return nk_ew_rows("cat_channels", stream, rows, (Ca + Cb) >> 3, Cat{(bf16_t*)a, (bf16_t*)b, (bf16_t*)out, Ca, Cb, 0});
}
extern "C" int nk_split_channels(const void* src, void* a, void* b, long rows, int Ca, int Cb, void* stream) {
  NK_CHECK_ARG(src && (a || b) && rows > 0 && Ca > 0 && Cb > 0 && (Ca & 7) == 0 && (Cb & 7) == 0);
  return nk_ew_rows("split_channels", stream, rows, (Ca + Cb) >> 3, Cat{(bf16_t*)a, (bf16_t*)b, (bf16_t*)src, Ca, Cb, 1});
}

// ---- parameter-free resampling (Upsample / Downsample with use_conv=False, the up / down ResBlock; openaimodel.py:96-197) ----
// The pixel ops run over their OUTPUT image; H, W, C are the entry point's.
// backward of nearest 2x upsampling: dx[n,h,w,:] = sum of the 2x2 block of dup
struct Up2Bwd {
  const bf16_t* dup; bf16_t* dx; int H, W, C;
  __device__ void operator()(long i, int n, int h, int w, int ch) const {
    const bf16_t* s = dup + (((long)n * 2 * H + 2 * h) * 2 * W + 2 * w) * C + ch * 8;
    float acc[8], f[8];
    ew_load(s, acc);
    ew_load(s + C, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
    ew_load(s + (long)2 * W * C, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
    ew_load(s + (long)2 * W * C + C, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
    ew_store(dx + i * 8, acc);
  }
};
// nearest 2x forward, materialised: up[n, h, w, :] = x[n, h/2, w/2, :]
struct Up2Fwd {
  const bf16_t* x; bf16_t* up; int H, W, C;
  __device__ void operator()(long i, int n, int h, int w, int ch) const {
    *(uint4_t*)(up + i * 8) = *(const uint4_t*)(x + (((long)n * H + (h >> 1)) * W + (w >> 1)) * C + ch * 8);
  }
};
extern "C" int nk_upsample2x_bwd(const void* dup, void* dx, int N, int H, int W, int C, void* stream) {
  NK_CHECK_ARG(dup && dx && N > 0 && H > 0 && W > 0 && C > 0 && (C & 7) == 0);
  return nk_ew_pixels("upsample2x_bwd", stream, N, H, W, C >> 3, Up2Bwd{(const bf16_t*)dup, (bf16_t*)dx, H, W, C});
}
extern "C" int nk_upsample2x_fwd(const void* x, void* up, int N, int H, int W, int C, void* stream) {
  NK_CHECK_ARG(x && up && N > 0 && H > 0 && W > 0 && C > 0 && (C & 7) == 0);
  return nk_ew_pixels("upsample2x_fwd", stream, N, 2 * H, 2 * W, C >> 3, Up2Fwd{(const bf16_t*)x, (bf16_t*)up, H, W, C});
}

// avg_pool2d(2, 2), floor mode: y[n, h, w, :] = mean of x[n, 2h..2h+1, 2w..2w+1, :], summed in fp32 and rounded once; an odd last row or
// column of x is not read
struct AvgPool2xFwd {
  const bf16_t* x; bf16_t* y; int H, W, C;
  __device__ void operator()(long i, int n, int h, int w, int ch) const {
    const bf16_t* s = x + (((long)n * H + 2 * h) * W + 2 * w) * C + ch * 8;
    float acc[8], f[8];
    ew_load(s, acc);
    ew_load(s + C, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
    ew_load(s + (long)W * C, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += f[e];
    ew_load(s + (long)W * C + C, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = (acc[e] + f[e]) * 0.25f;
    ew_store(y + i * 8, acc);
  }
};
// ... backward: dx[n, h, w, :] = dy[n, h/2, w/2, :] / 4; zeros in the odd last row or column the forward dropped
struct AvgPool2xBwd {
  const bf16_t* dy; bf16_t* dx; int H, W, C;
  __device__ void operator()(long i, int n, int h, int w, int ch) const {
    const int Ho = H >> 1, Wo = W >> 1;
    uint4_t out = {0u, 0u, 0u, 0u};
    if ((h >> 1) < Ho && (w >> 1) < Wo) {
      float f[8];
      ew_load(dy + (((long)n * Ho + (h >> 1)) * Wo + (w >> 1)) * C + ch * 8, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] *= 0.25f;
      out = pack8(f);
    }
    *(uint4_t*)(dx + i * 8) = out;
  }
};
extern "C" int nk_avgpool2x_fwd(const void* x, void* y, int N, int H, int W, int C, void* stream) {
  NK_CHECK_ARG(x && y && N > 0 && H > 1 && W > 1 && C > 0 && (C & 7) == 0);
  return nk_ew_pixels("avgpool2x_fwd", stream, N, H >> 1, W >> 1, C >> 3, AvgPool2xFwd{(const bf16_t*)x, (bf16_t*)y, H, W, C});
}
extern "C" int nk_avgpool2x_bwd(const void* dy, void* dx, int N, int H, int W, int C, void* stream) {
  NK_CHECK_ARG(dy && dx && N > 0 && H > 1 && W > 1 && C > 0 && (C & 7) == 0);
  return nk_ew_pixels("avgpool2x_bwd", stream, N, H, W, C >> 3, AvgPool2xBwd{(const bf16_t*)dy, (bf16_t*)dx, H, W, C});
}

// ---- layout / dtype boundary: NCHW (fp32 or bf16) <-> channels-last bf16 with channel padding ---
// tile of 32 pixels x 32 channels through LDS
template <typename SrcT>
__global__ void nchw_to_nhwc_kernel(const SrcT* __restrict__ src, bf16_t* __restrict__ dst, int C, int HW, int Cpad,
                                    float scale) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty 0..7
  for (int j = ty; j < 32; j += 8) {
    int c = c0 + j, p = p0 + tx;
    float v = 0.f;
    if (c < C && p < HW) {
      if constexpr (sizeof(SrcT) == 4) v = src[((long)n * C + c) * HW + p];
      else v = bf2f(src[((long)n * C + c) * HW + p]);
    }
    tile[j][tx] = v * scale;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int p = p0 + j, c = c0 + tx;
    if (p < HW && c < Cpad) dst[((long)n * HW + p) * Cpad + c] = f2bf(tile[tx][j]);
  }
}
template <typename DstT>
__global__ void nhwc_to_nchw_kernel(const bf16_t* __restrict__ src, DstT* __restrict__ dst, int C, int HW, int Cpad) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8) {
    int p = p0 + j, c = c0 + tx;
    tile[j][tx] = (p < HW && c < C) ? bf2f(src[((long)n * HW + p) * Cpad + c]) : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    int c = c0 + j, p = p0 + tx;
    if (c < C && p < HW) {
      float v = tile[tx][j];
      if constexpr (sizeof(DstT) == 4) dst[((long)n * C + c) * HW + p] = v;
      else dst[((long)n * C + c) * HW + p] = f2bf(v);
    }
  }
}
// ------------------------------------------------------------------------------------------------
// conv weight [Cout][KH*KW][Cin] -> [Cin][KH*KW flipped][Cout]: the weights of the convolution that IS the input gradient of a
// stride-1 "same" convolution (dx = conv(dy, wt), taps mirrored, channel roles swapped).  With them the 3 x 3 input gradients run on
// the forward halo-tile kernel (conv_halo.h) instead of the transposed-operand gather.  One 64 x 64 (co, ci) tile of one tap per
// block, transposed through LDS; 16-byte loads along ci, 16-byte stores along co.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_weight_flip_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wt, int Cout, int Cin, int taps) {
  __shared__ bf16_t tile[64][64 + 8];          // [ci][co], rows padded by 16 B
  const int tap = blockIdx.z, co0 = blockIdx.y * 64, ci0 = blockIdx.x * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + 256 * it;            // 64 rows (co) x 8 chunks (ci)
    const int r = idx >> 3, ch = idx & 7;
    uint4_t v = {0u, 0u, 0u, 0u};
    if (co0 + r < Cout && ci0 + ch * 8 < Cin) v = *(const uint4_t*)(w + ((long)(co0 + r) * taps + tap) * Cin + ci0 + ch * 8);
    const bf16_t* e = (const bf16_t*)&v;
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[ch * 8 + k][r] = e[k];
  }
  __syncthreads();
  const int tflip = taps - 1 - tap;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + 256 * it;            // 64 rows (ci) x 8 chunks (co)
    const int r = idx >> 3, ch = idx & 7;
    if (ci0 + r < Cin && co0 + ch * 8 < Cout)
      *(uint4_t*)(wt + ((long)(ci0 + r) * taps + tflip) * Cout + co0 + ch * 8) = *(const uint4_t*)&tile[r][ch * 8];
  }
}
extern "C" int nk_conv_weight_flip(const void* w, void* wt, int Cout, int Cin, int taps, void* stream) {
  NK_CHECK_ARG(w && wt && Cout > 0 && Cin > 0 && taps > 0 && taps <= 65535);
  NK_CHECK_ARG((Cout & 7) == 0 && (Cin & 7) == 0);
  hipLaunchKernelGGL(conv_weight_flip_kernel, dim3((Cin + 63) / 64, (Cout + 63) / 64, taps), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w, (bf16_t*)wt,
                     Cout, Cin, taps);
  return nk_check_launch("conv_weight_flip_kernel");
}

// ------------------------------------------------------------------------------------------------
// conv3x3(nearest_upsample_2x(x)) as four 2 x 2 phase convolutions of x (ops_gemm.hip: nk_conv2d_up2_*).  Output row 2i + a reads the
// upsampled rows 2i + a + kh - 1 = low-resolution rows i + a - 1 + u: for a = 0, u = 0 holds tap kh = 0 and u = 1 taps {1, 2}; for a = 1,
// u = 0 holds {0, 1} and u = 1 tap 2 -- taps kh = (u ? 1 + a : 0) .. + (u ^ a); columns alike with (b, v, kw).
//   wp[a*2+b][co][u*2+v][ci] = the sum of the taps of w[co][3][3][ci] that fall on (u, v): fp32 sum, rounded once
//   wd[ci][r*4+s][co]        = wp[(r+1)&1][(s+1)&1][co][1-(r>>1)][1-(s>>1)][ci]: the 4 x 4 / stride 2 / padding 1 convolution of dy that is
//                              the input gradient (the same rounded values, channel roles swapped)
// One 64 x 64 (co, ci) tile of one (phase, u, v) per block, transposed through LDS like conv_weight_flip_kernel.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void up2_phase_weights_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wp, bf16_t* __restrict__ wd, int Cout,
                                                                int Cin) {
  __shared__ bf16_t tile[64][64 + 8];          // [ci][co], rows padded by 16 B
  const int z = blockIdx.z, co0 = blockIdx.y * 64, ci0 = blockIdx.x * 64;
  const int a = z >> 3, b = (z >> 2) & 1, u = (z >> 1) & 1, v = z & 1;
  const int kh0 = u ? 1 + a : 0, khn = 1 + (u ^ a), kw0 = v ? 1 + b : 0, kwn = 1 + (v ^ b);
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + 256 * it;            // 64 rows (co) x 8 chunks (ci)
    const int r = idx >> 3, ch = idx & 7;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool in = co0 + r < Cout && ci0 + ch * 8 < Cin;
    if (in) {
      for (int kh = kh0; kh < kh0 + khn; ++kh)
        for (int kw = kw0; kw < kw0 + kwn; ++kw) {
          float f[8];
          ew_load(w + ((long)(co0 + r) * 9 + kh * 3 + kw) * Cin + ci0 + ch * 8, f);
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[k] += f[k];
        }
    }
    const uint4_t o = pack8(acc);
    if (in) *(uint4_t*)(wp + (((long)(z >> 2) * Cout + co0 + r) * 4 + (z & 3)) * Cin + ci0 + ch * 8) = o;
    const bf16_t* e = (const bf16_t*)&o;
#pragma unroll
    for (int k = 0; k < 8; ++k) tile[ch * 8 + k][r] = e[k];
  }
  if (!wd) return;
  __syncthreads();
  const int tap = (2 * (1 - u) + (1 - a)) * 4 + 2 * (1 - v) + (1 - b);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + 256 * it;            // 64 rows (ci) x 8 chunks (co)
    const int r = idx >> 3, ch = idx & 7;
    if (ci0 + r < Cin && co0 + ch * 8 < Cout)
      *(uint4_t*)(wd + ((long)(ci0 + r) * 16 + tap) * Cout + co0 + ch * 8) = *(const uint4_t*)&tile[r][ch * 8];
  }
}
extern "C" int nk_up2_phase_weights(const void* w, void* wp, void* wd, int Cout, int Cin, void* stream) {
  NK_CHECK_ARG(w && wp && Cout > 0 && Cin > 0 && (Cout & 7) == 0 && (Cin & 7) == 0 && (Cout + 63) / 64 <= 65535);
  NK_CHECK_ARG(nk_aligned16(w) && nk_aligned16(wp) && nk_aligned16(wd));
  hipLaunchKernelGGL(up2_phase_weights_kernel, dim3((Cin + 63) / 64, (Cout + 63) / 64, 16), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w,
                     (bf16_t*)wp, (bf16_t*)wd, Cout, Cin);
  return nk_check_launch("up2_phase_weights_kernel");
}

// the four phase images [4][N][H][W][C] (phase a*2+b holds the pixels (2h + a, 2w + b)) <-> the image [N][2H][2W][C]; each runs over its output
struct PixelShuffle2x {
  const bf16_t* ph; bf16_t* y; int N, H, W, C;
  __device__ void operator()(long i, int n, int h, int w, int ch) const {
    const int p = (h & 1) * 2 + (w & 1);
    *(uint4_t*)(y + i * 8) = *(const uint4_t*)(ph + ((((long)p * N + n) * H + (h >> 1)) * W + (w >> 1)) * C + ch * 8);
  }
};
struct PixelUnshuffle2x {
  const bf16_t* y; bf16_t* ph; int N, H, W, C;
  __device__ void operator()(long i, int pn, int h, int w, int ch) const {
    const int p = pn / N, n = pn - p * N;
    *(uint4_t*)(ph + i * 8) = *(const uint4_t*)(y + (((long)n * 2 * H + 2 * h + (p >> 1)) * 2 * W + 2 * w + (p & 1)) * C + ch * 8);
  }
};
extern "C" int nk_pixel_shuffle2x(const void* phases, void* y, int N, int H, int W, int C, void* stream) {
  NK_CHECK_ARG(phases && y && N > 0 && H > 0 && W > 0 && C > 0 && (C & 7) == 0 && nk_aligned16(phases) && nk_aligned16(y));
  NK_CHECK_ARG(4l * N < (1l << 31) && 2l * H < (1l << 31) && 2l * W < (1l << 31));
  return nk_ew_pixels("pixel_shuffle2x", stream, N, 2 * H, 2 * W, C >> 3, PixelShuffle2x{(const bf16_t*)phases, (bf16_t*)y, N, H, W, C});
}
extern "C" int nk_pixel_unshuffle2x(const void* y, void* phases, int N, int H, int W, int C, void* stream) {
  NK_CHECK_ARG(phases && y && N > 0 && H > 0 && W > 0 && C > 0 && (C & 7) == 0 && nk_aligned16(phases) && nk_aligned16(y));
  NK_CHECK_ARG(4l * N < (1l << 31) && 2l * H < (1l << 31) && 2l * W < (1l << 31));
  return nk_ew_pixels("pixel_unshuffle2x", stream, 4 * N, H, W, C >> 3, PixelUnshuffle2x{(const bf16_t*)y, (bf16_t*)phases, N, H, W, C});
}

// the phase weight gradients dwp fp32 [4][Cout][4][Cin] back onto the nine taps: dw[co][kh][kw][ci] (+)= sum over the phases (a, b), in that
// fixed order, of dwp[a*2+b][co][(kh > a)*2 + (kw > b)][ci]; dbias[co] (+)= the four phases' bias gradients.  Four floats per item; the
// bias items follow the weight items.  accumulate: 1 = add to what is there, 0 / 2 = store (see nk_conv2d_wgrad)
struct Up2FoldWgrad {
  const float* dwp; const float* dbp; float* dw; float* dbias; int Cout, Cin, add; long nw;
  __device__ void operator()(long i) const {
    float4_t s = {0.f, 0.f, 0.f, 0.f};
    float* dst;
    if (i < nw) {
      const int c4 = Cin >> 2;
      const long row = i / c4;                 // co * 9 + tap
      const int ci = (int)(i - row * c4) * 4;
      const long co = row / 9;
      const int tap = (int)(row - co * 9), kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int uv = (kh > (p >> 1)) * 2 + (kw > (p & 1));
        s += *(const float4_t*)(dwp + (((long)p * Cout + co) * 4 + uv) * Cin + ci);
      }
      dst = dw + row * Cin + ci;
    } else {
      const long co = (i - nw) * 4;
#pragma unroll
      for (int p = 0; p < 4; ++p) s += *(const float4_t*)(dbp + (long)p * Cout + co);
      dst = dbias + co;
    }
    if (add) s += *(const float4_t*)dst;
    *(float4_t*)dst = s;
  }
};
extern "C" int nk_up2_fold_wgrad(const float* dwp, const float* dbias_p, float* dw, float* dbias, int Cout, int Cin, int accumulate, void* stream) {
  NK_CHECK_ARG(dwp && dw && Cout > 0 && Cin > 0 && (Cout & 7) == 0 && (Cin & 7) == 0 && accumulate >= 0 && accumulate <= 2);
  NK_CHECK_ARG((dbias == nullptr) == (dbias_p == nullptr));
  NK_CHECK_ARG(nk_aligned16(dwp) && nk_aligned16(dw) && nk_aligned16(dbias_p) && nk_aligned16(dbias));
  const long nw = (long)Cout * 9 * (Cin >> 2);
  return nk_ew_flat("up2_fold_wgrad", stream, nw + (dbias ? Cout >> 2 : 0), Up2FoldWgrad{dwp, dbias_p, dw, dbias, Cout, Cin, accumulate == 1, nw});
}

// ------------------------------------------------------------------------------------------------
// 3 x 3 / stride 1 / padding 1 convolution of an image with 3 or 4 REAL channels (stored padded to 8): the VAE's conv_in
// (modules/diffusion/model.py:519, 3 -> 128 at 1024^2) and the UNet's (openaimodel.py:622-624, 4 -> 320).  As an implicit GEMM with K = 72
// the gather kernel spent 1.5 ms decoding taps for a 1 GB output, and a plain FMA kernel (a thread = 4 output channels, 108 FMAs and 9 unpacked
// 16-byte loads per pixel) took 3.65 ms: VALU-bound.  Here K = (tap, 4 channels) = 36, padded to 64 = two v_mfma_f32_16x16x32_bf16 steps:
// a wave owns 128 output channels (their 16 weight fragments live in registers for the whole launch) and walks groups of 16 pixels; a lane
// fetches the two or three 8-byte (4-channel) taps its k-group covers straight from HBM/L2 into the A fragment -- no LDS, no unpacking --
// and the 16 x 128 outputs leave through the tile engine's permlane16_swap epilogue as 16-byte stores.  HBM-bound (the output).
// (Channel 3 of a 3-channel image is zero padding in x and in the channel-padded weights, so one kernel serves both.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv3x3_few_channels_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w, const float* __restrict__ bias,
                                                                   bf16_t* __restrict__ y, int N, int H, int W, int Cout, int groups_per_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int co_base = blockIdx.y * 128;
  // weight fragments: block b = output channels co_base + 16 b + r; k-step 0 holds taps 2g, 2g + 1; k-step 1 holds tap 8 (k-group 0 only)
  bf16x8_t wf[8][2];
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int co = co_base + b * 16 + r;
    uint2_t t0 = {0u, 0u}, t1 = {0u, 0u}, t8 = {0u, 0u};
    if (co < Cout) {
      t0 = *(const uint2_t*)(w + ((long)co * 9 + 2 * g) * 8);
      t1 = *(const uint2_t*)(w + ((long)co * 9 + 2 * g + 1) * 8);
      if (g == 0) t8 = *(const uint2_t*)(w + ((long)co * 9 + 8) * 8);
    }
    wf[b][0] = __builtin_bit_cast(bf16x8_t, (uint4_t){t0.x, t0.y, t1.x, t1.y});
    wf[b][1] = __builtin_bit_cast(bf16x8_t, (uint4_t){t8.x, t8.y, 0u, 0u});
  }
  // after the epilogue's row swap lane group g holds channels (g & 1) * 16 + (g >> 1) * 8 .. + 7 of each 32-channel pair
  const int nloc = (g & 1) * 16 + (g >> 1) * 8;
  float bv[4][8];
#pragma unroll
  for (int h = 0; h < 4; ++h)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int co = co_base + h * 32 + nloc + e;
      bv[h][e] = (bias && co < Cout) ? bias[co] : 0.f;
    }
  const long total = (long)N * H * W;
  const long gw = (long)blockIdx.x * 4 + wave;                 // this wave's first group of 16 pixels
  const int HW = H * W;
  // tap offsets of this lane's k-group
  const int ta = 2 * g, tb = 2 * g + 1;
  const int dya = ta / 3 - 1, dxa = ta % 3 - 1, dyb = tb / 3 - 1, dxb = tb % 3 - 1;

  auto fetch = [&](long grp, uint2_t& a, uint2_t& b, uint2_t& c) {
    a = (uint2_t){0u, 0u}; b = a; c = a;
    const long pix = grp * 16 + r;
    if (pix >= total) return;
    const int n = (int)(pix / HW);
    const int rem = (int)(pix - (long)n * HW);
    const int py = rem / W, px = rem - py * W;
    const bf16_t* img = x + (long)n * HW * 8;
    int yy = py + dya, xx = px + dxa;
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) a = *(const uint2_t*)(img + ((long)yy * W + xx) * 8);
    yy = py + dyb; xx = px + dxb;
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) b = *(const uint2_t*)(img + ((long)yy * W + xx) * 8);
    if (g == 0) {
      yy = py + 1; xx = px + 1;
      if (yy < H && xx < W) c = *(const uint2_t*)(img + ((long)yy * W + xx) * 8);
    }
  };

  const long gstride = (long)gridDim.x * 4;
  uint2_t na, nb, nc;
  long grp = gw;
  fetch(grp, na, nb, nc);
  for (int it = 0; it < groups_per_wave; ++it, grp += gstride) {
    if (grp * 16 >= total) break;
    const bf16x8_t x0 = __builtin_bit_cast(bf16x8_t, (uint4_t){na.x, na.y, nb.x, nb.y});
    const bf16x8_t x1 = __builtin_bit_cast(bf16x8_t, (uint4_t){nc.x, nc.y, 0u, 0u});
    if (it + 1 < groups_per_wave) fetch(grp + gstride, na, nb, nc);       // the next group's taps fly during this group's MFMAs and stores
    float4_t acc[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[b][0], x0, (float4_t){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[b][1], x1, acc[b], 0, 0, 0);
    }
    // acc[b][e] = y[pixel r][channel co_base + 16 b + 4 g + e]
    const long pix = grp * 16 + r;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a_own = acc[2 * h][e], b_own = acc[2 * h + 1][e];
        auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(a_own), __float_as_uint(b_own), false, false);
        v[e] = __uint_as_float(sw[0]) + bv[h][e];
        v[4 + e] = __uint_as_float(sw[1]) + bv[h][4 + e];
      }
      const int co = co_base + h * 32 + nloc;
      if (pix < total && co < Cout) *(uint4_t*)(y + pix * Cout + co) = pack8(v);
    }
  }
}
extern "C" int nk_conv3x3_few_channels_fwd(const void* x, const void* w, const float* bias, void* y, int N, int H, int W, int Cout, int cin_real,
                                           void* stream) {
  // x [N][H][W][8] bf16 (channels >= cin_real are zero padding), w [Cout][3][3][8] bf16 (likewise), y [N][H][W][Cout] bf16, bias [Cout] fp32 or NULL
  NK_CHECK_ARG(x && w && y && N > 0 && H > 0 && W > 0 && Cout > 0 && (Cout & 7) == 0);
  NK_CHECK_ARG(cin_real == 3 || cin_real == 4);
  NK_CHECK_ARG((long)N * H * W < (1l << 31));
  const long groups = ((long)N * H * W + 15) / 16;
  // a wave keeps 16 weight fragments in registers: at least 32 pixel groups per wave to amortise loading them, ~8 workgroups per CU
  long blocks = (groups + 4 * 32 - 1) / (4 * 32);
  if (blocks > 2048) blocks = 2048;
  const int per_wave = (int)((groups + blocks * 4 - 1) / (blocks * 4));
  dim3 grid((unsigned)blocks, (unsigned)((Cout + 127) / 128));
  hipLaunchKernelGGL(conv3x3_few_channels_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)w, bias, (bf16_t*)y, N, H, W, Cout,
                     per_wave);
  return nk_check_launch("conv3x3_few_channels_kernel");
}

extern "C" int nk_nchw_to_nhwc(const void* src, int src_is_f32, void* dst, int N, int C, int HW, int Cpad, float scale,
                               void* stream) {
  NK_CHECK_ARG(src && dst && N > 0 && C > 0 && HW > 0 && Cpad >= C);
  dim3 grid((HW + 31) / 32, (Cpad + 31) / 32, N);
  if (src_is_f32)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src,
                       (bf16_t*)dst, C, HW, Cpad, scale);
  else
    hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src,
                       (bf16_t*)dst, C, HW, Cpad, scale);
  return nk_check_launch("nchw_to_nhwc");
}
extern "C" int nk_nhwc_to_nchw(const void* src, void* dst, int dst_is_f32, int N, int C, int HW, int Cpad,
                               void* stream) {
  NK_CHECK_ARG(src && dst && N > 0 && C > 0 && HW > 0 && Cpad >= C);
  dim3 grid((HW + 31) / 32, (C + 31) / 32, N);
  if (dst_is_f32)
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src,
                       (float*)dst, C, HW, Cpad);
  else
    hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src,
                       (bf16_t*)dst, C, HW, Cpad);
  return nk_check_launch("nhwc_to_nchw");
}

// ---- casts ----------------------------------------------------------------------------------------
__global__ void cast_f32_bf16_kernel(const float* __restrict__ s, bf16_t* __restrict__ d, long n) {
  const long n8 = n >> 3;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const float4_t a = *(const float4_t*)(s + i * 8), b = *(const float4_t*)(s + i * 8 + 4);
    float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    *(uint4_t*)(d + i * 8) = pack8(f);
  }
  if (blockIdx.x == 0) for (long i = n8 * 8 + threadIdx.x; i < n; i += blockDim.x) d[i] = f2bf(s[i]);
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ s, float* __restrict__ d, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) d[i] = bf2f(s[i]);
}
extern "C" int nk_cast_f32_to_bf16(const float* src, void* dst, long n, void* stream) {
  NK_CHECK_ARG(src && dst && n > 0 && nk_aligned16(src) && nk_aligned16(dst));
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(nk_ew_grid((n >> 3) + 1)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, src,
                     (bf16_t*)dst, n);
  return nk_check_launch("cast_f32_to_bf16");
}
extern "C" int nk_cast_bf16_to_f32(const void* src, float* dst, long n, void* stream) {
  NK_CHECK_ARG(src && dst && n > 0);
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(nk_ew_grid(n)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream,
                     (const bf16_t*)src, dst, n);
  return nk_check_launch("cast_bf16_to_f32");
}

// ---- bias gradient: out[n] (+)= sum_m dy[m][n] ---------------------------------------------------
// stage 1: per-block partial column sums part[split][N] (no atomics); stage 2: single-writer reduce over splits.
// A block is 16 row lanes x 16 chunk lanes (a chunk = 8 channels = 16 B): every row lane reads 256 contiguous bytes, a
// thread keeps four rows' loads in flight, and with 64 rows per split even M = 4096 gives hundreds of blocks (the
// earlier one-row-at-a-time layout ran at 1-2 TB/s: 12 ms of GPU time per step for bias gradients alone).
__global__ __launch_bounds__(256) void colsum_partial_kernel(const bf16_t* __restrict__ dy, float* __restrict__ part, long M, int N,
                                                             long ld, int rows_per_block) {
  __shared__ float ps[16][16 * 8 + 4];  // [row lane][chunk lane * 8 + e], combined in a fixed order (bitwise reproducible)
  const int tid = threadIdx.x;
  const int cx = tid & 15, ry = tid >> 4;
  const int chunk = blockIdx.y * 16 + cx;
  const bool cok = chunk < (N >> 3);
  dy += (long)blockIdx.z * M * ld;                     // batched form: blockIdx.z = one of gridDim.z row blocks of M rows each
  part += (long)blockIdx.z * gridDim.x * N;
  const long row_lo = (long)blockIdx.x * rows_per_block;
  const long row_hi = row_lo + rows_per_block < M ? row_lo + rows_per_block : M;
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = 0.f;
  if (cok) {
    for (long base = row_lo + ry; base < row_hi; base += 64) {      // four rows' loads in flight per pass
      uint4_t v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long r = base + 16 * i;
        v[i] = r < row_hi ? *(const uint4_t*)(dy + r * ld + chunk * 8) : (uint4_t){0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float f[8];
        unpack8(v[i], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += f[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) ps[ry][cx * 8 + e] = s[e];
  __syncthreads();
  if (tid < 128) {
    const int c = blockIdx.y * 128 + tid;
    if (c < N) {
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += ps[r][tid];
      part[(long)blockIdx.x * N + c] = a;
    }
  }
}
__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                             int nsplit, int N, int accumulate) {
  // 64 columns x 16 row groups in the order of nk_reduce_rows; batched form: blockIdx.y = row block
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  part += (long)blockIdx.y * nsplit * N;
  out += (long)blockIdx.y * N;
  nk_reduce_rows<16, 64, 1, 0, 4>(
      c < N, nsplit, [&](int r, float* a) { a[0] += part[(long)r * N + c]; }, [&](const float* a) { out[c] = accumulate ? out[c] + a[0] : a[0]; });
}
// sizes, split and launches: norm_plan.h (nk_colsum_plan)
extern "C" long nk_colsum_ws_floats(long M, int N) { return nk_colsum_plan(M, N, 1).ws_floats; }
extern "C" int nk_colsum_batched(const void* dy, float* out, float* ws, long M, int N, long ld, int nbatch, int accumulate, void* stream_) {
  // out[b][N] (+)= column sums of rows [b*M, (b+1)*M) of dy, b < nbatch, in ONE pair of launches (ws: nbatch x nk_colsum_ws_floats(M, N))
  hipStream_t stream = (hipStream_t)stream_;
  const NkColsumPlan p = nk_colsum_plan(M, N, nbatch);
  NORM_PLAN_OR_RETURN(p);
  NK_CHECK_ARG(dy && out && ws && (ld & 7) == 0);
  // while the launch log is on, each launch's plan line follows its name, as behind a tile-engine launch: what plan-only mode logs is
  // what a logged launch logs (tests/test_gemm_exact_gpu.py compares the two)
  char line[192];
  for (int i = 0; i < 2; ++i) {
    if (i == 0) NORM_LAUNCH(p.launch[0], colsum_partial_kernel, (const bf16_t*)dy, ws + p.part.off, M, N, ld, p.rows_per_block);
    else NORM_LAUNCH(p.launch[1], colsum_reduce_kernel, ws + p.part.off, out, p.nsplit, N, accumulate);
    if (int e = nk_check_launch(p.launch[i].name)) return e;
    if (nk_launch_log_mode()) { nk_norm_plan_line(p, i, line, sizeof(line)); nk_launch_log_add(nullptr, line); }
  }
  return NK_OK;
}
extern "C" int nk_colsum(const void* dy, float* out, float* ws, long M, int N, long ld, int accumulate, void* stream) {
  return nk_colsum_batched(dy, out, ws, M, N, ld, 1, accumulate, stream);
}

// ---- sinusoidal timestep embedding (modules/diffusion/util.py:152-177): [cos | sin] -------------
__global__ void timestep_embedding_kernel(const float* __restrict__ t, bf16_t* __restrict__ out, int B, int dim,
                                          float max_period) {
  const int half = dim >> 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * dim; i += gridDim.x * blockDim.x) {
    int b = i / dim, j = i - b * dim;
    float v = 0.f;
    if (j < 2 * half) {
      int k = j < half ? j : j - half;
      float freq = expf(-logf(max_period) * (float)k / (float)half);
      float arg = t[b] * freq;
      v = j < half ? cosf(arg) : sinf(arg);
    }
    out[i] = f2bf(v);
  }
}
extern "C" int nk_timestep_embedding(const float* t, void* out, int B, int dim, float max_period, void* stream) {
  NK_CHECK_ARG(t && out && B > 0 && dim > 0);
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((B * dim + 255) / 256), dim3(256), 0, (hipStream_t)stream, t,
                     (bf16_t*)out, B, dim, max_period);
  return nk_check_launch("timestep_embedding");
}

// ---- row softmax in place on bf16 [M][L] (unfused d=512 VAE mid attention, model.py:224-243) ----
__global__ __launch_bounds__(256) void softmax_rows_kernel(bf16_t* __restrict__ s, long M, int L) {
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    bf16_t* p = s + row * L;
    float mx = -INFINITY;
    for (int i = tid * 8; i < L; i += 256 * 8) {
      float f[8];
      unpack8(*(const uint4_t*)(p + i), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, f[e]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int i = tid * 8; i < L; i += 256 * 8) {
      float f[8];
      unpack8(*(const uint4_t*)(p + i), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += __expf(f[e] - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
    for (int i = tid * 8; i < L; i += 256 * 8) {
      float f[8];
      unpack8(*(const uint4_t*)(p + i), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = __expf(f[e] - mx) * inv;
      *(uint4_t*)(p + i) = pack8(f);
    }
    __syncthreads();
  }
}
// The same for rows of up to 16 384 elements (the SD VAE's 128 x 128 mid block at 1024^2, and everything smaller): a row is held in the
// block's registers between its one read and its one write -- 2 bytes in, 2 out per element where the general kernel reads the row three
// times (1.59 GB fetched per 0.54 GB score matrix: profiles/r03_pmc_summary.csv).
template <int NPT>     // 16-byte pieces per thread: L <= NPT * 2048
__global__ __launch_bounds__(256) void softmax_rows_reg_kernel(bf16_t* __restrict__ s, long M, int L) {
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    bf16_t* p = s + row * L;
    uint4_t v[NPT];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int i = (j * 256 + tid) * 8;
      v[j] = (uint4_t){0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};     // -inf: exp -> 0 past the end of the row
      if (i < L) v[j] = *(const uint4_t*)(p + i);
    }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      float f[8];
      unpack8(v[j], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) mx = fmaxf(mx, f[e]);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      float f[8];
      unpack8(v[j], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += __expf(f[e] - mx);
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int i = (j * 256 + tid) * 8;
      float f[8];
      unpack8(v[j], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = __expf(f[e] - mx) * inv;
      if (i < L) *(uint4_t*)(p + i) = pack8(f);
    }
    __syncthreads();
  }
}
extern "C" int nk_softmax_rows(void* s, long M, int L, void* stream) {
  NK_CHECK_ARG(s && M > 0 && L > 0 && (L & 7) == 0);
  const dim3 grid((int)(M < 8192 ? M : 8192));
  if (L <= 4096) hipLaunchKernelGGL(softmax_rows_reg_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)s, M, L);
  else if (L <= 8192) hipLaunchKernelGGL(softmax_rows_reg_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)s, M, L);
  else if (L <= 16384) hipLaunchKernelGGL(softmax_rows_reg_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)s, M, L);
  else hipLaunchKernelGGL(softmax_rows_kernel, dim3((int)(M < 4096 ? M : 4096)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)s, M, L);
  return nk_check_launch("softmax_rows");
}

// ---- backward of the row softmax, in place on dp: ds = p * (dp - sum_j dp*p) * scale ---------------
// (the VAE mid-block attention when the VAE itself is trained: its probabilities are kept from the forward pass)
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const bf16_t* __restrict__ p, bf16_t* __restrict__ dp, long M, int L,
                                                               float scale) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (long row = blockIdx.x; row < M; row += gridDim.x) {
    const bf16_t* pr = p + row * L;
    bf16_t* dr = dp + row * L;
    float dot = 0.f;
    for (int i = tid * 8; i < L; i += 256 * 8) {
      float a[8], b[8];
      unpack8(*(const uint4_t*)(pr + i), a);
      unpack8(*(const uint4_t*)(dr + i), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) dot += a[e] * b[e];
    }
    dot = wave_sum(dot);
    if (lane == 0) red[wave] = dot;
    __syncthreads();
    dot = red[0] + red[1] + red[2] + red[3];
    for (int i = tid * 8; i < L; i += 256 * 8) {
      float a[8], b[8];
      unpack8(*(const uint4_t*)(pr + i), a);
      unpack8(*(const uint4_t*)(dr + i), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = a[e] * (b[e] - dot) * scale;
      *(uint4_t*)(dr + i) = pack8(b);
    }
    __syncthreads();
  }
}
extern "C" int nk_softmax_rows_bwd(const void* p, void* dp, long M, int L, float scale, void* stream) {
  NK_CHECK_ARG(p && dp && M > 0 && L > 0 && (L & 7) == 0);
  hipLaunchKernelGGL(softmax_rows_bwd_kernel, dim3((int)(M < 4096 ? M : 4096)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)p,
                     (bf16_t*)dp, M, L, scale);
  return nk_check_launch("softmax_rows_bwd");
}

// ---- EDM noising + preconditioning (loss.py:117-140, denoiser.py:41-49) -------------------------
// z_t = x + sigma*eps (fp32, NCHW) ; net_in = bf16 channels-last (z_t * c_in), channels padded to Cpad
// One latent element, shared by both prepare kernels so that the compiler contracts the two expressions the same way in each:
// stores z_t, returns the (fp32) network input.
__device__ __forceinline__ float edm_noise_scale(float x, float eps, float sg, float ci, float* __restrict__ zt) {
  const float z = x + sg * eps;
  *zt = z;
  return z * ci;
}
__global__ void edm_prepare_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                   const float* __restrict__ sigma, const float* __restrict__ c_in,
                                   float* __restrict__ zt, bf16_t* __restrict__ net_in, int B, int C, int HW, int Cpad) {
  const long total = (long)B * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    int b = (int)(i / HW);
    int p = (int)(i - (long)b * HW);
    const float sg = sigma[b], ci = c_in[b];
    for (int c = 0; c < Cpad; ++c) {
      float v = 0.f;
      if (c < C) {
        long o = ((long)b * C + c) * HW + p;
        v = edm_noise_scale(x[o], eps[o], sg, ci, zt + o);
      }
      net_in[i * Cpad + c] = f2bf(v);
    }
  }
}
// The same with channel-concat conditioning (OpenAIWrapper.forward, modules/diffusion/wrappers.py:33: the denoiser scales the latents,
// the wrapper joins `extra` behind them UNSCALED): net_in[b][p][c] = bf16(z_t*c_in) for c < C, bf16(extra[b][c-C][p]) for
// C <= c < C+Ce, 0 up to Cpad.  extra: fp32 NCHW [B][Ce][HW].  One thread per pixel, NCHW reads coalesced across pixels, the
// token side one 16-byte vector per 8 channels (Cpad % 8 == 0).
__global__ __launch_bounds__(NK_EW_THREADS) void edm_prepare_cat_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                                     const float* __restrict__ sigma, const float* __restrict__ c_in,
                                                                     const float* __restrict__ extra, float* __restrict__ zt,
                                                                     bf16_t* __restrict__ net_in, int B, int C, int Ce, int HW, int Cpad) {
  const long total = (long)B * HW;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / HW);
    const int p = (int)(i - (long)b * HW);
    const float sg = sigma[b], ci = c_in[b];
    for (int c0 = 0; c0 < Cpad; c0 += 8) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        f[e] = 0.f;
        if (c < C) {
          const long o = ((long)b * C + c) * HW + p;
          f[e] = edm_noise_scale(x[o], eps[o], sg, ci, zt + o);
        } else if (c < C + Ce) {
          f[e] = extra[((long)b * Ce + (c - C)) * HW + p];
        }
      }
      *(uint4_t*)(net_in + i * Cpad + c0) = pack8(f);
    }
  }
}
extern "C" int nk_edm_prepare(const float* x, const float* eps, const float* sigma, const float* c_in, float* zt,
                              void* net_in, int B, int C, int HW, int Cpad, void* stream) {
  NK_CHECK_ARG(x && eps && sigma && c_in && zt && net_in && B > 0 && C > 0 && HW > 0 && Cpad >= C);
  hipLaunchKernelGGL(edm_prepare_kernel, dim3(nk_ew_grid((long)B * HW)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, x,
                     eps, sigma, c_in, zt, (bf16_t*)net_in, B, C, HW, Cpad);
  return nk_check_launch("edm_prepare");
}
extern "C" int nk_edm_prepare_cat(const float* x, const float* eps, const float* sigma, const float* c_in, const float* extra,
                                  float* zt, void* net_in, int B, int C, int Ce, int HW, int Cpad, void* stream) {
  NK_CHECK_ARG(x && eps && sigma && c_in && zt && net_in && B > 0 && C > 0 && HW > 0 && Ce >= 0 && (extra || Ce == 0));
  NK_CHECK_ARG(Cpad >= C + Ce && (Cpad & 7) == 0 && Cpad - (C + Ce) < 8);
  hipLaunchKernelGGL(edm_prepare_cat_kernel, dim3(nk_ew_grid((long)B * HW)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, x,
                     eps, sigma, c_in, extra, zt, (bf16_t*)net_in, B, C, Ce, HW, Cpad);
  return nk_check_launch("edm_prepare_cat");
}

// ---- EDM loss forward + its gradient w.r.t. the network output (loss.py:142-157, functions.py:91-94)
// D = net_out*c_out + z_t*c_skip ; loss[b] = w[b] * mean_chw((D - target)^2)
// dnet = upstream * w[b] * 2/(C*HW) * (D - target) * c_out       (bf16 channels-last, padded channels = 0)
// one workgroup per sample (the latents are MB-sized): a fixed-order reduction keeps the loss bit-reproducible
__global__ __launch_bounds__(1024) void edm_loss_kernel(const bf16_t* __restrict__ net_out, const float* __restrict__ zt,
                                                        const float* __restrict__ target, const float* __restrict__ c_out,
                                                        const float* __restrict__ c_skip, const float* __restrict__ w,
                                                        float* __restrict__ loss, bf16_t* __restrict__ dnet, int B, int C,
                                                        int HW, int Cpad, float upstream) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const float co = c_out[b], cs = c_skip[b], wb = w[b];
  const float inv_cnt = 1.0f / ((float)C * (float)HW);
  const float gscale = upstream * wb * 2.0f * inv_cnt * co;
  float acc = 0.f;
  for (int p = threadIdx.x; p < HW; p += blockDim.x) {
    for (int c = 0; c < Cpad; ++c) {
      float g = 0.f;
      if (c < C) {
        long o = ((long)b * C + c) * HW + p;
        float D = bf2f(net_out[((long)b * HW + p) * Cpad + c]) * co + zt[o] * cs;
        float diff = D - target[o];
        acc += diff * diff;
        g = diff * gscale;
      }
      if (dnet) dnet[((long)b * HW + p) * Cpad + c] = f2bf(g);
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    loss[b] = t * inv_cnt * wb;
  }
}
extern "C" int nk_edm_loss(const void* net_out, const float* zt, const float* target, const float* c_out,
                           const float* c_skip, const float* w, float* loss, void* dnet, int B, int C, int HW, int Cpad,
                           float upstream, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  NK_CHECK_ARG(net_out && zt && target && c_out && c_skip && w && loss && B > 0 && C > 0 && HW > 0 && Cpad >= C);
  hipLaunchKernelGGL(edm_loss_kernel, dim3(B), dim3(1024), 0, stream, (const bf16_t*)net_out, zt, target, c_out,
                     c_skip, w, loss, (bf16_t*)dnet, B, C, HW, Cpad, upstream);
  return nk_check_launch("edm_loss");
}

// ---- flat fused AdamW over the whole parameter buffer; also refreshes the bf16 shadow ----------
__global__ void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, bf16_t* __restrict__ shadow, long n, float lr, float b1,
                                  float b2, float eps, float wd, float bc1, float bc2, float gscale, const unsigned* health) {
  if (*(const volatile unsigned*)health) return;     // a flagged backward: leave masters, moments and shadows untouched
  const long n4 = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4_t pp = *(float4_t*)(p + i * 4);
    const float4_t gg = *(const float4_t*)(g + i * 4);
    float4_t mm = *(float4_t*)(m + i * 4), vv = *(float4_t*)(v + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float gr = gg[e] * gscale;
      mm[e] = b1 * mm[e] + (1.f - b1) * gr;
      vv[e] = b2 * vv[e] + (1.f - b2) * gr * gr;
      float upd = (mm[e] / bc1) / (sqrtf(vv[e] / bc2) + eps);
      pp[e] = pp[e] * (1.f - lr * wd) - lr * upd;
    }
    *(float4_t*)(p + i * 4) = pp;
    *(float4_t*)(m + i * 4) = mm;
    *(float4_t*)(v + i * 4) = vv;
    uint2_t s;
    s.x = pack2bf(pp[0], pp[1]);
    s.y = pack2bf(pp[2], pp[3]);
    *(uint2_t*)(shadow + i * 4) = s;
  }
}
extern "C" int nk_adamw_flat(float* p, const float* g, float* m, float* v, void* shadow, long n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
  NK_CHECK_ARG(p && g && m && v && shadow && n > 0 && (n & 3) == 0 && step >= 1);
  if (int e = nk_health_poll()) return e;
  const unsigned* health = nk_health_word();
  if (!health) { nk_set_error(__FILE__, __LINE__, "health word allocation failed"); return NK_ERR_LAUNCH; }
  float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adamw_flat_kernel, dim3(nk_ew_grid(n >> 2)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, p, g, m, v,
                     (bf16_t*)shadow, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, health);
  if (int e = nk_check_launch("adamw_flat")) return e;
  nk_health_snapshot((hipStream_t)stream);
  return NK_OK;
}
