// Fused multi-tensor Adafactor over the flat parameter / gradient buffers.
// Replaces the reference's per-tensor Python loop (`optimizers/adafactor.py:162-255`: ~1 700 tensors x ~15 small kernels,
// `_approx_sq_grad` :154-159, `_rms` :150-151, `_get_lr` :133-147) with three launches per CHUNK of tensors:
//
//   A  statistics   matrices: row / column partial sums of g^2+eps per 256x64 tile; the last tile of a strip turns them into the row /
//                   column EMAs and a partial sum of the row EMA (its mean).
//                   conv (factored over the 3x3 taps of every (o,i) pair, as the reference's rule "last two dims" implies
//                   for OIHW weights) and vectors: state update and u = g / sqrt(v) in one go, partial sum of u^2; the last block of the
//                   tensor turns the sums into its step size (below)
//   B  matrices     partial sum of u^2,  u = g * rsqrt(row_i / mean_row) * rsqrt(col_j); the tensor's last block: RMS(u) -> clip
//                   denominator, RMS(p) -> relative step size, scale = lr / denominator
//   C  apply        p -= wd*lr*p + scale*u ; bf16 shadow rewritten ; partial sum of p^2 (next step's RMS(p))
//
// A chunk is a run of consecutive tensors (host-chosen size).  Per parameter the passes move g three times, p once in and once
// out and the bf16 shadow out: 22 B against fused AdamW's 30, and no m / v buffers (-20 GB for the SDXL UNet).  Every launch of a chunk
// depends on the one before, each with its ramp and tail, while the second and third read of a chunk's gradients only stay in the 256 MB
// Infinity Cache for small chunks: the default chunk is 128 MB (NK_AF_CHUNK_MB).  Every reduction goes through per-tile
// partials combined in a fixed order: no atomics on values, bitwise reproducible.  The tile walk, the strip finish, the conv pairs and the
// vector loop are optim_common.h's, shared with CAME.
//
// First moment (beta1, reference adafactor.py:194-196, 242-245; nk_adafactor_chunk_momentum): passes A and B as above, then pass C as
// af_apply_momentum_kernel, which keeps m = beta1*m + (1-beta1)*scale*u per element and applies p -= wd*lr*p + m.  m is one flat fp32 buffer
// with the masters' layout and offsets, read and written once in pass C: 22 B of that pass against 14, 30 B per parameter and step against
// 22, and 4 B of state per parameter (+10.3 GB for the SDXL UNet).  It is a kernel of its own and not a template parameter of
// af_apply_kernel: as one template the momentum-free instantiation came out of the compiler with another schedule (packed multiplies,
// other registers), and that pass is the benchmark's.
#include "../../include/neurosis_hip.h"
#include "nk_common.h"
#include "optim_common.h"

struct NkAfTensor {      // mirrored by neurosis_amd/optim.py (AF_TENSOR_DTYPE); 80 bytes
  long off;              // element offset of the tensor in master / grad / shadow
  long row_off;          // matrix: row EMA [d0]; conv: [O][KH][I]; vector: full second moment [numel]   (offset in `state`)
  long col_off;          // matrix: col EMA [d1]; conv: [O][KW][I]
  long ws_row;           // matrix: row partials [ntc][d0], offset in the chunk workspace
  long ws_col;           // matrix: col partials [ntr][d1]
  int kind;              // 0 vector, 1 matrix [d0][d1], 2 conv stored [O=d0][KH][KW][I=d1]
  int d0, d1;
  int kh, kw;
  int item0, nitems;     // this tensor's range in the item table
  int mr0;               // matrix: first slot of its row-EMA partial sums (one per 256-row strip) in `mean_row`
  int cnt0;              // first of this tensor's "blocks done" counters: [0] the tensor's, matrices: [1 + tr] row strips, [1 + ntr + tc] column strips
  int pad;
};
static_assert(sizeof(NkAfTensor) == 80, "mirrored by neurosis_amd/optim.py");

struct NkAfArgs {
  float* master; const float* grad; bf16_t* shadow; float* state; float* ws;
  const NkAfTensor* tensors; const NkAfItem* items;
  float* u2_part;      // [nitems] partial sums of u^2
  float* p2_part;      // [nitems] partial sums of p^2 after the update (read by the NEXT step's F2)
  float* mean_row;     // per matrix: one partial sum of the row EMA per 256-row strip (slots mr0...)
  unsigned* counters;  // "blocks done" counters (zero before the step; every one is back at zero when its last block has passed)
  float* scale;        // [ntensors] lr / max(1, rms(u)/clip)
  float* lr_t;         // [ntensors]
  int item_lo, item_hi, tensor_lo, tensor_hi;
  float beta2t, eps1, eps2, clip, rel_step, weight_decay, grad_scale;
  int scale_parameter;
  const unsigned* health;   // backward-health word (errors.hip): non-zero -> every kernel of the step returns at once
};

// conv weights, pass C
template <class CV>
__device__ __forceinline__ float af_conv_apply(const NkAfArgs& a, const NkAfTensor& t, const CV& cv, int tr, int tid, float gs, float sc, float decay) {
  float acc = 0.f;
  fac_for_pairs(tr, tid, t.d0, t.d1, [&](int o, int i) {
    float g[3][3], row[3], col[3], f[3][3];
    fac_conv_load(cv, a.state, t.row_off, t.col_off, o, i, row, col);
    cv.taps([&](int x, int y) { g[x][y] = a.grad[t.off + cv.tap(o, i, x, y)] * gs; });
    fac_conv_factor(cv, row, col, f);
    cv.taps([&](int x, int y) {
      const long e = t.off + cv.tap(o, i, x, y);
      const float pn = a.master[e] * decay - sc * (f[x][y] * g[x][y]);
      a.master[e] = pn;
      a.shadow[e] = f2bf(pn);
      acc += pn * pn;
    });
  });
  return acc;
}

// one tensor's step size from its items' partial sums (RMS(u) -> clip denominator, RMS(p) -> relative step size)
__device__ __forceinline__ void af_tensor_scale(const NkAfArgs& a, const NkAfTensor& t, int ti, int tid, float* red) {
  float su = 0.f, sp = 0.f;
  for (int i = tid; i < t.nitems; i += 256) {
    su += AF_FETCH(a.u2_part + t.item0 + i);       // (this launch's blocks)
    sp += a.p2_part[t.item0 + i];                  // (an earlier launch: the previous step's apply pass)
  }
  su = block_sum_256(su, red);
  sp = block_sum_256(sp, red);
  if (tid == 0) {
    const float numel = af_tensor_numel(t.kind, t.d0, t.d1, t.kh, t.kw);
    const float rms_u = sqrtf(su / numel);
    const float denom = fmaxf(1.0f, rms_u / a.clip);
    const float rms_p = sqrtf(sp) / sqrtf(numel);
    const float lr = (a.scale_parameter ? fmaxf(a.eps2, rms_p) : 1.0f) * a.rel_step;
    a.lr_t[ti] = lr;
    a.scale[ti] = lr / denom;
  }
}

__global__ __launch_bounds__(256) void af_stats_kernel(const NkAfArgs a) {
  AF_HEALTH_GATE(a);
  __shared__ FacStatsLds L;
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkAfTensor t = a.tensors[it.tensor];
  const int tid = threadIdx.x;
  const float gs = a.grad_scale;
  if (t.kind == 1) {
    const FacTile T(it, t.d0, t.d1, tid);
    float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int i0 = 0; i0 < AF_TR / 16; i0 += 4) {
      float4_t g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) g[u] = T.load(a.grad + t.off, T.row(i0 + u));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool ok = T.ok(T.row(i0 + u));
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float gg = g[u][e] * gs;
          v[e] = ok ? gg * gg + a.eps1 : 0.f;
        }
        fac_tile_add_row(T, L, cs, i0 + u, v);
      }
    }
    fac_strip_finish(a, t, it, T, L, cs, tid, a.beta2t, 1.0f - a.beta2t, t.row_off, t.col_off, t.mr0);
    return;
  }
  float acc = 0.f;
  if (t.kind == 2) {
    fac_conv_dispatch(t, [&](auto cv) { acc = fac_conv_stats(a, t, cv, it.tr, tid, t.row_off, t.col_off, a.beta2t, 1.0f - a.beta2t); });
  } else {
    fac_for_elems(it.tr, tid, t.d0, [&](long e) {
      const float g = a.grad[t.off + e] * gs;
      float* st = a.state + t.row_off + e;
      const float v = fac_ema(*st, a.beta2t, g * g + a.eps1, 1.0f - a.beta2t);
      *st = v;
      const float u = g * rsqrtf(v);
      acc += u * u;
    });
  }
  acc = block_sum_256(acc, L.red);
  if (tid == 0) AF_PUBLISH(a.u2_part + a.item_lo + blockIdx.x, acc);
  // convolutions and vectors have their update's RMS now: the last block of the tensor turns it into the step size
  if (af_last_block(a.counters + t.cnt0, (unsigned)t.nitems, tid, &L.flag[0])) af_tensor_scale(a, t, it.tensor, tid, L.red);
}

// matrices: partial sum of u^2 per tile
__global__ __launch_bounds__(256) void af_u2_kernel(const NkAfArgs a) {
  AF_HEALTH_GATE(a);
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkAfTensor t = a.tensors[it.tensor];
  if (t.kind != 1) return;
  fac_matrix_u2(a, t, it, t.row_off, t.col_off, [&](int tid, float* red) { af_tensor_scale(a, t, it.tensor, tid, red); });
}

__global__ __launch_bounds__(256) void af_apply_kernel(const NkAfArgs a) {
  AF_HEALTH_GATE(a);
  __shared__ float red[4];
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkAfTensor t = a.tensors[it.tensor];
  const int tid = threadIdx.x;
  const float gs = a.grad_scale;
  const float sc = a.scale[it.tensor];
  const float decay = 1.0f - a.weight_decay * a.lr_t[it.tensor];
  float acc = 0.f;
  if (t.kind == 1) {
    const FacTile T(it, t.d0, t.d1, tid);
    const float mr = fac_mean_slots(a.mean_row, t.mr0, t.d0);
    float ci[4];
    T.col_factors(a.state + t.col_off, ci);
#pragma unroll 1
    for (int i0 = 0; i0 < AF_TR / 16; i0 += 4) {
      float4_t g[4], p[4];
      float rf[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = T.row(i0 + u);
        const bool ok = T.ok(r);
        const long o = t.off + T.at(r);
        g[u] = T.load(ok, a.grad + o);
        p[u] = T.load(ok, a.master + o);
        rf[u] = ok ? rsqrtf(a.state[t.row_off + r] / mr) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = T.row(i0 + u);
        if (!T.ok(r)) continue;
        float4_t pn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pn[e] = p[u][e] * decay - sc * (rf[u] * ci[e] * (g[u][e] * gs));
          acc += pn[e] * pn[e];
        }
        T.store(a.master, a.shadow, t.off, r, pn);
      }
    }
  } else if (t.kind == 2) {
    fac_conv_dispatch(t, [&](auto cv) { acc = af_conv_apply(a, t, cv, it.tr, tid, gs, sc, decay); });
  } else {
    fac_for_elems(it.tr, tid, t.d0, [&](long e) {
      const float g = a.grad[t.off + e] * gs;
      const float u = g * rsqrtf(a.state[t.row_off + e]);
      const float pn = a.master[t.off + e] * decay - sc * u;
      a.master[t.off + e] = pn;
      a.shadow[t.off + e] = f2bf(pn);
      acc += pn * pn;
    });
  }
  acc = block_sum_256(acc, red);
  if (tid == 0) a.p2_part[a.item_lo + blockIdx.x] = acc;
}

// ---- pass C with the first moment: m = beta1 m + (1 - beta1) scale u,  p = p decay - m -------------------------------------------------
struct AfMoment { float* m; float b1, omb1; };      // the buffer (the masters' layout and offsets), beta1 and 1 - beta1

template <class CV>
__device__ __forceinline__ float af_conv_apply_momentum(const NkAfArgs& a, const AfMoment& mo, const NkAfTensor& t, const CV& cv, int tr, int tid, float gs,
                                                        float sc, float decay) {
  float acc = 0.f;
  fac_for_pairs(tr, tid, t.d0, t.d1, [&](int o, int i) {
    float g[3][3], row[3], col[3], f[3][3];
    fac_conv_load(cv, a.state, t.row_off, t.col_off, o, i, row, col);
    cv.taps([&](int x, int y) { g[x][y] = a.grad[t.off + cv.tap(o, i, x, y)] * gs; });
    fac_conv_factor(cv, row, col, f);
    cv.taps([&](int x, int y) {
      const long e = t.off + cv.tap(o, i, x, y);
      const float mn = fac_ema(mo.m[e], mo.b1, sc * (f[x][y] * g[x][y]), mo.omb1);
      const float pn = a.master[e] * decay - mn;
      mo.m[e] = mn;
      a.master[e] = pn;
      a.shadow[e] = f2bf(pn);
      acc += pn * pn;
    });
  });
  return acc;
}

__global__ __launch_bounds__(256) void af_apply_momentum_kernel(const NkAfArgs a, const AfMoment mo) {
  AF_HEALTH_GATE(a);
  __shared__ float red[4];
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkAfTensor t = a.tensors[it.tensor];
  const int tid = threadIdx.x;
  const float gs = a.grad_scale;
  const float sc = a.scale[it.tensor];
  const float decay = 1.0f - a.weight_decay * a.lr_t[it.tensor];
  float acc = 0.f;
  if (t.kind == 1) {
    const FacTile T(it, t.d0, t.d1, tid);
    const float mr = fac_mean_slots(a.mean_row, t.mr0, t.d0);
    float ci[4];
    T.col_factors(a.state + t.col_off, ci);
#pragma unroll 1
    for (int i0 = 0; i0 < AF_TR / 16; i0 += 4) {
      float4_t g[4], p[4], m[4];
      float rf[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = T.row(i0 + u);
        const bool ok = T.ok(r);
        const long o = t.off + T.at(r);
        g[u] = T.load(ok, a.grad + o);
        p[u] = T.load(ok, a.master + o);
        m[u] = T.load(ok, mo.m + o);
        rf[u] = ok ? rsqrtf(a.state[t.row_off + r] / mr) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = T.row(i0 + u);
        if (!T.ok(r)) continue;
        float4_t pn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          m[u][e] = fac_ema(m[u][e], mo.b1, sc * (rf[u] * ci[e] * (g[u][e] * gs)), mo.omb1);
          pn[e] = p[u][e] * decay - m[u][e];
          acc += pn[e] * pn[e];
        }
        *(float4_t*)(mo.m + t.off + T.at(r)) = m[u];
        T.store(a.master, a.shadow, t.off, r, pn);
      }
    }
  } else if (t.kind == 2) {
    fac_conv_dispatch(t, [&](auto cv) { acc = af_conv_apply_momentum(a, mo, t, cv, it.tr, tid, gs, sc, decay); });
  } else {
    fac_for_elems(it.tr, tid, t.d0, [&](long e) {
      const float g = a.grad[t.off + e] * gs;
      const float u = g * rsqrtf(a.state[t.row_off + e]);
      const float mn = fac_ema(mo.m[t.off + e], mo.b1, sc * u, mo.omb1);
      const float pn = a.master[t.off + e] * decay - mn;
      mo.m[t.off + e] = mn;
      a.master[t.off + e] = pn;
      a.shadow[t.off + e] = f2bf(pn);
      acc += pn * pn;
    });
  }
  acc = block_sum_256(acc, red);
  if (tid == 0) a.p2_part[a.item_lo + blockIdx.x] = acc;
}

// partial sums of p^2 for the FIRST step (afterwards pass C leaves them behind); the item partition is pass C's
__global__ __launch_bounds__(256) void af_init_p2_kernel(const NkAfArgs a) {
  __shared__ float red[4];
  const NkAfItem it = a.items[a.item_lo + blockIdx.x];
  const NkAfTensor t = a.tensors[it.tensor];
  const int tid = threadIdx.x;
  float acc = 0.f;
  if (t.kind == 1) {
    const FacTile T(it, t.d0, t.d1, tid);
    for (int i = 0; i < AF_TR / 16; ++i) {
      const int r = T.row(i);
      if (T.ok(r)) {
        const float4_t p = T.load(a.master + t.off, r);
        acc += p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
      }
    }
  } else if (t.kind == 2) {
    // (an item's pairs are a strided set of elements; summing p^2 needs no pairing, only the same partition)
    const int taps = t.kh * t.kw, I = t.d1;
    fac_for_pairs(it.tr, tid, t.d0, I, [&](int o, int i) {
      for (int x = 0; x < taps; ++x) { const float p = a.master[t.off + ((long)o * taps + x) * I + i]; acc += p * p; }
    });
  } else {
    fac_for_elems(it.tr, tid, t.d0, [&](long e) { const float p = a.master[t.off + e]; acc += p * p; });
  }
  acc = block_sum_256(acc, red);
  if (tid == 0) a.p2_part[a.item_lo + blockIdx.x] = acc;
}

static int af_check(const NkAdafactorArgs* h) {
  NK_CHECK_ARG(h && h->master && h->grad && h->shadow && h->state && h->ws && h->tensors && h->items);
  NK_CHECK_ARG(h->u2_part && h->p2_part && h->mean_row && h->scale && h->lr_t && h->counters);
  NK_CHECK_ARG(h->item_hi > h->item_lo && h->tensor_hi > h->tensor_lo);
  return NK_OK;
}
static NkAfArgs af_args(const NkAdafactorArgs* h) {      // (all but the health word)
  NkAfArgs a;
  a.master = h->master; a.grad = h->grad; a.shadow = (bf16_t*)h->shadow; a.state = h->state; a.ws = h->ws;
  a.tensors = (const NkAfTensor*)h->tensors; a.items = (const NkAfItem*)h->items;
  a.u2_part = h->u2_part; a.p2_part = h->p2_part; a.mean_row = h->mean_row; a.scale = h->scale; a.lr_t = h->lr_t;
  a.counters = h->counters;
  a.item_lo = h->item_lo; a.item_hi = h->item_hi; a.tensor_lo = h->tensor_lo; a.tensor_hi = h->tensor_hi;
  a.beta2t = h->beta2t; a.eps1 = h->eps1; a.eps2 = h->eps2; a.clip = h->clip_threshold; a.rel_step = h->rel_step;
  a.weight_decay = h->weight_decay; a.grad_scale = h->grad_scale; a.scale_parameter = h->scale_parameter;
  a.health = nullptr;
  return a;
}

extern "C" long nk_adafactor_tensor_bytes(void) { return (long)sizeof(NkAfTensor); }

extern "C" int nk_adafactor_init(const NkAdafactorArgs* h, void* stream) {
  if (int e = af_check(h)) return e;
  NkAfArgs a = af_args(h);
  a.health = nk_health_word();      // (allocated here at the latest; the kernel has no gate and does not read it)
  NK_OPT_LAUNCH(af_init_p2_kernel, a.item_hi - a.item_lo, (hipStream_t)stream, a);
  return NK_OK;
}

// one step of a chunk; mo: the first moment of nk_adafactor_chunk_momentum, or null
static int af_chunk(const NkAdafactorArgs* h, const AfMoment* mo, hipStream_t stream) {
  if (int e = af_check(h)) return e;
  NkAfArgs a = af_args(h);
  if (int e = nk_opt_begin(h->tensor_lo == 0, &a.health)) return e;
  const int nitems = a.item_hi - a.item_lo;
  NK_OPT_LAUNCH(af_stats_kernel, nitems, stream, a);
  if (h->has_matrix) NK_OPT_LAUNCH(af_u2_kernel, nitems, stream, a);
  if (mo) {
    hipLaunchKernelGGL(af_apply_momentum_kernel, dim3(nitems), dim3(256), 0, stream, a, *mo);
    if (int e = nk_check_launch("af_apply_momentum_kernel")) return e;
  } else {
    NK_OPT_LAUNCH(af_apply_kernel, nitems, stream, a);
  }
  return nk_opt_end(stream);
}

extern "C" int nk_adafactor_chunk(const NkAdafactorArgs* h, void* stream) { return af_chunk(h, nullptr, (hipStream_t)stream); }

extern "C" int nk_adafactor_chunk_momentum(const NkAdafactorArgs* h, float* exp_avg, float beta1, void* stream) {
  NK_CHECK_ARG(exp_avg && beta1 >= 0.0f && beta1 < 1.0f);
  const AfMoment mo{exp_avg, beta1, 1.0f - beta1};
  return af_chunk(h, &mo, (hipStream_t)stream);
}

// ---- LitEma.forward (modules/ema.py:40-59) over the flat buffer: shadow -= (1 - decay) * (shadow - p) -------------------
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema, const float* __restrict__ p, long n4, float omd) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    float4_t e = ((const float4_t*)ema)[i];
    const float4_t q = ((const float4_t*)p)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] -= omd * (e[k] - q[k]);
    ((float4_t*)ema)[i] = e;
  }
}
extern "C" int nk_ema_flat(float* ema, const float* p, long n, float one_minus_decay, void* stream) {
  NK_CHECK_ARG(ema && p && n > 0 && (n & 3) == 0);
  long blocks = (n / 4 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(ema_flat_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ema, p, n / 4, one_minus_decay);
  return nk_check_launch("ema_flat_kernel");
}
