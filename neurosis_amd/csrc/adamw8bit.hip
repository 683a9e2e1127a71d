// Fused 8-bit blockwise AdamW over the flat parameter / gradient buffers: bitsandbytes' blockwise 8-bit Adam (AdamW8bit) as ONE launch per
// step.  No reference counterpart (the reference's sdxl-te config names bitsandbytes.optim.AdamW8bit); the algorithm is defined in
// neurosis_amd/optim.py (FlatAdamW8bit) and restated in pure torch by tests/golden/make_golden_adamw8bit.py.
//
// Work mapping: every parameter is cut into blocks of 256 consecutive elements (its physical order; the last block may be short).  One
// wavefront owns one block at a time -- 4 elements per lane: a float4 of p and of g, one 32-bit word of four codes each for m and v -- and
// walks A8_BPW consecutive blocks; a workgroup is four such waves.  A wave finds the tensor of its first block by a 64-ary search of the
// per-tensor prefix table `blk_start` (two rounds of one load per lane for the ~1 700 UNet tensors), then steps forward through it.
// Parameter offsets in the store are 64-aligned, not 256-aligned: the float4 accesses are aligned, the codes of block b are bytes
// [256 b, 256 b + 256) of their own buffers.
//
// Per element: dequantize m = qmap1[c1] * absmax1, v = qmap2[c2] * absmax2; m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2;
// p = p (1 - lr wd) - lr (m / bc1) / (sqrt(v / bc2) + eps) with the unquantized new moments; then absmax = max |m| over the block -- a
// butterfly over the wave, no LDS and no barrier -- and the code of the nearest map entry to m / absmax (lowest index on a tie; an absmax
// of 0 stores the code of 0.0).  The two maps sit in LDS (2 KB); the nearest entry is a branch-free binary search there plus one
// comparison of the two neighbours: the rounded distance |q - x| is monotone on either side of x, so the argmin is one of them.
// Tensors below min_8bit_size keep fp32 m / v and take the plain AdamW step in a wave-uniform branch.
//
// Floating-point contraction is off in this file: every multiply, add, divide and sqrt rounds once, as the pure-torch restatement's
// element-wise ops do, so its codes are the kernel's.  Per 8-bit parameter: p read and written, g read, two codes read and written, the bf16
// shadow written: 18 B against AdamW's 30.  No atomics: the step is bitwise reproducible.  Returns at once while the backward-health
// word is raised (masters, codes, absmax, fp32 state and shadows untouched).
#include "../../include/neurosis_hip.h"
#include "nk_common.h"
#include "optim_common.h"

#pragma clang fp contract(off)

#define A8_BLOCK 256   // elements per quantization block (one wavefront)
#define A8_WAVES 4     // waves per workgroup
#define A8_BPW 4       // consecutive blocks per wave

struct NkA8Tensor {    // mirrored by neurosis_amd/optim.py (A8_TENSOR_DTYPE); 24 bytes
  long off;            // element offset of the tensor in master / grad / shadow
  long soff;           // is8 == 0: element offset of its fp32 m / v in m32 / v32
  int numel;
  int is8;             // 1: 8-bit blockwise state; 0: fp32 state (numel < min_8bit_size)
};
static_assert(sizeof(NkA8Tensor) == 24, "mirrored by neurosis_amd/optim.py");

struct NkA8Args {
  float* master; const float* grad; bf16_t* shadow;
  unsigned char* code1; unsigned char* code2; float* absmax1; float* absmax2;
  float* m32; float* v32;
  const float* qmap1; const float* qmap2;
  const NkA8Tensor* tensors; const int* blk_start;
  int ntensors, nblocks;
  float beta1, beta2, omb1, omb2, eps, lr, decay, bc1, bc2, grad_scale;   // omb = 1 - beta, bc = bias corrections, decay = 1 - lr wd: host doubles
  const unsigned* health;
};

// the tensor whose blocks [blk_start[t], blk_start[t + 1]) hold block `gb` (blk_start strictly increasing, blk_start[nt] = nblocks)
__device__ __forceinline__ int a8_find_tensor(const int* blk_start, int nt, int gb, int lane) {
  int lo = 0, hi = nt;                     // invariant: blk_start[lo] <= gb < blk_start[hi]
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) >> 6;
    const int idx = lo + lane * step;
    const bool le = idx < hi && blk_start[idx] <= gb;
    const int cnt = __popcll(__ballot(le));     // the sampled entries <= gb are a prefix of the lanes; lane 0 (idx = lo) is one of them
    lo += (cnt - 1) * step;
    hi = min(hi, lo + step);
  }
  return lo;
}

// index of the map entry nearest to x; the lowest one on a tie
__device__ __forceinline__ unsigned a8_nearest(const float* q, float x) {
  int pos = 0;
#pragma unroll
  for (int s = 128; s >= 1; s >>= 1)
    if (q[pos + s - 1] <= x) pos += s;     // pos = #{i < 255 : q[i] <= x}: q[pos - 1] <= x < q[pos] (pos < 255)
  if (pos == 0) return 0u;
  return fabsf(x - q[pos - 1]) <= fabsf(q[pos] - x) ? (unsigned)(pos - 1) : (unsigned)pos;
}

__global__ __launch_bounds__(256) void adamw8bit_kernel(const NkA8Args a) {
  AF_HEALTH_GATE(a);
  __shared__ float q1[256], q2[256];
  q1[threadIdx.x] = a.qmap1[threadIdx.x];
  q2[threadIdx.x] = a.qmap2[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  int gb = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * A8_WAVES + (threadIdx.x >> 6)) * A8_BPW);
  if (gb >= a.nblocks) return;
  const int gb_end = min(gb + A8_BPW, a.nblocks);
  int t = __builtin_amdgcn_readfirstlane(a8_find_tensor(a.blk_start, a.ntensors, gb, lane));
  for (; gb < gb_end; ++gb) {
    while (gb >= a.blk_start[t + 1]) ++t;
    const NkA8Tensor T = a.tensors[t];
    const int e0 = (gb - a.blk_start[t]) * A8_BLOCK + 4 * lane;     // this lane's first element in the tensor
    const int nv = min(4, T.numel - e0);                              // valid elements of this lane (<= 0: none)
    float* pp = a.master + T.off + e0;
    const float* gp = a.grad + T.off + e0;
    float4_t p = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f};
    if (nv == 4) {
      p = *(const float4_t*)pp;
      g = *(const float4_t*)gp;
    } else {
      for (int e = 0; e < nv; ++e) { p[e] = pp[e]; g[e] = gp[e]; }
    }
    float4_t m, v;
    if (T.is8) {
      const unsigned c1 = *(const unsigned*)(a.code1 + (long)gb * A8_BLOCK + 4 * lane);
      const unsigned c2 = *(const unsigned*)(a.code2 + (long)gb * A8_BLOCK + 4 * lane);
      const float am1 = a.absmax1[gb], am2 = a.absmax2[gb];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        m[e] = q1[(c1 >> (8 * e)) & 255u] * am1;
        v[e] = q2[(c2 >> (8 * e)) & 255u] * am2;
      }
    } else {
      const float* mp = a.m32 + T.soff + e0;
      const float* vp = a.v32 + T.soff + e0;
      m = (float4_t){0.f, 0.f, 0.f, 0.f};
      v = m;
      if (nv == 4) {
        m = *(const float4_t*)mp;
        v = *(const float4_t*)vp;
      } else {
        for (int e = 0; e < nv; ++e) { m[e] = mp[e]; v[e] = vp[e]; }
      }
    }
    float mx1 = 0.f, mx2 = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < nv) {
        const float gr = g[e] * a.grad_scale;
        const float g2 = gr * gr;
        m[e] = a.beta1 * m[e] + a.omb1 * gr;
        v[e] = a.beta2 * v[e] + a.omb2 * g2;
        const float upd = (m[e] / a.bc1) / (sqrtf(v[e] / a.bc2) + a.eps);
        p[e] = p[e] * a.decay - a.lr * upd;
      } else {
        m[e] = 0.f;
        v[e] = 0.f;
      }
      mx1 = fmaxf(mx1, fabsf(m[e]));
      mx2 = fmaxf(mx2, fabsf(v[e]));
    }
    if (T.is8) {
      mx1 = wave_max(mx1);
      mx2 = wave_max(mx2);
      unsigned c1 = 0u, c2 = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c1 |= a8_nearest(q1, mx1 > 0.f ? m[e] / mx1 : 0.f) << (8 * e);
        c2 |= a8_nearest(q2, mx2 > 0.f ? v[e] / mx2 : 0.f) << (8 * e);
      }
      *(unsigned*)(a.code1 + (long)gb * A8_BLOCK + 4 * lane) = c1;
      *(unsigned*)(a.code2 + (long)gb * A8_BLOCK + 4 * lane) = c2;
      if (lane == 0) {
        a.absmax1[gb] = mx1;
        a.absmax2[gb] = mx2;
      }
    } else {
      float* mp = a.m32 + T.soff + e0;
      float* vp = a.v32 + T.soff + e0;
      if (nv == 4) {
        *(float4_t*)mp = m;
        *(float4_t*)vp = v;
      } else {
        for (int e = 0; e < nv; ++e) { mp[e] = m[e]; vp[e] = v[e]; }
      }
    }
    bf16_t* sp = a.shadow + T.off + e0;
    if (nv == 4) {
      *(float4_t*)pp = p;
      uint2_t s;
      s.x = pack2bf(p[0], p[1]);
      s.y = pack2bf(p[2], p[3]);
      *(uint2_t*)sp = s;
    } else {
      for (int e = 0; e < nv; ++e) { pp[e] = p[e]; sp[e] = f2bf(p[e]); }
    }
  }
}

extern "C" long nk_adamw8bit_tensor_bytes(void) { return (long)sizeof(NkA8Tensor); }

extern "C" int nk_adamw8bit_step(const NkAdamW8bitArgs* h, void* stream_) {
  NK_CHECK_ARG(h && h->master && h->grad && h->shadow && h->code1 && h->code2 && h->absmax1 && h->absmax2);
  NK_CHECK_ARG(h->m32 && h->v32 && h->qmap1 && h->qmap2 && h->tensors && h->blk_start);
  NK_CHECK_ARG(h->ntensors > 0 && h->nblocks >= h->ntensors);
  hipStream_t stream = (hipStream_t)stream_;
  NkA8Args a;
  a.master = h->master; a.grad = h->grad; a.shadow = (bf16_t*)h->shadow;
  a.code1 = h->code1; a.code2 = h->code2; a.absmax1 = h->absmax1; a.absmax2 = h->absmax2; a.m32 = h->m32; a.v32 = h->v32;
  a.qmap1 = h->qmap1; a.qmap2 = h->qmap2; a.tensors = (const NkA8Tensor*)h->tensors; a.blk_start = h->blk_start;
  a.ntensors = h->ntensors; a.nblocks = h->nblocks;
  a.beta1 = h->beta1; a.beta2 = h->beta2; a.omb1 = h->one_minus_beta1; a.omb2 = h->one_minus_beta2; a.eps = h->eps; a.lr = h->lr;
  a.decay = h->decay; a.bc1 = h->bc1; a.bc2 = h->bc2; a.grad_scale = h->grad_scale;
  if (int e = nk_opt_begin(true, &a.health)) return e;      // (one launch per step: every call is the step's first chunk)
  const int per_wg = A8_WAVES * A8_BPW;
  NK_OPT_LAUNCH(adamw8bit_kernel, (a.nblocks + per_wg - 1) / per_wg, stream, a);
  return nk_opt_end(stream);
}
