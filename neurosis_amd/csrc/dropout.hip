// Dropout of the UNet / VAE blocks (gfx950): counter-based masks, never stored.
//
// The mask is a pure function of (seed, step, site, element index): Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), one call
// per 8 consecutive elements = one 16-byte bf16 vector.  With e = row * cols + col the logical element index (row strides play no part) and
// v = e / 8:
//     counter = (v & 0xffffffff, v >> 32, site, step & 0xffffffff)        key = (seed & 0xffffffff, seed >> 32)
//     element j = e % 8 takes the 16-bit half (word[j >> 1] >> (16 * (j & 1))) & 0xffff and is KEPT iff half >= thr,
// thr = round(p * 65536) and scale = 1 / (1 - p) (fp32) both computed on the host.  Arithmetic, so that fp32 on a CPU reproduces every bit:
//     kept: m = fmul_rn(float(x), scale)      dropped: m = +0      y = bf16_rne(m), or bf16_rne(fadd_rn(float(residual), m))
// (the _rn intrinsics: no contraction into an FMA).  The backward is the same function applied to dy; a recomputation that passes the same
// (token, site) regenerates the same mask.  tests/dropout_ref.py restates all of this in plain Python.
//
// seed and step are READ FROM DEVICE MEMORY (`token`), not taken as launch arguments: the training step replays from hipGraphs whose launch
// arguments are frozen at capture, and the mask must still change every step.  nk_dropout_draw advances the per-device counter and fills a
// token inside the captured chain.
#include "../../include/neurosis_hip.h"
#include "nk_common.h"

#define DROPOUT_THREADS 256
#define DROPOUT_MAX_BLOCKS 2048      // memory-bound: ~8 workgroups per CU, grid-stride the rest

__device__ __forceinline__ uint4_t philox4x32_10(uint4_t c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    uint4_t n;
    n.x = hi1 ^ c.y ^ k0;
    n.y = lo1;
    n.z = hi0 ^ c.w ^ k1;
    n.w = lo0;
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// x, residual and y may alias one another (in place): every lane reads its 16 bytes before it writes them, and no lane touches another's.
// The element index is 64-bit (total = rows * cols / 8 vectors, v up to 2^61); nothing in the test suite exercises indices >= 2^32.
__global__ __launch_bounds__(DROPOUT_THREADS) void dropout_kernel(const bf16_t* x, const bf16_t* residual, bf16_t* y, long total, int cpr, long ld_x,
                                                                  long ld_res, long ld_y, const unsigned long long* __restrict__ token, unsigned site,
                                                                  unsigned thr, float scale) {
  const unsigned long long seed = token[0], step = token[1];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  for (long v = blockIdx.x * (long)blockDim.x + threadIdx.x; v < total; v += (long)gridDim.x * blockDim.x) {
    const long row = v / cpr;
    const long col = (v - row * cpr) * 8;
    uint4_t c;
    c.x = (unsigned)v;
    c.y = (unsigned)((unsigned long long)v >> 32);
    c.z = site;
    c.w = (unsigned)step;
    const uint4_t w = philox4x32_10(c, k0, k1);
    const unsigned word[4] = {w.x, w.y, w.z, w.w};
    float f[8];
    unpack8(*(const uint4_t*)(x + row * ld_x + col), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned half = (word[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      f[j] = half >= thr ? __fmul_rn(f[j], scale) : 0.0f;
    }
    if (residual) {
      float r[8];
      unpack8(*(const uint4_t*)(residual + row * ld_res + col), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = __fadd_rn(r[j], f[j]);
    }
    *(uint4_t*)(y + row * ld_y + col) = pack8(f);
  }
}

// state = {seed, step} (the per-device counter), token = {seed, step} of THIS draw
__global__ void dropout_draw_kernel(unsigned long long* state, unsigned long long* token) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long seed = state[0], step = state[1] + 1;
    state[1] = step;
    token[0] = seed;
    token[1] = step;
  }
}

extern "C" int nk_dropout(const void* x, const void* residual, void* y, long rows, int cols, long ld_x, long ld_res, long ld_y, const void* token,
                          int site, int thr, float scale, void* stream) {
  NK_CHECK_ARG(x && y && token && rows > 0 && cols > 0 && (cols & 7) == 0);
  NK_CHECK_ARG(ld_x >= cols && ld_y >= cols && (ld_x & 7) == 0 && (ld_y & 7) == 0 && nk_aligned16(x) && nk_aligned16(y));
  NK_CHECK_ARG(!residual || (ld_res >= cols && (ld_res & 7) == 0 && nk_aligned16(residual)));
  NK_CHECK_ARG(((uintptr_t)token & 7) == 0 && site >= 0 && thr >= 0 && thr <= 65536);
  const int cpr = cols >> 3;
  const long total = rows * cpr;
  long blocks = (total + DROPOUT_THREADS - 1) / DROPOUT_THREADS;
  if (blocks > DROPOUT_MAX_BLOCKS) blocks = DROPOUT_MAX_BLOCKS;
  hipLaunchKernelGGL(dropout_kernel, dim3((unsigned)blocks), dim3(DROPOUT_THREADS), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)residual,
                     (bf16_t*)y, total, cpr, ld_x, ld_res, ld_y, (const unsigned long long*)token, (unsigned)site, (unsigned)thr, scale);
  return nk_check_launch("dropout");
}

extern "C" int nk_dropout_draw(void* state, void* token, void* stream) {
  NK_CHECK_ARG(state && token && ((uintptr_t)state & 7) == 0 && ((uintptr_t)token & 7) == 0);
  hipLaunchKernelGGL(dropout_draw_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long*)state, (unsigned long long*)token);
  return nk_check_launch("dropout_draw");
}
