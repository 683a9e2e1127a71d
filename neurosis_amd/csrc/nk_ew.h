// The map core of the HBM-bound elementwise kernels (elementwise.hip, gan.hip): the grid-stride loop, the three index decodes, the 16-byte
// chunk load / store and the launch, once each.  An op is a functor that holds its pointers and its arithmetic; the core calls it once per
// work item (a chunk = 8 bf16 = 16 B):
//   flat    op(i)                  item i of a flat array
//   rows    op(i, row, ch)         chunk ch of row `row`, rows of cpr chunks
//   pixels  op(i, n, h, w, ch)     chunk ch of pixel (n, h, w) of a channels-last [N][H][W][cpr * 8] image (the op's iteration space)
// Indices are 64-bit throughout.  An op loads everything an item needs before it stores, and its pointers are plain struct members (they
// carry no noalias), so a destination may be one of the sources (GegluFwdS's s may be u).
#pragma once
#include <type_traits>
#include "nk_common.h"

#define NK_EW_THREADS 256
#define NK_EW_CAP 8192      // blocks; the loop strides over the rest
static inline int nk_ew_grid(long items, int cap = NK_EW_CAP) {
  const long b = (items + NK_EW_THREADS - 1) / NK_EW_THREADS;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

__device__ __forceinline__ void ew_load(const bf16_t* p, float* f) { unpack8(*(const uint4_t*)p, f); }
__device__ __forceinline__ void ew_store(bf16_t* p, const float* f) { *(uint4_t*)p = pack8(f); }
// the same chunk of 8 values in fp32 storage (32 B, 16-byte aligned): no conversion
__device__ __forceinline__ void ew_load(const float* p, float* f) {
  const float4_t lo = *(const float4_t*)p, hi = *(const float4_t*)(p + 4);
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
  f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}
__device__ __forceinline__ void ew_store(float* p, const float* f) {
  *(float4_t*)p = float4_t{f[0], f[1], f[2], f[3]};
  *(float4_t*)(p + 4) = float4_t{f[4], f[5], f[6], f[7]};
}

// the grid-stride loop.  The block size is the launcher's constant, not blockDim.x: read in a device function, blockDim.x costs a vector
// load and a wait at the head of every kernel (in a __global__ body the compiler folds it into a scalar kernarg load)
template <class F>
__device__ __forceinline__ void nk_ew_for(long total, F f) {
  for (long i = blockIdx.x * (long)NK_EW_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * NK_EW_THREADS) f(i);
}
template <class Op>
__global__ void nk_ew_flat_kernel(Op op, long total) { nk_ew_for(total, op); }
template <class Op>
__global__ void nk_ew_rows_kernel(Op op, long rows, int cpr) {
  nk_ew_for(rows * cpr, [&](long i) {
    const long row = i / cpr;
    op(i, row, (int)(i - row * cpr));
  });
}
template <class Op>
__global__ void nk_ew_pixels_kernel(Op op, int N, int H, int W, int cpr) {
  nk_ew_for((long)N * H * W * cpr, [&](long i) {
    const long pix = i / cpr, t = pix / W;
    op(i, (int)(t / H), (int)(t % H), (int)(pix % W), (int)(i % cpr));
  });
}

// host side: grid min(ceil(items / 256), cap), block 256, on `stream`; returns nk_check_launch(name)
template <class K, class... A>
static inline int nk_ew_launch(const char* name, void* stream, long items, int cap, K kernel, A... args) {
  hipLaunchKernelGGL(kernel, dim3(nk_ew_grid(items, cap)), dim3(NK_EW_THREADS), 0, (hipStream_t)stream, args...);
  return nk_check_launch(name);
}
template <class Op>
static inline int nk_ew_flat(const char* name, void* stream, long items, Op op, int cap = NK_EW_CAP) {
  return nk_ew_launch(name, stream, items, cap, nk_ew_flat_kernel<Op>, op, items);
}
template <class Op>
static inline int nk_ew_rows(const char* name, void* stream, long rows, int cpr, Op op, int cap = NK_EW_CAP) {
  return nk_ew_launch(name, stream, rows * cpr, cap, nk_ew_rows_kernel<Op>, op, rows, cpr);
}
template <class Op>
static inline int nk_ew_pixels(const char* name, void* stream, int N, int H, int W, int cpr, Op op, int cap = NK_EW_CAP) {
  return nk_ew_launch(name, stream, (long)N * H * W * cpr, cap, nk_ew_pixels_kernel<Op>, op, N, H, W, cpr);
}
// a template instance from a runtime mode: f(std::integral_constant<int, mode>) for LO <= mode <= HI (the caller has checked the range)
template <int LO, int HI, class F>
static inline int nk_ew_mode(int mode, F f) {
  if constexpr (LO == HI) return f(std::integral_constant<int, LO>{});
  else return mode == LO ? f(std::integral_constant<int, LO>{}) : nk_ew_mode<LO + 1, HI>(mode, f);
}
