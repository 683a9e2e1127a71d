// The single-writer partial-row reducer: the one body behind every kernel that sums rows of fp32 partials into one value per column without
// atomics (colpart_reduce_kernel, colpart_reduce_mod_kernel, gn_dmod_kernel, colpart_reduce_batch_kernel, gn_reduce_partials_kernel in
// norm.hip; colsum_reduce_kernel in elementwise.hip).
#pragma once
#include "nk_common.h"

// A block of RG x COLS threads, thread (ty, tx) = (threadIdx.x / COLS, threadIdx.x % COLS), owns COLS columns; `ok` says whether this
// thread's column exists.  THE ORDER -- the project's reproducibility guarantee for parameter gradients and GroupNorm sums -- is:
//   1. thread (ty, tx) starts from 0 and adds the terms of rows ty, ty + RG, ty + 2 RG, ... < nrows in ascending order (term(r, acc) adds
//      row r's NACC terms to acc[0 .. NACC));
//   2. after one barrier, row group 0 adds the LDS slots of row groups 1 ... RG - 1 to its own sum in ascending order;
//   3. finish(acc) writes the column's result: one writer per column.
// PAD floats behind each LDS row keep a 32-column layout off the bank stride; UNROLL > 0 is the `#pragma unroll` factor of step 1 (the
// loads of that many rows in flight per thread), 0 leaves the loop to the compiler.
template <int RG, int COLS, int NACC, int PAD, int UNROLL, class Term, class Finish>
__device__ __forceinline__ void nk_reduce_rows(bool ok, int nrows, Term term, Finish finish) {
  __shared__ float sm[NACC][RG][COLS + PAD];
  const int tx = threadIdx.x % COLS, ty = threadIdx.x / COLS;
  float acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = 0.f;
  if (ok) {
    if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
      for (int r = ty; r < nrows; r += RG) term(r, acc);
    } else {
      for (int r = ty; r < nrows; r += RG) term(r, acc);
    }
  }
#pragma unroll
  for (int k = 0; k < NACC; ++k) sm[k][ty][tx] = acc[k];
  __syncthreads();
  if (ty == 0 && ok) {
#pragma unroll
    for (int j = 1; j < RG; ++j) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) acc[k] += sm[k][j][tx];
    }
    finish(acc);
  }
}
