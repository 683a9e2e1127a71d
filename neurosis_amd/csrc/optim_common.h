// Device helpers shared by the fused multi-tensor optimizers (optim.hip: Adafactor, came.hip: CAME): the work item of a chunk, the tile
// geometry, the backward-health gate, the element count of a table entry, the fixed-order block reduction and the "last block done" hand-off.
#pragma once
#include "nk_common.h"

struct NkAfItem { int tensor, tr, tc, pad; };   // one block's work: tensor index, tile row (or pair / element block), tile column

// (wave-uniform scalar load; `volatile` so it is not hoisted or cached across the check)
#define AF_HEALTH_GATE(a) do { if (*(const volatile unsigned*)(a).health) return; } while (0)

#define AF_TR 256   // matrix tile rows
#define AF_TC 64    // matrix tile cols
#define AF_CONV_PAIRS 1024
#define AF_VEC 1024

// number of elements of a tensor-table entry, as the float the RMS divisions use (vector: d0; matrix: d0 x d1; conv: O x I x KH x KW)
__device__ __forceinline__ float af_tensor_numel(int kind, int d0, int d1, int kh, int kw) {
  return kind == 0 ? (float)d0 : (float)d0 * (float)d1 * (float)(kind == 2 ? kh * kw : 1);
}

__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// "last block done": count this block in; true (for every thread of the block) in the block that completes `total`.
// No fences: an agent-scope release / acquire writes back and invalidates the XCD's WHOLE L2 -- with every block of a 1 000-block launch
// doing that beside the next step's VAE encoder the step went from 165 to 238 ms (round 4, first version).  Instead every handed-off
// value is STORED with an agent-scope atomic store (sc1: written through to the coherence point) and drained (vmcnt(0)) before the
// block is counted, and the finishing block LOADS them with agent-scope atomic loads (sc1: past its own non-coherent L2 lines) --
// the second valid form of MI355X_MICROARCH.md "Correctness boundaries".
#define AF_PUBLISH(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define AF_FETCH(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
__device__ __forceinline__ bool af_last_block(unsigned* counter, unsigned total, int tid, unsigned* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this thread's published values have been acknowledged
  __syncthreads();
  if (tid == 0) {
    const unsigned old = atomicAdd(counter, 1u);
    *flag = old + 1u == total;
    if (old + 1u == total) AF_PUBLISH(counter, 0u);   // back to zero for the next step (nobody else touches it any more)
  }
  __syncthreads();
  return *flag != 0u;
}

