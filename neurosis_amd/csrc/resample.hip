// Separable banded resampler on dense fp32 planes: y[p] = Wv . x[p] . Wh^T for p < P, [P][H][W] -> [P][OH][OW].
// Antialiased bicubic resize (F.interpolate(mode="bicubic", antialias=True): the resize_input / resize_target options of the autoencoder
// losses, vae_lpips_discr.py:104-107,326-329) is one call with torch's tables; its adjoint is THE SAME call with the transposed tables
// (the windows are monotone, so the transposes are banded too).  The tables come from the host (neurosis_amd/resample.py, float64 -> fp32):
// per output index a window start, a tap count and a zero-padded row of `taps` weights.  No atomics: every output is one fma chain in tap
// order, so the result is bit-identical from run to run.
//
// Two passes through the workspace, lanes along the contiguous x axis in both:
//   rows (Wv): out[p][oy][x] = sum_t wv[oy][t] * in[p][start[oy] + t][x].  A thread owns 16 bytes of an output row (4 bytes when the
//              row length is no multiple of 4 or a pointer is not 16-byte aligned: rows of such a plane do not keep their alignment);
//              the weight is one address per row, the loads and the store are whole-wave contiguous.
//   cols (Wh): out[r][ox] = sum_t wh[ox][t] * in[r][start[ox] + t] over the P * rows flat rows.  The reads are a gather (lane stride =
//              the scale factor), so there is no 16-byte form of them; a thread owns ONE ox of RS_COL_ROWS consecutive rows, which
//              amortises its weight load (lane stride = taps floats, the expensive access of this pass) over that many data loads, and a
//              wave stores 256 contiguous bytes per row.
// The order is the one with the smaller intermediate: rows first when OH * W <= H * OW.
#include "../../include/neurosis_hip.h"
#include "nk_common.h"

#define RS_COL_ROWS 4

template <typename VT>
__global__ __launch_bounds__(256) void resample_rows_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ start,
                                                            const int* __restrict__ count, const float* __restrict__ wt, int taps, long total,
                                                            int Hin, int Hout, int Wv) {
  const long e = blockIdx.x * 256L + threadIdx.x;      // output vector e = (p * Hout + oy) * Wv + xv
  if (e >= total) return;
  const long row = e / Wv;
  const int xv = (int)(e - row * Wv);
  const long p = row / Hout;
  const int oy = (int)(row - p * Hout);
  const int s = max(start[oy], 0);
  const int c = min(min(count[oy], taps), Hin - s);     // a window never leaves the plane, whatever the table says
  const float* __restrict__ w = wt + (long)oy * taps;
  const VT* __restrict__ src = (const VT*)in + (p * Hin + s) * Wv + xv;
  VT acc = (VT)(0.f);
  for (int t = 0; t < c; ++t) acc = w[t] * src[(long)t * Wv] + acc;
  ((VT*)out)[e] = acc;
}

__global__ __launch_bounds__(256) void resample_cols_kernel(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ start,
                                                            const int* __restrict__ count, const float* __restrict__ wt, int taps, long total,
                                                            long nrows, int Win, int Wout) {
  const long e = blockIdx.x * 256L + threadIdx.x;      // e = row group * Wout + ox
  if (e >= total) return;
  const long rg = e / Wout;
  const int ox = (int)(e - rg * Wout);
  const int s = max(start[ox], 0);
  const int c = min(min(count[ox], taps), Win - s);
  const float* __restrict__ w = wt + (long)ox * taps;
  const long r0 = rg * RS_COL_ROWS;
  const float* __restrict__ src = in + r0 * Win + s;
  float* __restrict__ dst = out + r0 * Wout + ox;
  const long live = nrows - r0;
  if (live >= RS_COL_ROWS) {
    float acc[RS_COL_ROWS];
#pragma unroll
    for (int k = 0; k < RS_COL_ROWS; ++k) acc[k] = 0.f;
    for (int t = 0; t < c; ++t) {
      const float wv = w[t];
#pragma unroll
      for (int k = 0; k < RS_COL_ROWS; ++k) acc[k] = __builtin_fmaf(wv, src[(long)k * Win + t], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < RS_COL_ROWS; ++k) dst[(long)k * Wout] = acc[k];
  } else {
    for (int k = 0; k < (int)live; ++k) {                // the last rows of the last plane: the same chains, one row at a time
      float acc = 0.f;
      for (int t = 0; t < c; ++t) acc = __builtin_fmaf(w[t], src[(long)k * Win + t], acc);
      dst[(long)k * Wout] = acc;
    }
  }
}

static bool rs_rows_first(int H, int W, int OH, int OW) { return (long)OH * W <= (long)H * OW; }

extern "C" long nk_resample_ws_floats(long P, int H, int W, int OH, int OW) {
  if (P < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return 0;
  return P * (rs_rows_first(H, W, OH, OW) ? (long)OH * W : (long)H * OW);
}

static void rs_rows(const float* in, float* out, const int* start, const int* count, const float* wt, int taps, long P, int Hin, int Hout, int Wd,
                    hipStream_t stream) {
  if (Wd % 4 == 0 && nk_aligned16(in) && nk_aligned16(out)) {
    const long total = P * Hout * (Wd / 4);
    hipLaunchKernelGGL(resample_rows_kernel<float4_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, start, count, wt, taps,
                       total, Hin, Hout, Wd / 4);
  } else {
    const long total = P * Hout * Wd;
    hipLaunchKernelGGL(resample_rows_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, start, count, wt, taps,
                       total, Hin, Hout, Wd);
  }
}

static void rs_cols(const float* in, float* out, const int* start, const int* count, const float* wt, int taps, long nrows, int Win, int Wout,
                    hipStream_t stream) {
  const long total = (nrows + RS_COL_ROWS - 1) / RS_COL_ROWS * Wout;
  hipLaunchKernelGGL(resample_cols_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, start, count, wt, taps, total, nrows,
                     Win, Wout);
}

extern "C" int nk_resample_planes(const float* x, float* y, float* ws, const int* v_start, const int* v_count, const float* v_weights, int v_taps,
                                  const int* h_start, const int* h_count, const float* h_weights, int h_taps, long P, int H, int W, int OH, int OW,
                                  void* stream_) {
  NK_CHECK_ARG(P >= 0 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && v_taps >= 1 && h_taps >= 1);
  if (P == 0) return NK_OK;
  NK_CHECK_ARG(x && y && ws && v_start && v_count && v_weights && h_start && h_count && h_weights);
  // one thread per output element at the most: the flat indices stay far inside 64 bits and the grids inside 2^31 workgroups
  const long biggest = (long)(H > OH ? H : OH) * (W > OW ? W : OW);
  if (P > (1L << 38) / biggest) {
    nk_set_error(__FILE__, __LINE__, "resample_planes: P * max(H, OH) * max(W, OW) <= 2^38");
    return NK_ERR_ARG;
  }
  hipStream_t stream = (hipStream_t)stream_;
  if (rs_rows_first(H, W, OH, OW)) {
    rs_rows(x, ws, v_start, v_count, v_weights, v_taps, P, H, OH, W, stream);           // [P][H][W]  -> [P][OH][W]
    rs_cols(ws, y, h_start, h_count, h_weights, h_taps, P * OH, W, OW, stream);         //            -> [P][OH][OW]
  } else {
    rs_cols(x, ws, h_start, h_count, h_weights, h_taps, P * H, W, OW, stream);          // [P][H][W]  -> [P][H][OW]
    rs_rows(ws, y, v_start, v_count, v_weights, v_taps, P, H, OH, OW, stream);          //            -> [P][OH][OW]
  }
  return nk_check_launch("resample_planes");
}
