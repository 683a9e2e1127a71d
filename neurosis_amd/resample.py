"""Host tables of the antialiased bicubic resize (`F.interpolate(mode="bicubic", antialias=True)`, align_corners=False) for the banded
resampler of csrc/resample.hip.

Along one axis the resize is a matrix M [n_out x n_in] whose rows are windows of the Keys cubic (a = -0.5) stretched by the scale factor
when downscaling, each divided by its sum (ATen's UpSampleKernel.cpp: `_compute_indices_min_size_weights_aa` with `aa_filter`).  The
matrix is built here in float64 -- plain numpy, no GPU -- and stored as a `Band` (window start, tap count, zero-padded fp32 weights per
row).  Its transpose, the table of the adjoint, is derived from the SAME float64 matrix: the windows move monotonically with the row, so
the columns are bands as well.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

__all__ = ["Band", "axis_matrix", "axis_windows", "band_of", "axis_bands", "device_tables"]


def keys_cubic(t: np.ndarray, a: float = -0.5) -> np.ndarray:
    t = np.abs(np.asarray(t, dtype=np.float64))
    inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    outer = a * (((t - 5.0) * t + 8.0) * t - 4.0)
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def axis_windows(n_in: int, n_out: int):
    """(xmin, xmax) int arrays [n_out]: output i reads inputs xmin[i] .. xmax[i] - 1."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    xmin = np.empty(n_out, dtype=np.int64)
    xmax = np.empty(n_out, dtype=np.int64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        xmin[i] = max(0, int(c - support + 0.5))          # int() truncates towards zero, as the C++ cast does
        xmax[i] = min(n_in, int(c + support + 0.5))
    return xmin, xmax


def axis_matrix(n_in: int, n_out: int) -> np.ndarray:
    """The dense float64 matrix [n_out, n_in] of the resize along one axis."""
    scale = n_in / n_out
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    xmin, xmax = axis_windows(n_in, n_out)
    M = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        j = np.arange(xmax[i] - xmin[i], dtype=np.float64)
        w = keys_cubic((j + xmin[i] - c + 0.5) * inv)
        M[i, xmin[i]:xmax[i]] = w / w.sum()
    return M


@dataclass(frozen=True)
class Band:
    """A banded matrix [n_out x n_in]: row i has its non-zeros in columns start[i] .. start[i] + count[i] - 1."""

    start: np.ndarray      # int32 [n_out]
    count: np.ndarray      # int32 [n_out]
    weights: np.ndarray    # float32 [n_out, taps], rows padded with zeros
    n_in: int

    @property
    def n_out(self) -> int:
        return int(self.start.shape[0])

    @property
    def taps(self) -> int:
        return int(self.weights.shape[1])

    def dense(self) -> np.ndarray:
        M = np.zeros((self.n_out, self.n_in), dtype=np.float64)
        for i in range(self.n_out):
            M[i, self.start[i]:self.start[i] + self.count[i]] = self.weights[i, :self.count[i]]
        return M


def band_of(M: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> Band:
    """Band of the float64 matrix M whose row i is supported on columns lo[i] .. hi[i] - 1 (every row non-empty)."""
    n_out, n_in = M.shape
    count = (hi - lo).astype(np.int64)
    if (count < 1).any() or (lo < 0).any() or (hi > n_in).any():
        raise ValueError("band_of: a window is empty or leaves the input")
    taps = int(count.max())
    weights = np.zeros((n_out, taps), dtype=np.float32)
    for i in range(n_out):
        weights[i, :count[i]] = M[i, lo[i]:hi[i]]       # the fp32 rounding happens here, once
    return Band(lo.astype(np.int32), count.astype(np.int32), weights, int(n_in))


@lru_cache(maxsize=256)
def axis_bands(n_in: int, n_out: int):
    """(forward Band [n_out x n_in], transposed Band [n_in x n_out]) of the resize along one axis, both from one float64 matrix."""
    M = axis_matrix(n_in, n_out)
    xmin, xmax = axis_windows(n_in, n_out)
    fwd = band_of(M, xmin, xmax)
    # column j is read by the outputs i with xmin[i] <= j < xmax[i]; xmin and xmax do not decrease with i, so these are consecutive
    lo = np.searchsorted(xmax, np.arange(n_in), side="right")          # first i with xmax[i] > j
    hi = np.searchsorted(xmin, np.arange(n_in), side="right")          # first i with xmin[i] > j
    if (np.diff(xmin) < 0).any() or (np.diff(xmax) < 0).any():
        raise AssertionError("resize windows are not monotone")
    if (hi <= lo).any():
        raise NotImplementedError(f"resize {n_in} -> {n_out}: an input element no output reads (its adjoint row is empty)")
    return fwd, band_of(np.ascontiguousarray(M.T), lo, hi)


_device_tables: dict = {}


def device_tables(n_in: int, n_out: int, device):
    """((start, count, weights, taps) forward, the same transposed) as device tensors, cached per (n_in, n_out, device).  The first
    use copies from the host, which a stream capture cannot record: build the tables (one eager call) before capturing."""
    import torch

    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(n_in), int(n_out), str(device))
    hit = _device_tables.get(key)
    if hit is not None:
        return hit
    from . import ops

    if ops.capturing() or (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        raise RuntimeError(f"resize {n_in} -> {n_out}: the resampler's tables are not on {device} yet and a stream capture cannot copy them "
                           "there; run the resize once eagerly (or call neurosis_amd.resample.device_tables) before capturing")
    out = []
    for band in axis_bands(int(n_in), int(n_out)):
        out.append((torch.from_numpy(band.start).to(device), torch.from_numpy(band.count).to(device),
                    torch.from_numpy(band.weights).contiguous().to(device), band.taps))
    _device_tables[key] = tuple(out)
    return _device_tables[key]
