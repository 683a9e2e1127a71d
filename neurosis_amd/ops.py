"""Tensor-level wrappers over the C-ABI (neurosis_amd.lib) and the forward/backward op pairs the modules
are composed from.

Conventions
  * activations are bf16 CUDA(=HIP) tensors.  A "token matrix" is a 2-D tensor [M, C] whose last stride is
    1 (it may be a column slice of a wider buffer).  An image batch is an `Img`: a token matrix of its
    pixels in channels-last order plus (N, H, W).
  * every `*_fwd` returns `(out, bwd)`; `bwd(grad_out, ...)` returns the input gradient(s) and writes the
    parameter gradients IN PLACE into `param.grad` (fp32), through the HIP kernels.  Nothing here calls
    a PyTorch compute kernel on activation-sized data.
  * PyTorch provides memory (torch.empty), streams and autograd plumbing only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import weakref
from dataclasses import dataclass
from typing import Callable, Optional

import torch
from torch import Tensor

from . import lib
from .lib import NkAttnDesc, NkConvDesc, call, query

BF16 = torch.bfloat16


class EngineState:
    """Training-step flags of ONE engine (= one FlatParamStore; `store.state`).  They used to be process-global, which let two
    engines in one process (the GAN step's autoencoder and discriminator stores, a test next to a model) leak the accumulate
    flag and the side stream into each other.  Parameters that belong to no store use the default instance `ops.state`."""

    _live = weakref.WeakSet()

    def __init__(self, wgrad_stream=None):
        self.grad_accumulate = False  # False: weight-grad kernels overwrite; True: they add (micro-batch accumulation)
        self.assume_zeroed = False  # True: a caller guarantees .grad buffers are all-zero before the first micro-batch (split-K skips its memset)
        self.wgrad_stream = wgrad_stream  # optional side HIP stream: weight-gradient GEMMs run there, concurrently with the dgrad chain
        # the small same-shape weight gradients of one transformer block (attn1.to_out, attn2.to_q, attn2.to_out: 1280 x 1280 =
        # 80 tiles of 128 x 160 each) as ONE batched launch (nk_linear_wgrad_batched): 240 tiles = one full round of the two-group
        # kernel, 49.7 us for the three against 3 x 45.4 us one by one (tools/bench_g2.py).  (Round 1 measured batching -2 % with the
        # 128 x 128 kernels, which gained nothing from the fuller grid, and with the block's LARGE weight gradients deferred too.)
        # In the real two-stream step the step TIME does not move (tools/ab_step.py, interleaved rounds, GC frozen: 184.4 vs 185.3,
        # 188.0 vs 187.8, 188.4 vs 188.0 ms; bench.py with graph replay 186.4 / 188.8 vs 186.9 / 187.1): the side stream is not the
        # critical path.  What moves is the kernel time behind it: 140 fewer launches per step, linear weight gradients 500 -> 570
        # TFLOP/s serialized (314 -> 339 in the step), the tile engine 644 -> 662 serialized and 498 -> 508 in the step.  On by default since the chain
        # replays from hipGraphs (the deferred launches used to lengthen the host path); NK_BATCH_WGRADS=0 turns it off.
        self.batch_wgrads = os.environ.get("NK_BATCH_WGRADS", "1") != "0"
        # LayerNorm gamma / beta gradients on the weight-gradient stream.  Launched from Python this measured SLOWER (217.6 vs
        # 203.9 ms/step in round 1, +5.5 ms in round 2: 210 more cross-stream event waits per step delay the weight-gradient GEMMs
        # queued behind them).  Under hipGraph replay those waits are gone -- the parked launches become part of each segment's
        # side-stream graph -- and the main chain sheds ~4 ms of small kernels: 177.2 / 177.1 vs 178.2 / 178.7 ms/step (bench.py,
        # alternating).  So: None = automatic -- on exactly for launches that are being CAPTURED for replay (`deferred` is a list), off for
        # every eager launch (NK_GRAPH=0, a chain whose capture failed, the frozen towers, bench.py's instrumented eager replays); True / False force it.
        self.norm_params_on_side_stream: Optional[bool] = None
        # hipGraph capture of a backward chain (neurosis_amd/graphs.py): while `deferred` is a list, on_wgrad_stream() parks the
        # side-stream work there instead of launching it, and the chain reports the end of each top-level block to
        # `segment_hook`, which captures the parked launches as that segment's own graph
        self.deferred: Optional[list] = None
        self.segment_hook: Optional[Callable] = None
        EngineState._live.add(self)

    def derived(self) -> "EngineState":
        """A state that shares this one's side stream but always overwrites (channel-padded stand-in parameters)."""
        return EngineState(self.wgrad_stream)


_capture_depth = 0


def capturing() -> bool:
    """True while neurosis_amd.graphs records a launch sequence: caches of weight-derived tensors must be refilled (in place)
    rather than trusted, so that the refill is part of the graph."""
    return _capture_depth > 0


class capture_scope:
    def __enter__(self):
        global _capture_depth
        _capture_depth += 1

    def __exit__(self, *exc):
        global _capture_depth
        _capture_depth -= 1


state = EngineState()
state.param_epoch = 0  # process-wide "some parameter changed" counter (keys of captured graphs); bumped by every store


def state_of(p) -> EngineState:
    """The engine state that governs parameter `p`: its own tag, its store's, or the default."""
    if p is not None:
        st = getattr(p, "_nk_state", None)
        if st is not None:
            return st
        store = getattr(p, "_nk_store", None)
        if store is not None:
            return store.state
    return state


def wgrad_mode(p=None) -> int:
    """accumulate argument of the weight-gradient kernels (see include/neurosis_hip.h) for parameter `p`."""
    st = state_of(p)
    if st.grad_accumulate:
        return 1
    return 2 if st.assume_zeroed else 0


# Whether the forward now running will be followed by a backward (its closures are kept).  torch.is_grad_enabled() cannot answer that
# inside the autograd bridge: torch.autograd.Function.forward always runs with grad mode off.  nn.NkFunction.forward raises the flag around
# `run`; the activation-dropping policies (ResBlock.use_checkpoint, BasicTransformerBlock.checkpoint / .recompute) read it.
# The flag is per THREAD: a validation or data-loader thread that runs a forward of its own must not see the training thread's.
# Callers that drive `module.fwd(...)` and the returned closure themselves (outside nn.NkFunction) and want the checkpoint / recompute
# policies honoured wrap the forward in `with ops.recording_backward():` -- without it the blocks keep their activations (correct, not lean).
_recording = threading.local()


class recording_backward:
    """`with ops.recording_backward():` -- the forward launched inside will be followed by a backward through its closure."""

    def __enter__(self):
        _recording.depth = getattr(_recording, "depth", 0) + 1

    def __exit__(self, *exc):
        _recording.depth -= 1


def recording() -> bool:
    return getattr(_recording, "depth", 0) > 0


def on_wgrad_stream(fn: Callable[[], None], *reads: Tensor, owner=None) -> None:
    """Run `fn` (kernels that only WRITE parameter gradients of `owner`'s engine) on that engine's side stream if it has one.

    Weight-gradient GEMMs are off the critical path of backward (nothing downstream reads them until the optimizer /
    all-reduce), and most of them -- like the dgrad GEMMs they sit next to -- do not fill 256 CUs x 2 workgroups on
    their own (e.g. 1280x1280 outputs = 100 tiles).  Issuing them on a second HIP stream lets the hardware co-schedule
    both kernels' workgroups, which recovers the tile-quantisation tail of each without split-K atomics.
    `reads` are the activation tensors fn consumes: they are pinned to the side stream for the caching allocator."""
    st = state_of(owner)
    side = st.wgrad_stream
    if side is None:
        fn()
        return
    if st.deferred is not None:
        st.deferred.append((fn, reads))
        return
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    for t in reads:
        if t is not None:
            t.record_stream(side)


class WgradQueue:
    """Collects weight-gradient GEMMs and issues those of identical shape as ONE batched launch (blockIdx.z).
    Used per transformer block: its attn1.to_out / attn2.to_q / attn2.to_out gradients are three 100-tile grids."""

    def __init__(self, owner=None):
        self.items = []  # (dy, x, dw2d)
        self.colparts = []  # (part, dgamma, dbeta, nrows, C, accumulate)
        self.owner = owner

    MAX_ELEMS = 2 << 20     # weights up to 1280 x 1280: larger ones fill the chip alone and should not wait for the end of the block

    @classmethod
    def takes(cls, weight: Tensor) -> bool:
        return weight.numel() <= cls.MAX_ELEMS

    def add(self, dy: Tensor, x: Tensor, dw: Tensor, db: Optional[Tensor] = None) -> None:
        """db: the layer's bias gradient [N] (fp32), summed from dy by the same launch"""
        self.items.append((dy, x, dw, db))

    def add_colpart(self, part: Tensor, dgamma: Tensor, dbeta: Tensor, nrows: int, Cc: int, accumulate: bool) -> None:
        """partial rows of a one-pass LayerNorm backward (nk_layernorm_bwd_rows): reduced with the block's other ones in one launch"""
        self.colparts.append((part, dgamma, dbeta, nrows, Cc, accumulate))

    def flush(self) -> None:
        colparts, self.colparts = self.colparts, []
        if colparts:
            on_wgrad_stream(lambda: colpart_reduce(colparts), *[c[0] for c in colparts], owner=self.owner)
        items, self.items = self.items, []
        if not items:
            return
        groups = {}
        for it in items:
            dy, x, dw, _db = it
            key = (dy.shape[0], dy.shape[1], x.shape[1], dy.stride(0), x.stride(0), dw.stride(0))
            groups.setdefault(key, []).append(it)
        mode = wgrad_mode(self.owner)

        def run():
            for (M, N, K, lddy, ldx, lddw), its in groups.items():
                for i in range(0, len(its), 8):
                    chunk = its[i:i + 8]
                    if len(chunk) == 1:
                        gemm_tn_f32(chunk[0][0], chunk[0][1], chunk[0][2], mode, dbias=chunk[0][3])
                        continue
                    n = len(chunk)
                    arr = C.c_void_p * n
                    call("nk_linear_wgrad_batched", arr(*[c[0].data_ptr() for c in chunk]), arr(*[c[1].data_ptr() for c in chunk]),
                         arr(*[c[2].data_ptr() for c in chunk]), arr(*[None if c[3] is None else c[3].data_ptr() for c in chunk]), n, M, N, K,
                         lddy, ldx, lddw, mode, _stream())

        on_wgrad_stream(run, *[t for it in items for t in it[:2]], owner=self.owner)


def colpart_reduce(entries) -> None:
    """dgamma / dbeta of several one-pass LayerNorm backwards from their partial rows, NK_COLPART_MAX per launch (current stream)"""
    for i in range(0, len(entries), lib.NK_COLPART_MAX):
        chunk = entries[i:i + lib.NK_COLPART_MAX]
        b = lib.NkColpartBatch()
        for z, (part, dgamma, dbeta, nrows, Cc, acc) in enumerate(chunk):
            b.part[z], b.dgamma[z], b.dbeta[z] = part.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr()
            b.nrows[z], b.C[z], b.accumulate[z] = nrows, Cc, int(acc)
        b.n = len(chunk)
        call("nk_colpart_reduce_batch", C.byref(b), _stream())


_wgrad_queue: Optional[WgradQueue] = None


class batched_wgrads:
    """Context manager: inside it, linear_fwd's backward defers bias-free bookkeeping of weight gradients to a queue that is
    flushed (batched by shape) on exit."""

    def __init__(self, owner=None):
        self.owner = owner      # a parameter of the block: selects the engine whose flags apply

    def __enter__(self):
        global _wgrad_queue
        self.prev = _wgrad_queue
        _wgrad_queue = WgradQueue(self.owner) if state_of(self.owner).batch_wgrads else None
        return _wgrad_queue

    def __exit__(self, *exc):
        global _wgrad_queue
        q, _wgrad_queue = _wgrad_queue, self.prev
        if exc[0] is None and q is not None:
            q.flush()
        return False


def join_wgrad_stream(owner=None) -> None:
    """Make the current stream wait for every weight-gradient kernel issued so far (on `owner`'s engine's side stream, or, with
    no owner, on every live engine's)."""
    if owner is not None:
        st = state_of(owner)
        side = st.wgrad_stream
        if side is not None and st.deferred is None:
            torch.cuda.current_stream().wait_stream(side)
        return
    seen = set()
    for st in list(EngineState._live):
        side = st.wgrad_stream
        if side is not None and st.deferred is None and id(side) not in seen:
            seen.add(id(side))
            torch.cuda.current_stream().wait_stream(side)


def _ws(n_floats: int, device) -> Tensor:
    return torch.empty(n_floats, dtype=torch.float32, device=device)


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check2d(t: Tensor, name: str):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != BF16 or not t.is_cuda:
        raise ValueError(f"{name}: expected a 2-D bf16 CUDA tensor with unit inner stride, got {tuple(t.shape)} {t.dtype} {t.stride()} {t.device}")


@dataclass
class Img:
    """Channels-last image batch: t is [N*H*W, C] (row = pixel)."""

    t: Tensor
    N: int
    H: int
    W: int
    sums: Optional[Tensor] = None    # GroupNorm sums of THIS tensor, [N, 2G] fp32 (entry 2g = sum, 2g+1 = sum of squares per group), when the
    #                                  kernel that produced it emitted them (conv2d_fwd(stats_groups=G)): groupnorm_fwd then skips its statistics pass

    @property
    def C(self) -> int:
        return self.t.shape[1]

    @staticmethod
    def from_nchw(x: Tensor) -> "Img":
        """View a logical-NCHW bf16 tensor in channels_last memory format as an Img (no copy); otherwise convert."""
        N, Cc, H, W = x.shape
        if x.dtype == BF16 and x.permute(0, 2, 3, 1).is_contiguous():
            return Img(x.permute(0, 2, 3, 1).reshape(N * H * W, Cc), N, H, W)
        return Img(nchw_to_tokens(x, Cc), N, H, W)

    def to_nchw(self) -> Tensor:
        """Logical NCHW view (channels_last memory format) of the same storage."""
        return self.t.view(self.N, self.H, self.W, self.C).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------
# parameter plumbing: bf16 shadows and fp32 grads
# ------------------------------------------------------------------------------------------------
def _param_stamp(p: Tensor):
    """What a cached derivative of parameter `p` (bf16 shadow, channel-padded copy) is valid for.  Store-managed parameters are
    updated by raw-pointer kernels, which torch's version counter does not see: they go by the global epoch the store bumps.
    Everything else (frozen VAE / text-encoder weights, stand-alone modules) goes by the tensor's own version counter and
    address, so that an optimizer step on the UNet does not invalidate 850 M frozen parameters' shadows every step."""
    st = getattr(p, "_nk_store", None)
    if st is not None:
        return ("epoch", id(st), st.epoch)
    return ("version", p._version, p.data_ptr())


def shadow(p: Tensor) -> Tensor:
    """bf16 copy of an fp32 parameter in the same physical layout (flat store view, or cached cast)."""
    if getattr(p, "_nk_store", None) is not None:
        return p._nk_shadow            # store-managed: rewritten with the masters by the fused optimizers / store.refresh()
    s = getattr(p, "_nk_shadow", None)
    stamp = _param_stamp(p)
    if s is not None and getattr(p, "_nk_shadow_stamp", None) == stamp:
        return s
    flat = _phys_flat(p)
    n = flat.numel()
    if s is not None and n % 8 == 0 and s.numel() == n and s.device == p.device:
        # same tensor, new values (an in-place update): re-cast into the SAME buffer -- captured graphs hold its address
        call("nk_cast_f32_to_bf16", flat.data_ptr(), s.data_ptr(), n, _stream())
        p._nk_shadow_stamp = stamp
        return s
    s = torch.empty(flat.numel(), dtype=BF16, device=p.device)
    if n % 8 == 0:
        call("nk_cast_f32_to_bf16", flat.data_ptr(), s.data_ptr(), n, _stream())
    else:  # tiny odd-sized parameters
        pad = torch.zeros((n + 7) // 8 * 8, dtype=torch.float32, device=p.device)
        pad[:n] = flat
        s8 = torch.empty(pad.numel(), dtype=BF16, device=p.device)
        call("nk_cast_f32_to_bf16", pad.data_ptr(), s8.data_ptr(), pad.numel(), _stream())
        s = s8[:n]
    p._nk_shadow = s
    p._nk_shadow_stamp = stamp
    return s


def _phys_flat(p: Tensor) -> Tensor:
    """The parameter's storage as a flat fp32 tensor in physical order (conv weights: [O][KH][KW][I])."""
    d = p.detach()
    if d.dim() == 4:
        d = d.permute(0, 2, 3, 1)
    if not d.is_contiguous():
        raise ValueError("parameter storage must be dense (conv weights in channels_last memory format)")
    return d.reshape(-1)


def grad_flat(p: Tensor) -> Tensor:
    """fp32 gradient buffer of p in physical order (allocated zeroed on first use)."""
    if p.grad is None:
        g = torch.zeros_like(p, memory_format=torch.preserve_format)
        p.grad = g
    g = p.grad
    if g.dim() == 4:
        g = g.permute(0, 2, 3, 1)
    if not g.is_contiguous():
        raise ValueError("parameter .grad must share the parameter's physical layout")
    return g.reshape(-1)


def w2d(p: Tensor) -> Tensor:
    """bf16 shadow as the [out, K] matrix the kernels read."""
    return shadow(p).view(p.shape[0], -1)


def g2d(p: Tensor) -> Tensor:
    return grad_flat(p).view(p.shape[0], -1)


def conv_weight_param(out_ch: int, in_ch: int, kh: int, kw: int) -> torch.nn.Parameter:
    """fp32 OIHW parameter whose storage is [O][KH][KW][I] (channels_last), the layout the kernels read."""
    base = torch.empty(out_ch, kh, kw, in_ch)
    return torch.nn.Parameter(base.permute(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------
# layout / dtype boundary
# ------------------------------------------------------------------------------------------------
def nchw_to_tokens(x: Tensor, cpad: int, scale: float = 1.0) -> Tensor:
    """NCHW (fp32 or bf16, contiguous) -> channels-last bf16 [N*H*W, cpad] (extra channels zero)."""
    N, Cc, H, W = x.shape
    x = x.contiguous()
    if x.dtype not in (torch.float32, BF16):
        raise ValueError(f"unsupported dtype {x.dtype}")
    out = torch.empty(N * H * W, cpad, dtype=BF16, device=x.device)
    call("nk_nchw_to_nhwc", x.data_ptr(), int(x.dtype == torch.float32), out.data_ptr(), N, Cc, H * W, cpad, scale, _stream())
    return out


def tokens_to_nchw(t: Tensor, N: int, Cc: int, H: int, W: int, dtype=torch.float32) -> Tensor:
    """channels-last bf16 [N*H*W, cpad] -> contiguous NCHW tensor of `dtype` holding the first Cc channels."""
    _check2d(t, "t")
    out = torch.empty(N, Cc, H, W, dtype=dtype, device=t.device)
    call("nk_nhwc_to_nchw", t.data_ptr(), out.data_ptr(), int(dtype == torch.float32), N, Cc, H * W, t.shape[1], _stream())
    return out


def cast_bf16(x: Tensor) -> Tensor:
    """fp32 -> bf16 of a contiguous tensor (numel % 8 == 0)."""
    if x.dtype == BF16:
        return x
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=BF16, device=x.device)
    n = x.numel()
    if n % 8:
        raise ValueError("cast_bf16 needs numel % 8 == 0")
    call("nk_cast_f32_to_bf16", x.data_ptr(), out.data_ptr(), n, _stream())
    return out


def add(a: Tensor, b: Tensor) -> Tensor:
    if a.shape != b.shape or not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("add: contiguous tensors of equal shape expected")
    out = torch.empty_like(a)
    call("nk_add", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream())
    return out


# ------------------------------------------------------------------------------------------------
# Linear
# ------------------------------------------------------------------------------------------------
def gemm_nt(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None, alpha: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """y = alpha * x @ w^T + bias + residual ; x [M,K], w [N,K] bf16, bias fp32 [N], residual bf16 [M,N]."""
    _check2d(x, "x")
    _check2d(w, "w")
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"gemm_nt: K mismatch {x.shape} vs {w.shape}")
    if out is None:
        out = torch.empty(M, N, dtype=BF16, device=x.device)
    if residual is not None:
        _check2d(residual, "residual")
    call("nk_linear_fwd", x.data_ptr(), w.data_ptr(), _p(bias), _p(residual), out.data_ptr(), M, N, K, x.stride(0), w.stride(0),
         residual.stride(0) if residual is not None else 0, out.stride(0), float(alpha), _stream())
    return out


def gemm_nt_batched(xs, ws, outs=None):
    """[x_i @ w_i^T] for same-shape bias-free problems, up to eight per launch (nk_linear_fwd_batched).  xs / ws: lists of 2-D bf16
    matrices (unit inner stride, equal shapes and row strides); returns the list of outputs."""
    M, K = xs[0].shape
    N = ws[0].shape[0]
    for x, w in zip(xs, ws):
        _check2d(x, "x")
        _check2d(w, "w")
        if x.shape != (M, K) or w.shape != (N, K) or x.stride(0) != xs[0].stride(0) or w.stride(0) != ws[0].stride(0):
            raise ValueError("gemm_nt_batched: every problem must have the same shape and strides")
    if outs is None:
        outs = [torch.empty(M, N, dtype=BF16, device=xs[0].device) for _ in xs]
    for i in range(0, len(xs), 8):
        n = min(8, len(xs) - i)
        arr = C.c_void_p * n
        call("nk_linear_fwd_batched", arr(*[t.data_ptr() for t in xs[i:i + n]]), arr(*[t.data_ptr() for t in ws[i:i + n]]),
             arr(*[t.data_ptr() for t in outs[i:i + n]]), n, M, N, K, xs[0].stride(0), ws[0].stride(0), outs[0].stride(0), _stream())
    return outs


def gemm_nn(dy: Tensor, w: Tensor, dx_add: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """dx = dy @ w + dx_add ; dy [M,N], w [N,K]."""
    _check2d(dy, "dy")
    _check2d(w, "w")
    M, N = dy.shape
    K = w.shape[1]
    if w.shape[0] != N:
        raise ValueError(f"gemm_nn: N mismatch {dy.shape} vs {w.shape}")
    if out is None:
        out = torch.empty(M, K, dtype=BF16, device=dy.device)
    if dx_add is not None:
        _check2d(dx_add, "dx_add")
    call("nk_linear_dgrad", dy.data_ptr(), w.data_ptr(), _p(dx_add), out.data_ptr(), M, N, K, dy.stride(0), w.stride(0),
         dx_add.stride(0) if dx_add is not None else 0, out.stride(0), _stream())
    return out


def gemm_tn_f32(dy: Tensor, x: Tensor, dw: Tensor, accumulate, dbias: Optional[Tensor] = None) -> None:
    """dw (+)= dy^T @ x ; dy [M,N], x [M,K], dw fp32 [N,K].  dbias fp32 [N] (+)= column sums of dy, from the same launch."""
    _check2d(dy, "dy")
    _check2d(x, "x")
    M, N = dy.shape
    K = x.shape[1]
    if x.shape[0] != M or dw.shape != (N, K) or dw.dtype != torch.float32 or dw.stride(1) != 1:
        raise ValueError(f"gemm_tn_f32: bad shapes {dy.shape} {x.shape} {dw.shape}")
    if dbias is None:
        call("nk_linear_wgrad", dy.data_ptr(), x.data_ptr(), dw.data_ptr(), M, N, K, dy.stride(0), x.stride(0), dw.stride(0), int(accumulate), _stream())
        return
    if dbias.shape != (N,) or dbias.dtype != torch.float32 or not dbias.is_contiguous():
        raise ValueError(f"gemm_tn_f32: dbias must be a dense fp32 [{N}] tensor")
    call("nk_linear_wgrad_bias", dy.data_ptr(), x.data_ptr(), dw.data_ptr(), dbias.data_ptr(), M, N, K, dy.stride(0), x.stride(0), dw.stride(0),
         int(accumulate), _stream())


def colsum(dy: Tensor, out: Tensor, accumulate: bool) -> None:
    _check2d(dy, "dy")
    M, N = dy.shape
    ws = _ws(query("nk_colsum_ws_floats", M, N), dy.device)
    call("nk_colsum", dy.data_ptr(), out.data_ptr(), ws.data_ptr(), M, N, dy.stride(0), int(accumulate), _stream())


def linear_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor] = None, need_dx: bool = True, x_saved=None):
    """nn.Linear forward on a token matrix, with optional fused residual add.
    bwd(dy, dx_add=None) -> dx (None if need_dx is False); writes weight.grad / bias.grad.
    x_saved: a zero-argument callable that REBUILDS x for the weight gradient (selective recompute: the caller drops x after the forward)."""
    y = gemm_nt(x, w2d(weight), bias, residual)
    return y, _linear_bwd(x if x_saved is None else x_saved, weight, bias, need_dx)


def geglu_save_enabled() -> bool:
    """NK_GEGLU_SAVE: 1 (default) = FeedForward keeps s = [gelu(g) | a gelu'(g)] of its projection instead of u = [a | g] (round 6: the GEGLU
    derivative is evaluated where the cdf already is -- the forward's epilogue -- and the fused input gradient multiplies); 0 = u (A/B runs)"""
    return os.environ.get("NK_GEGLU_SAVE", "1") != "0"


def linear_geglu_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor], x_saved=None, save_derivative: bool = False):
    """FeedForward.net[0] = GEGLU (modules/attention.py:50-57): u = x @ weight^T + bias [M, 2I] and h = u[:, :I] * gelu(u[:, I:]) [M, I].
    One launch (the GEGLU in the projection's epilogue, nk_linear_fwd_geglu) where the 256 x 256 kernel takes the shape -- the two SDXL
    FeedForward widths at batch 4 -- else the GEMM followed by the GEGLU kernel.  Returns (u, h, bwd); bwd(du) as linear_fwd's.
    save_derivative: the first result is s = [gelu(g) | a gelu'(g)] [M, 2I] instead of u (u is never written): hand it to the output
    projection's backward as `geglu_s` (nk_linear_dgrad_geglu_s)."""
    _check2d(x, "x")
    M, K = x.shape
    I2 = weight.shape[0]
    I = I2 // 2
    wq = w2d(weight)
    if I2 % 2 == 0 and x.is_contiguous() and query("nk_linear_fwd_geglu_ok", M, I, K):
        u = torch.empty(M, I2, dtype=BF16, device=x.device)
        h = torch.empty(M, I, dtype=BF16, device=x.device)
        call("nk_linear_fwd_geglu_s" if save_derivative else "nk_linear_fwd_geglu", x.data_ptr(), wq.data_ptr(), _p(bias), u.data_ptr(), h.data_ptr(), M, I, K,
             x.stride(0), wq.stride(0), u.stride(0), h.stride(0), _stream())
    else:
        u = gemm_nt(x, wq, bias, None)
        if save_derivative:
            h = torch.empty(M, I, dtype=BF16, device=x.device)
            call("nk_geglu_fwd_s", u.data_ptr(), h.data_ptr(), u.data_ptr(), M, I, _stream())       # in place: u becomes s
        else:
            h = geglu_fwd(u)[0]
    return u, h, _linear_bwd(x if x_saved is None else x_saved, weight, bias, True)


def _linear_bwd(x_in, weight: Tensor, bias: Optional[Tensor], need_dx: bool):
    def bwd(dy: Tensor, dx_add: Optional[Tensor] = None, geglu_u: Optional[Tensor] = None, geglu_s: Optional[Tensor] = None):
        """geglu_u = the [a | g] matrix whose GEGLU produced x (FeedForward): the returned gradient is then d/du [M, 2K], the GEGLU
        backward applied in the input-gradient GEMM's epilogue (nk_linear_dgrad_geglu).  geglu_s = the saved-derivative form
        [gelu(g) | a gelu'(g)] of linear_geglu_fwd(save_derivative=True) instead (nk_linear_dgrad_geglu_s)."""
        entry = "nk_linear_dgrad_geglu"
        if geglu_s is not None:
            if geglu_u is not None:
                raise ValueError("linear bwd: geglu_u and geglu_s are exclusive")
            geglu_u, entry = geglu_s, "nk_linear_dgrad_geglu_s"
        x = x_in() if callable(x_in) else x_in         # (selective recompute: the layer's input is rebuilt now, on the current stream)
        queued = _wgrad_queue is not None and _wgrad_queue.takes(weight) and dy.is_contiguous() and x.is_contiguous()
        # the bias gradient (column sums of dy) comes out of the weight-gradient launch: every parameter gradient is OVERWRITTEN by its
        # (single) producer unless accumulating -- the same mode for both
        db = grad_flat(bias) if bias is not None else None
        if queued:
            _wgrad_queue.add(dy, x, g2d(weight), db)
        else:
            on_wgrad_stream(lambda: gemm_tn_f32(dy, x, g2d(weight), wgrad_mode(weight), dbias=db), dy, x, owner=weight)
        if not need_dx:
            return None
        if geglu_u is not None:
            if dx_add is not None:
                raise ValueError("linear bwd: geglu_u and dx_add are exclusive")
            M, N = dy.shape
            K = weight.shape[1]
            _check2d(geglu_u, "geglu_u")
            if geglu_u.shape != (M, 2 * K):
                raise ValueError(f"linear bwd: geglu_u must be [{M}, {2 * K}], got {tuple(geglu_u.shape)}")
            du = torch.empty(M, 2 * K, dtype=BF16, device=dy.device)
            wq = w2d(weight)
            call(entry, dy.data_ptr(), wq.data_ptr(), geglu_u.data_ptr(), du.data_ptr(), M, N, K, dy.stride(0), wq.stride(0),
                 geglu_u.stride(0), du.stride(0), _stream())
            return du
        return gemm_nn(dy, w2d(weight), dx_add)

    return bwd


# ------------------------------------------------------------------------------------------------
# Conv2d (implicit GEMM)
# ------------------------------------------------------------------------------------------------
def _conv_desc(N, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, upsample) -> NkConvDesc:
    return NkConvDesc(N, H, W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, int(upsample))


def groupnorm_sums(x: Img, groups: int) -> Tensor:
    """[N, 2*groups] fp32 sums / sums of squares of x per (image, group): x.sums when its producer emitted them, else one pass over x."""
    if x.sums is not None and x.sums.shape == (x.N, 2 * groups):
        return x.sums
    sums = torch.empty(x.N, 2 * groups, dtype=torch.float32, device=x.t.device)
    ws = _ws(query("nk_groupnorm_ws_floats", x.N, x.H * x.W, x.C, groups), x.t.device)
    call("nk_groupnorm_sums", x.t.data_ptr(), sums.data_ptr(), ws.data_ptr(), x.N, x.H * x.W, x.C, groups, _stream())
    return sums


UP2_PHASES_MIN_WORK = 1 << 28


def up2_phases_take(pixels: int, Cin: int, Cout: int) -> bool:
    """Does conv3x3(nearest_upsample_2x(x)) run as four 2 x 2 phase convolutions of x (nk_conv2d_up2_*: 4/9 of the fused gather's products)?
    NK_UP2_PHASES, read per call: 0 = never (the fused-upsample gather), 2 = every qualifying call (tests), 1 / unset = by size.  The phase
    path trades 5/9 of the products of forward, input gradient and weight gradient for about eight more launches and four passes over y / dy:
    at ~800 TFLOP/s the saved products are worth those ~30 us from about pixels * Cin * Cout = 2e8 on (reasoned from the launch count, not
    measured at the threshold; the UNet's layers are at 6.7e9, measured).  Below it the fused gather also keeps small models on one rounding
    of the weights."""
    mode = os.environ.get("NK_UP2_PHASES", "1")
    if mode == "0":
        return False
    return mode == "2" or pixels * Cin * Cout >= UP2_PHASES_MIN_WORK


def conv2d_fwd(x: Img, weight: Tensor, bias: Optional[Tensor], stride: int = 1, padding=1, upsample: bool = False,
               rowvec: Optional[Tensor] = None, residual: Optional[Tensor] = None, need_dx: bool = True,
               asym_pad: bool = False, stats_groups: Optional[int] = None, cin_real: Optional[int] = None):
    """nn.Conv2d forward on channels-last data as implicit GEMM.
    padding: int (symmetric) ; asym_pad=True reproduces ConstantPad2d((0,1,0,1)) + padding 0 (model.py:71-79).
    rowvec: bf16 [N, Cout] added to every pixel of image n (ResBlock emb_out); residual: bf16 [N*Ho*Wo, Cout].
    stats_groups = G: the output Img carries `.sums` (its GroupNorm sums over G groups) when the kernel can emit them.
    cin_real = 3 | 4: x's 8 channels are 3 or 4 real ones plus zero padding (image / latent inputs): the forward of a plain 3 x 3
    stride-1 convolution then runs as the register-resident FMA kernel instead of a K = 72 implicit GEMM.
    upsample=True: the convolution of the nearest-2x upsampling of x, which is never written; a 3 x 3 / stride 1 / padding 1 one without
    rowvec or residual runs as four 2 x 2 phase convolutions of x where up2_phases_take() says so (nk_conv2d_up2_*; NK_UP2_PHASES).
    bwd(dy) -> (dx Img | None, d_rowvec | None)."""
    Cout, Cin, KH, KW = weight.shape
    if x.C != Cin:
        raise ValueError(f"conv2d: input has {x.C} channels, weight expects {Cin}")
    Hin, Win = (2 * x.H, 2 * x.W) if upsample else (x.H, x.W)
    if asym_pad:
        pad_t = pad_l = 0
        Ho = (Hin + 1 - KH) // stride + 1
        Wo = (Win + 1 - KW) // stride + 1
    else:
        pad_t = pad_l = int(padding)
        Ho = (Hin + 2 * pad_t - KH) // stride + 1
        Wo = (Win + 2 * pad_l - KW) // stride + 1
    d = _conv_desc(x.N, x.H, x.W, Cin, Cout, KH, KW, stride, pad_t, pad_l, Ho, Wo, upsample)
    y = torch.empty(x.N * Ho * Wo, Cout, dtype=BF16, device=x.t.device)
    _check2d(x.t, "x")
    if not x.t.is_contiguous():
        raise ValueError("conv2d: x must be dense channels-last")
    tiles = query("nk_conv2d_stats_tiles", C.byref(d), stats_groups) if stats_groups else 0
    sums_out = None
    up2 = (upsample and KH == 3 and KW == 3 and stride == 1 and pad_t == 1 and not asym_pad and rowvec is None and residual is None and not tiles
           and up2_phases_take(x.N * x.H * x.W, Cin, Cout))
    if tiles:
        dev = x.t.device
        part = torch.empty(x.N, tiles, 2 * stats_groups, dtype=torch.float32, device=dev)
        call("nk_conv2d_fwd_stats", C.byref(d), x.t.data_ptr(), w2d(weight).data_ptr(), _p(bias), _p(rowvec), _p(residual), y.data_ptr(),
             part.data_ptr(), stats_groups, _stream())
        sums_out = torch.empty(x.N, 2 * stats_groups, dtype=torch.float32, device=dev)
        ws = _ws(query("nk_groupnorm_sums_ws_floats", x.N, tiles, stats_groups), dev)
        call("nk_groupnorm_sums_from_parts", part.data_ptr(), sums_out.data_ptr(), ws.data_ptr(), x.N, tiles, stats_groups, _stream())
    elif (cin_real in (3, 4) and Cin == 8 and KH == 3 and KW == 3 and stride == 1 and pad_t == 1 and not asym_pad and not upsample and rowvec is None
          and residual is None and Cout % 8 == 0):
        call("nk_conv3x3_few_channels_fwd", x.t.data_ptr(), w2d(weight).data_ptr(), _p(bias), y.data_ptr(), x.N, x.H, x.W, Cout, cin_real, _stream())
    elif up2:
        # the four 2 x 2 phase convolutions of x (nk_conv2d_up2_*): wp / wd are the summed weights of this step, wd kept for the input gradient
        dev = x.t.device
        wp = torch.empty(16 * Cout * Cin, dtype=BF16, device=dev)
        wd = torch.empty(16 * Cout * Cin, dtype=BF16, device=dev) if need_dx else None
        call("nk_up2_phase_weights", w2d(weight).data_ptr(), wp.data_ptr(), _p(wd), Cout, Cin, _stream())
        ws = torch.empty(query("nk_conv2d_up2_ws_bytes", C.byref(d), 0), dtype=torch.uint8, device=dev)
        call("nk_conv2d_up2_fwd", C.byref(d), x.t.data_ptr(), wp.data_ptr(), _p(bias), y.data_ptr(), ws.data_ptr(), _stream())
        del wp, ws
    else:
        call("nk_conv2d_fwd", C.byref(d), x.t.data_ptr(), w2d(weight).data_ptr(), _p(bias), _p(rowvec), _p(residual), y.data_ptr(), _stream())
    out = Img(y, x.N, Ho, Wo, sums_out)

    def up2_wgrad(dy: Tensor):
        ws = torch.empty(query("nk_conv2d_up2_ws_bytes", C.byref(d), 2), dtype=torch.uint8, device=dy.device)
        if bias is not None:
            call("nk_conv2d_up2_wgrad_bias", C.byref(d), dy.data_ptr(), x.t.data_ptr(), g2d(weight).data_ptr(), grad_flat(bias).data_ptr(), wgrad_mode(weight),
                 ws.data_ptr(), _stream())
        else:
            call("nk_conv2d_up2_wgrad", C.byref(d), dy.data_ptr(), x.t.data_ptr(), g2d(weight).data_ptr(), wgrad_mode(weight), ws.data_ptr(), _stream())

    def bwd(dy: Tensor):
        _check2d(dy, "dy")
        if not dy.is_contiguous():
            raise ValueError("conv2d bwd: dy must be dense")
        acc = state_of(weight).grad_accumulate

        if weight.requires_grad and up2:
            on_wgrad_stream(lambda: up2_wgrad(dy), dy, x.t, owner=weight)
        elif weight.requires_grad:          # frozen convolutions (the LPIPS trunk) only pass the gradient through
            if bias is not None:       # the bias gradient rides in the weight-gradient launch
                on_wgrad_stream(lambda: call("nk_conv2d_wgrad_bias", C.byref(d), dy.data_ptr(), x.t.data_ptr(), g2d(weight).data_ptr(), grad_flat(bias).data_ptr(),
                                             wgrad_mode(weight), _stream()), dy, x.t, owner=weight)
            else:
                on_wgrad_stream(lambda: call("nk_conv2d_wgrad", C.byref(d), dy.data_ptr(), x.t.data_ptr(), g2d(weight).data_ptr(), wgrad_mode(weight), _stream()),
                                dy, x.t, owner=weight)
        drow = None
        if rowvec is not None:
            drow32 = torch.empty(x.N, Cout, dtype=torch.float32, device=dy.device)
            ws = _ws(x.N * query("nk_colsum_ws_floats", Ho * Wo, Cout), dy.device)
            call("nk_colsum_batched", dy.data_ptr(), drow32.data_ptr(), ws.data_ptr(), Ho * Wo, Cout, dy.stride(0), x.N, 0, _stream())   # one pair of launches, not one per image
            drow = cast_bf16(drow32)
        dx = None
        if need_dx and up2:       # one 4 x 4 / stride 2 convolution of dy straight onto the low-resolution grid
            dxt = torch.empty(x.N * x.H * x.W, Cin, dtype=BF16, device=dy.device)
            call("nk_conv2d_up2_dgrad", C.byref(d), dy.data_ptr(), wd.data_ptr(), dxt.data_ptr(), _stream())
            dx = Img(dxt, x.N, x.H, x.W)
        elif need_dx:
            dxt = torch.empty(x.N * Hin * Win, Cin, dtype=BF16, device=dy.device)
            # the input gradient of a stride-1 3 x 3 "same" convolution is such a convolution of dy with the mirrored, channel-swapped
            # weights: where the halo-tile forward kernel takes that shape it runs there (one small transposing pass over the weights,
            # re-done per step because they change), otherwise on the transposed-operand gather kernel
            if query("nk_conv2d_dgrad_flipped_ok", C.byref(d)):
                wt = torch.empty(Cin * 9 * Cout, dtype=BF16, device=dy.device)
                call("nk_conv_weight_flip", w2d(weight).data_ptr(), wt.data_ptr(), Cout, Cin, 9, _stream())
                call("nk_conv2d_dgrad_flipped", C.byref(d), dy.data_ptr(), wt.data_ptr(), dxt.data_ptr(), _stream())
            else:
                call("nk_conv2d_dgrad", C.byref(d), dy.data_ptr(), w2d(weight).data_ptr(), dxt.data_ptr(), _stream())
            if upsample:
                dsm = torch.empty(x.N * x.H * x.W, Cin, dtype=BF16, device=dy.device)
                call("nk_upsample2x_bwd", dxt.data_ptr(), dsm.data_ptr(), x.N, x.H, x.W, Cin, _stream())
                dxt = dsm
            dx = Img(dxt, x.N, x.H, x.W)
        return dx, drow

    return out, bwd


# ------------------------------------------------------------------------------------------------
# norms / activations
# ------------------------------------------------------------------------------------------------
def groupnorm_fwd(x: Img, weight: Tensor, bias: Tensor, groups: int, eps: float, silu: bool, mod: Optional[Tensor] = None):
    """GroupNorm (+SiLU).  bwd(dy, dx_add=None) -> dx token matrix.
    With mod, the scale-shift modulated form: y = silu?(GN(x) * (1 + scale) + shift), mod = bf16 [N, 2C] with scale in the first C columns and
    shift in the last (ResBlock use_scale_shift_norm, openaimodel.py:332-336); bwd(dy, dx_add=None) -> (dx token matrix, dmod [N, 2C])."""
    what = "groupnorm" if mod is None else "groupnorm_mod"
    if not x.t.is_contiguous():
        raise ValueError(f"{what}: x must be dense channels-last")
    N, HW, Cc = x.N, x.H * x.W, x.C
    if mod is not None:
        _check2d(mod, "mod")
        if tuple(mod.shape) != (N, 2 * Cc) or not mod.is_contiguous():
            raise ValueError(f"groupnorm_mod: mod must be a dense [{N}, {2 * Cc}] (scale | shift) matrix, got {tuple(mod.shape)}")
    entry, mp = "nk_" + what, () if mod is None else (mod.data_ptr(),)      # the modulated entry points take mod behind beta
    y = torch.empty_like(x.t)
    mean = torch.empty(N, groups, dtype=torch.float32, device=x.t.device)
    rstd = torch.empty_like(mean)
    nws = query("nk_groupnorm_ws_floats", N, HW, Cc, groups)
    if x.sums is not None and x.sums.shape == (N, 2 * groups):
        # the producer's statistics epilogue already summed x: the normalisation pass alone
        call(entry + "_apply", x.t.data_ptr(), x.sums.data_ptr(), weight.data_ptr(), bias.data_ptr(), *mp, y.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), N, HW, Cc, groups, float(eps), int(silu), _stream())
    else:
        ws = _ws(nws, x.t.device)
        call(entry + "_fwd", x.t.data_ptr(), weight.data_ptr(), bias.data_ptr(), *mp, y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
             ws.data_ptr(), N, HW, Cc, groups, float(eps), int(silu), _stream())

    def bwd(dy: Tensor, dx_add: Optional[Tensor] = None):
        dx = torch.empty_like(x.t)
        dmod = () if mod is None else (torch.empty_like(mod),)
        ws2 = _ws(nws, dy.device)
        call(entry + "_bwd", dy.data_ptr(), x.t.data_ptr(), weight.data_ptr(), bias.data_ptr(), *mp, mean.data_ptr(), rstd.data_ptr(),
             _p(dx_add), dx.data_ptr(), grad_flat(weight).data_ptr(), grad_flat(bias).data_ptr(), *(t.data_ptr() for t in dmod), ws2.data_ptr(),
             N, HW, Cc, groups, int(silu), int(state_of(weight).grad_accumulate), _stream())
        return (dx, *dmod) if dmod else dx

    return Img(y, x.N, x.H, x.W), bwd


def groupnorm_mod_fwd(x: Img, weight: Tensor, bias: Tensor, mod: Tensor, groups: int, eps: float, silu: bool):
    """groupnorm_fwd with the per-image scale-shift modulation mod (required here): bwd -> (dx, dmod)."""
    if mod is None:
        raise ValueError("groupnorm_mod: mod is required")
    return groupnorm_fwd(x, weight, bias, groups, eps, silu, mod=mod)


def layernorm_fwd(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5):
    """LayerNorm over the last dim of a dense token matrix.  bwd(dy, dx_add=None) -> dx."""
    _check2d(x, "x")
    if not x.is_contiguous():
        raise ValueError("layernorm: x must be dense")
    M, Cc = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    call("nk_layernorm_fwd", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, Cc, float(eps), _stream())

    def bwd(dy: Tensor, dx_add: Optional[Tensor] = None):
        dx = torch.empty_like(x)
        acc = state_of(weight).grad_accumulate
        if os.environ.get("NK_LN_FUSED", "1") != "0":
            # one pass over dy and x (round 5): dx and one row of dgamma / dbeta partials per workgroup; the rows are reduced later, off the
            # critical path -- with the block's other LayerNorms in ONE launch behind its batched weight gradients when a WgradQueue is
            # open (BasicTransformerBlock.bwd), else right away on the weight-gradient stream
            rows = query("nk_layernorm_part_rows", M)
            part = torch.empty(rows * 2 * Cc, dtype=torch.float32, device=dy.device)
            call("nk_layernorm_bwd_rows", dy.data_ptr(), x.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dx_add),
                 dx.data_ptr(), part.data_ptr(), M, Cc, _stream())
            entry = (part, grad_flat(weight), grad_flat(bias), rows, Cc, bool(acc))
            if _wgrad_queue is not None:
                _wgrad_queue.add_colpart(*entry)
            else:
                on_wgrad_stream(lambda: colpart_reduce([entry]), part, owner=weight)
            return dx
        # NK_LN_FUSED=0: the three-kernel form of rounds 2-4 (dx on the main chain; a second pass over dy, x for the parameter gradients and
        # their column reduce on the weight-gradient stream)
        ws = _ws(query("nk_layernorm_ws_floats", M, Cc), dy.device)
        call("nk_layernorm_bwd_dx", dy.data_ptr(), x.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dx_add),
             dx.data_ptr(), M, Cc, _stream())

        def params():   # gamma / beta gradients
            call("nk_layernorm_bwd_params", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                 grad_flat(weight).data_ptr(), grad_flat(bias).data_ptr(), ws.data_ptr(), M, Cc, int(acc), _stream())

        st_ = state_of(weight)
        if st_.norm_params_on_side_stream if st_.norm_params_on_side_stream is not None else st_.deferred is not None:
            on_wgrad_stream(params, dy, x, mean, rstd, ws, owner=weight)
        else:
            params()
        return dx

    return y, bwd


def rmsnorm(x: Tensor, weight: Tensor, eps: float = 1e-6) -> Tensor:
    """T5LayerNorm over the last dim of a dense bf16 token matrix: x * rsqrt(mean(x^2) + eps) * weight (fp32 weight); forward only."""
    _check2d(x, "x")
    if not x.is_contiguous():
        raise ValueError("rmsnorm: x must be dense")
    M, Cc = x.shape
    if weight.dtype != torch.float32 or weight.numel() != Cc or not weight.is_contiguous():
        raise ValueError(f"rmsnorm: weight must be a dense fp32 vector of {Cc} elements, got {weight.dtype} {tuple(weight.shape)}")
    y = torch.empty_like(x)
    call("nk_rmsnorm_fwd", x.data_ptr(), weight.data_ptr(), y.data_ptr(), M, Cc, float(eps), _stream())
    return y


def rmsnorm_fwd(x: Tensor, weight: Tensor, eps: float = 1e-6):
    """rmsnorm with its backward (the T5 towers under training): (y, bwd(dy, dx_add=None) -> dx), y with rmsnorm()'s bits.  bwd writes
    weight.grad in the parameter's engine mode (nk_rmsnorm_bwd: partial rows and the fixed-order column reducer)."""
    _check2d(x, "x")
    if not x.is_contiguous():
        raise ValueError("rmsnorm: x must be dense")
    M, Cc = x.shape
    if weight.dtype != torch.float32 or weight.numel() != Cc or not weight.is_contiguous():
        raise ValueError(f"rmsnorm: weight must be a dense fp32 vector of {Cc} elements, got {weight.dtype} {tuple(weight.shape)}")
    y = torch.empty_like(x)
    rstd = torch.empty(M, dtype=torch.float32, device=x.device)
    call("nk_rmsnorm_fwd_rstd", x.data_ptr(), weight.data_ptr(), y.data_ptr(), rstd.data_ptr(), M, Cc, float(eps), _stream())

    def bwd(dy: Tensor, dx_add: Optional[Tensor] = None) -> Tensor:
        if dy.shape != x.shape or dy.dtype != BF16 or not dy.is_contiguous():
            raise ValueError("rmsnorm bwd: dy must be a dense bf16 tensor of x's shape")
        if dx_add is not None and (dx_add.shape != x.shape or dx_add.dtype != BF16 or not dx_add.is_contiguous()):
            raise ValueError("rmsnorm bwd: dx_add must be a dense bf16 tensor of x's shape")
        dx = torch.empty_like(x)
        ws = _ws(query("nk_rmsnorm_bwd_ws_floats", M, Cc), x.device)
        call("nk_rmsnorm_bwd", dy.data_ptr(), x.data_ptr(), weight.data_ptr(), rstd.data_ptr(), _p(dx_add), dx.data_ptr(), grad_flat(weight).data_ptr(),
             ws.data_ptr(), M, Cc, int(state_of(weight).grad_accumulate), _stream())
        return dx

    return y, bwd


GATED_ACT_KINDS = ("gated-gelu", "gelu_new", "relu")


def gated_act_fwd(u: Tensor, kind: str):
    """gated_act with its backward: (y, bwd(dy) -> du), du of u's shape (nk_gated_gelu_tanh_bwd; nk_act_bwd modes 2 / 3 for the ungated kinds)"""
    y = gated_act(u, kind)

    def bwd(dy: Tensor) -> Tensor:
        if dy.shape != y.shape or dy.dtype != BF16 or not dy.is_contiguous():
            raise ValueError(f"gated_act bwd: dy must be a dense bf16 {tuple(y.shape)} tensor")
        du = torch.empty_like(u)
        if kind == "gated-gelu":
            call("nk_gated_gelu_tanh_bwd", dy.data_ptr(), u.data_ptr(), du.data_ptr(), u.shape[0], u.shape[1] // 2, _stream())
        else:
            call("nk_act_bwd", dy.data_ptr(), u.data_ptr(), du.data_ptr(), u.numel(), 2 if kind == "gelu_new" else 3, _stream())
        return du

    return y, bwd


def gated_act(u: Tensor, kind: str) -> Tensor:
    """The activation of a T5 FeedForward on the dense bf16 output u of its input projection, forward only.  "gated-gelu" (T5 v1.1, ByT5):
    u [M, 2 I] = [wi_0 x | wi_1 x] -> gelu_new(u[:, :I]) * u[:, I:], [M, I]; "gelu_new" and "relu" (T5 v1.0) are ungated, [M, I] -> [M, I]."""
    _check2d(u, "u")
    if not u.is_contiguous():
        raise ValueError("gated_act: u must be dense")
    if kind == "gated-gelu":
        M, I2 = u.shape
        if I2 % 16:
            raise ValueError(f"gated_act: u must be [M, 2 I] with I % 8 == 0, got {tuple(u.shape)}")
        y = torch.empty(M, I2 // 2, dtype=BF16, device=u.device)
        call("nk_gated_gelu_tanh_fwd", u.data_ptr(), y.data_ptr(), M, I2 // 2, _stream())
        return y
    if kind in ("gelu_new", "relu"):
        y = torch.empty_like(u)
        call("nk_gelu_fwd", u.data_ptr(), y.data_ptr(), u.numel(), 2 if kind == "gelu_new" else 3, _stream())
        return y
    raise ValueError(f"gated_act: kind must be one of {GATED_ACT_KINDS}, got {kind!r}")


def geglu_fwd(u: Tensor):
    _check2d(u, "u")
    M, I2 = u.shape
    inner = I2 // 2
    y = torch.empty(M, inner, dtype=BF16, device=u.device)
    call("nk_geglu_fwd", u.data_ptr(), y.data_ptr(), M, inner, _stream())

    def bwd(dy: Tensor):
        du = torch.empty_like(u)
        call("nk_geglu_bwd", dy.data_ptr(), u.data_ptr(), du.data_ptr(), M, inner, _stream())
        return du

    return y, bwd


def gelu(x: Tensor, quick: bool = False) -> Tensor:
    """exact GELU, or x * sigmoid(1.702 x) with quick=True; forward only (frozen text encoders; gelu_fwd has the backward)"""
    y = torch.empty_like(x)
    call("nk_gelu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), int(quick), _stream())
    return y


def gelu_fwd(x: Tensor, quick: bool = False):
    """(gelu(x), bwd) for the trainable text towers; bwd(dy) -> dx = dy * gelu'(x) (nk_gelu_bwd, same mode)"""
    if not x.is_contiguous():
        raise ValueError("gelu_fwd: x must be dense")
    y = gelu(x, quick)

    def bwd(dy: Tensor) -> Tensor:
        if dy.shape != x.shape or dy.dtype != BF16 or not dy.is_contiguous():
            raise ValueError("gelu bwd: dy must be a dense bf16 tensor of x's shape")
        dx = torch.empty_like(x)
        call("nk_gelu_bwd", dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), int(quick), _stream())
        return dx

    return y, bwd


EMBEDDING_BWD_MAX_TOKENS = 8192      # include/neurosis_hip.h: NK_EMBEDDING_BWD_MAX_TOKENS


def embedding_bwd(ids: Tensor, dx: Tensor, table: Tensor, positions: Optional[Tensor]) -> None:
    """Gradients of x[b * L + l] = table[ids[b, l]] + positions[l] (the text towers' embedding) written into table.grad / positions.grad
    (fp32), in the parameters' engine mode: the first micro-batch overwrites (rows nothing hit come out zero), later ones add.  Deterministic
    (nk_embedding_bwd: fixed-order sums, no atomics).  ids [B, L] int64; dx [B * L, C] bf16.  positions=None: no position table (T5)."""
    _check2d(dx, "dx")
    B, L = ids.shape
    V, Cc = table.shape
    P = positions.shape[0] if positions is not None else 0
    if ids.dtype != torch.int64 or not ids.is_contiguous() or dx.shape != (B * L, Cc) or (positions is not None and positions.shape[1] != Cc):
        raise ValueError(f"embedding_bwd: ids [B, L] int64 and dx [B * L, {Cc}] expected, got {tuple(ids.shape)} {ids.dtype}, {tuple(dx.shape)}")
    if B * L > EMBEDDING_BWD_MAX_TOKENS:
        raise NotImplementedError(f"embedding_bwd: at most {EMBEDDING_BWD_MAX_TOKENS} tokens per call (the duplicate-id scans are quadratic), got {B} x {L}")
    call("nk_embedding_bwd", ids.data_ptr(), dx.data_ptr(), dx.stride(0), grad_flat(table).data_ptr(),
         grad_flat(positions).data_ptr() if positions is not None else None, B, L, V, P, Cc, wgrad_mode(table), _stream())


def _label_ids(ids: Tensor, op: str) -> Tensor:
    if not ids.is_cuda:
        raise NotImplementedError(f"{op}: ids is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if ids.dim() != 1 or ids.dtype != torch.int64:
        raise ValueError(f"{op}: ids must be an int64 [B] tensor, got {tuple(ids.shape)} {ids.dtype}")
    return ids.contiguous()


def label_rows(table: Tensor, ids: Tensor, add: Optional[Tensor] = None, out_dtype=torch.float32) -> Tensor:
    """out[b] = table[ids[b]] (+ add[b]) (nk_label_rows_fwd): the label embedding of a class-conditional UNet and ClassEmbedder.  table fp32
    [V, D] (the master itself: one rounding, at the end), ids int64 [B], add bf16 [B, D]; out [B, D] fp32 or bf16.  An id outside [0, V) gives
    a NaN row: it is never an address and cannot pass unnoticed."""
    ids = _label_ids(ids, "label_rows")
    t = table.detach()
    if not t.is_cuda:
        raise NotImplementedError("label_rows: table is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or t.shape[1] % 8:
        raise ValueError(f"label_rows: table must be a dense fp32 [V, D] matrix with D % 8 == 0, got {tuple(t.shape)} {t.dtype}")
    if out_dtype not in (torch.float32, BF16):
        raise ValueError(f"label_rows: out_dtype is torch.float32 or torch.bfloat16, got {out_dtype}")
    V, D = t.shape
    B = ids.shape[0]
    if add is not None and (add.shape != (B, D) or add.dtype != BF16 or not add.is_contiguous() or not add.is_cuda):
        raise ValueError(f"label_rows: add must be a dense bf16 [{B}, {D}] tensor, got {tuple(add.shape)} {add.dtype}")
    out = torch.empty(B, D, dtype=out_dtype, device=t.device)
    call("nk_label_rows_fwd", t.data_ptr(), ids.data_ptr(), _p(add), out.data_ptr(), int(out_dtype == torch.float32), B, V, D, _stream())
    return out


def label_rows_bwd(ids: Tensor, d: Tensor, table: Tensor) -> None:
    """The gradient of label_rows written into table.grad (fp32) in the parameter's engine mode, as embedding_bwd does (whose kernel this is,
    with one token per sample and no position table): the first micro-batch overwrites the whole table -- rows no sample hit come out zero --,
    later ones add.  Each row is the fp32 sum of its samples' rows of d in ascending b: the same bits on every run.  d [B, D] bf16 or fp32."""
    ids = _label_ids(ids, "label_rows_bwd")
    if not d.is_cuda:
        raise NotImplementedError("label_rows_bwd: d is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    B = ids.shape[0]
    V, D = table.shape
    if d.dim() != 2 or d.shape != (B, D) or d.dtype not in (torch.float32, BF16) or d.stride(1) != 1:
        raise ValueError(f"label_rows_bwd: d must be a bf16 or fp32 [{B}, {D}] matrix with unit inner stride, got {tuple(d.shape)} {d.dtype}")
    if B > EMBEDDING_BWD_MAX_TOKENS:
        raise NotImplementedError(f"label_rows_bwd: at most {EMBEDDING_BWD_MAX_TOKENS} samples per call (the duplicate-id scans are quadratic), got {B}")
    call("nk_label_rows_bwd", ids.data_ptr(), d.data_ptr(), d.stride(0), int(d.dtype == torch.float32), grad_flat(table).data_ptr(), B, V, D,
         wgrad_mode(table), _stream())


def linear1_fwd(y: Tensor, weight: Tensor, bias: Tensor, add: Optional[Tensor] = None, need_dy: bool = False):
    """nn.Linear(1, D) on y fp32 [B, 1] (the "continuous" label embedding): out bf16 [B, D] = y weight^T + bias (+ add), fp32 arithmetic on the
    fp32 masters, one rounding (nk_linear1_fwd; K = 1 is no shape for the MFMA GEMMs).  bwd(d) -> dy fp32 [B, 1] (None unless need_dy) and
    writes weight.grad [D, 1] / bias.grad [D] in the parameters' engine mode: sums over b in ascending order."""
    if not y.is_cuda:
        raise NotImplementedError("linear1_fwd: y is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    D = weight.shape[0]
    if y.dim() != 2 or y.shape[1] != 1 or y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError(f"linear1_fwd: y must be a dense fp32 [B, 1] tensor, got {tuple(y.shape)} {y.dtype}")
    if tuple(weight.shape) != (D, 1) or tuple(bias.shape) != (D,) or weight.dtype != torch.float32 or bias.dtype != torch.float32 or D % 8:
        raise ValueError(f"linear1_fwd: weight fp32 [D, 1] and bias fp32 [D] with D % 8 == 0 expected, got {tuple(weight.shape)} {tuple(bias.shape)}")
    B = y.shape[0]
    if add is not None and (add.shape != (B, D) or add.dtype != BF16 or not add.is_contiguous()):
        raise ValueError(f"linear1_fwd: add must be a dense bf16 [{B}, {D}] tensor, got {tuple(add.shape)} {add.dtype}")
    out = torch.empty(B, D, dtype=BF16, device=y.device)
    call("nk_linear1_fwd", y.data_ptr(), weight.data_ptr(), bias.data_ptr(), _p(add), out.data_ptr(), B, D, _stream())

    def bwd(d: Tensor) -> Optional[Tensor]:
        if d.shape != (B, D) or d.dtype != BF16 or not d.is_contiguous():
            raise ValueError(f"linear1 bwd: d must be a dense bf16 [{B}, {D}] tensor, got {tuple(d.shape)} {d.dtype}")
        dy = torch.empty(B, 1, dtype=torch.float32, device=d.device) if need_dy else None
        call("nk_linear1_bwd", d.data_ptr(), y.data_ptr(), weight.data_ptr(), grad_flat(weight).data_ptr(), grad_flat(bias).data_ptr(), _p(dy), B, D,
             wgrad_mode(weight), _stream())
        return dy

    return out, bwd


def gather_rows_bwd(dsel: Tensor, idx: Tensor, L: int) -> Tensor:
    """backward of sel[b] = x[b * L + idx[b]]: the dense [B * L, C] gradient of x, zero except the gathered rows (nk_gather_rows_bwd)"""
    _check2d(dsel, "dsel")
    B, Cc = dsel.shape
    if idx.shape != (B,) or idx.dtype != torch.int64 or not idx.is_contiguous():
        raise ValueError("gather_rows_bwd: idx must be a dense int64 [B] tensor")
    dx = torch.empty(B * L, Cc, dtype=BF16, device=dsel.device)
    call("nk_gather_rows_bwd", dsel.data_ptr(), dsel.stride(0), idx.data_ptr(), dx.data_ptr(), B, L, Cc, _stream())
    return dx


def wgrad_few_rows(x: Tensor, dy: Tensor, dw: Tensor, accumulate: bool) -> None:
    """dw [K, N] fp32 (+)= x^T dy over the M <= 256 rows of x [M, K] and dy [M, N] (nk_wgrad_few_rows)"""
    _check2d(x, "x")
    _check2d(dy, "dy")
    M, K = x.shape
    N = dy.shape[1]
    if dy.shape[0] != M or dw.shape != (K, N) or dw.dtype != torch.float32 or dw.stride(1) != 1:
        raise ValueError(f"wgrad_few_rows: bad shapes {tuple(x.shape)} {tuple(dy.shape)} {tuple(dw.shape)}")
    call("nk_wgrad_few_rows", x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), dw.data_ptr(), dw.stride(0), M, K, N, int(accumulate), _stream())


def leaky_relu_fwd(x: Tensor, slope: float = 0.2):
    """(y, bwd); bwd(dy) -> dx"""
    y = torch.empty_like(x)
    call("nk_leaky_relu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), float(slope), _stream())

    def bwd(dy: Tensor) -> Tensor:
        dx = torch.empty_like(dy)
        call("nk_leaky_relu_bwd", dy.data_ptr(), y.data_ptr(), dx.data_ptr(), dy.numel(), float(slope), _stream())
        return dx

    return y, bwd


def maxpool2x2_fwd(x: Img):
    """2x2 / stride 2 max pooling on channels-last tokens.  (y Img, bwd); bwd(dy tokens) -> dx tokens"""
    y = torch.empty(x.N * (x.H // 2) * (x.W // 2), x.C, dtype=BF16, device=x.t.device)
    call("nk_maxpool2x2_fwd", x.t.data_ptr(), y.data_ptr(), x.N, x.H, x.W, x.C, _stream())

    def bwd(dy: Tensor) -> Tensor:
        dx = torch.empty_like(x.t)
        call("nk_maxpool2x2_bwd", dy.data_ptr(), x.t.data_ptr(), dx.data_ptr(), x.N, x.H, x.W, x.C, _stream())
        return dx

    return Img(y, x.N, x.H // 2, x.W // 2), bwd


def avgpool2x_fwd(x: Img):
    """avg_pool2d(2, 2) (floor mode: an odd last row or column is dropped) on channels-last tokens -- Downsample(use_conv=False) and the
    down ResBlock (openaimodel.py:146-197).  (y Img, bwd); bwd(dy tokens) -> dx tokens, zero where the forward read nothing."""
    if not x.t.is_contiguous():
        raise ValueError("avgpool2x: x must be dense channels-last")
    if x.H < 2 or x.W < 2:
        raise ValueError(f"avgpool2x: a {x.H} x {x.W} image has no 2 x 2 window")
    y = torch.empty(x.N * (x.H // 2) * (x.W // 2), x.C, dtype=BF16, device=x.t.device)
    call("nk_avgpool2x_fwd", x.t.data_ptr(), y.data_ptr(), x.N, x.H, x.W, x.C, _stream())
    N, H, W, Cc = x.N, x.H, x.W, x.C

    def bwd(dy: Tensor) -> Tensor:
        dx = torch.empty(N * H * W, Cc, dtype=BF16, device=dy.device)
        call("nk_avgpool2x_bwd", dy.data_ptr(), dx.data_ptr(), N, H, W, Cc, _stream())
        return dx

    return Img(y, N, H // 2, W // 2), bwd


def upsample2x_fwd(x: Img):
    """Nearest 2x upsampling as a materialised copy -- Upsample(use_conv=False) and the skip path of the up ResBlock (where a convolution
    follows, its gather does this for free: conv2d_fwd(upsample=True)).  (y Img, bwd); bwd(dy tokens) -> dx tokens."""
    if not x.t.is_contiguous():
        raise ValueError("upsample2x: x must be dense channels-last")
    N, H, W, Cc = x.N, x.H, x.W, x.C
    y = torch.empty(N * 4 * H * W, Cc, dtype=BF16, device=x.t.device)
    call("nk_upsample2x_fwd", x.t.data_ptr(), y.data_ptr(), N, H, W, Cc, _stream())

    def bwd(dy: Tensor) -> Tensor:
        dx = torch.empty(N * H * W, Cc, dtype=BF16, device=dy.device)
        call("nk_upsample2x_bwd", dy.data_ptr(), dx.data_ptr(), N, H, W, Cc, _stream())
        return dx

    return Img(y, N, 2 * H, 2 * W), bwd


def maxpool_fwd(x: Img, kernel_size: int, stride: int):
    """nn.MaxPool2d(kernel_size, stride) (no padding, floor mode) on channels-last tokens.  (y Img, bwd); bwd(dy tokens) -> dx tokens"""
    if kernel_size == 2 and stride == 2 and x.H % 2 == 0 and x.W % 2 == 0:
        return maxpool2x2_fwd(x)
    Ho, Wo = (x.H - kernel_size) // stride + 1, (x.W - kernel_size) // stride + 1
    y = torch.empty(x.N * Ho * Wo, x.C, dtype=BF16, device=x.t.device)
    call("nk_maxpool_fwd", x.t.data_ptr(), y.data_ptr(), x.N, x.H, x.W, x.C, kernel_size, stride, _stream())

    def bwd(dy: Tensor) -> Tensor:
        dx = torch.empty_like(x.t)
        call("nk_maxpool_bwd", dy.data_ptr(), x.t.data_ptr(), dx.data_ptr(), x.N, x.H, x.W, x.C, kernel_size, stride, _stream())
        return dx

    return Img(y, x.N, Ho, Wo), bwd


def lpips_layer(f0: Img, f1: Img, w: Tensor, out: Tensor, accumulate: bool, eps: float = 1e-10):
    """out[n] (+)= LPIPS distance of one feature layer (see nk_lpips_layer_fwd); returns bwd(upstream[N]) -> d/d f1 tokens"""
    N, HW, Cc = f0.N, f0.H * f0.W, f0.C
    ws = _ws(query("nk_lpips_layer_ws_floats", N, HW), f0.t.device)
    call("nk_lpips_layer_fwd", f0.t.data_ptr(), f1.t.data_ptr(), w.data_ptr(), out.data_ptr(), ws.data_ptr(), N, HW, Cc, float(eps), int(accumulate), _stream())

    def bwd(upstream: Tensor) -> Tensor:
        d = torch.empty_like(f1.t)
        call("nk_lpips_layer_bwd", f0.t.data_ptr(), f1.t.data_ptr(), w.data_ptr(), upstream.data_ptr(), d.data_ptr(), N, HW, Cc, float(eps), _stream())
        return d

    return bwd


def batchnorm_fwd(x: Tensor, weight: Tensor, bias: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], eps: float = 1e-5,
                  momentum: float = 0.1, slope: float = 1.0):
    """nn.BatchNorm2d in training mode on a token matrix [N*H*W, C] (batch statistics per channel), with the LeakyReLU that follows
    it in the PatchGAN fused in (slope 1.0 = none).  Updates the running statistics in place.  bwd(dy) -> dx."""
    _check2d(x, "x")
    if not x.is_contiguous():
        raise ValueError("batchnorm: x must be dense")
    M, Cc = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(Cc, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    nws = query("nk_batchnorm_ws_floats", M, Cc)
    call("nk_batchnorm_fwd", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(running_mean),
         _p(running_var), _ws(nws, x.device).data_ptr(), M, Cc, float(eps), float(momentum), float(slope), _stream())

    def bwd(dy: Tensor) -> Tensor:
        dx = torch.empty_like(x)
        call("nk_batchnorm_bwd", dy.data_ptr(), x.data_ptr(), y.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
             grad_flat(weight).data_ptr(), grad_flat(bias).data_ptr(), _ws(nws, x.device).data_ptr(), M, Cc, float(slope), int(state_of(weight).grad_accumulate),
             _stream())
        return dx

    return y, bwd


def batchnorm_eval(x: Tensor, weight: Tensor, bias: Tensor, running_mean: Tensor, running_var: Tensor, eps: float = 1e-5, slope: float = 1.0) -> Tensor:
    """nn.BatchNorm2d in evaluation mode on a token matrix [M, C] (running statistics), with the following LeakyReLU fused in."""
    _check2d(x, "x")
    if not x.is_contiguous():
        raise ValueError("batchnorm: x must be dense")
    M, Cc = x.shape
    y = torch.empty_like(x)
    call("nk_batchnorm_eval", x.data_ptr(), weight.data_ptr(), bias.data_ptr(), running_mean.data_ptr(), running_var.data_ptr(), y.data_ptr(),
         _ws(Cc + 64, x.device).data_ptr(), M, Cc, float(eps), float(slope), _stream())
    return y


def silu_fwd(x: Tensor):
    y = torch.empty_like(x)
    call("nk_silu_fwd", x.data_ptr(), y.data_ptr(), x.numel(), _stream())

    def bwd(dy: Tensor):
        dx = torch.empty_like(x)
        call("nk_silu_bwd", dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), _stream())
        return dx

    return y, bwd


# ------------------------------------------------------------------------------------------------
# dropout: counter-based masks, never stored (csrc/dropout.hip has the definition; tests/dropout_ref.py restates it)
# ------------------------------------------------------------------------------------------------
# One persistent {seed, step} pair of 64-bit words per device.  It is created on first use (seed = torch.initial_seed(), step = 0) and never
# reallocated: captured graphs hold its address, dropout_seed() writes INTO it.  A "draw" (nk_dropout_draw, one lane) advances the step and
# copies {seed, step} into a token; every mask of one micro-batch of one model reads that token, told apart by a site id.  Ranks seeded
# alike draw alike (as under Lightning's seed_everything): dropout_seed(seed + rank) is the way out.  The counter is not part of any
# state_dict (torch's generator state is not either).
_dropout = threading.local()          # .token: the current draw's token (per thread, like _recording)
_dropout_states: dict = {}            # device index -> int64 [2] tensor {seed, step}


def _as_i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def _dropout_state_tensor(device=None) -> Tensor:
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"dropout: the counter lives on a GPU, got device {dev}")
    idx = torch.cuda.current_device() if dev.index is None else dev.index
    st = _dropout_states.get(idx)
    if st is None:
        if capturing():
            raise RuntimeError("dropout: the first draw on a device cannot happen inside a hipGraph capture (it allocates the counter)")
        st = _dropout_states[idx] = torch.tensor([_as_i64(torch.initial_seed()), 0], dtype=torch.int64, device=torch.device("cuda", idx))
    return st


def dropout_seed(seed: int, step: int = 0, device=None) -> None:
    """Set the dropout counter of `device` (default: the current one) to (seed, step), in place: graphs captured earlier stay valid and draw
    from the new pair on their next replay."""
    st = _dropout_state_tensor(device)
    st.copy_(torch.tensor([_as_i64(int(seed)), _as_i64(int(step))], dtype=torch.int64))


def dropout_state(device=None) -> tuple:
    """(seed, step) of `device`'s dropout counter; step = the number of draws since dropout_seed / creation.  Synchronises."""
    seed, step = _dropout_state_tensor(device).tolist()
    return seed & ((1 << 64) - 1), step & ((1 << 64) - 1)


def dropout_consts(p: float) -> tuple:
    """(thr, scale) the kernel takes for rate p: keep iff the element's 16-bit half >= thr = round(p * 65536) (the rate is thereby quantised
    to 1 / 65536); scale = 1 / (1 - p), rounded to fp32 where it is passed"""
    return int(round(p * 65536)), 1.0 / (1.0 - p)


def check_dropout_rate(p, owner: str) -> float:
    """p in [0, 1) or ValueError naming `owner`.  (The reference's nn.Dropout also takes p = 1, all zeros: refused here, 1 / (1 - p) has no value.)"""
    try:
        ok = 0.0 <= float(p) < 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{owner}: dropout must be a rate in [0, 1), got {p!r}")
    return float(p)


def dropout_draw(device=None) -> Tensor:
    """Open a draw: advance `device`'s step and return the token {seed, step} (int64 [2], a fresh device tensor -- under a hipGraph capture it
    comes from the chain's pool, so every replay fills the same address).  The token becomes the current one of this thread: dropout_fwd binds
    it.  Callers: the entry of a training forward (dropout_open); backward, checkpoint re-runs and selective recompute never draw."""
    st = _dropout_state_tensor(device)
    tok = torch.empty(2, dtype=torch.int64, device=st.device)
    call("nk_dropout_draw", st.data_ptr(), tok.data_ptr(), _stream())
    _dropout.token = tok
    return tok


def dropout_open(top) -> bool:
    """Entry of a forward of module `top`: when some module under it is training with a dropout rate > 0, give every such module its site id
    -- its index in top.modules(), a function of the structure alone -- and draw.  Otherwise nothing happens (no launch, no step)."""
    sites = [(i, m) for i, m in enumerate(top.modules()) if m.training and getattr(m, "dropout_p", 0.0) > 0.0]
    if not sites:
        return False
    for i, m in sites:
        m.__dict__["_nk_site"] = i
    p = next(top.parameters(), None)
    dropout_draw(p.device if p is not None and p.is_cuda else None)
    return True


def dropout_site(module) -> int:
    """the site id dropout_open gave `module`; a module used on its own is index 0 of its own modules()"""
    return module.__dict__.get("_nk_site", 0)


def dropout_token(required: bool = True) -> Optional[Tensor]:
    tok = getattr(_dropout, "token", None)
    if tok is None and required:
        raise RuntimeError("dropout: no draw is open on this thread (ops.dropout_draw() / ops.dropout_open(module) at the entry of the forward)")
    return tok


class dropout_token_scope:
    """`with ops.dropout_token_scope(tok):` -- re-install the token of an earlier forward around its re-run (activation checkpointing)."""

    def __init__(self, token: Optional[Tensor]):
        self.token = token

    def __enter__(self):
        self.prev = getattr(_dropout, "token", None)
        _dropout.token = self.token

    def __exit__(self, *exc):
        _dropout.token = self.prev


def dropout_mask_like(x: Tensor, p: float, site: int, token: Tensor, residual: Optional[Tensor] = None, inplace: bool = True) -> Tensor:
    """Apply the (token, site) mask of rate p, times 1 / (1 - p), to the token matrix x [rows, cols] (+ residual): in place, or into a new dense
    tensor.  x may be a column slice of a wider buffer -- the mask goes by the LOGICAL index row * cols + col -- so one mask over [M, I]
    can be laid over each half of an [M, 2I] buffer.  cols % 8 == 0 and 16-byte-aligned rows."""
    _check2d(x, "x")
    rows, cols = x.shape
    y = x if inplace else torch.empty(rows, cols, dtype=BF16, device=x.device)
    if residual is not None:
        _check2d(residual, "residual")
        if residual.shape != x.shape:
            raise ValueError(f"dropout: residual {tuple(residual.shape)} does not match x {tuple(x.shape)}")
    for name, t in (("x", x), ("residual", residual)):
        if t is not None and (cols % 8 or t.stride(0) % 8 or t.data_ptr() % 16):
            raise ValueError(f"dropout: {name} needs cols % 8 == 0 and 16-byte-aligned rows, got shape {tuple(t.shape)} stride {t.stride()}")
    if token.dtype != torch.int64 or token.numel() != 2 or token.device != x.device:
        raise ValueError("dropout: token must be the int64 [2] tensor of ops.dropout_draw() on x's device")
    if rows == 0:
        return y
    thr, scale = dropout_consts(check_dropout_rate(p, "dropout"))
    call("nk_dropout", x.data_ptr(), _p(residual), y.data_ptr(), rows, cols, x.stride(0), residual.stride(0) if residual is not None else 0, y.stride(0),
         token.data_ptr(), int(site), thr, scale, _stream())
    return y


def dropout_fwd(x: Tensor, p: float, site: int, residual: Optional[Tensor] = None, inplace: bool = False):
    """nn.Dropout(p) in training mode on a token matrix, with an optional residual added behind it: y = residual + x * mask / (1 - p).
    The CURRENT token is bound into the closure, so a backward -- or a recomputation -- that runs after later draws regenerates the mask of
    its own forward.  bwd(dy, inplace=False) -> dx = dy * mask / (1 - p) (the residual branch is the caller's)."""
    tok = dropout_token()
    y = dropout_mask_like(x, p, site, tok, residual, inplace)

    def bwd(dy: Tensor, inplace: bool = False) -> Tensor:
        return dropout_mask_like(dy, p, site, tok, None, inplace)

    return y, bwd


def cat_fwd(a: Img, b: Img):
    """torch.cat([a, b], dim=1) on channels-last images.  bwd(dout) -> (da, db) token matrices."""
    if (a.N, a.H, a.W) != (b.N, b.H, b.W):
        raise ValueError("cat: spatial shapes differ")
    rows = a.t.shape[0]
    out = torch.empty(rows, a.C + b.C, dtype=BF16, device=a.t.device)
    call("nk_cat_channels", a.t.data_ptr(), b.t.data_ptr(), out.data_ptr(), rows, a.C, b.C, _stream())
    Ca, Cb = a.C, b.C

    def bwd(dout: Tensor):
        da = torch.empty(rows, Ca, dtype=BF16, device=dout.device)
        db = torch.empty(rows, Cb, dtype=BF16, device=dout.device)
        call("nk_split_channels", dout.data_ptr(), da.data_ptr(), db.data_ptr(), rows, Ca, Cb, _stream())
        return da, db

    return Img(out, a.N, a.H, a.W), bwd


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _attn_desc(q: Tensor, k: Tensor, v: Tensor, o: Tensor, B: int, heads: int, dim_head: int, scale: float, causal: bool) -> NkAttnDesc:
    """the kernels' problem record for q / o [B*Lq, H*D], k / v [B*Lk, H*D] token matrices (the gradient side: _attn_grads)"""
    d = NkAttnDesc()
    Lq, Lk = q.shape[0] // B, k.shape[0] // B
    d.B, d.H, d.Lq, d.Lk, d.D = B, heads, Lq, Lk, dim_head
    d.sq, d.sk, d.sv, d.so = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    d.bq, d.bk, d.bv, d.bo = Lq * q.stride(0), Lk * k.stride(0), Lk * v.stride(0), Lq * o.stride(0)
    d.scale = float(scale)
    d.causal = int(causal)
    return d


def _attn_grads(d: NkAttnDesc, who: str, do: Tensor, dq: Optional[Tensor], dk: Optional[Tensor], dv: Optional[Tensor]):
    """The gradient side of `d`: (dq, dk, dv), each allocated dense where not given (column slices of one buffer allowed where given) and
    held to its shape like do, with their strides written into d."""
    HD = d.H * d.D
    grads = []
    for n, t, L in (("do", do, d.Lq), ("dq", dq, d.Lq), ("dk", dk, d.Lk), ("dv", dv, d.Lk)):
        if t is None:
            t = torch.empty(d.B * L, HD, dtype=BF16, device=do.device)
        _check2d(t, n)
        if t.shape != (d.B * L, HD):
            raise ValueError(f"{who}: {n} must be [{d.B * L}, {HD}], got {tuple(t.shape)}")
        grads.append(t)
    do, dq, dk, dv = grads
    d.sdq, d.sdk, d.sdv, d.sdo = dq.stride(0), dk.stride(0), dv.stride(0), do.stride(0)
    d.bdq, d.bdk, d.bdv, d.bdo = d.Lq * dq.stride(0), d.Lk * dk.stride(0), d.Lk * dv.stride(0), d.Lq * do.stride(0)
    return dq, dk, dv


def attention_fwd(q: Tensor, k: Tensor, v: Tensor, B: int, heads: int, dim_head: int, causal: bool = False, need_lse: bool = True,
                  return_lse: bool = False):
    """softmax(q k^T / sqrt(d)) v.  q [B*Lq, H*D], k/v [B*Lk, H*D] token matrices (column slices allowed).
    bwd(do) -> (dq, dk, dv) dense token matrices.  causal=True has no backward here (attention_causal_fwd has one).
    dim_head = 512 (the VAE mid block): csrc/attn512.h forward (need_lse=False skips the log-sum-exp output: inference), csrc/attn512_bwd.h backward."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _check2d(t, n)
    Lq = q.shape[0] // B
    o = torch.empty(B * Lq, heads * dim_head, dtype=BF16, device=q.device)
    lse = torch.empty(B, heads, Lq, dtype=torch.float32, device=q.device) if (need_lse or dim_head != 512) else None
    d = _attn_desc(q, k, v, o, B, heads, dim_head, float(dim_head) ** -0.5, causal)
    call("nk_attention_fwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr() if lse is not None else None,
         _stream())

    def bwd(do: Tensor, dq: Optional[Tensor] = None, dk: Optional[Tensor] = None, dv: Optional[Tensor] = None):
        if dim_head > 160 and dim_head != 512:
            raise NotImplementedError("attention backward: head dim <= 160, or 512 (csrc/attn512_bwd.h)")
        if lse is None:
            raise ValueError("attention backward needs the forward's log-sum-exp: call attention_fwd(..., need_lse=True)")
        dq, dk, dv = _attn_grads(d, "attention_fwd bwd", do, dq, dk, dv)
        delta = _ws(query("nk_attention_bwd_ws_floats", C.byref(d)), do.device)
        call("nk_attention_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(),
             dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), _stream())
        return dq, dk, dv

    if return_lse:              # [B, heads, Lq] fp32, natural log of the row sums of exp(scale q k^T) (the chunked recompute backward rebuilds P from it)
        return o, bwd, lse
    return o, bwd


ATTN_RELBIAS_MAX_L = 1024      # csrc/attn_plan.h


def attention_relbias_fwd(q: Tensor, k: Tensor, v: Tensor, B: int, heads: int, dim_head: int, rel: Tensor, scale: float = 1.0) -> Tensor:
    """softmax(scale q k^T + rel[h][j - i + L - 1]) v, forward only: the T5 encoders' bidirectional self-attention with its relative position
    bias (T5 does not scale: scale = 1).  q / k / v [B*L, H*D] token matrices (column slices of a fused projection allowed); rel fp32
    [heads, 2 L - 1], indexed by key minus query position.  Returns the dense bf16 [B*L, H*D] output."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _check2d(t, n)
    L = q.shape[0] // B
    if k.shape[0] != q.shape[0] or v.shape[0] != q.shape[0]:
        raise ValueError("attention_relbias_fwd: self-attention (q, k and v over the same tokens)")
    if L > ATTN_RELBIAS_MAX_L:
        raise NotImplementedError(f"attention_relbias_fwd: at most {ATTN_RELBIAS_MAX_L} tokens per sequence (the head's bias table lives in LDS), got L = {L}")
    if rel.dtype != torch.float32 or tuple(rel.shape) != (heads, 2 * L - 1) or not rel.is_contiguous() or rel.device != q.device:
        raise ValueError(f"attention_relbias_fwd: rel must be a dense fp32 [{heads}, {2 * L - 1}] tensor on {q.device}, got {rel.dtype} {tuple(rel.shape)}")
    o = torch.empty(B * L, heads * dim_head, dtype=BF16, device=q.device)
    d = _attn_desc(q, k, v, o, B, heads, dim_head, scale, False)
    call("nk_attention_relbias_fwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), rel.data_ptr(), _stream())
    return o


def attention_relbias_train(q: Tensor, k: Tensor, v: Tensor, B: int, heads: int, dim_head: int, rel: Tensor, scale: float, d_rel: Tensor):
    """attention_relbias_fwd with its backward (the T5 towers under training): (o, bwd(do, dq=None, dk=None, dv=None) -> (dq, dk, dv)), o with
    attention_relbias_fwd's bits.  bwd ADDS the table's gradient into d_rel, fp32 [heads, 2 L - 1] (zeroed by the caller: one tower sums
    every layer into one buffer; bwd(..., accumulate=False) overwrites it); dq / dk / dv may be given as column slices of one buffer.
    Every output is bitwise reproducible."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _check2d(t, n)
    L = q.shape[0] // B
    if k.shape[0] != q.shape[0] or v.shape[0] != q.shape[0]:
        raise ValueError("attention_relbias_train: self-attention (q, k and v over the same tokens)")
    if L > ATTN_RELBIAS_MAX_L:
        raise NotImplementedError(f"attention_relbias_train: at most {ATTN_RELBIAS_MAX_L} tokens per sequence (the head's bias table lives in LDS), got L = {L}")
    for n, t in (("rel", rel), ("d_rel", d_rel)):
        if t.dtype != torch.float32 or tuple(t.shape) != (heads, 2 * L - 1) or not t.is_contiguous() or t.device != q.device:
            raise ValueError(f"attention_relbias_train: {n} must be a dense fp32 [{heads}, {2 * L - 1}] tensor on {q.device}, got {t.dtype} {tuple(t.shape)}")
    o = torch.empty(B * L, heads * dim_head, dtype=BF16, device=q.device)
    lse = torch.empty(B, heads, L, dtype=torch.float32, device=q.device)
    d = _attn_desc(q, k, v, o, B, heads, dim_head, scale, False)
    call("nk_attention_relbias_fwd_lse", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), rel.data_ptr(), _stream())

    def bwd(do: Tensor, dq: Optional[Tensor] = None, dk: Optional[Tensor] = None, dv: Optional[Tensor] = None, accumulate: bool = True):
        dq, dk, dv = _attn_grads(d, "attention_relbias_train bwd", do, dq, dk, dv)
        ws = _ws(query("nk_attention_relbias_bwd_ws_floats", C.byref(d)), do.device)
        call("nk_attention_relbias_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(),
             dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), rel.data_ptr(), d_rel.data_ptr(), ws.data_ptr(), int(accumulate), _stream())
        return dq, dk, dv

    bwd.lse = lse      # (tests read it)
    return o, bwd


def relbias_bucket_sum(d_rel: Tensor, buckets: Tensor, weight: Tensor) -> None:
    """relative_attention_bias.weight's gradient [num_buckets, heads] from the table's, d_rel fp32 [heads, 2 L - 1]: every table entry added
    to its bucket's row in a fixed order, into weight.grad in the parameter's engine mode (ops.wgrad_mode, as embedding_bwd).  buckets:
    the int tensor [2 L - 1] of relative_buckets()."""
    heads, nrel = d_rel.shape
    if d_rel.dtype != torch.float32 or not d_rel.is_contiguous() or tuple(weight.shape[1:]) != (heads,) or buckets.numel() != nrel or nrel % 2 == 0:
        raise ValueError(f"relbias_bucket_sum: d_rel fp32 [heads, 2 L - 1], buckets [2 L - 1] and weight [num_buckets, heads] expected, got "
                         f"{tuple(d_rel.shape)} {tuple(buckets.shape)} {tuple(weight.shape)}")
    b32 = buckets.to(device=d_rel.device, dtype=torch.int32).contiguous()
    call("nk_relbias_bucket_sum", d_rel.data_ptr(), b32.data_ptr(), grad_flat(weight).data_ptr(), heads, (nrel + 1) // 2, weight.shape[0],
         wgrad_mode(weight), _stream())


def attention_causal_fwd(q: Tensor, k: Tensor, v: Tensor, B: int, heads: int, dim_head: int = 64):
    """Causal self-attention WITH a backward (the trained text towers): the forward is attention_fwd(causal=True), launch for launch;
    bwd(do, dq=None, dk=None, dv=None) -> (dq, dk, dv) through nk_attention_bwd_causal (head dim 64, at most 96 tokens).  dq / dk / dv may be
    given as column slices of one buffer (the packed QKV projection's gradient)."""
    L = q.shape[0] // B
    if dim_head != 64 or L > 96 or k.shape[0] != q.shape[0] or v.shape[0] != q.shape[0]:
        raise NotImplementedError(f"attention_causal_fwd: the backward takes head dim 64 and at most 96 tokens (self-attention), got D = {dim_head}, L = {L}")
    o, _, lse = attention_fwd(q, k, v, B, heads, dim_head, causal=True, return_lse=True)

    def bwd(do: Tensor, dq: Optional[Tensor] = None, dk: Optional[Tensor] = None, dv: Optional[Tensor] = None):
        d = _attn_desc(q, k, v, o, B, heads, dim_head, float(dim_head) ** -0.5, True)
        dq, dk, dv = _attn_grads(d, "attention_causal_fwd bwd", do, dq, dk, dv)
        call("nk_attention_bwd_causal", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(),
             dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), _stream())
        return dq, dk, dv

    return o, bwd


def attention_unfused(q: Tensor, k: Tensor, v: Tensor, B: int) -> Tensor:
    """Single-head attention with any head dim via two MFMA GEMMs and a row softmax (inference only;
    the VAE mid block, modules/diffusion/model.py:224-243).  q/k/v dense [B*L, D]."""
    L = q.shape[0] // B
    D = q.shape[1]
    out = torch.empty_like(q)
    s = torch.empty(L, L, dtype=BF16, device=q.device)
    for b in range(B):
        sl = slice(b * L, (b + 1) * L)
        gemm_nt(q[sl], k[sl], alpha=float(D) ** -0.5, out=s)
        call("nk_softmax_rows", s.data_ptr(), L, L, _stream())
        gemm_nn(s, v[sl], out=out[sl])
    return out


ATTN512_FLASH_MAX_L = 2048    # tokens per sample up to which the flash backward kernels are the faster form (NK_ATTN512_BWD=auto)
ATTN512_BWD_CHUNK = 2048      # query rows per backward chunk: the recomputed score / probability block is [chunk, L] bf16 (64 MB at L = 16384)


def attention512_fwd(q: Tensor, k: Tensor, v: Tensor, B: int):
    """Single-head attention of head dim 512 WITH a backward (the VAE mid block when the autoencoder is trained: modules/diffusion/model.py:224-243,
    models/autoencoder.py:280-293).  Forward: the one-kernel flash forward of csrc/attn512.h -- nothing of size L x L is kept (rounds 2-4 kept
    the [B, L, L] probabilities of a two-GEMM forward).  Backward, two forms (round 5):
      flash     -- csrc/attn512_bwd.h: one kernel template for dQ (32 queries per workgroup) and dK / dV (32 keys per workgroup), the scores
                   recomputed tile by tile in registers from the forward's log-sum-exp; nothing of size L x L anywhere;
      recompute -- per sample and per chunk of ATTN512_BWD_CHUNK query rows the probabilities are rebuilt through HBM (scores GEMM + row
                   softmax) and consumed at once by the four gradient GEMMs (dP = dO V^T, dV += P^T dO, dS = P o (dP - rowsum(P o dP)) / sqrt(D),
                   dQ = dS K, dK += dS^T Q): working set [chunk, L].
    q / k / v dense [B*L, D]; bwd(do) -> (dq, dk, dv)."""
    L, D = q.shape[0] // B, q.shape[1]
    if D != 512:
        raise ValueError(f"attention512_fwd: head dim 512 only, got {D} (head dims <= 160: attention_fwd)")
    scale = float(D) ** -0.5
    # NK_ATTN512_BWD: "auto" (default) = the flash backward kernels (csrc/attn512_bwd.h: scores recomputed tile by tile in registers from the
    # forward's log-sum-exp, nothing in HBM) up to ATTN512_FLASH_MAX_L tokens, the chunked recompute beyond; "1" / "0" force one or the other.
    # Measured (tools/bench_attn512_bwd.py, batch 4): L = 1024 (config 5) 250 vs 449 us; L = 4096 1.71 vs 1.17 ms; L = 16384 (batch 1) 6.6 vs
    # 2.8 ms -- the flash kernels are correct and lean, not tuned (one wave per SIMD, register-staged tiles): the tile engine's GEMMs win once
    # the [chunk, L] scratch is large enough to run them at speed.
    mode = os.environ.get("NK_ATTN512_BWD", "auto")
    if mode == "1" or (mode == "auto" and L <= ATTN512_FLASH_MAX_L):
        out, b_att = attention_fwd(q, k, v, B, 1, D, need_lse=True)
        return out, (lambda do: b_att(do))
    # (nk_softmax_rows takes rows of whole 16-byte chunks only -- say so HERE, not in a backward that follows a forward which
    # accepted the shape.  The recompute form rebuilds P from bf16-ROUNDED scores (gemm_nt writes bf16), not from the flash forward's fp32
    # scores: at logits of 30-50 the two differ by several per cent per element -- INTEGRATION.md section 6, NK_ATTN512_BWD.)
    if L % 8:
        raise ValueError(f"attention512_fwd: the chunked recompute backward (L = {L} > {ATTN512_FLASH_MAX_L} tokens per sample, or NK_ATTN512_BWD=0) "
                         f"needs L % 8 == 0; NK_ATTN512_BWD=1 selects the flash backward, which takes any length")
    out, _, lse = attention_fwd(q, k, v, B, 1, D, need_lse=True, return_lse=True)
    return out, _attention_recompute_bwd(q, k, v, B, lse=lse.reshape(B * L))


def attention_anydim_fwd(q: Tensor, k: Tensor, v: Tensor, B: int):
    """Single-head attention of ANY head dim (a multiple of 8) WITH a backward: the reference's AttnBlock trains at whatever channel count the
    autoencoder's last level has (modules/diffusion/model.py:224-243); head dims <= 160 and 512 have flash kernels (attention_fwd, attention512_fwd),
    everything else -- a VAE with ch * ch_mult[-1] of 256 or 384 -- takes this form: the two-GEMM forward of attention_unfused and
    the chunked recompute backward shared with attention512_fwd.  Working set [L, L] bf16 forward, [chunk, L] backward.  q / k / v dense [B*L, D]."""
    L, D = q.shape[0] // B, q.shape[1]
    if D % 8 or L % 8:
        raise ValueError(f"attention_anydim_fwd: head dim and tokens per sample must be multiples of 8, got D = {D}, L = {L}")
    return attention_unfused(q, k, v, B), _attention_recompute_bwd(q, k, v, B)


def _attention_recompute_bwd(q: Tensor, k: Tensor, v: Tensor, B: int, lse: Optional[Tensor] = None):
    """bwd(do) -> (dq, dk, dv) of single-head attention by recomputing the probabilities chunk by chunk (attention512_fwd has the formulae).

    lse ([B*L] fp32: the flash forward's log-sum-exp per query row) makes the rebuilt probabilities follow the forward's.  The scores
    GEMM writes bf16; a score of 40 has a bf16 spacing of 0.25, so exp() of the ROUNDED score is off by up to 13 % -- while the forward exponentiated
    fp32 scores.  With lse the row's log-sum-exp is subtracted INSIDE the GEMM, before the rounding: q gets eight more columns holding -lse / scale as
    three bf16 pieces (exact to 2^-24 relative) and k eight more of ones, so the accumulator holds scale q.k - lse in fp32 and what is rounded to bf16
    is log p: <= 0, with |log p| <= 4 for every entry that carries weight -- spacing <= 2^-6, 1.6 % at worst, typically 0.4 %.  nk_softmax_rows then
    renormalises the row (its sum is 1 up to those roundings)."""
    L, D = q.shape[0] // B, q.shape[1]
    scale = float(D) ** -0.5
    if lse is not None:
        neg = -lse.to(torch.float32) / scale
        p1 = neg.to(BF16)
        r1 = neg - p1.float()
        p2 = r1.to(BF16)
        p3 = (r1 - p2.float()).to(BF16)
        q_aug = torch.cat([q, torch.stack([p1, p2, p3], dim=1), torch.zeros(q.shape[0], 5, dtype=BF16, device=q.device)], dim=1)
        ones = torch.zeros(k.shape[0], 8, dtype=BF16, device=k.device)
        ones[:, :3] = 1.0
        k_aug = torch.cat([k, ones], dim=1)
    else:
        q_aug, k_aug = q, k

    def bwd(do: Tensor):
        _check2d(do, "do")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        dk32 = torch.empty(L, D, dtype=torch.float32, device=q.device)
        dv32 = torch.empty(L, D, dtype=torch.float32, device=q.device)
        for b in range(B):
            for c0 in range(0, L, ATTN512_BWD_CHUNK):
                rows = slice(b * L + c0, b * L + min(c0 + ATTN512_BWD_CHUNK, L))
                keys = slice(b * L, (b + 1) * L)
                n = rows.stop - rows.start
                p = gemm_nt(q_aug[rows], k_aug[keys], alpha=scale)                 # scores [n, L] (minus the row's log-sum-exp where known) ...
                call("nk_softmax_rows", p.data_ptr(), n, L, _stream())             # ... -> probabilities, as the forward's
                dp = gemm_nt(do[rows], v[keys])                                     # dP = dO V^T
                gemm_tn_f32(p, do[rows], dv32, c0 > 0)                              # dV (+)= P^T dO
                call("nk_softmax_rows_bwd", p.data_ptr(), dp.data_ptr(), n, L, scale, _stream())    # dP -> dS (scaled), in place
                gemm_nn(dp, k[keys], out=dq[rows])                                  # dQ = dS K
                gemm_tn_f32(dp, q[rows], dk32, c0 > 0)                              # dK (+)= dS^T Q
            dv[b * L:(b + 1) * L].copy_(cast_bf16(dv32))
            dk[b * L:(b + 1) * L].copy_(cast_bf16(dk32))
        return dq, dk, dv

    return bwd


# ------------------------------------------------------------------------------------------------
# vector quantizer (csrc/vq.hip)
# ------------------------------------------------------------------------------------------------
VQ_MAX_D, VQ_MAX_CODES = 256, 65536


def _vq_rows(t: Tensor, name: str, op: str) -> Tensor:
    """fp32 [N, D] device matrix with unit inner stride (a column slice of a wider matrix is taken as it is)"""
    if not t.is_cuda:
        raise NotImplementedError(f"{op}: {name} is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError(f"{op}: {name} must be a 2-D fp32 tensor, got {tuple(t.shape)} {t.dtype}")
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _vq_idx(idx: Tensor, N: int, op: str) -> Tensor:
    if not idx.is_cuda:
        raise NotImplementedError(f"{op}: idx is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if idx.dtype != torch.int64 or idx.numel() != N:
        raise ValueError(f"{op}: idx must hold {N} int64 indices, got {tuple(idx.shape)} {idx.dtype}")
    return idx.reshape(-1).contiguous()


def vq_search(z: Tensor, codebook: Tensor) -> Tensor:
    """idx [N] int64 = argmin_j (|e_j|^2 - 2 z_i . e_j) over the codebook [n_e, D] for every row of z [N, D] (nk_vq_search: exact fp32 on the
    matrix pipe, lowest index among equal scores, NaN scores never chosen; the [N, n_e] distance matrix is never written)."""
    z, codebook = _vq_rows(z, "z", "vq_search"), _vq_rows(codebook, "codebook", "vq_search").contiguous()
    N, D = z.shape
    n_e = codebook.shape[0]
    if codebook.shape[1] != D:
        raise ValueError(f"vq_search: z [N, {D}] against a codebook of width {codebook.shape[1]}")
    idx = torch.empty(N, dtype=torch.int64, device=z.device)
    ws = _ws(max(query("nk_vq_search_ws_floats", N, n_e), 1), z.device)
    call("nk_vq_search", z.data_ptr(), z.stride(0), codebook.data_ptr(), ws.data_ptr(), idx.data_ptr(), N, D, n_e, _stream())
    return idx


def vq_code_stats(idx: Tensor, z: Tensor, n_e: int):
    """(count [n_e] int64, sum [n_e, D] fp32): how many rows of z chose each code and the sum of those rows, added in row order
    (nk_vq_code_stats: deterministic, no atomics; codes nobody chose are exact zeros)."""
    z = _vq_rows(z, "z", "vq_code_stats")
    N, D = z.shape
    idx = _vq_idx(idx, N, "vq_code_stats")
    count = torch.zeros(n_e, dtype=torch.int64, device=z.device)
    total = torch.zeros(n_e, D, dtype=torch.float32, device=z.device)
    call("nk_vq_code_stats", idx.data_ptr(), z.data_ptr(), z.stride(0), count.data_ptr(), total.data_ptr(), N, D, int(n_e), _stream())
    return count, total


def vq_quantize(idx: Tensor, codebook: Tensor, z: Tensor, hw: int = 1, out: Optional[Tensor] = None):
    """(z_q, sumsq): z_q = codebook[idx] written as fp32 [N // hw, D, hw] (row i of z = b * hw + p: NCHW with hw = H * W; hw = 1 gives
    the [N, D] matrix), sumsq = sum (z_q - z)^2 as a device scalar from a fixed-order reduction (nk_vq_quantize)."""
    z, codebook = _vq_rows(z, "z", "vq_quantize"), _vq_rows(codebook, "codebook", "vq_quantize").contiguous()
    N, D = z.shape
    idx = _vq_idx(idx, N, "vq_quantize")
    if codebook.shape[1] != D or hw < 1 or N % hw:
        raise ValueError(f"vq_quantize: z {tuple(z.shape)}, codebook {tuple(codebook.shape)}, hw = {hw}")
    if out is None:
        out = torch.empty((N, D) if hw == 1 else (N // hw, D, hw), dtype=torch.float32, device=z.device)
    elif out.numel() != N * D or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("vq_quantize: out must be a dense fp32 device tensor of N * D elements")
    sumsq = torch.empty((), dtype=torch.float32, device=z.device)
    ws = _ws(query("nk_vq_quantize_ws_floats", N), z.device)
    call("nk_vq_quantize", idx.data_ptr(), codebook.data_ptr(), z.data_ptr(), z.stride(0), out.data_ptr(), sumsq.data_ptr(), ws.data_ptr(), N, D,
         codebook.shape[0], int(hw), _stream())
    return out, sumsq


# ------------------------------------------------------------------------------------------------
# Gumbel-softmax quantizer (csrc/gumbel.hip)
# ------------------------------------------------------------------------------------------------
def _gumbel_token(token: Tensor, device, op: str) -> Tensor:
    if token.dtype != torch.int64 or token.numel() != 2 or token.device != device or not token.is_contiguous():
        raise ValueError(f"{op}: token must be the int64 [2] tensor of ops.dropout_draw() on the data's device")
    return token


def _gumbel_bf16(t: Tensor, N: int, n: int, name: str, op: str) -> Tensor:
    if not t.is_cuda or t.dtype != BF16 or tuple(t.shape) != (N, n) or not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be a dense bf16 [{N}, {n}] device tensor, got {tuple(t.shape)} {t.dtype} {t.stride()}")
    return t


def gumbel_logits(z: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """logits [N, n] fp32 = z [N, h] @ weight [n, h]^T + bias [n] (nk_gumbel_logits: exact fp32 on the matrix pipe, the fma chain in rising k
    and one rounded add of the bias; a column slice of a wider z is taken as it is)."""
    z, weight = _vq_rows(z, "z", "gumbel_logits"), _vq_rows(weight, "weight", "gumbel_logits").contiguous()
    N, h = z.shape
    n = weight.shape[0]
    if weight.shape[1] != h or not bias.is_cuda or bias.dtype != torch.float32 or tuple(bias.shape) != (n,):
        raise ValueError(f"gumbel_logits: z [N, {h}] against weight {tuple(weight.shape)} and bias {tuple(bias.shape)} {bias.dtype}")
    logits = torch.empty(N, n, dtype=torch.float32, device=z.device)
    call("nk_gumbel_logits", z.data_ptr(), z.stride(0), weight.data_ptr(), bias.contiguous().data_ptr(), logits.data_ptr(), n, N, h, n, _stream())
    return logits


def gumbel_noise(rows: int, cols: int, site: int, token: Tensor) -> Tensor:
    """g [rows, cols] fp32: the Gumbel noise of (token, site), a pure function of the logical element index (nk_gumbel_noise;
    tests/gumbel_reference.py restates it)."""
    if not token.is_cuda:
        raise NotImplementedError("gumbel_noise: the token is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    token = _gumbel_token(token, token.device, "gumbel_noise")
    if rows < 0 or cols < 1 or site < 0:
        raise ValueError(f"gumbel_noise: rows >= 0, cols >= 1 and site >= 0, got {rows}, {cols}, {site}")
    g = torch.empty(rows, cols, dtype=torch.float32, device=token.device)
    call("nk_gumbel_noise", g.data_ptr(), int(rows), int(cols), token.data_ptr(), int(site), _stream())
    return g


def _inv_tau(tau: float, op: str) -> float:
    tau = float(tau)
    if not tau > 0.0:
        raise ValueError(f"{op}: the temperature must be positive, got {tau!r}")
    return 1.0 / tau


def gumbel_softmax_fwd(logits: Tensor, tau: float, *, noise: Optional[Tensor] = None, token: Optional[Tensor] = None, site: int = 0):
    """(y, idx, kl): y = softmax((logits + g) / tau) as bf16 [N, n], idx [N] int64 its argmax (lowest index among equal scores), kl the device
    scalar mean_i sum_j q_j log(q_j n + 1e-10) with q = softmax(logits).  g is `noise` (fp32 [N, n]) or, with noise=None, the noise of
    (token, site) generated inside the kernel -- bitwise what gumbel_noise(N, n, site, token) would have passed."""
    logits = _vq_rows(logits, "logits", "gumbel_softmax_fwd")
    N, n = logits.shape
    if (noise is None) == (token is None):
        raise ValueError("gumbel_softmax_fwd: exactly one of noise= and token=")
    if noise is not None:
        if not noise.is_cuda or noise.dtype != torch.float32 or tuple(noise.shape) != (N, n):
            raise ValueError(f"gumbel_softmax_fwd: noise must be an fp32 [{N}, {n}] device tensor, got {tuple(noise.shape)} {noise.dtype}")
        noise = noise.contiguous()
    else:
        token = _gumbel_token(token, logits.device, "gumbel_softmax_fwd")
    y = torch.empty(N, n, dtype=BF16, device=logits.device)
    idx = torch.empty(N, dtype=torch.int64, device=logits.device)
    kl = torch.empty((), dtype=torch.float32, device=logits.device)
    ws = _ws(query("nk_gumbel_softmax_ws_floats", N), logits.device)
    call("nk_gumbel_softmax_fwd", logits.data_ptr(), logits.stride(0), _p(noise), _p(token), int(site), _inv_tau(tau, "gumbel_softmax_fwd"),
         y.data_ptr(), idx.data_ptr(), kl.data_ptr(), ws.data_ptr(), N, n, _stream())
    return y, idx, kl


def gumbel_softmax_bwd(logits: Tensor, y: Tensor, G: Tensor, tau: float, w_kl: float) -> Tensor:
    """d [N, n] bf16, written IN PLACE over G: the gradient of <G, y> + w_kl * kl with respect to the logits, y and kl those of
    gumbel_softmax_fwd (nk_gumbel_softmax_bwd)."""
    logits = _vq_rows(logits, "logits", "gumbel_softmax_bwd")
    N, n = logits.shape
    y, G = _gumbel_bf16(y, N, n, "y", "gumbel_softmax_bwd"), _gumbel_bf16(G, N, n, "G", "gumbel_softmax_bwd")
    call("nk_gumbel_softmax_bwd", logits.data_ptr(), logits.stride(0), y.data_ptr(), G.data_ptr(), _inv_tau(tau, "gumbel_softmax_bwd"), float(w_kl),
         N, n, _stream())
    return G


GUMBEL_WIDTH_RULE = "a multiple of 8 (the 16-byte operand rule of the bf16 GEMMs behind the gradients: ops.gemm_nt / gemm_nn / gemm_tn_f32)"


def gumbel_quantize(rows: Tensor, W: Tensor, bias: Tensor, E: Tensor, Wb: Tensor, Eb: Tensor, tau: float, hard: bool, *,
                    noise: Optional[Tensor] = None, token: Optional[Tensor] = None, site: int = 0):
    """The Gumbel-softmax bottleneck on latent rows [N, h] fp32: W [n, h], bias [n], E [n, d] the fp32 projection and codebook, Wb / Eb their
    bf16 copies.  Returns (z_q [N, d] fp32, idx [N], kl, logits, y, bwd): hard -> z_q = E[idx] (the straight-through one-hot), else
    z_q = y @ E (bf16 operands, fp32 accumulation).  bwd(dz_rows fp32 [N, d], w_kl) -> (d_rows bf16 [N, h], d bf16 [N, n], dz bf16 [N, d]):
    the gradient of <dz, z_q> + w_kl * kl with respect to the rows and to the logits, and the bf16 copy of dz the caller's weight
    gradients read (dW = d^T rows, db = colsum d, dE = y^T dz or the per-code sum of dz)."""
    N, d = rows.shape[0], E.shape[1]
    logits = gumbel_logits(rows, W, bias)
    y, idx, kl = gumbel_softmax_fwd(logits, tau, noise=noise, token=token, site=site)
    if hard:
        z_q, _ = vq_quantize(idx, E, torch.zeros(N, d, dtype=torch.float32, device=rows.device))
    else:
        z_q = gemm_nn(y, Eb).float()

    def bwd(dz_rows: Tensor, w_kl: float):
        dzb = cast_bf16(dz_rows)
        dl = gumbel_softmax_bwd(logits, y, gemm_nt(dzb, Eb), tau, w_kl)
        return gemm_nn(dl, Wb), dl, dzb

    return z_q, idx, kl, logits, y, bwd


# ------------------------------------------------------------------------------------------------
# antialiased bicubic resize (csrc/resample.hip; host tables in neurosis_amd/resample.py)
# ------------------------------------------------------------------------------------------------
def _resize_planes(x: Tensor, out_hw, transposed: bool, op: str) -> Tensor:
    """x fp32 NCHW -> [N, C, *out_hw] through nk_resample_planes: with the forward tables of (H, W) -> out_hw, or (transposed) with the
    transposed tables of out_hw -> (H, W), i.e. the adjoint of the resize that produced something of x's size."""
    from .resample import device_tables

    if not x.is_cuda:
        raise NotImplementedError(f"{op}: the input is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"{op}: expected an fp32 NCHW tensor, got {tuple(x.shape)} {x.dtype}")
    N, Cc, H, W = x.shape
    OH, OW = int(out_hw[0]), int(out_hw[1])
    if OH < 1 or OW < 1 or H < 1 or W < 1:
        raise ValueError(f"{op}: sizes must be positive, got {(H, W)} -> {(OH, OW)}")
    x = x.contiguous()
    if transposed:
        v, h = device_tables(OH, H, x.device)[1], device_tables(OW, W, x.device)[1]
    else:
        v, h = device_tables(H, OH, x.device)[0], device_tables(W, OW, x.device)[0]
    y = torch.empty(N, Cc, OH, OW, dtype=torch.float32, device=x.device)
    P = N * Cc
    if P == 0:
        return y
    ws = _ws(max(query("nk_resample_ws_floats", P, H, W, OH, OW), 1), x.device)
    call("nk_resample_planes", x.data_ptr(), y.data_ptr(), ws.data_ptr(), v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), v[3], h[0].data_ptr(),
         h[1].data_ptr(), h[2].data_ptr(), h[3], P, H, W, OH, OW, _stream())
    return y


def resize_bicubic_aa(x: Tensor, size):
    """(y, bwd): y = F.interpolate(x, size, mode="bicubic", antialias=True) for fp32 NCHW x, through the banded resampler with float64-built
    tables; bwd(dy) -> dx is the same kernel with the transposed tables (deterministic, no atomics).  Equal sizes return x itself and an
    identity bwd (torch's result is the bit-exact identity there)."""
    if not x.is_cuda:
        raise NotImplementedError("resize_bicubic_aa: the input is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"resize_bicubic_aa: expected an fp32 NCHW tensor, got {tuple(x.shape)} {x.dtype}")
    OH, OW = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    N, Cc, H, W = x.shape
    if (OH, OW) == (H, W):
        return x, lambda dy: dy
    y = _resize_planes(x, (OH, OW), False, "resize_bicubic_aa")

    def bwd(dy: Tensor) -> Tensor:
        if tuple(dy.shape) != (N, Cc, OH, OW):
            raise ValueError(f"resize_bicubic_aa backward: expected a gradient of shape {(N, Cc, OH, OW)}, got {tuple(dy.shape)}")
        return _resize_planes(dy, (H, W), True, "resize_bicubic_aa backward")

    return y, bwd


def resize_bicubic_aa_bwd(dy: Tensor, size) -> Tensor:
    """dx [N, C, *size] = R^T dy for the resize R: size -> dy's height and width (the backward of resize_bicubic_aa without its forward)."""
    IH, IW = int(size[0]), int(size[1])
    if dy.is_cuda and dy.dim() == 4 and tuple(dy.shape[2:]) == (IH, IW):
        return dy
    return _resize_planes(dy, (IH, IW), True, "resize_bicubic_aa_bwd")


# ------------------------------------------------------------------------------------------------
# frozen ViT towers of the DreamSim loss (csrc/vit.hip): what is not a transformer layer
# ------------------------------------------------------------------------------------------------
def _vit_image(x: Tensor, patch: int, op: str):
    if not x.is_cuda:
        raise NotImplementedError(f"{op}: the input is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{op}: expected a dense fp32 NCHW tensor with 3 channels, got {tuple(x.shape)} {x.dtype}")
    N, _, H, W = x.shape
    if patch % 8 or H % patch or W % patch:
        raise ValueError(f"{op}: height and width must be multiples of the patch size (itself a multiple of 8), got {(H, W)} and patch {patch}")
    return N, H, W, (H // patch) * (W // patch)


def vit_affine(scale, shift, lo: float = -math.inf, hi: float = math.inf):
    """the host array {a_0..2, b_0..2, lo, hi} of vit_patchify: each value is a_c * clamp(x, lo, hi) + b_c"""
    return (C.c_float * 8)(*[float(v) for v in scale], *[float(v) for v in shift], float(lo), float(hi))


def vit_patchify(x: Tensor, patch: int, affine) -> Tensor:
    """x fp32 NCHW [N, 3, H, W] -> bf16 rows [N * Np, 3 p p], row (n, py, px), column (c, ky, kx) (nn.Conv2d's weight order), each value the bf16
    rounding of a_c * clamp(x, lo, hi) + b_c (`affine` from vit_affine)."""
    N, H, W, Np = _vit_image(x, patch, "vit_patchify")
    rows = torch.empty(N * Np, 3 * patch * patch, dtype=BF16, device=x.device)
    call("nk_vit_patchify", x.data_ptr(), rows.data_ptr(), affine, N, H, W, patch, _stream())
    return rows


def vit_patchify_bwd(drows: Tensor, x: Tensor, patch: int, affine, out: Optional[Tensor] = None) -> Tensor:
    """The adjoint of vit_patchify at x: fp32 NCHW a_c * drows, zero where the forward clamped.  With `out` (fp32, x's shape) the result is ADDED
    to it (the towers of an ensemble add their input gradients in a fixed order); one writer per pixel, no atomics."""
    N, H, W, Np = _vit_image(x, patch, "vit_patchify_bwd")
    _check2d(drows, "drows")
    if tuple(drows.shape) != (N * Np, 3 * patch * patch) or not drows.is_contiguous():
        raise ValueError(f"vit_patchify_bwd: drows must be a dense [{N * Np}, {3 * patch * patch}] matrix, got {tuple(drows.shape)}")
    if out is not None and (out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device):
        raise ValueError("vit_patchify_bwd: out must be a dense fp32 tensor of x's shape on x's device")
    dx = torch.empty_like(x) if out is None else out
    call("nk_vit_patchify_bwd", drows.data_ptr(), x.data_ptr(), dx.data_ptr(), affine, N, H, W, patch, int(out is not None), _stream())
    return dx


def vit_tokens(patches: Tensor, cls: Tensor, pos: Tensor, N: int) -> Tensor:
    """tokens FP32 [N (Np + 1), E] (a tower's residual stream is fp32, vit_add_ln): row 0 of a sample is cls + pos[0], row 1 + i patch row i + pos[1 + i]; patches bf16 [N Np, E] (the patch
    GEMM's output, bias included), cls fp32 [E], pos fp32 [Np + 1, E]."""
    _check2d(patches, "patches")
    E = patches.shape[1]
    Np = patches.shape[0] // max(N, 1)
    if N < 1 or Np < 1 or Np * N != patches.shape[0] or not patches.is_contiguous() or E % 8:
        raise ValueError(f"vit_tokens: patches must be a dense [N * Np, E] matrix with E % 8 == 0, got {tuple(patches.shape)} for N = {N}")
    for name, t, shape in (("cls", cls, (E,)), ("pos", pos, (Np + 1, E))):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != patches.device:
            raise ValueError(f"vit_tokens: {name} must be a dense fp32 {shape} tensor on the patches' device, got {tuple(t.shape)} {t.dtype}")
    tokens = torch.empty(N * (Np + 1), E, dtype=torch.float32, device=patches.device)
    call("nk_vit_tokens", patches.data_ptr(), cls.data_ptr(), pos.data_ptr(), tokens.data_ptr(), N, Np, E, _stream())
    return tokens


def vit_tokens_bwd(dtokens: Tensor, N: int) -> Tensor:
    """The adjoint of vit_tokens w.r.t. the patch rows: dtokens bf16 [N (Np + 1), E] -> [N Np, E], the cls rows dropped."""
    _check2d(dtokens, "dtokens")
    L, E = dtokens.shape[0] // max(N, 1), dtokens.shape[1]
    if N < 1 or L < 2 or L * N != dtokens.shape[0] or not dtokens.is_contiguous() or E % 8:
        raise ValueError(f"vit_tokens_bwd: dtokens must be a dense [N * (Np + 1), E] matrix with E % 8 == 0, got {tuple(dtokens.shape)} for N = {N}")
    dpatches = torch.empty(N * (L - 1), E, dtype=BF16, device=dtokens.device)
    call("nk_vit_tokens_bwd", dtokens.data_ptr(), dpatches.data_ptr(), N, L - 1, E, _stream())
    return dpatches


def vit_add_ln(x: Tensor, branch: Optional[Tensor], norm: Optional[torch.nn.LayerNorm], copy: bool = False, y_f32: bool = False):
    """The seam between a frozen tower's fp32 residual stream x [M, E] and the bf16 GEMMs (nk_vit_add_ln):  x += branch IN PLACE (bf16 [M, E];
    skipped when None), then y = norm(x) as bf16 (or fp32 with y_f32: norm_pre, whose output is the stream) when a norm is given.
    Returns (y or None, xb or None, mean, rstd): xb is x rounded to bf16 (copy=True), which with mean / rstd [M] is what
    layernorm_bwd_dx reads in the backward."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"vit_add_ln: x must be a dense fp32 CUDA matrix, got {tuple(x.shape)} {x.dtype}")
    M, E = x.shape
    if branch is not None:
        _check2d(branch, "branch")
        if branch.shape != x.shape or not branch.is_contiguous():
            raise ValueError(f"vit_add_ln: branch must be a dense bf16 matrix of x's shape {tuple(x.shape)}, got {tuple(branch.shape)}")
    if norm is None and branch is None and not copy:
        raise ValueError("vit_add_ln: nothing to do")
    y = mean = rstd = None
    if norm is not None:
        y = torch.empty(M, E, dtype=torch.float32 if y_f32 else BF16, device=x.device)
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
    xb = torch.empty(M, E, dtype=BF16, device=x.device) if copy else None
    call("nk_vit_add_ln", x.data_ptr(), _p(branch), _p(norm.weight) if norm is not None else None, _p(norm.bias) if norm is not None else None, _p(y),
         int(y_f32), _p(xb), _p(mean), _p(rstd), M, E, float(norm.eps) if norm is not None else 1.0, _stream())
    return y, xb, mean, rstd


def vit_cls_head(tokens: Tensor, N: int, norm: Optional[torch.nn.LayerNorm], head: Optional[torch.nn.Linear], tape_from: Optional[int] = None):
    """(embedding fp32 [N, width], bwd): the cls row of each of the N samples of a dense FP32 token matrix [N * L, E] through the final
    LayerNorm (when given) and the head (when given), in fp32 on the fp32 parameters (nk_vit_cls_head_fwd).  With tape_from = s,
    bwd(d embedding[s:] fp32) -> bf16 [N - s, E], the gradient w.r.t. the cls rows of samples s..N-1; no parameter gradient exists."""
    if tokens.dim() != 2 or tokens.dtype != torch.float32 or not tokens.is_cuda or N < 1 or tokens.shape[0] % N or not tokens.is_contiguous():
        raise ValueError(f"vit_cls_head: tokens must be a dense fp32 CUDA [N * L, E] matrix, got {tuple(tokens.shape)} {tokens.dtype} for N = {N}")
    L, E = tokens.shape[0] // N, tokens.shape[1]
    for p in ([norm.weight, norm.bias] if norm is not None else []) + ([head.weight, head.bias] if head is not None else []):
        if p is not None and (p.dtype != torch.float32 or not p.is_contiguous() or p.device != tokens.device):
            raise ValueError("vit_cls_head: the norm's and the head's parameters must be dense fp32 tensors on the tokens' device")
    nc = head.weight.shape[0] if head is not None else E
    out = torch.empty(N, nc, dtype=torch.float32, device=tokens.device)
    mean = torch.empty(N, dtype=torch.float32, device=tokens.device)
    rstd = torch.empty_like(mean)
    gamma, beta = (norm.weight, norm.bias) if norm is not None else (None, None)
    W, bias = (head.weight, head.bias) if head is not None else (None, None)
    call("nk_vit_cls_head_fwd", tokens.data_ptr(), L * E, _p(gamma), _p(beta), _p(W), _p(bias), out.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, E, nc,
         float(norm.eps) if norm is not None else 1.0, _stream())
    if tape_from is None:
        return out, None
    s = tape_from

    def bwd(dout: Tensor) -> Tensor:
        dout = dout.to(torch.float32).contiguous()
        if tuple(dout.shape) != (N - s, nc):
            raise ValueError(f"vit_cls_head backward: expected a gradient of shape {(N - s, nc)}, got {tuple(dout.shape)}")
        dcls = torch.empty(N - s, E, dtype=BF16, device=tokens.device)
        call("nk_vit_cls_head_bwd", dout.data_ptr(), tokens[s * L:].data_ptr(), L * E, _p(gamma), _p(W), mean[s:].data_ptr(), rstd[s:].data_ptr(),
             dcls.data_ptr(), N - s, E, nc, _stream())
        return dcls

    return out, bwd


def dreamsim_head(f: Tensor, eps: float = 1e-8):
    """(d [B], bwd): f fp32 [2, B, Dz]; z = f / |f| - mean(f / |f|) per vector, d_b = 1 - F.cosine_similarity(z[0], z[1], eps).
    bwd(upstream [B]) -> d sum_b upstream_b d_b / d f[1], fp32 [B, Dz]; f[0] (the input image's features) gets no gradient."""
    if not f.is_cuda:
        raise NotImplementedError("dreamsim_head: the input is a CPU tensor; the HIP kernels run on the GPU only, there is no CPU path")
    if f.dim() != 3 or f.shape[0] != 2 or f.dtype != torch.float32 or not f.is_contiguous():
        raise ValueError(f"dreamsim_head: expected a dense fp32 [2, B, Dz] tensor, got {tuple(f.shape)} {f.dtype}")
    _, B, Dz = f.shape
    d = torch.empty(B, dtype=torch.float32, device=f.device)
    call("nk_dreamsim_head_fwd", f.data_ptr(), d.data_ptr(), B, Dz, float(eps), _stream())

    def bwd(upstream: Tensor) -> Tensor:
        up = upstream.to(torch.float32).contiguous()
        if tuple(up.shape) != (B,) or up.device != f.device:
            raise ValueError(f"dreamsim_head backward: upstream must be [{B}] on f's device, got {tuple(up.shape)}")
        df1 = torch.empty(B, Dz, dtype=torch.float32, device=f.device)
        call("nk_dreamsim_head_bwd", f.data_ptr(), up.data_ptr(), df1.data_ptr(), B, Dz, float(eps), _stream())
        return df1

    return d, bwd


def layernorm_bwd_dx(dy: Tensor, x: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor, dx_add: Optional[Tensor] = None) -> Tensor:
    """The input gradient of a LayerNorm alone (nk_layernorm_bwd_dx): no gamma / beta gradient is launched.  dx_add joins the result."""
    for name, t in (("dy", dy), ("x", x)) + ((("dx_add", dx_add),) if dx_add is not None else ()):
        _check2d(t, name)
        if t.shape != x.shape or not t.is_contiguous():
            raise ValueError(f"layernorm_bwd_dx: {name} must be a dense matrix of x's shape {tuple(x.shape)}, got {tuple(t.shape)}")
    M, Cc = x.shape
    if mean.numel() != M or rstd.numel() != M:
        raise ValueError(f"layernorm_bwd_dx: mean / rstd must hold {M} rows")
    dx = torch.empty_like(x)
    call("nk_layernorm_bwd_dx", dy.data_ptr(), x.data_ptr(), weight.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _p(dx_add), dx.data_ptr(), M, Cc, _stream())
    return dx


def gelu_bwd(dy: Tensor, x: Tensor, quick: bool = False) -> Tensor:
    """dx = dy * gelu'(x) (nk_gelu_bwd): gelu_fwd's backward without its closure"""
    if dy.shape != x.shape or dy.dtype != BF16 or x.dtype != BF16 or not dy.is_contiguous() or not x.is_contiguous():
        raise ValueError("gelu_bwd: dy and x must be dense bf16 tensors of one shape")
    dx = torch.empty_like(x)
    call("nk_gelu_bwd", dy.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), int(quick), _stream())
    return dx


def attention_bwd(q: Tensor, k: Tensor, v: Tensor, o: Tensor, lse: Tensor, do: Tensor, B: int, heads: int, dim_head: int, dq: Tensor, dk: Tensor,
                  dv: Tensor) -> None:
    """The backward of the non-causal attention_fwd from its saved tensors (or the row slices of them that belong to B whole samples):
    q / o / do / dq [B*Lq, H*D], k / v / dk / dv [B*Lk, H*D] token matrices (column slices allowed), lse fp32 [B, heads, Lq] dense."""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        _check2d(t, n)
    if dim_head > 160:
        raise NotImplementedError("attention_bwd: head dim <= 160")
    Lq = q.shape[0] // B
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != B * heads * Lq:
        raise ValueError(f"attention_bwd: lse must be a dense fp32 [{B}, {heads}, {Lq}] tensor")
    d = _attn_desc(q, k, v, o, B, heads, dim_head, float(dim_head) ** -0.5, False)
    _attn_grads(d, "attention_bwd", do, dq, dk, dv)
    delta = _ws(query("nk_attention_bwd_ws_floats", C.byref(d)), do.device)
    call("nk_attention_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(),
         dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr(), _stream())


# ------------------------------------------------------------------------------------------------
# misc
# ------------------------------------------------------------------------------------------------
def timestep_embedding(t: Tensor, dim: int, max_period: float = 10000.0) -> Tensor:
    tf = t.to(torch.float32).contiguous()
    out = torch.empty(tf.shape[0], dim, dtype=BF16, device=t.device)
    call("nk_timestep_embedding", tf.data_ptr(), out.data_ptr(), tf.shape[0], dim, float(max_period), _stream())
    return out
