"""`torch.library` registration of the HIP kernels: namespace `neurosis_hip` (SURVEY.md section 8(b) "C-ABI / op surface",
north_star "exposed as PyTorch-ROCm custom ops").

The training step itself does not go through the dispatcher -- the UNet is one explicit forward/backward chain over the
C-ABI -- but every kernel family is ALSO a dispatcher-visible op here, so a caller outside this package
(the reference's own modules, `torch.compile`, a C++ host of libtorch) can use them one by one:

    torch.ops.neurosis_hip.linear(x, w, bias)                      differentiable (autograd -> _dgrad / _wgrad ops)
    torch.ops.neurosis_hip.layernorm(x, gamma, beta, eps)           "
    torch.ops.neurosis_hip.groupnorm_silu(x, gamma, beta, N, groups, eps, silu)
    torch.ops.neurosis_hip.groupnorm_mod(x, gamma, beta, mod, N, groups, eps, silu)     scale-shift norm; also differentiable in mod
    torch.ops.neurosis_hip.avgpool2x(x, N, H, W) / upsample2x_nearest(x, N, H, W)       the parameter-free resamplers
    torch.ops.neurosis_hip.geglu(u)                                 "
    torch.ops.neurosis_hip.attention(q, k, v, B, heads)             "
    torch.ops.neurosis_hip.conv2d(x, w, bias, N, H, W, stride, padding)     channels-last tokens in / out
    ... and the raw `*_fwd / *_dgrad / *_wgrad / *_bwd` ops they are made of, `timestep_embedding`, `nchw_to_nlc`, `nlc_to_nchw`.

Dispatch keys: CUDA (= HIP on ROCm) only, plus Meta kernels (shapes / dtypes, so FakeTensor tracing and `torch.compile`
work).  There is deliberately NO CPU key: the product has no CPU path (the oracle under oracle/ is test infrastructure), so a
CPU tensor gets torch's own "not implemented for CPU" error.  Conventions are those of neurosis_amd.ops: bf16 token matrices
[rows, C] with unit inner stride, fp32 parameters cast by the caller (weights here are bf16 operands), fp32 statistics.

Reference call sites per op: include/neurosis_hip.h (each C entry point cites them) and INTEGRATION.md section 5.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import ops
from .ops import BF16, Img

NS = "neurosis_hip"
_CUDA = "cuda"


def _op(name: str, mutates=()):
    return torch.library.custom_op(f"{NS}::{name}", mutates_args=mutates, device_types=_CUDA)


# ---------------------------------------------------------------------------------------------------------------
# Linear: y = alpha * x @ w^T + bias + residual
# ---------------------------------------------------------------------------------------------------------------
@_op("linear_fwd")
def linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None, alpha: float = 1.0) -> Tensor:
    return ops.gemm_nt(x, w, bias, residual, alpha)


@linear_fwd.register_fake
def _(x, w, bias=None, residual=None, alpha=1.0):
    return x.new_empty(x.shape[0], w.shape[0])


@_op("linear_dgrad")
def linear_dgrad(dy: Tensor, w: Tensor) -> Tensor:
    return ops.gemm_nn(dy, w)


@linear_dgrad.register_fake
def _(dy, w):
    return dy.new_empty(dy.shape[0], w.shape[1])


@_op("linear_wgrad")
def linear_wgrad(dy: Tensor, x: Tensor) -> Tensor:
    dw = torch.empty(dy.shape[1], x.shape[1], dtype=torch.float32, device=dy.device)
    ops.gemm_tn_f32(dy, x, dw, False)
    return dw


@linear_wgrad.register_fake
def _(dy, x):
    return dy.new_empty(dy.shape[1], x.shape[1], dtype=torch.float32)


@_op("colsum")
def colsum(dy: Tensor) -> Tensor:
    out = torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device)
    ops.colsum(dy, out, False)
    return out


@colsum.register_fake
def _(dy):
    return dy.new_empty(dy.shape[1], dtype=torch.float32)


@_op("linear")
def linear(x: Tensor, w: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    return ops.gemm_nt(x, w, bias)


@linear.register_fake
def _(x, w, bias=None):
    return x.new_empty(x.shape[0], w.shape[0])


def _linear_setup(ctx, inputs, output):
    x, w, bias = inputs
    ctx.save_for_backward(x, w)
    ctx.has_bias = bias is not None


def _linear_bwd(ctx, dy):
    x, w = ctx.saved_tensors
    dy = dy.contiguous()
    dx = torch.ops.neurosis_hip.linear_dgrad(dy, w) if ctx.needs_input_grad[0] else None
    dw = torch.ops.neurosis_hip.linear_wgrad(dy, x).to(w.dtype) if ctx.needs_input_grad[1] else None
    db = torch.ops.neurosis_hip.colsum(dy) if ctx.has_bias and ctx.needs_input_grad[2] else None
    return dx, dw, db


linear.register_autograd(_linear_bwd, setup_context=_linear_setup)


# ---------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------
@_op("layernorm_fwd")
def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5) -> Tuple[Tensor, Tensor, Tensor]:
    M, C = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ops.call("nk_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, C, float(eps), ops._stream())
    return y, mean, rstd


@layernorm_fwd.register_fake
def _(x, gamma, beta, eps=1e-5):
    return torch.empty_like(x), x.new_empty(x.shape[0], dtype=torch.float32), x.new_empty(x.shape[0], dtype=torch.float32)


@_op("layernorm_bwd")
def layernorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    M, C = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    ws = ops._ws(ops.query("nk_layernorm_ws_floats", M, C), x.device)
    ops.call("nk_layernorm_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(), dg.data_ptr(),
             db.data_ptr(), ws.data_ptr(), M, C, 0, ops._stream())
    return dx, dg, db


@layernorm_bwd.register_fake
def _(dy, x, gamma, mean, rstd):
    return torch.empty_like(x), gamma.new_empty(gamma.shape, dtype=torch.float32), gamma.new_empty(gamma.shape, dtype=torch.float32)


@_op("layernorm")
def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5) -> Tensor:
    return torch.ops.neurosis_hip.layernorm_fwd(x, gamma, beta, eps)[0]


@layernorm.register_fake
def _(x, gamma, beta, eps=1e-5):
    return torch.empty_like(x)


def _ln_setup(ctx, inputs, output):
    x, gamma, beta, eps = inputs
    _, mean, rstd = torch.ops.neurosis_hip.layernorm_fwd(x, gamma, beta, eps)     # statistics for backward (x is kept, not y)
    ctx.save_for_backward(x, gamma, mean, rstd)


def _ln_bwd(ctx, dy):
    x, gamma, mean, rstd = ctx.saved_tensors
    dx, dg, db = torch.ops.neurosis_hip.layernorm_bwd(dy.contiguous(), x, gamma, mean, rstd)
    return dx, dg, db, None


layernorm.register_autograd(_ln_bwd, setup_context=_ln_setup)


# ---------------------------------------------------------------------------------------------------------------
# GroupNorm (+SiLU) on channels-last tokens [N*HW, C]
# ---------------------------------------------------------------------------------------------------------------
def _gn_fwd_eager(x, gamma, beta, mod, N, groups, eps, silu):
    """the eager body of groupnorm_silu_fwd (mod None) and groupnorm_mod_fwd: (y, mean, rstd)"""
    HW, C = x.shape[0] // N, x.shape[1]
    y = torch.empty_like(x)
    mean = torch.empty(N, groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, C, groups), x.device)
    mp = () if mod is None else (mod.data_ptr(),)
    ops.call("nk_groupnorm_fwd" if mod is None else "nk_groupnorm_mod_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *mp, y.data_ptr(), mean.data_ptr(),
             rstd.data_ptr(), ws.data_ptr(), N, HW, C, groups, float(eps), int(silu), ops._stream())
    return y, mean, rstd


def _gn_bwd_eager(dy, x, gamma, beta, mod, mean, rstd, N, groups, silu):
    """the eager body of groupnorm_silu_bwd (mod None) and groupnorm_mod_bwd: (dx, dgamma, dbeta) and, with mod, dmod"""
    HW, C = x.shape[0] // N, x.shape[1]
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    dmod = () if mod is None else (torch.empty_like(mod),)
    ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, C, groups), x.device)
    mp = () if mod is None else (mod.data_ptr(),)
    ops.call("nk_groupnorm_bwd" if mod is None else "nk_groupnorm_mod_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *mp, mean.data_ptr(),
             rstd.data_ptr(), None, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), *(t.data_ptr() for t in dmod), ws.data_ptr(), N, HW, C, groups, int(silu), 0,
             ops._stream())
    return (dx, dg, db, *dmod)


@_op("groupnorm_silu_fwd")
def groupnorm_silu_fwd(x: Tensor, gamma: Tensor, beta: Tensor, N: int, groups: int, eps: float, silu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    return _gn_fwd_eager(x, gamma, beta, None, N, groups, eps, silu)


@groupnorm_silu_fwd.register_fake
def _(x, gamma, beta, N, groups, eps, silu):
    return torch.empty_like(x), x.new_empty(N, groups, dtype=torch.float32), x.new_empty(N, groups, dtype=torch.float32)


@_op("groupnorm_silu_bwd")
def groupnorm_silu_bwd(dy: Tensor, x: Tensor, gamma: Tensor, beta: Tensor, mean: Tensor, rstd: Tensor, N: int, groups: int, silu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    return _gn_bwd_eager(dy, x, gamma, beta, None, mean, rstd, N, groups, silu)


@groupnorm_silu_bwd.register_fake
def _(dy, x, gamma, beta, mean, rstd, N, groups, silu):
    return torch.empty_like(x), gamma.new_empty(gamma.shape, dtype=torch.float32), gamma.new_empty(gamma.shape, dtype=torch.float32)


@_op("groupnorm_silu")
def groupnorm_silu(x: Tensor, gamma: Tensor, beta: Tensor, N: int, groups: int, eps: float, silu: bool) -> Tensor:
    return torch.ops.neurosis_hip.groupnorm_silu_fwd(x, gamma, beta, N, groups, eps, silu)[0]


@groupnorm_silu.register_fake
def _(x, gamma, beta, N, groups, eps, silu):
    return torch.empty_like(x)


def _gn_setup(ctx, inputs, output):
    x, gamma, beta, N, groups, eps, silu = inputs
    _, mean, rstd = torch.ops.neurosis_hip.groupnorm_silu_fwd(x, gamma, beta, N, groups, eps, silu)
    ctx.save_for_backward(x, gamma, beta, mean, rstd)
    ctx.meta = (N, groups, silu)


def _gn_bwd(ctx, dy):
    x, gamma, beta, mean, rstd = ctx.saved_tensors
    N, groups, silu = ctx.meta
    dx, dg, db = torch.ops.neurosis_hip.groupnorm_silu_bwd(dy.contiguous(), x, gamma, beta, mean, rstd, N, groups, silu)
    return dx, dg, db, None, None, None, None


groupnorm_silu.register_autograd(_gn_bwd, setup_context=_gn_setup)


# ... with the per-image scale-shift modulation of the ADM ResBlock: y = silu?(GN(x) * (1 + mod[:, :C]) + mod[:, C:]), mod bf16 [N, 2C]
@_op("groupnorm_mod_fwd")
def groupnorm_mod_fwd(x: Tensor, gamma: Tensor, beta: Tensor, mod: Tensor, N: int, groups: int, eps: float, silu: bool) -> Tuple[Tensor, Tensor, Tensor]:
    return _gn_fwd_eager(x, gamma, beta, mod, N, groups, eps, silu)


@groupnorm_mod_fwd.register_fake
def _(x, gamma, beta, mod, N, groups, eps, silu):
    return torch.empty_like(x), x.new_empty(N, groups, dtype=torch.float32), x.new_empty(N, groups, dtype=torch.float32)


@_op("groupnorm_mod_bwd")
def groupnorm_mod_bwd(dy: Tensor, x: Tensor, gamma: Tensor, beta: Tensor, mod: Tensor, mean: Tensor, rstd: Tensor, N: int, groups: int,
                      silu: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    return _gn_bwd_eager(dy, x, gamma, beta, mod, mean, rstd, N, groups, silu)


@groupnorm_mod_bwd.register_fake
def _(dy, x, gamma, beta, mod, mean, rstd, N, groups, silu):
    return torch.empty_like(x), gamma.new_empty(gamma.shape, dtype=torch.float32), gamma.new_empty(gamma.shape, dtype=torch.float32), torch.empty_like(mod)


@_op("groupnorm_mod")
def groupnorm_mod(x: Tensor, gamma: Tensor, beta: Tensor, mod: Tensor, N: int, groups: int, eps: float, silu: bool) -> Tensor:
    return torch.ops.neurosis_hip.groupnorm_mod_fwd(x, gamma, beta, mod, N, groups, eps, silu)[0]


@groupnorm_mod.register_fake
def _(x, gamma, beta, mod, N, groups, eps, silu):
    return torch.empty_like(x)


def _gnm_setup(ctx, inputs, output):
    x, gamma, beta, mod, N, groups, eps, silu = inputs
    _, mean, rstd = torch.ops.neurosis_hip.groupnorm_mod_fwd(x, gamma, beta, mod, N, groups, eps, silu)
    ctx.save_for_backward(x, gamma, beta, mod, mean, rstd)
    ctx.meta = (N, groups, silu)


def _gnm_bwd(ctx, dy):
    x, gamma, beta, mod, mean, rstd = ctx.saved_tensors
    N, groups, silu = ctx.meta
    dx, dg, db, dmod = torch.ops.neurosis_hip.groupnorm_mod_bwd(dy.contiguous(), x, gamma, beta, mod, mean, rstd, N, groups, silu)
    return dx, dg, db, dmod, None, None, None, None


groupnorm_mod.register_autograd(_gnm_bwd, setup_context=_gnm_setup)


# ---------------------------------------------------------------------------------------------------------------
# GEGLU: y = u[:, :I] * gelu_erf(u[:, I:])
# ---------------------------------------------------------------------------------------------------------------
@_op("geglu_fwd")
def geglu_fwd(u: Tensor) -> Tensor:
    return ops.geglu_fwd(u)[0]


@geglu_fwd.register_fake
def _(u):
    return u.new_empty(u.shape[0], u.shape[1] // 2)


@_op("geglu_bwd")
def geglu_bwd(dy: Tensor, u: Tensor) -> Tensor:
    du = torch.empty_like(u)
    ops.call("nk_geglu_bwd", dy.data_ptr(), u.data_ptr(), du.data_ptr(), u.shape[0], u.shape[1] // 2, ops._stream())
    return du


@geglu_bwd.register_fake
def _(dy, u):
    return torch.empty_like(u)


@_op("geglu")
def geglu(u: Tensor) -> Tensor:
    return ops.geglu_fwd(u)[0]


@geglu.register_fake
def _(u):
    return u.new_empty(u.shape[0], u.shape[1] // 2)


geglu.register_autograd(lambda ctx, dy: torch.ops.neurosis_hip.geglu_bwd(dy.contiguous(), ctx.saved_tensors[0]),
                        setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0]))


# ---------------------------------------------------------------------------------------------------------------
# attention: softmax(q k^T / sqrt(d)) v on token matrices [B*L, heads*d]
# ---------------------------------------------------------------------------------------------------------------
def _attn_desc(q, k, v, o, B, heads):
    d = ops.NkAttnDesc()
    dh = q.shape[1] // heads
    Lq, Lk = q.shape[0] // B, k.shape[0] // B
    d.B, d.H, d.Lq, d.Lk, d.D = B, heads, Lq, Lk, dh
    d.sq, d.sk, d.sv, d.so = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    d.bq, d.bk, d.bv, d.bo = Lq * q.stride(0), Lk * k.stride(0), Lk * v.stride(0), Lq * o.stride(0)
    d.scale = float(dh) ** -0.5
    d.causal = 0
    return d, Lq, Lk


@_op("attention_fwd")
def attention_fwd(q: Tensor, k: Tensor, v: Tensor, B: int, heads: int) -> Tuple[Tensor, Tensor]:
    import ctypes as C

    o = torch.empty(q.shape[0], q.shape[1], dtype=BF16, device=q.device)
    d, Lq, _ = _attn_desc(q, k, v, o, B, heads)
    lse = torch.empty(B, heads, Lq, dtype=torch.float32, device=q.device)
    ops.call("nk_attention_fwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), ops._stream())
    return o, lse


@attention_fwd.register_fake
def _(q, k, v, B, heads):
    return q.new_empty(q.shape[0], q.shape[1]), q.new_empty(B, heads, q.shape[0] // B, dtype=torch.float32)


@_op("attention_bwd")
def attention_bwd(do: Tensor, q: Tensor, k: Tensor, v: Tensor, o: Tensor, lse: Tensor, B: int, heads: int) -> Tuple[Tensor, Tensor, Tensor]:
    import ctypes as C

    d, Lq, Lk = _attn_desc(q, k, v, o, B, heads)
    dq, dk, dv = (torch.empty(t.shape[0], t.shape[1], dtype=BF16, device=q.device) for t in (q, k, v))
    d.sdq, d.sdk, d.sdv, d.sdo = dq.stride(0), dk.stride(0), dv.stride(0), do.stride(0)
    d.bdq, d.bdk, d.bdv, d.bdo = Lq * dq.stride(0), Lk * dk.stride(0), Lk * dv.stride(0), Lq * do.stride(0)
    ws = ops._ws(ops.query("nk_attention_bwd_ws_floats", C.byref(d)), q.device)
    ops.call("nk_attention_bwd", C.byref(d), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(), dq.data_ptr(), dk.data_ptr(),
             dv.data_ptr(), ws.data_ptr(), ops._stream())
    return dq, dk, dv


@attention_bwd.register_fake
def _(do, q, k, v, o, lse, B, heads):
    return q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape)


@_op("attention")
def attention(q: Tensor, k: Tensor, v: Tensor, B: int, heads: int) -> Tensor:
    return torch.ops.neurosis_hip.attention_fwd(q, k, v, B, heads)[0]


@attention.register_fake
def _(q, k, v, B, heads):
    return q.new_empty(q.shape[0], q.shape[1])


def _attn_setup(ctx, inputs, output):
    q, k, v, B, heads = inputs
    o, lse = torch.ops.neurosis_hip.attention_fwd(q, k, v, B, heads)
    ctx.save_for_backward(q, k, v, o, lse)
    ctx.meta = (B, heads)


def _attn_bwd(ctx, do):
    q, k, v, o, lse = ctx.saved_tensors
    dq, dk, dv = torch.ops.neurosis_hip.attention_bwd(do.contiguous(), q, k, v, o, lse, *ctx.meta)
    return dq, dk, dv, None, None


attention.register_autograd(_attn_bwd, setup_context=_attn_setup)


# ---------------------------------------------------------------------------------------------------------------
# Conv2d as implicit GEMM on channels-last tokens: x [N*H*W, Cin], w [Cout, KH, KW, Cin] (bf16) -> [N*Ho*Wo, Cout]
# ---------------------------------------------------------------------------------------------------------------
def _conv_geom(N, H, W, w, stride, padding):
    Cout, KH, KW, Cin = w.shape
    Ho, Wo = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    return ops._conv_desc(N, H, W, Cin, Cout, KH, KW, stride, padding, padding, Ho, Wo, False), Ho, Wo


@_op("conv2d_fwd")
def conv2d_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], N: int, H: int, W: int, stride: int, padding: int) -> Tensor:
    import ctypes as C

    d, Ho, Wo = _conv_geom(N, H, W, w, stride, padding)
    y = torch.empty(N * Ho * Wo, w.shape[0], dtype=BF16, device=x.device)
    ops.call("nk_conv2d_fwd", C.byref(d), x.data_ptr(), w.data_ptr(), ops._p(bias), None, None, y.data_ptr(), ops._stream())
    return y


@conv2d_fwd.register_fake
def _(x, w, bias, N, H, W, stride, padding):
    KH, KW = w.shape[1], w.shape[2]
    return x.new_empty(N * ((H + 2 * padding - KH) // stride + 1) * ((W + 2 * padding - KW) // stride + 1), w.shape[0])


@_op("conv2d_dgrad")
def conv2d_dgrad(dy: Tensor, w: Tensor, N: int, H: int, W: int, stride: int, padding: int) -> Tensor:
    import ctypes as C

    d, _, _ = _conv_geom(N, H, W, w, stride, padding)
    dx = torch.empty(N * H * W, w.shape[3], dtype=BF16, device=dy.device)
    ops.call("nk_conv2d_dgrad", C.byref(d), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), ops._stream())
    return dx


@conv2d_dgrad.register_fake
def _(dy, w, N, H, W, stride, padding):
    return dy.new_empty(N * H * W, w.shape[3])


@_op("conv2d_wgrad")
def conv2d_wgrad(dy: Tensor, x: Tensor, Cout: int, KH: int, KW: int, N: int, H: int, W: int, stride: int, padding: int) -> Tensor:
    import ctypes as C

    Cin = x.shape[1]
    Ho, Wo = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    d = ops._conv_desc(N, H, W, Cin, Cout, KH, KW, stride, padding, padding, Ho, Wo, False)
    dw = torch.empty(Cout, KH, KW, Cin, dtype=torch.float32, device=x.device)
    ops.call("nk_conv2d_wgrad", C.byref(d), dy.data_ptr(), x.data_ptr(), dw.data_ptr(), 0, ops._stream())
    return dw


@conv2d_wgrad.register_fake
def _(dy, x, Cout, KH, KW, N, H, W, stride, padding):
    return x.new_empty(Cout, KH, KW, x.shape[1], dtype=torch.float32)


@_op("conv2d")
def conv2d(x: Tensor, w: Tensor, bias: Optional[Tensor], N: int, H: int, W: int, stride: int, padding: int) -> Tensor:
    return torch.ops.neurosis_hip.conv2d_fwd(x, w, bias, N, H, W, stride, padding)


@conv2d.register_fake
def _(x, w, bias, N, H, W, stride, padding):
    KH, KW = w.shape[1], w.shape[2]
    return x.new_empty(N * ((H + 2 * padding - KH) // stride + 1) * ((W + 2 * padding - KW) // stride + 1), w.shape[0])


def _conv_setup(ctx, inputs, output):
    x, w, bias, N, H, W, stride, padding = inputs
    ctx.save_for_backward(x, w)
    ctx.meta = (N, H, W, stride, padding, bias is not None)


def _conv_bwd(ctx, dy):
    x, w = ctx.saved_tensors
    N, H, W, stride, padding, has_bias = ctx.meta
    dy = dy.contiguous()
    dx = torch.ops.neurosis_hip.conv2d_dgrad(dy, w, N, H, W, stride, padding) if ctx.needs_input_grad[0] else None
    dw = torch.ops.neurosis_hip.conv2d_wgrad(dy, x, w.shape[0], w.shape[1], w.shape[2], N, H, W, stride, padding).to(w.dtype) if ctx.needs_input_grad[1] else None
    db = torch.ops.neurosis_hip.colsum(dy) if has_bias and ctx.needs_input_grad[2] else None
    return dx, dw, db, None, None, None, None, None


conv2d.register_autograd(_conv_bwd, setup_context=_conv_setup)


# ---------------------------------------------------------------------------------------------------------------
# glue
# ---------------------------------------------------------------------------------------------------------------
@_op("timestep_embedding")
def timestep_embedding(t: Tensor, dim: int, max_period: float = 10000.0) -> Tensor:
    return ops.timestep_embedding(t, dim, max_period)


@timestep_embedding.register_fake
def _(t, dim, max_period=10000.0):
    return t.new_empty(t.shape[0], dim, dtype=BF16)


# ---------------------------------------------------------------------------------------------------------------
# label embeddings (openaimodel.py:574-590 num_classes an int / "continuous"; encoders/classed.py ClassEmbedder)
# ---------------------------------------------------------------------------------------------------------------
@_op("label_rows")
def label_rows(table: Tensor, ids: Tensor, add: Optional[Tensor] = None, out_f32: bool = True) -> Tensor:
    return ops.label_rows(table, ids, add, torch.float32 if out_f32 else BF16)


@label_rows.register_fake
def _(table, ids, add=None, out_f32=True):
    return table.new_empty(ids.shape[0], table.shape[1], dtype=torch.float32 if out_f32 else BF16)


@_op("label_rows_bwd")
def label_rows_bwd(ids: Tensor, d: Tensor, V: int) -> Tensor:
    B, D = d.shape
    d = d.contiguous()
    dtable = torch.empty(V, D, dtype=torch.float32, device=d.device)
    ops.call("nk_label_rows_bwd", ids.contiguous().data_ptr(), d.data_ptr(), D, int(d.dtype == torch.float32), dtable.data_ptr(), B, V, D, 0, ops._stream())
    return dtable


@label_rows_bwd.register_fake
def _(ids, d, V):
    return d.new_empty(V, d.shape[1], dtype=torch.float32)


def _label_rows_setup(ctx, inputs, output):
    table, ids, add, _ = inputs
    ctx.save_for_backward(ids)
    ctx.V = table.shape[0]


def _label_rows_bwd(ctx, d):
    (ids,) = ctx.saved_tensors
    need = tuple(ctx.needs_input_grad) + (False,) * 4      # (an absent optional input may have no entry)
    dt = torch.ops.neurosis_hip.label_rows_bwd(ids, d.contiguous(), ctx.V) if need[0] else None
    return dt, None, (d.to(BF16) if need[2] else None), None


label_rows.register_autograd(_label_rows_bwd, setup_context=_label_rows_setup)


@_op("linear1_fwd")
def linear1_fwd(y: Tensor, w: Tensor, bias: Tensor, add: Optional[Tensor] = None) -> Tensor:
    return ops.linear1_fwd(y, w, bias, add)[0]


@linear1_fwd.register_fake
def _(y, w, bias, add=None):
    return y.new_empty(y.shape[0], w.shape[0], dtype=BF16)


@_op("linear1_bwd")
def linear1_bwd(d: Tensor, y: Tensor, w: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    B, D = d.shape
    dw, db = torch.empty(D, 1, dtype=torch.float32, device=d.device), torch.empty(D, dtype=torch.float32, device=d.device)
    dy = torch.empty(B, 1, dtype=torch.float32, device=d.device)
    ops.call("nk_linear1_bwd", d.data_ptr(), y.data_ptr(), w.data_ptr(), dw.data_ptr(), db.data_ptr(), dy.data_ptr(), B, D, 0, ops._stream())
    return dy, dw, db


@linear1_bwd.register_fake
def _(d, y, w):
    return y.new_empty(y.shape), w.new_empty(w.shape), w.new_empty(w.shape[0])


@_op("linear1")
def linear1(y: Tensor, w: Tensor, bias: Tensor, add: Optional[Tensor] = None) -> Tensor:
    return ops.linear1_fwd(y, w, bias, add)[0]


@linear1.register_fake
def _(y, w, bias, add=None):
    return y.new_empty(y.shape[0], w.shape[0], dtype=BF16)


def _linear1_setup(ctx, inputs, output):
    y, w, bias, add = inputs
    ctx.save_for_backward(y, w)


def _linear1_bwd(ctx, d):
    y, w = ctx.saved_tensors
    d = d.contiguous()
    dy, dw, db = torch.ops.neurosis_hip.linear1_bwd(d, y, w)
    need = tuple(ctx.needs_input_grad) + (False,) * 4      # (an absent optional input may have no entry)
    return (dy if need[0] else None), (dw if need[1] else None), (db if need[2] else None), (d if need[3] else None)


linear1.register_autograd(_linear1_bwd, setup_context=_linear1_setup)


@_op("nchw_to_nlc")
def nchw_to_nlc(x: Tensor, cpad: int) -> Tensor:
    return ops.nchw_to_tokens(x, cpad)


@nchw_to_nlc.register_fake
def _(x, cpad):
    return x.new_empty(x.shape[0] * x.shape[2] * x.shape[3], cpad, dtype=BF16)


@_op("nlc_to_nchw")
def nlc_to_nchw(t: Tensor, N: int, C: int, H: int, W: int) -> Tensor:
    return ops.tokens_to_nchw(t, N, C, H, W)


@nlc_to_nchw.register_fake
def _(t, N, C, H, W):
    return t.new_empty(N, C, H, W, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------
# upsample2x_nearest_cat: the two data-movement ops of the UNet decoder (openaimodel.py:140 F.interpolate(scale_factor=2, mode="nearest")
# in Upsample.forward -- here folded into the following 3 x 3 convolution's gather, so only its BACKWARD exists as a kernel -- and :836
# torch.cat([h, hs.pop()], dim=1) on channels-last tokens).
# ---------------------------------------------------------------------------------------------------------------
@_op("cat_channels")
def cat_channels(a: Tensor, b: Tensor) -> Tensor:
    out = torch.empty(a.shape[0], a.shape[1] + b.shape[1], dtype=BF16, device=a.device)
    ops.call("nk_cat_channels", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0], a.shape[1], b.shape[1], ops._stream())
    return out


@cat_channels.register_fake
def _(a, b):
    return a.new_empty(a.shape[0], a.shape[1] + b.shape[1])


@_op("split_channels")
def split_channels(x: Tensor, Ca: int) -> Tuple[Tensor, Tensor]:
    rows, Cb = x.shape[0], x.shape[1] - Ca
    a, b = torch.empty(rows, Ca, dtype=BF16, device=x.device), torch.empty(rows, Cb, dtype=BF16, device=x.device)
    ops.call("nk_split_channels", x.data_ptr(), a.data_ptr(), b.data_ptr(), rows, Ca, Cb, ops._stream())
    return a, b


@split_channels.register_fake
def _(x, Ca):
    return x.new_empty(x.shape[0], Ca), x.new_empty(x.shape[0], x.shape[1] - Ca)


def _cat_setup(ctx, inputs, output):
    ctx.Ca = inputs[0].shape[1]


def _cat_bwd(ctx, dout):
    da, db = torch.ops.neurosis_hip.split_channels(dout.contiguous(), ctx.Ca)
    return da, db


cat_channels.register_autograd(_cat_bwd, setup_context=_cat_setup)


@_op("upsample2x_nearest_bwd")
def upsample2x_nearest_bwd(dup: Tensor, N: int, H: int, W: int) -> Tensor:
    """dup [N*2H*2W, C] (gradient on the upsampled grid) -> [N*H*W, C]: the 2 x 2 sum-pool that is nearest-upsampling's adjoint"""
    C_ = dup.shape[1]
    dx = torch.empty(N * H * W, C_, dtype=BF16, device=dup.device)
    ops.call("nk_upsample2x_bwd", dup.data_ptr(), dx.data_ptr(), N, H, W, C_, ops._stream())
    return dx


@upsample2x_nearest_bwd.register_fake
def _(dup, N, H, W):
    return dup.new_empty(N * H * W, dup.shape[1])


@_op("upsample2x_nearest")
def upsample2x_nearest(x: Tensor, N: int, H: int, W: int) -> Tensor:
    """Upsample.forward without its conv (openaimodel.py:126-143, use_conv=False): x [N*H*W, C] -> [N*2H*2W, C]"""
    up = torch.empty(N * 4 * H * W, x.shape[1], dtype=BF16, device=x.device)
    ops.call("nk_upsample2x_fwd", x.data_ptr(), up.data_ptr(), N, H, W, x.shape[1], ops._stream())
    return up


@upsample2x_nearest.register_fake
def _(x, N, H, W):
    return x.new_empty(N * 4 * H * W, x.shape[1])


upsample2x_nearest.register_autograd(lambda ctx, dup: (torch.ops.neurosis_hip.upsample2x_nearest_bwd(dup.contiguous(), *ctx.geom), None, None, None),
                                     setup_context=lambda ctx, inputs, output: setattr(ctx, "geom", inputs[1:]))


@_op("avgpool2x")
def avgpool2x(x: Tensor, N: int, H: int, W: int) -> Tensor:
    """Downsample.forward without its conv (openaimodel.py:183-197, use_conv=False): avg_pool2d(2, 2), x [N*H*W, C] -> [N*(H//2)*(W//2), C]"""
    y = torch.empty(N * (H // 2) * (W // 2), x.shape[1], dtype=BF16, device=x.device)
    ops.call("nk_avgpool2x_fwd", x.data_ptr(), y.data_ptr(), N, H, W, x.shape[1], ops._stream())
    return y


@avgpool2x.register_fake
def _(x, N, H, W):
    return x.new_empty(N * (H // 2) * (W // 2), x.shape[1])


@_op("avgpool2x_bwd")
def avgpool2x_bwd(dy: Tensor, N: int, H: int, W: int) -> Tensor:
    """dy [N*(H//2)*(W//2), C] -> dx [N*H*W, C]: a quarter of each window's gradient to its four inputs, zeros in a dropped odd row / column"""
    dx = torch.empty(N * H * W, dy.shape[1], dtype=BF16, device=dy.device)
    ops.call("nk_avgpool2x_bwd", dy.data_ptr(), dx.data_ptr(), N, H, W, dy.shape[1], ops._stream())
    return dx


@avgpool2x_bwd.register_fake
def _(dy, N, H, W):
    return dy.new_empty(N * H * W, dy.shape[1])


avgpool2x.register_autograd(lambda ctx, dy: (torch.ops.neurosis_hip.avgpool2x_bwd(dy.contiguous(), *ctx.geom), None, None, None),
                            setup_context=lambda ctx, inputs, output: setattr(ctx, "geom", inputs[1:]))


@_op("upsample2x_nearest_conv")
def upsample2x_nearest_conv(x: Tensor, w: Tensor, bias: Optional[Tensor], N: int, H: int, W: int) -> Tensor:
    """Upsample.forward with use_conv (openaimodel.py:126-143): nearest x2 then 3 x 3 / padding 1 conv, the upsampled map never written"""
    import ctypes as C

    Cout, KH, KW, Cin = w.shape
    d = ops._conv_desc(N, H, W, Cin, Cout, KH, KW, 1, 1, 1, 2 * H, 2 * W, True)
    y = torch.empty(N * 4 * H * W, Cout, dtype=BF16, device=x.device)
    ops.call("nk_conv2d_fwd", C.byref(d), x.data_ptr(), w.data_ptr(), ops._p(bias), None, None, y.data_ptr(), ops._stream())
    return y


@upsample2x_nearest_conv.register_fake
def _(x, w, bias, N, H, W):
    return x.new_empty(N * 4 * H * W, w.shape[0])


# ---------------------------------------------------------------------------------------------------------------
# edm_loss: StandardDiffusionLoss "edm" arithmetic around the network (loss.py:117-157, denoiser.py:41-53, functions.py:91-94)
# ---------------------------------------------------------------------------------------------------------------
@_op("edm_prepare")
def edm_prepare(x: Tensor, eps: Tensor, sigma: Tensor, c_in: Tensor, cpad: int) -> Tuple[Tensor, Tensor]:
    """z_t = x + sigma * eps (fp32 NCHW) and the network input bf16(z_t * c_in) as channels-last tokens padded to cpad channels"""
    B, Cc, H, W = x.shape
    zt = torch.empty_like(x)
    net_in = torch.empty(B * H * W, cpad, dtype=BF16, device=x.device)
    ops.call("nk_edm_prepare", x.data_ptr(), eps.data_ptr(), sigma.data_ptr(), c_in.data_ptr(), zt.data_ptr(), net_in.data_ptr(), B, Cc, H * W, cpad, ops._stream())
    return zt, net_in


@edm_prepare.register_fake
def _(x, eps, sigma, c_in, cpad):
    return torch.empty_like(x), x.new_empty(x.shape[0] * x.shape[2] * x.shape[3], cpad, dtype=BF16)


@_op("edm_prepare_cat")
def edm_prepare_cat(x: Tensor, eps: Tensor, sigma: Tensor, c_in: Tensor, extra: Tensor, cpad: int) -> Tuple[Tensor, Tensor]:
    """edm_prepare for a concat-conditioned UNet (OpenAIWrapper.forward, wrappers.py:33): the network input carries bf16(extra) -- fp32
    NCHW [B, Ce, H, W], NOT scaled by c_in -- in channels C..C+Ce-1 behind bf16(z_t * c_in); cpad = C + Ce rounded up to 8"""
    B, Cc, H, W = x.shape
    zt = torch.empty_like(x)
    net_in = torch.empty(B * H * W, cpad, dtype=BF16, device=x.device)
    ops.call("nk_edm_prepare_cat", x.data_ptr(), eps.data_ptr(), sigma.data_ptr(), c_in.data_ptr(), extra.data_ptr(), zt.data_ptr(), net_in.data_ptr(),
             B, Cc, extra.shape[1], H * W, cpad, ops._stream())
    return zt, net_in


@edm_prepare_cat.register_fake
def _(x, eps, sigma, c_in, extra, cpad):
    return torch.empty_like(x), x.new_empty(x.shape[0] * x.shape[2] * x.shape[3], cpad, dtype=BF16)


@_op("sample_prepare_cat")
def sample_prepare_cat(x: Tensor, c_in: Tensor, extra_u: Optional[Tensor], extra_c: Tensor, cpad: int, rep: int) -> Tensor:
    """The sampler's network input for a concat-conditioned UNet: bf16 tokens [rep * B * H * W, cpad], channels < C = c_in * x in every
    replica, channels C..C+Ce-1 = extra_u in replica 0 and extra_c in replica 1 (rep == 1: extra_c; extra_u may be None), unscaled"""
    B, Cc, H, W = x.shape
    net_in = torch.empty(rep * B * H * W, cpad, dtype=BF16, device=x.device)
    ops.call("nk_sample_prepare_cat", x.data_ptr(), c_in.data_ptr(), ops._p(extra_u), extra_c.data_ptr(), net_in.data_ptr(), B, Cc, extra_c.shape[1], H * W,
             cpad, rep, ops._stream())
    return net_in


@sample_prepare_cat.register_fake
def _(x, c_in, extra_u, extra_c, cpad, rep):
    return x.new_empty(rep * x.shape[0] * x.shape[2] * x.shape[3], cpad, dtype=BF16)


@_op("edm_loss_fwd")
def edm_loss_fwd(net_out: Tensor, zt: Tensor, target: Tensor, c_out: Tensor, c_skip: Tensor, w: Tensor) -> Tensor:
    """loss[b] = w[b] * mean((net_out * c_out + z_t * c_skip - target)^2): net_out bf16 tokens [B*H*W, Cpad], z_t / target fp32 NCHW"""
    B, Cc, H, W = zt.shape
    loss = torch.empty(B, dtype=torch.float32, device=zt.device)
    ops.call("nk_edm_loss", net_out.data_ptr(), zt.data_ptr(), target.data_ptr(), c_out.data_ptr(), c_skip.data_ptr(), w.data_ptr(), loss.data_ptr(), None,
             B, Cc, H * W, net_out.shape[1], 1.0, ops._stream())
    return loss


@edm_loss_fwd.register_fake
def _(net_out, zt, target, c_out, c_skip, w):
    return zt.new_empty(zt.shape[0], dtype=torch.float32)


@_op("edm_loss_bwd")
def edm_loss_bwd(dloss: Tensor, net_out: Tensor, zt: Tensor, target: Tensor, c_out: Tensor, c_skip: Tensor, w: Tensor) -> Tensor:
    """d sum_b(dloss[b] * loss[b]) / d net_out, bf16 tokens"""
    B, Cc, H, W = zt.shape
    wg = (w * dloss.float()).contiguous()
    dnet = torch.empty_like(net_out)
    scratch = torch.empty(B, dtype=torch.float32, device=zt.device)
    ops.call("nk_edm_loss", net_out.data_ptr(), zt.data_ptr(), target.data_ptr(), c_out.data_ptr(), c_skip.data_ptr(), wg.data_ptr(), scratch.data_ptr(),
             dnet.data_ptr(), B, Cc, H * W, net_out.shape[1], 1.0, ops._stream())
    return dnet


@edm_loss_bwd.register_fake
def _(dloss, net_out, zt, target, c_out, c_skip, w):
    return torch.empty_like(net_out)


@_op("edm_loss")
def edm_loss(net_out: Tensor, zt: Tensor, target: Tensor, c_out: Tensor, c_skip: Tensor, w: Tensor) -> Tensor:
    return torch.ops.neurosis_hip.edm_loss_fwd(net_out, zt, target, c_out, c_skip, w)


@edm_loss.register_fake
def _(net_out, zt, target, c_out, c_skip, w):
    return zt.new_empty(zt.shape[0], dtype=torch.float32)


def _edm_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _edm_bwd(ctx, dloss):
    net_out, zt, target, c_out, c_skip, w = ctx.saved_tensors
    return torch.ops.neurosis_hip.edm_loss_bwd(dloss.contiguous(), net_out, zt, target, c_out, c_skip, w), None, None, None, None, None


edm_loss.register_autograd(_edm_bwd, setup_context=_edm_setup)


# ---------------------------------------------------------------------------------------------------------------
# flat_allreduce_{start, wait}: the data-parallel exchange of a flat gradient buffer as two ops (what Lightning's DDP reducer does
# behind autograd hooks for the reference; neurosis_amd.dp.FlatGradReducer underneath: RCCL on its own stream, joined by `wait`).
# The reducer is found by the buffer's address: one per flat gradient buffer and process.
# ---------------------------------------------------------------------------------------------------------------
_reducers: dict = {}


def _reducer_for(flat: Tensor):
    from .dp import FlatGradReducer

    key = (flat.data_ptr(), flat.numel())
    r = _reducers.get(key)
    if r is None:
        r = _reducers[key] = FlatGradReducer(flat)
    return r


@_op("flat_allreduce_start", mutates=("flat",))
def flat_allreduce_start(flat: Tensor, lo: int, hi: int) -> None:
    """begin summing flat[lo:hi] over the ranks (asynchronous: ordered behind the current stream, running on the exchange stream)"""
    _reducer_for(flat).reduce_range(lo, hi)


@flat_allreduce_start.register_fake
def _(flat, lo, hi):
    return None


@_op("flat_allreduce_wait", mutates=("flat",))
def flat_allreduce_wait(flat: Tensor) -> None:
    """make the current stream wait for every reduction started on this buffer"""
    _reducer_for(flat).finish()


@flat_allreduce_wait.register_fake
def _(flat):
    return None


# ---------------------------------------------------------------------------------------------------------------
# the fused entry points of round 3
# ---------------------------------------------------------------------------------------------------------------
@_op("conv2d_fwd_stats")
def conv2d_fwd_stats(x: Tensor, w: Tensor, bias: Optional[Tensor], N: int, H: int, W: int, groups: int) -> Tuple[Tensor, Tensor]:
    """3 x 3 / stride 1 / padding 1 convolution that also returns the GroupNorm sums of its output, [N, 2 * groups] fp32
    (entry 2g = sum, 2g + 1 = sum of squares); from the kernel's epilogue where the halo-tile kernel takes the shape, else a statistics pass"""
    import ctypes as C

    Cout, KH, KW, Cin = w.shape
    d = ops._conv_desc(N, H, W, Cin, Cout, KH, KW, 1, 1, 1, H, W, False)
    y = torch.empty(N * H * W, Cout, dtype=BF16, device=x.device)
    sums = torch.empty(N, 2 * groups, dtype=torch.float32, device=x.device)
    tiles = ops.query("nk_conv2d_stats_tiles", C.byref(d), groups) if (KH, KW) == (3, 3) else 0
    if tiles:
        part = torch.empty(N, tiles, 2 * groups, dtype=torch.float32, device=x.device)
        ops.call("nk_conv2d_fwd_stats", C.byref(d), x.data_ptr(), w.data_ptr(), ops._p(bias), None, None, y.data_ptr(), part.data_ptr(), groups, ops._stream())
        ws = ops._ws(ops.query("nk_groupnorm_sums_ws_floats", N, tiles, groups), x.device)
        ops.call("nk_groupnorm_sums_from_parts", part.data_ptr(), sums.data_ptr(), ws.data_ptr(), N, tiles, groups, ops._stream())
    else:
        ops.call("nk_conv2d_fwd", C.byref(d), x.data_ptr(), w.data_ptr(), ops._p(bias), None, None, y.data_ptr(), ops._stream())
        ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, H * W, Cout, groups), x.device)
        ops.call("nk_groupnorm_sums", y.data_ptr(), sums.data_ptr(), ws.data_ptr(), N, H * W, Cout, groups, ops._stream())
    return y, sums


@conv2d_fwd_stats.register_fake
def _(x, w, bias, N, H, W, groups):
    return x.new_empty(N * H * W, w.shape[0]), x.new_empty(N, 2 * groups, dtype=torch.float32)


@_op("linear_fwd_geglu")
def linear_fwd_geglu(x: Tensor, w: Tensor, bias: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """FeedForward.net[0] (GEGLU): u = x @ w^T + bias [M, 2I] and h = u[:, :I] * gelu(u[:, I:]) [M, I] -- one launch where the 256 x 256 kernel
    takes the shape (ops.linear_geglu_fwd), else the projection followed by the GEGLU kernel"""
    M, K = x.shape
    I = w.shape[0] // 2
    if x.is_contiguous() and w.is_contiguous() and ops.query("nk_linear_fwd_geglu_ok", M, I, K):
        u = torch.empty(M, 2 * I, dtype=BF16, device=x.device)
        h = torch.empty(M, I, dtype=BF16, device=x.device)
        ops.call("nk_linear_fwd_geglu", x.data_ptr(), w.data_ptr(), ops._p(bias), u.data_ptr(), h.data_ptr(), M, I, K, x.stride(0), w.stride(0), u.stride(0),
                 h.stride(0), ops._stream())
        return u, h
    u = torch.ops.neurosis_hip.linear_fwd(x, w, bias)
    return u, torch.ops.neurosis_hip.geglu_fwd(u)


@linear_fwd_geglu.register_fake
def _(x, w, bias):
    return x.new_empty(x.shape[0], w.shape[0]), x.new_empty(x.shape[0], w.shape[0] // 2)


@_op("linear_dgrad_geglu")
def linear_dgrad_geglu(dy: Tensor, w: Tensor, u: Tensor) -> Tensor:
    """FeedForward backward through net[2] and the GEGLU in one launch: du [M, 2I] from dy [M, N], w [N, I], u = [a | g] [M, 2I]"""
    M, N = dy.shape
    I = w.shape[1]
    du = torch.empty(M, 2 * I, dtype=BF16, device=dy.device)
    ops.call("nk_linear_dgrad_geglu", dy.data_ptr(), w.data_ptr(), u.data_ptr(), du.data_ptr(), M, N, I, dy.stride(0), w.stride(0), u.stride(0), du.stride(0),
             ops._stream())
    return du


@linear_dgrad_geglu.register_fake
def _(dy, w, u):
    return dy.new_empty(dy.shape[0], 2 * w.shape[1])


# ---------------------------------------------------------------------------------------------------------------
# dropout: y = residual + x * mask(token, site) / (1 - p), the mask regenerated from a counter (csrc/dropout.hip), never stored
# ---------------------------------------------------------------------------------------------------------------
@_op("dropout")
def dropout(x: Tensor, token: Tensor, p: float, site: int, residual: Optional[Tensor] = None) -> Tensor:
    """nn.Dropout(p) in training mode on a bf16 token matrix [rows, cols] (cols % 8 == 0), optional residual added behind the mask.  token:
    the int64 [2] {seed, step} tensor of neurosis_amd.ops.dropout_draw().  Its own backward is the same call on the gradient."""
    return ops.dropout_mask_like(x, p, site, token, residual, inplace=False)


@dropout.register_fake
def _(x, token, p, site, residual=None):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


dropout.register_autograd(lambda ctx, dy: (torch.ops.neurosis_hip.dropout(dy.contiguous(), ctx.saved_tensors[0], ctx.p, ctx.site), None, None, None,
                                           dy if ctx.has_residual else None),
                          setup_context=lambda ctx, inputs, output: (ctx.save_for_backward(inputs[1]), setattr(ctx, "p", inputs[2]),
                                                                     setattr(ctx, "site", inputs[3]), setattr(ctx, "has_residual", inputs[4] is not None)))


# ---------------------------------------------------------------------------------------------------------------
# vector quantizer (csrc/vq.hip): code search, per-code statistics, straight-through gather with the VQ loss
# ---------------------------------------------------------------------------------------------------------------
@_op("vq_search")
def vq_search(z: Tensor, codebook: Tensor) -> Tensor:
    """idx [N] int64: the nearest code of every row of z [N, D] fp32 in codebook [n_e, D] fp32 (exact fp32, lowest index among equal scores).
    Not differentiable: the indices are integers."""
    return ops.vq_search(z, codebook)


@vq_search.register_fake
def _(z, codebook):
    return z.new_empty(z.shape[0], dtype=torch.int64)


@_op("vq_code_stats")
def vq_code_stats(idx: Tensor, z: Tensor, n_e: int) -> Tuple[Tensor, Tensor]:
    """(count [n_e] int64, sum [n_e, D] fp32) of the rows of z by the code they chose; deterministic"""
    return ops.vq_code_stats(idx, z, n_e)


@vq_code_stats.register_fake
def _(idx, z, n_e):
    return z.new_empty(n_e, dtype=torch.int64), z.new_empty(n_e, z.shape[1], dtype=torch.float32)


@_op("vq_quantize")
def vq_quantize(z: Tensor, codebook: Tensor, idx: Tensor, beta: float = 0.25) -> Tuple[Tensor, Tensor]:
    """(z_q, loss) of VectorQuantizer for z [N, D] fp32 and the indices of vq_search: z_q = codebook[idx], straight-through (its gradient
    goes to z unchanged), loss = beta * mean((sg[z_q] - z)^2) + mean((z_q - sg[z])^2)."""
    z_q, sumsq = ops.vq_quantize(idx, codebook, z)
    mse = sumsq / z.numel()
    return z_q, beta * mse + mse


@vq_quantize.register_fake
def _(z, codebook, idx, beta=0.25):
    return torch.empty_like(z, memory_format=torch.contiguous_format), z.new_empty(())


def _vq_quantize_setup(ctx, inputs, output):
    z, codebook, idx, beta = inputs
    ctx.save_for_backward(z, codebook, idx, output[0])
    ctx.beta = beta


def _vq_quantize_bwd(ctx, d_zq, d_loss):
    z, codebook, idx, z_q = ctx.saved_tensors
    k = d_loss * (2.0 / z.numel())
    dz = dE = None
    if ctx.needs_input_grad[0]:
        dz = d_zq + (k * ctx.beta) * (z - z_q)
    if ctx.needs_input_grad[1]:
        count, total = torch.ops.neurosis_hip.vq_code_stats(idx, z, codebook.shape[0])
        dE = k * (count.to(torch.float32).unsqueeze(1) * codebook - total)
    return dz, dE, None, None


vq_quantize.register_autograd(_vq_quantize_bwd, setup_context=_vq_quantize_setup)


# ---------------------------------------------------------------------------------------------------------------
# Gumbel-softmax quantizer (csrc/gumbel.hip): exact-fp32 logits, counter-based noise, the row passes, and the whole bottleneck
# ---------------------------------------------------------------------------------------------------------------
@_op("gumbel_logits")
def gumbel_logits(z: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """logits [N, n] fp32 = z [N, h] @ weight [n, h]^T + bias, the fp32 fma chain in k order (not differentiable here: gumbel_quantize is)"""
    return ops.gumbel_logits(z, weight, bias)


@gumbel_logits.register_fake
def _(z, weight, bias):
    return z.new_empty(z.shape[0], weight.shape[0])


@_op("gumbel_noise")
def gumbel_noise(rows: int, cols: int, site: int, token: Tensor) -> Tensor:
    """g [rows, cols] fp32: the Gumbel noise of (token, site); token the int64 [2] {seed, step} tensor of neurosis_amd.ops.dropout_draw()"""
    return ops.gumbel_noise(rows, cols, site, token)


@gumbel_noise.register_fake
def _(rows, cols, site, token):
    return token.new_empty(rows, cols, dtype=torch.float32)


@_op("gumbel_softmax_fwd")
def gumbel_softmax_fwd(logits: Tensor, tau: float, noise: Optional[Tensor] = None, token: Optional[Tensor] = None, site: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """(y bf16 [N, n], idx int64 [N], kl scalar) of softmax((logits + g) / tau), g = noise or the generator's under (token, site)"""
    return ops.gumbel_softmax_fwd(logits, tau, noise=noise, token=token, site=site)


@gumbel_softmax_fwd.register_fake
def _(logits, tau, noise=None, token=None, site=0):
    return logits.new_empty(logits.shape, dtype=BF16), logits.new_empty(logits.shape[0], dtype=torch.int64), logits.new_empty(())


@_op("gumbel_softmax_bwd")
def gumbel_softmax_bwd(logits: Tensor, y: Tensor, G: Tensor, tau: float, w_kl: float) -> Tensor:
    """d [N, n] bf16: the gradient of <G, y> + w_kl * kl with respect to the logits (G is left untouched here; ops.gumbel_softmax_bwd works in place)"""
    return ops.gumbel_softmax_bwd(logits, y, G.clone(), tau, w_kl)


@gumbel_softmax_bwd.register_fake
def _(logits, y, G, tau, w_kl):
    return torch.empty_like(G, memory_format=torch.contiguous_format)


@_op("gumbel_quantize")
def gumbel_quantize(z: Tensor, proj_w: Tensor, proj_b: Tensor, embed: Tensor, noise: Tensor, tau: float, hard: bool,
                    kl_weight: float) -> Tuple[Tensor, Tensor, Tensor]:
    """(z_q [N, d] fp32, loss, idx [N]) of GumbelQuantizer on latent rows z [N, h] fp32: proj_w [n, h], proj_b [n], embed [n, d] fp32, noise
    [N, n] fp32 Gumbel values; loss = kl_weight * KL.  Differentiable in z, proj_w, proj_b and embed (bf16 GEMM gradients)."""
    z_q, idx, kl, _, _, _ = ops.gumbel_quantize(z.contiguous(), proj_w, proj_b, embed, ops.cast_bf16(proj_w), ops.cast_bf16(embed), tau, hard, noise=noise)
    return z_q, kl_weight * kl, idx


@gumbel_quantize.register_fake
def _(z, proj_w, proj_b, embed, noise, tau, hard, kl_weight):
    return z.new_empty(z.shape[0], embed.shape[1]), z.new_empty(()), z.new_empty(z.shape[0], dtype=torch.int64)


def _gumbel_quantize_setup(ctx, inputs, output):
    z, proj_w, proj_b, embed, noise, ctx.tau, ctx.hard, ctx.kl_weight = inputs
    ctx.save_for_backward(z, proj_w, proj_b, embed, noise, output[2])


def _gumbel_quantize_bwd(ctx, d_zq, d_loss, d_idx):
    """the forward is run again from the saved inputs (same noise, same bits), then the closure's backward"""
    z, proj_w, proj_b, embed, noise, idx = ctx.saved_tensors
    z = z.contiguous()
    n = proj_w.shape[0]
    _, _, _, _, y, bwd = ops.gumbel_quantize(z, proj_w, proj_b, embed, ops.cast_bf16(proj_w), ops.cast_bf16(embed), ctx.tau, ctx.hard, noise=noise)
    dz_rows = d_zq.float().contiguous()
    d_rows, dl, dzb = bwd(dz_rows, float(d_loss) * ctx.kl_weight)
    dW = torch.empty_like(proj_w)
    db = torch.empty_like(proj_b)
    ops.gemm_tn_f32(dl, ops.cast_bf16(z), dW, False, dbias=db)
    if ctx.hard:
        dE = ops.vq_code_stats(idx, dz_rows, n)[1]
    else:
        dE = torch.empty_like(embed)
        ops.gemm_tn_f32(y, dzb, dE, False)
    return d_rows.float(), dW, db, dE, None, None, None, None


gumbel_quantize.register_autograd(_gumbel_quantize_bwd, setup_context=_gumbel_quantize_setup)


# ---------------------------------------------------------------------------------------------------------------
# antialiased bicubic resize (csrc/resample.hip): fp32 NCHW planes, forward and adjoint on one banded kernel
# ---------------------------------------------------------------------------------------------------------------
@_op("resize_bicubic_aa")
def resize_bicubic_aa(x: Tensor, out_h: int, out_w: int) -> Tensor:
    """F.interpolate(x, (out_h, out_w), mode="bicubic", antialias=True) for fp32 NCHW x; differentiable (its backward is resize_bicubic_aa_bwd)."""
    y, _ = ops.resize_bicubic_aa(x, (out_h, out_w))
    return y.clone() if y is x else y          # (an op may not return its input; equal sizes are the identity)


@resize_bicubic_aa.register_fake
def _(x, out_h, out_w):
    return x.new_empty(x.shape[0], x.shape[1], out_h, out_w)


@_op("resize_bicubic_aa_bwd")
def resize_bicubic_aa_bwd(dy: Tensor, in_h: int, in_w: int) -> Tensor:
    """dx [N, C, in_h, in_w] = R^T dy for the resize R from (in_h, in_w) to dy's size: the same kernel with the transposed tables."""
    dx = ops.resize_bicubic_aa_bwd(dy, (in_h, in_w))
    return dx.clone() if dx is dy else dx


@resize_bicubic_aa_bwd.register_fake
def _(dy, in_h, in_w):
    return dy.new_empty(dy.shape[0], dy.shape[1], in_h, in_w)


def _resize_setup(ctx, inputs, output):
    ctx.in_hw = tuple(inputs[0].shape[2:])


def _resize_bwd(ctx, dy):
    return torch.ops.neurosis_hip.resize_bicubic_aa_bwd(dy.contiguous(), ctx.in_hw[0], ctx.in_hw[1]), None, None


resize_bicubic_aa.register_autograd(_resize_bwd, setup_context=_resize_setup)
# the adjoint is linear too: its backward is the forward resize
resize_bicubic_aa_bwd.register_autograd(lambda ctx, dx: (torch.ops.neurosis_hip.resize_bicubic_aa(dx.contiguous(), ctx.out_hw[0], ctx.out_hw[1]), None, None),
                                        setup_context=lambda ctx, inputs, output: setattr(ctx, "out_hw", tuple(inputs[0].shape[2:])))


OPS = ("resize_bicubic_aa", "resize_bicubic_aa_bwd", "vq_search", "vq_code_stats", "vq_quantize", "groupnorm_mod_fwd", "groupnorm_mod_bwd", "groupnorm_mod", "upsample2x_nearest", "avgpool2x", "avgpool2x_bwd", "dropout", "cat_channels", "split_channels", "upsample2x_nearest_bwd", "upsample2x_nearest_conv", "edm_prepare", "edm_prepare_cat", "sample_prepare_cat", "edm_loss_fwd", "edm_loss_bwd", "edm_loss",
       "flat_allreduce_start", "flat_allreduce_wait", "conv2d_fwd_stats", "linear_dgrad_geglu", "linear_fwd_geglu", "linear_fwd", "linear_dgrad", "linear_wgrad", "colsum", "linear", "layernorm_fwd", "layernorm_bwd", "layernorm", "groupnorm_silu_fwd",
       "groupnorm_silu_bwd", "groupnorm_silu", "geglu_fwd", "geglu_bwd", "geglu", "attention_fwd", "attention_bwd", "attention", "conv2d_fwd",
       "conv2d_dgrad", "conv2d_wgrad", "conv2d", "timestep_embedding", "nchw_to_nlc", "nlc_to_nchw", "gumbel_logits", "gumbel_noise", "gumbel_softmax_fwd",
       "gumbel_softmax_bwd", "gumbel_quantize")
