"""Float64 CPU restatement of the ADM block family, written from the math (NCHW tensors, plain torch arithmetic):

  * the scale-shift modulated GroupNorm, forward and the closed-form backward the HIP kernels implement;
  * the two parameter-free resamplers (nearest 2x, avg_pool 2x2 in floor mode) with their adjoints;
  * the ResBlock in its three variants (scale-shift norm, down, up -- any combination), differentiable through torch autograd.

Scale-shift norm: emb_out = Linear(SiLU(emb)) is [N, 2C]; scale = the FIRST C columns, shift = the LAST C;
    u = xhat * gamma_c + beta_c,  z = u * (1 + s_nc) + t_nc,  y = silu(z)
which is a GroupNorm with the per-image affine gamma'_nc = gamma_c (1 + s_nc), beta'_nc = beta_c (1 + s_nc) + t_nc.
Backward, with dz = dy * silu'(z), A_nc = sum_hw dz, B_nc = sum_hw dz * xhat:
    d_shift_nc = A_nc                          d_scale_nc = gamma_c B_nc + beta_c A_nc
    dbeta_c = sum_n (1 + s_nc) A_nc            dgamma_c = sum_n (1 + s_nc) B_nc
    dx = rstd * (dz gamma' - mean_group(dz gamma') - xhat * mean_group(dz gamma' xhat))        (GroupNorm's own, with gamma' for gamma)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

F64 = torch.float64


def _stats(x, groups, eps):
    N, C, H, W = x.shape
    xg = x.reshape(N, groups, -1)
    mean = xg.mean(2, keepdim=True)
    var = ((xg - mean) ** 2).mean(2, keepdim=True)
    rstd = (var + eps).rsqrt()
    return ((xg - mean) * rstd).reshape(N, C, H, W), rstd.reshape(N, groups)


def gn_mod_fwd(x, gamma, beta, scale, shift, groups=32, eps=1e-5, silu=True, swap=False):
    """x [N, C, H, W]; gamma, beta [C]; scale, shift [N, C].  swap=True reads the two halves of emb_out the wrong way round (the
    negative control of the GPU test)."""
    if swap:
        scale, shift = shift, scale
    xhat, _ = _stats(x, groups, eps)
    u = xhat * gamma[None, :, None, None] + beta[None, :, None, None]
    z = u * (1.0 + scale[:, :, None, None]) + shift[:, :, None, None]
    return z * torch.sigmoid(z) if silu else z


def gn_mod_bwd(dy, x, gamma, beta, scale, shift, groups=32, eps=1e-5, silu=True):
    """the closed form above -> dx, dgamma, dbeta, d_scale, d_shift"""
    N, C, H, W = x.shape
    xhat, rstd = _stats(x, groups, eps)
    s1 = 1.0 + scale
    gp = gamma[None, :] * s1                       # gamma'_nc
    bp = beta[None, :] * s1 + shift                # beta'_nc
    z = xhat * gp[:, :, None, None] + bp[:, :, None, None]
    if silu:
        sg = torch.sigmoid(z)
        dz = dy * (sg * (1.0 + z * (1.0 - sg)))
    else:
        dz = dy
    A = dz.sum((2, 3))
    B = (dz * xhat).sum((2, 3))
    d_shift = A
    d_scale = gamma[None, :] * B + beta[None, :] * A
    dbeta = (s1 * A).sum(0)
    dgamma = (s1 * B).sum(0)
    t = dz * gp[:, :, None, None]
    m1 = t.reshape(N, groups, -1).mean(2)
    m2 = (t * xhat).reshape(N, groups, -1).mean(2)
    cpg = C // groups
    rep = lambda v: v.repeat_interleave(cpg, 1)[:, :, None, None]
    dx = rep(rstd) * (t - rep(m1) - xhat * rep(m2))
    return dx, dgamma, dbeta, d_scale, d_shift


def upsample2x(x):
    N, C, H, W = x.shape
    return x[:, :, :, None, :, None].expand(N, C, H, 2, W, 2).reshape(N, C, 2 * H, 2 * W)


def upsample2x_bwd(dup):
    N, C, H2, W2 = dup.shape
    return dup.reshape(N, C, H2 // 2, 2, W2 // 2, 2).sum((3, 5))


def avgpool2x(x):
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    return x[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).sum((3, 5)) * 0.25


def avgpool2x_bwd(dy, H, W):
    """the gradient on the [H, W] grid: a quarter of dy to each of a window's four inputs, zero in a dropped odd row / column"""
    N, C, Ho, Wo = dy.shape
    dx = torch.zeros(N, C, H, W, dtype=dy.dtype)
    dx[:, :, :2 * Ho, :2 * Wo] = upsample2x(dy) * 0.25
    return dx


def _silu(v):
    return v * torch.sigmoid(v)


def resblock(sd: dict, x, emb, use_scale_shift_norm=False, up=False, down=False, eps=1e-5):
    """The ResBlock on a state_dict of its parameters (the reference's key names), any of the three ADM options.  The skip connection is
    whatever the state_dict holds: none (identity), a 1x1 or a 3x3 kernel."""
    zero = torch.zeros(x.shape[0], x.shape[1], dtype=x.dtype)
    h = gn_mod_fwd(x, sd["in_layers.0.weight"], sd["in_layers.0.bias"], zero, zero, 32, eps, silu=True)
    if up:
        h, x = upsample2x(h), upsample2x(x)
    elif down:
        h, x = avgpool2x(h), avgpool2x(x)
    w1 = sd["in_layers.2.weight"]
    h = F.conv2d(h, w1, sd["in_layers.2.bias"], padding=w1.shape[-1] // 2)
    emb_out = F.linear(_silu(emb), sd["emb_layers.1.weight"], sd["emb_layers.1.bias"])
    Cout = w1.shape[0]
    gn2 = (sd["out_layers.0.weight"], sd["out_layers.0.bias"])
    if use_scale_shift_norm:
        h = gn_mod_fwd(h, *gn2, emb_out[:, :Cout], emb_out[:, Cout:], 32, eps, silu=True)
    else:
        h = h + emb_out[:, :, None, None]
        zc = torch.zeros_like(emb_out)
        h = gn_mod_fwd(h, *gn2, zc, zc, 32, eps, silu=True)
    w2 = sd["out_layers.3.weight"]
    h = F.conv2d(h, w2, sd["out_layers.3.bias"], padding=w2.shape[-1] // 2)
    if "skip_connection.weight" in sd:
        ws = sd["skip_connection.weight"]
        x = F.conv2d(x, ws, sd["skip_connection.bias"], padding=ws.shape[-1] // 2)
    return x + h


# ---- fixture access (tests/golden/make_golden_adm.py stores large activations at sampled pixels, weight gradients as sampled rows) ----
def stored_view(entry: dict, t):
    """(the part of the full tensor t that the fixture entry holds, the stored values)"""
    if "full" in entry:
        return t, entry["full"]
    return t.flatten(2)[:, :, entry["pixels"]], entry["values"]


def stored_rows(g, rows: int, conv_cin: int):
    if g.dim() == 4:
        return g[:rows, :conv_cin]
    return g[:rows] if g.dim() >= 2 else g
