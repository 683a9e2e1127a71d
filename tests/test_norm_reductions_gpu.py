"""The normalisation kernels' reductions at the sizes the training step runs, against float64 references computed by torch on the GPU
from the same bf16 inputs: GroupNorm (+SiLU) forward / backward, the stand-alone GroupNorm sums, the convolution's statistics epilogue
(one- and two-level partial sums) with the apply-only GroupNorm behind it, LayerNorm (both backward forms) and the PatchGAN's BatchNorm.

Three kinds of check:
  exact   inputs in {-1, 0, 1} (sparse ternary convolution weights): every partial sum is an integer below 2^24, so every fp32 sum is
          exact in any order and the kernel must equal the float64 sum bit for bit -- a dropped, doubled or misplaced partial shows.
  bounded every element against the float64 reference, within a bound derived from the arithmetic (below), never from measurements.
  same    two runs on the same inputs are bit-identical (the kernels reduce in a fixed order, without atomics).

Bounds.  u = 2^-24 is the fp32 unit roundoff.  An fp32 reduction is held to |got - ref| <= RED * sum|terms|, RED = 1e-5, computed in
float64: condition-aware, so it stays meaningful where a sum nearly cancels.  RED is the worst-case error of a serial chain of 168 fp32
adds; the kernels' chains are 100-300 adds (thread-serial rows, then fixed-order LDS / partial-row combines), and the rounding errors of
independent adds grow as sqrt(chain) * u ~ 1e-6, so RED holds with a wide margin while a dropped partial out of ~10^3 does not.
Statistics (mean, rstd) are held to that bound carried through their formulas: GroupNorm and BatchNorm form the variance in one pass,
E[x^2] - E[x]^2, so their rstd bound grows as (|mean| / sigma)^2; LayerNorm's two passes do not.  The bf16 outputs (y, dx) are checked
against the float64 formula evaluated with the kernel's OWN fp32 statistics (checked separately above), within one bf16 ulp of the
reference plus a floor of 4-8 u times the magnitude of the fp32 terms the kernel adds (for dx: the terms that cancel, |A dz|,
rstd^2 |s2| / cnt (|x| + |mean|), rstd |s1| / cnt, |dx_add|) plus the propagated bounds of the reductions it consumes.  Every check
prints its worst error as a fraction of its bound ("[bound] ...": pytest -rP shows them).

Sizes: the SDXL UNet at the 128^2 latent (batch 4), its up-path concatenations (2560 channels = two channel slabs), the SD VAE encoder at
1024^2 (4 M elements per group, 1 024 row splits, 4 096 epilogue tiles), the 104 x 152 / 832 x 1216 bucket, the autoencoder's training
batch (32 x 256^2), groups that straddle a channel slab, G = 1 and C = 4096; LayerNorm at the transformer and text-encoder widths and at
widths that leave a lane a partial chunk; BatchNorm at the PatchGAN's M = 30 752 .. 131 072.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RED = 1e-5
F64 = torch.float64
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


@pytest.fixture(autouse=True)
def _free_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _ulp_bf16(ref):
    """one bf16 ulp (8 significant bits) of each element of a float64 tensor"""
    a = ref.abs().clamp_min(2.0 ** -126)
    mant, _ = torch.frexp(a)          # a = mant * 2^e, 0.5 <= mant < 1: a / mant = 2^e exactly
    return a / mant * 2.0 ** -8


def _check(label, got, ref, bound):
    """|got - ref| <= bound elementwise (all float64 or promoted); prints the worst error as a fraction of the bound"""
    got = got.to(F64)
    assert torch.isfinite(got).all(), f"{label}: non-finite output"
    ratio = (got - ref).abs() / bound.clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"[bound] {label}: worst error / bound = {worst:.3g}")
    if not worst <= 1.0:
        i = int(ratio.argmax())
        g, r, b = got.reshape(-1)[i], ref.reshape(-1)[i], bound.reshape(-1)[i]
        raise AssertionError(f"{label}: |got - ref| = {float((g - r).abs()):.4g} > bound {float(b):.4g} at flat index {i} "
                             f"(got {float(g):.8g}, ref {float(r):.8g}; worst error / bound {worst:.3g})")


def _check_bf16(label, got, ref, floor):
    _check(label, got, ref, _ulp_bf16(ref) + floor)


def _exact(label, got, ref):
    got = got.to(F64)
    if not torch.equal(got, ref):
        i = int((got - ref).abs().argmax())
        raise AssertionError(f"{label}: not bit-exact: {int((got != ref).sum())} of {got.numel()} differ, e.g. flat index {i}: "
                             f"got {float(got.reshape(-1)[i])}, ref {float(ref.reshape(-1)[i])}")
    print(f"[exact] {label}: bit-exact ({got.numel()} values)")


def _same(label, a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{label}: {k} differs between two runs on the same inputs"


def _one_pass_bounds(S2, A1, mean, var, cnt, eps):
    """bounds of the mean (absolute) and of rstd (relative) that GroupNorm / BatchNorm form from fp32 sums S1 (its magnitude sum A1)
    and S2 in one pass: mean = S1 / cnt, var = S2 / cnt - mean^2, rstd = rsqrt(var + eps)"""
    err_m = RED * A1 / cnt + 2 * U * mean.abs()
    err_var = (RED + 3 * U) * S2 / cnt + 2 * mean.abs() * err_m + err_m ** 2 + U * (mean ** 2 + var)
    e = err_var / (var + eps)
    return err_m, err_var, 0.5 * e * (1 + e) + 4 * U


# ================================================================================================================================
# GroupNorm
# ================================================================================================================================
def _gn_x(N, HW, C, G, ratio, scale, seed):
    """bf16 [N*HW, C]; each group's mean sits at +-ratio standard deviations (alternating sign by group)"""
    x = torch.randn(N * HW, C, generator=_gen(seed), device="cuda")
    if ratio:
        x += ratio * (((torch.arange(C, device="cuda") // (C // G)) % 2) * 2 - 1).float()
    return (x * scale).to(BF16)


def _gn_truth(x, N, HW, C, G):
    """per (image, group), float64: sum, sum |x|, sum of squares, mean, two-pass variance"""
    S1, A1, S2, var = (torch.empty(N, G, dtype=F64, device="cuda") for _ in range(4))
    for n in range(N):
        xd = x[n * HW:(n + 1) * HW].to(F64).view(HW, G, C // G)
        S1[n], A1[n], S2[n] = xd.sum((0, 2)), xd.abs().sum((0, 2)), (xd * xd).sum((0, 2))
        var[n] = ((xd - (S1[n] / (HW * C // G))[None, :, None]) ** 2).sum((0, 2))
    cnt = HW * C // G
    return S1, A1, S2, S1 / cnt, var / cnt


def _gn_raw(ops, x, N, HW, C, G, eps, silu, w, b, sums=None):
    """nk_groupnorm_fwd (or nk_groupnorm_apply given sums) with the mean / rstd it emits, which ops.groupnorm_fwd keeps to itself"""
    y = torch.empty_like(x)
    mean, rstd = (torch.empty(N, G, dtype=torch.float32, device="cuda") for _ in range(2))
    if sums is None:
        ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, C, G), x.device)
        ops.call("nk_groupnorm_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(),
                 N, HW, C, G, float(eps), int(silu), ops._stream())
    else:
        ops.call("nk_groupnorm_apply", x.data_ptr(), sums.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(),
                 rstd.data_ptr(), N, HW, C, G, float(eps), int(silu), ops._stream())
    return y, mean, rstd


def _per_channel(v, C, G):
    return v.to(F64).repeat_interleave(C // G)


def _gn_apply_ref(xd, m, rs, gamma, beta, silu):
    """float64 y of one image given the kernel's per-channel mean / rstd, and the floor of the fp32 arithmetic (y = x * a + (beta - m * a),
    a = rstd * gamma; SiLU through __expf)"""
    a = rs * gamma
    z = (xd - m) * a + beta
    floor = 4 * U * ((xd * a).abs() + (m * a).abs() + beta.abs())
    if not silu:
        return z, floor, z
    y = z * torch.sigmoid(z)
    return y, 1.1 * floor + 64 * U * y.abs(), z


def _gn_check_stats(label, mean, rstd, truth, cnt, eps):
    S1, A1, S2, m, var = truth
    err_m, _, rel = _one_pass_bounds(S2, A1, m, var, cnt, eps)
    rs = (var + eps).rsqrt()
    _check(f"{label} mean", mean, m, err_m)
    _check(f"{label} rstd", rstd, rs, rel * rs)


def run_groupnorm(ops, N, H, W, C, G, eps, silu, *, ratio=0.0, scale=1.0, dx_add=True, accumulate=False, seed=0, check=True):
    """GroupNorm (+SiLU) forward and backward through ops.groupnorm_fwd, and the stand-alone sums; returns every output"""
    from neurosis_amd.ops import EngineState, Img

    HW, cnt, cpg = H * W, H * W * (C // G), C // G
    x = _gn_x(N, HW, C, G, ratio, scale, seed)
    g = _gen(seed + 1)
    gamma = (torch.rand(C, generator=g, device="cuda") + 0.5) * torch.where(torch.rand(C, generator=g, device="cuda") < 0.2, -1.0, 1.0)
    beta = torch.randn(C, generator=g, device="cuda") * 0.3
    dy = (torch.randn(N * HW, C, generator=g, device="cuda") * scale).to(BF16)
    dxa = torch.randn(N * HW, C, generator=g, device="cuda").to(BF16) if dx_add else None
    w, b = torch.nn.Parameter(gamma.clone()), torch.nn.Parameter(beta.clone())
    g0w = g0b = None
    if accumulate:
        w._nk_state = EngineState()
        w._nk_state.grad_accumulate = True
        g0w, g0b = torch.randn(C, generator=g, device="cuda") * 10, torch.randn(C, generator=g, device="cuda") * 10
        w.grad, b.grad = g0w.clone(), g0b.clone()

    sums = ops.groupnorm_sums(Img(x, N, H, W), G)
    y_raw, mean, rstd = _gn_raw(ops, x, N, HW, C, G, eps, silu, w, b)
    out, bwd = ops.groupnorm_fwd(Img(x, N, H, W), w, b, G, eps, silu)
    assert torch.equal(out.t, y_raw), "ops.groupnorm_fwd and nk_groupnorm_fwd disagree"
    dx = bwd(dy, dxa)
    res = dict(y=out.t, mean=mean, rstd=rstd, sums=sums, dx=dx, dgamma=w.grad.clone(), dbeta=b.grad.clone())
    if not check:
        return res
    label = f"gn N{N} {H}x{W} C{C} G{G} r{ratio:g} s{scale:g}{' silu' if silu else ''}"

    truth = _gn_truth(x, N, HW, C, G)
    S1, A1, S2 = truth[:3]
    _check(f"{label} sums", sums.view(N, G, 2)[..., 0], S1, RED * A1)
    _check(f"{label} sums of squares", sums.view(N, G, 2)[..., 1], S2, RED * S2)
    _gn_check_stats(label, mean, rstd, truth, cnt, eps)
    del truth

    g64, b64 = gamma.to(F64), beta.to(F64)
    da = torch.zeros(C, dtype=F64, device="cuda")
    db, ea, eb = torch.zeros_like(da), torch.zeros_like(da), torch.zeros_like(da)
    worst_y = worst_dx = 0.0
    for n in range(N):
        rows = slice(n * HW, (n + 1) * HW)
        xd = x[rows].to(F64)
        m, rs = _per_channel(mean[n], C, G), _per_channel(rstd[n], C, G)
        yref, floor, z = _gn_apply_ref(xd, m, rs, g64, b64, silu)
        _check_bf16(f"{label} y[{n}]", out.t[rows], yref, floor)
        del yref
        a = rs * g64
        xh = (xd - m) * rs
        d = dy[rows].to(F64)
        if silu:
            err_z = 4 * U * ((xd * a).abs() + (m * a).abs() + b64.abs())
            s = torch.sigmoid(z)
            dsil = s * (1 + z * (1 - s))
            dz_err = d.abs() * (0.5 * err_z + 64 * U * (1 + z.abs()))
            dz = d * dsil
            del s, dsil, err_z
        else:
            dz, dz_err = d, torch.zeros_like(d)
        del z, floor
        ac, bc = dz.sum(0), (dz * xh).sum(0)
        eac = RED * dz.abs().sum(0) + dz_err.sum(0)
        ebc = (RED + 2 * U) * (dz * xh).abs().sum(0) + (dz_err * xh.abs()).sum(0)
        da += ac; db += bc; ea += eac; eb += ebc
        s1 = (g64 * ac).view(G, cpg).sum(1)
        s2 = (g64 * bc).view(G, cpg).sum(1)
        es1 = (g64.abs() * eac).view(G, cpg).sum(1) + RED * (g64 * ac).abs().view(G, cpg).sum(1)
        es2 = (g64.abs() * ebc).view(G, cpg).sum(1) + RED * (g64 * bc).abs().view(G, cpg).sum(1)
        s1, s2, es1, es2 = (_per_channel(t, C, G) for t in (s1, s2, es1, es2))
        add = dxa[rows].to(F64) if dxa is not None else 0.0
        dxref = rs * (dz * g64 - (s1 + xh * s2) / cnt) + add
        terms = (a * dz).abs() + rs * rs * s2.abs() / cnt * (xd.abs() + m.abs()) + rs * s1.abs() / cnt
        if dxa is not None:
            terms = terms + add.abs()
        floor = rs * (es1 + xh.abs() * es2) / cnt + a.abs() * dz_err + 8 * U * terms
        _check_bf16(f"{label} dx[{n}]", dx[rows], dxref, floor)
        del xd, xh, d, dz, dz_err, dxref, terms, floor, add
    if accumulate:
        _check(f"{label} dgamma (accumulated)", w.grad, g0w.to(F64) + db, eb + U * (g0w.to(F64) + db).abs() + U * g0w.abs())
        _check(f"{label} dbeta (accumulated)", b.grad, g0b.to(F64) + da, ea + U * (g0b.to(F64) + da).abs() + U * g0b.abs())
    else:
        _check(f"{label} dgamma", w.grad, db, eb)
        _check(f"{label} dbeta", b.grad, da, ea)
    return res


GN_CASES = [
    # (N, H, W, C, G, eps, silu, dx_add, accumulate)
    (4, 128, 128, 320, 32, 1e-5, True, True, False),      # UNet 128^2 latent
    (4, 64, 64, 640, 32, 1e-5, True, False, True),
    (4, 32, 32, 1280, 32, 1e-5, True, True, False),
    (4, 32, 32, 2560, 32, 1e-5, True, True, True),        # up-path concatenations: 2560 > 2048 channels = two channel slabs
    (4, 64, 64, 1920, 32, 1e-5, True, True, False),
    (4, 128, 128, 960, 32, 1e-5, True, False, False),
    (4, 64, 64, 640, 32, 1e-6, False, True, False),       # transformer norms
    (4, 32, 32, 1280, 32, 1e-6, False, False, True),
    (1, 1024, 1024, 128, 32, 1e-6, True, True, False),    # VAE encoder at 1024^2: 1 024 row splits, 4 M elements per group
    (4, 512, 512, 256, 32, 1e-6, True, True, False),
    (4, 256, 256, 512, 32, 1e-6, True, False, False),
    (4, 104, 152, 320, 32, 1e-5, True, True, False),      # the 104 x 152 bucket (ragged last row split)
    (1, 832, 1216, 128, 32, 1e-6, True, True, False),
    (32, 256, 256, 128, 32, 1e-6, True, True, True),      # autoencoder training batch
    (2, 32, 32, 2304, 3, 1e-5, True, True, False),        # groups of 768 channels straddle the two 1152-channel slabs
    (4, 64, 64, 320, 1, 1e-5, True, True, False),         # one group
    (2, 32, 32, 4096, 32, 1e-5, False, True, False),      # GN_MAXC
]


@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: f"N{c[0]}-{c[1]}x{c[2]}-C{c[3]}-G{c[4]}")
def test_groupnorm_real_sizes(ops, case):
    N, H, W, C, G, eps, silu, dx_add, acc = case
    run_groupnorm(ops, N, H, W, C, G, eps, silu, dx_add=dx_add, accumulate=acc, seed=N + C + G)


@pytest.mark.parametrize("ratio,scale", [(8, 1.0), (32, 1.0), (0, 1e3), (0, 1e-3), (8, 1e3)])
@pytest.mark.parametrize("shape", [(4, 128, 128, 320, 1e-5, True), (1, 1024, 1024, 128, 1e-6, True), (4, 32, 32, 1280, 1e-6, False)],
                         ids=["unet320", "vae1024", "unet1280-nosilu"])
def test_groupnorm_mean_offset_and_scale(ops, shape, ratio, scale):
    """|mean| / sigma of 8 and 32 (the one-pass variance's rstd bound grows as its square), SD-VAE-like magnitudes (1e3) and tiny
    ones (1e-3, where eps dominates rstd)"""
    N, H, W, C, eps, silu = shape
    run_groupnorm(ops, N, H, W, C, 32, eps, silu, ratio=ratio, scale=scale, seed=7)


@pytest.mark.parametrize("N,H,W,C,G", [(1, 1024, 1024, 128, 32), (4, 32, 32, 2560, 32), (2, 32, 32, 2304, 3), (4, 128, 128, 320, 1)])
def test_groupnorm_sums_exact(ops, N, H, W, C, G):
    """ternary x and dy: the per-group sums / sums of squares and the (SiLU-free) dbeta are integers below 2^24, exact in any
    summation order.  The emitted mean is the exact sum times a rounded 1 / cnt: u relative plus half an ulp of the product (<= 1.5 ulp)"""
    from neurosis_amd.ops import Img

    HW, cnt = H * W, H * W * (C // G)
    g = _gen(11)
    x = torch.randint(-1, 2, (N * HW, C), generator=g, device="cuda").to(BF16)
    dy = torch.randint(-1, 2, (N * HW, C), generator=g, device="cuda").to(BF16)
    S1, _, S2, m, _ = _gn_truth(x, N, HW, C, G)
    sums = ops.groupnorm_sums(Img(x, N, H, W), G).view(N, G, 2)
    _exact("gn sums", sums[..., 0], S1)
    _exact("gn sums of squares", sums[..., 1], S2)
    w, b = torch.nn.Parameter(torch.rand(C, device="cuda") + 0.5), torch.nn.Parameter(torch.zeros(C, device="cuda"))
    _, mean, _ = _gn_raw(ops, x, N, HW, C, G, 1e-6, False, w, b)
    m32 = m.float()
    ulp = (torch.nextafter(m32.abs(), torch.tensor(float("inf"), device="cuda")) - m32.abs()).to(F64)
    _check("gn mean (exact sums)", mean, m, 0.5 * ulp + U * m.abs())
    _, bwd = ops.groupnorm_fwd(Img(x, N, H, W), w, b, G, 1e-6, False)
    bwd(dy)
    _exact("gn dbeta", b.grad, dy.to(F64).sum(0))


def test_groupnorm_reproducible_at_vae_1024(ops):
    a = run_groupnorm(ops, 1, 1024, 1024, 128, 32, 1e-6, True, ratio=4, seed=3, check=False)
    b = run_groupnorm(ops, 1, 1024, 1024, 128, 32, 1e-6, True, ratio=4, seed=3, check=False)
    _same("groupnorm 1024^2", a, b)


# ================================================================================================================================
# the convolution's GroupNorm statistics epilogue, and the apply-only GroupNorm behind it
# ================================================================================================================================
def _conv_tiles(ops, N, H, W, Cin, Cout, G):
    d = ops._conv_desc(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, H, W, False)
    return ops.query("nk_conv2d_stats_tiles", ctypes.byref(d), G)


def _conv_weight(ops, w):
    p = ops.conv_weight_param(*w.shape)
    p.data.copy_(w)
    return torch.nn.Parameter(p.data.cuda(), requires_grad=False)


@pytest.mark.parametrize("N,H,W,two_level", [(2, 256, 256, True), (2, 128, 128, False)])
def test_conv_stats_epilogue_exact(ops, N, H, W, two_level):
    """ternary x, seven +-1 weights per output channel, zero bias: every output is an integer with |y| <= 7, so its per-group sums
    (< 2^24 at 256^2 x 4 channels per group) are exact in any order.  256^2 has 256 tiles per image: nk_groupnorm_sums_from_parts
    takes the two-level sum (> 128 partial rows); 128^2 has 128 and takes the one-level sum."""
    from neurosis_amd.ops import Img

    Cin = Cout = 128
    G = 32
    tiles = _conv_tiles(ops, N, H, W, Cin, Cout, G)
    assert (tiles > 128) == two_level, f"{tiles} epilogue tiles per image: the test no longer covers the {'two' if two_level else 'one'}-level sum"
    g = _gen(21)
    x = torch.randint(-1, 2, (N * H * W, Cin), generator=g, device="cuda").to(BF16)
    w = torch.zeros(Cout, Cin * 9, device="cuda")
    taps = torch.rand(Cout, Cin * 9, generator=g, device="cuda").argsort(1)[:, :7]
    signs = torch.randint(0, 2, (Cout, 7), generator=g, device="cuda").float() * 2 - 1
    w.scatter_(1, taps, signs)
    w = w.view(Cout, Cin, 3, 3)
    out = ops.conv2d_fwd(Img(x, N, H, W), _conv_weight(ops, w), torch.zeros(Cout, device="cuda"), need_dx=False, stats_groups=G)[0]
    assert out.sums is not None, "this convolution must take the halo-tile kernel with its statistics epilogue"
    # y[n, o] = sum over the seven taps of sign * x_padded[n, ci, h + kh, w + kw]
    xp = torch.nn.functional.pad(x.to(F64).view(N, H, W, Cin).permute(0, 3, 1, 2), (1, 1, 1, 1))
    yref = torch.zeros(N, Cout, H, W, dtype=F64, device="cuda")
    for o, (tt, ss) in enumerate(zip(taps.tolist(), signs.tolist())):
        for t, s in zip(tt, ss):
            ci, kh, kw = t // 9, (t % 9) // 3, t % 3
            yref[:, o] += s * xp[:, ci, kh:kh + H, kw:kw + W]
    yref = yref.permute(0, 2, 3, 1).reshape(N * H * W, Cout)
    _exact(f"conv {H}x{W} output", out.t, yref)
    yg = yref.view(N, H * W, G, Cout // G)
    sums = out.sums.view(N, G, 2)
    _exact(f"conv epilogue sums ({tiles} tiles)", sums[..., 0], yg.sum((1, 3)))
    _exact(f"conv epilogue sums of squares ({tiles} tiles)", sums[..., 1], (yg * yg).sum((1, 3)))


@pytest.mark.parametrize("N,H,W,ratio,scale", [(1, 1024, 1024, 0, 1.0), (1, 1024, 1024, 8, 1.0), (1, 1024, 1024, 32, 1.0),
                                               (1, 832, 1216, 0, 1.0), (1, 832, 1216, 0, 1e3), (1, 832, 1216, 0, 1e-3), (4, 256, 256, 8, 1.0)])
def test_conv_stats_epilogue_real_sizes(ops, N, H, W, ratio, scale):
    """the VAE encoder's 128 -> 128 convolution at 1024^2 (4 096 tiles per image) and 832 x 1216 (3 952): the epilogue's sums against
    float64 sums of the tensor the convolution wrote, then the apply-only GroupNorm's statistics and output.  The bias puts each group's
    mean at +-ratio output standard deviations."""
    from neurosis_amd.ops import Img

    C, G, eps = 128, 32, 1e-6
    tiles = _conv_tiles(ops, N, H, W, C, C, G)
    assert tiles == ((W + 31) // 32) * (H // 8) and tiles > 128, tiles
    HW, cnt = H * W, H * W * (C // G)
    g = _gen(31)
    x = torch.randn(N * HW, C, generator=g, device="cuda").to(BF16)
    w = torch.randn(C, C, 3, 3, generator=g, device="cuda") * (9 * C) ** -0.5 * scale
    sign = (((torch.arange(C, device="cuda") // (C // G)) % 2) * 2 - 1).float()
    bias = (torch.randn(C, generator=g, device="cuda") * 0.1 + ratio * sign) * scale
    out = ops.conv2d_fwd(Img(x, N, H, W), _conv_weight(ops, w), bias, need_dx=False, stats_groups=G)[0]
    assert out.sums is not None
    label = f"conv epilogue {N}x{H}x{W} r{ratio:g} s{scale:g} ({tiles} tiles)"
    truth = _gn_truth(out.t, N, HW, C, G)
    S1, A1, S2 = truth[:3]
    sums = out.sums.view(N, G, 2)
    _check(f"{label} sums", sums[..., 0], S1, RED * A1)
    _check(f"{label} sums of squares", sums[..., 1], S2, RED * S2)
    gamma, beta = torch.rand(C, generator=g, device="cuda") + 0.5, torch.randn(C, generator=g, device="cuda") * 0.3
    y, mean, rstd = _gn_raw(ops, out.t, N, HW, C, G, eps, True, gamma, beta, sums=out.sums)
    assert torch.equal(ops.groupnorm_fwd(out, gamma, beta, G, eps, True)[0].t, y)
    _gn_check_stats(label, mean, rstd, truth, cnt, eps)
    for n in range(N):
        rows = slice(n * HW, (n + 1) * HW)
        yref, floor, _ = _gn_apply_ref(out.t[rows].to(F64), _per_channel(mean[n], C, G), _per_channel(rstd[n], C, G),
                                       gamma.to(F64), beta.to(F64), True)
        _check_bf16(f"{label} apply-only y[{n}]", y[rows], yref, floor)


# ================================================================================================================================
# LayerNorm (two-pass statistics; one-pass fused backward or the three-kernel form)
# ================================================================================================================================
def run_layernorm(ops, M, C, *, ratio=0.0, dx_add=True, seed=0, check=True):
    g = _gen(seed)
    x = torch.randn(M, C, generator=g, device="cuda")
    if ratio:
        x += ratio * torch.where(torch.rand(M, 1, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    x = x.to(BF16)
    gamma = torch.rand(C, generator=g, device="cuda") + 0.5
    beta = torch.randn(C, generator=g, device="cuda") * 0.3
    dy = torch.randn(M, C, generator=g, device="cuda").to(BF16)
    dxa = torch.randn(M, C, generator=g, device="cuda").to(BF16) if dx_add else None
    w, b = torch.nn.Parameter(gamma.clone()), torch.nn.Parameter(beta.clone())
    eps = 1e-5
    mean, rstd = (torch.empty(M, dtype=torch.float32, device="cuda") for _ in range(2))
    y_raw = torch.empty_like(x)
    ops.call("nk_layernorm_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), y_raw.data_ptr(), mean.data_ptr(), rstd.data_ptr(), M, C, eps,
             ops._stream())
    y, bwd = ops.layernorm_fwd(x, w, b, eps)
    assert torch.equal(y, y_raw), "ops.layernorm_fwd and nk_layernorm_fwd disagree"
    dx = bwd(dy, dxa)
    ops.join_wgrad_stream()
    res = dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=w.grad.clone(), dbeta=b.grad.clone())
    if not check:
        return res
    label = f"ln {M}x{C} r{ratio:g}"

    xd = x.to(F64)
    m = xd.mean(1, keepdim=True)
    var = ((xd - m) ** 2).mean(1, keepdim=True)
    err_m = RED * xd.abs().sum(1, keepdim=True) / C + 2 * U * m.abs()
    err_var = err_m ** 2 + (RED + 4 * U) * (var + err_m ** 2)
    e = err_var / (var + eps)
    rs = (var + eps).rsqrt()
    _check(f"{label} mean", mean, m[:, 0], err_m[:, 0])
    _check(f"{label} rstd", rstd, rs[:, 0], ((0.5 * e * (1 + e) + 4 * U) * rs)[:, 0])
    mk, rk = mean.to(F64)[:, None], rstd.to(F64)[:, None]
    g64, b64 = gamma.to(F64), beta.to(F64)
    xh = (xd - mk) * rk
    _check_bf16(f"{label} y", y, xh * g64 + b64, 4 * U * ((xh * g64).abs() + b64.abs()))
    d = dy.to(F64)
    dg = d * g64
    s1, s2 = dg.mean(1, keepdim=True), (dg * xh).mean(1, keepdim=True)
    es1 = RED * dg.abs().sum(1, keepdim=True) / C
    es2 = (RED + 3 * U) * (dg * xh).abs().sum(1, keepdim=True) / C
    add = dxa.to(F64) if dxa is not None else 0.0
    dxref = add + rk * (dg - s1 - xh * s2)
    floor = rk * (es1 + xh.abs() * es2) + 8 * U * (rk * (dg.abs() + s1.abs() + (xh * s2).abs()) + (add.abs() if dxa is not None else 0.0))
    _check_bf16(f"{label} dx", dx, dxref, floor)
    _check(f"{label} dgamma", w.grad, (d * xh).sum(0), (RED + 3 * U) * (d * xh).abs().sum(0))
    _check(f"{label} dbeta", b.grad, d.sum(0), RED * d.abs().sum(0))
    return res


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("M,C,dx_add", [(16384, 640, True), (4096, 1280, True), (308, 768, False), (308, 1280, False), (4100, 520, True),
                                        (1000, 1032, True), (2048, 2048, True)])
def test_layernorm_real_sizes(ops, M, C, dx_add, fused, monkeypatch):
    """16 384 x 640: eight rows per wave at the 512-block cap; 520 and 1032 = 8 (64 k + 1): one lane holds a partial row of chunks;
    2048 = LN_MAXCH's limit"""
    monkeypatch.setenv("NK_LN_FUSED", fused)
    run_layernorm(ops, M, C, dx_add=dx_add, seed=M + C)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("ratio", [8, 32, 128])
def test_layernorm_mean_offset(ops, ratio, fused, monkeypatch):
    """two-pass statistics: the bounds stay those of a centred input at |mean| / sigma = 128"""
    monkeypatch.setenv("NK_LN_FUSED", fused)
    run_layernorm(ops, 4096, 1280, ratio=ratio, seed=ratio)


def test_layernorm_reproducible(ops, monkeypatch):
    monkeypatch.setenv("NK_LN_FUSED", "1")
    _same("layernorm 16384 x 640", run_layernorm(ops, 16384, 640, seed=5, check=False), run_layernorm(ops, 16384, 640, seed=5, check=False))


# ================================================================================================================================
# BatchNorm (PatchGAN, training mode, fused LeakyReLU)
# ================================================================================================================================
def run_batchnorm(ops, M, C, slope, *, ratio=0.0, scale=1.0, ternary=False, momentum=0.1, seed=0, check=True):
    g = _gen(seed)
    if ternary:
        x = torch.randint(-1, 2, (M, C), generator=g, device="cuda").to(BF16)
        dy = torch.randint(-1, 2, (M, C), generator=g, device="cuda").to(BF16)
    else:
        sign = torch.where(torch.arange(C, device="cuda") % 2 == 0, 1.0, -1.0)
        x = ((torch.randn(M, C, generator=g, device="cuda") + ratio * sign) * scale).to(BF16)
        dy = torch.randn(M, C, generator=g, device="cuda").to(BF16)
    gamma = torch.rand(C, generator=g, device="cuda") + 0.5
    beta = torch.randn(C, generator=g, device="cuda") * 0.3
    rm0 = torch.randn(C, generator=g, device="cuda") * scale
    rv0 = (torch.rand(C, generator=g, device="cuda") + 0.5) * scale * scale
    eps = 1e-5
    w, b = torch.nn.Parameter(gamma.clone()), torch.nn.Parameter(beta.clone())
    mean, rstd = (torch.empty(C, dtype=torch.float32, device="cuda") for _ in range(2))
    y_raw = torch.empty_like(x)
    rm_raw, rv_raw = rm0.clone(), rv0.clone()
    ws = ops._ws(ops.query("nk_batchnorm_ws_floats", M, C), x.device)
    ops.call("nk_batchnorm_fwd", x.data_ptr(), w.data_ptr(), b.data_ptr(), y_raw.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rm_raw.data_ptr(),
             rv_raw.data_ptr(), ws.data_ptr(), M, C, eps, momentum, slope, ops._stream())
    rm, rv = rm0.clone(), rv0.clone()
    y, bwd = ops.batchnorm_fwd(x, w, b, rm, rv, eps, momentum, slope)
    assert torch.equal(y, y_raw) and torch.equal(rm, rm_raw) and torch.equal(rv, rv_raw), "ops.batchnorm_fwd and nk_batchnorm_fwd disagree"
    dx = bwd(dy)
    y_eval = ops.batchnorm_eval(x, w, b, rm, rv, eps, slope)
    res = dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv, dx=dx, dgamma=w.grad.clone(), dbeta=b.grad.clone(), y_eval=y_eval)
    if not check:
        return res
    label = f"bn {M}x{C} slope{slope:g} r{ratio:g} s{scale:g}{' ternary' if ternary else ''}"

    xd = x.to(F64)
    S, A, Q = xd.sum(0), xd.abs().sum(0), (xd * xd).sum(0)
    m = S / M
    var = ((xd - m) ** 2).sum(0) / M
    if ternary:   # integer sums: s / M is one correctly rounded fp32 division, and dbeta (slope 1) an exact integer
        _exact(f"{label} mean", mean, (S.float().cpu() / torch.tensor(float(M))).to(F64).cuda())
    err_m, err_var, rel = _one_pass_bounds(Q, A, m, var, M, eps)
    rs = (var + eps).rsqrt()
    _check(f"{label} mean", mean, m, err_m)
    _check(f"{label} rstd", rstd, rs, rel * rs)
    rm_ref = (1 - momentum) * rm0.to(F64) + momentum * m
    _check(f"{label} running mean", rm, rm_ref, momentum * err_m + 4 * U * ((1 - momentum) * rm0.to(F64).abs() + momentum * m.abs()))
    unb = M / (M - 1)
    rv_ref = (1 - momentum) * rv0.to(F64) + momentum * var * unb
    _check(f"{label} running var", rv, rv_ref, momentum * unb * err_var + 4 * U * ((1 - momentum) * rv0.to(F64) + momentum * var * unb))

    mk, rk = mean.to(F64), rstd.to(F64)
    g64, b64 = gamma.to(F64), beta.to(F64)
    leaky = lambda t: torch.where(t >= 0, t, t * slope)
    xh = (xd - mk) * rk
    _check_bf16(f"{label} y", y, leaky(xh * g64 + b64), 4 * U * ((xh * g64).abs() + b64.abs()))
    rse = (rv.to(F64) + eps).rsqrt()
    xe = (xd - rm.to(F64)) * rse
    _check_bf16(f"{label} eval y", y_eval, leaky(xe * g64 + b64), 8 * U * ((xe * g64).abs() + b64.abs()))
    del xe
    gr = torch.where(y.to(F64) > 0, dy.to(F64), dy.to(F64) * slope)
    s, q = gr.sum(0), (gr * xh).sum(0)
    es = RED * gr.abs().sum(0) + (U * gr.abs().sum(0) if slope != 1.0 else 0.0)
    eq = (RED + 4 * U) * (gr * xh).abs().sum(0)
    if ternary and slope == 1.0:
        _exact(f"{label} dbeta", b.grad, s)
    _check(f"{label} dbeta", b.grad, s, es)
    _check(f"{label} dgamma", w.grad, q, eq)
    a = g64 * rk
    dxref = a * (gr - s / M - xh * q / M)
    floor = a.abs() * (es + xh.abs() * eq) / M + 8 * U * a.abs() * (gr.abs() + s.abs() / M + (xh * q).abs() / M)
    _check_bf16(f"{label} dx", dx, dxref, floor)
    return res


@pytest.mark.parametrize("slope", [0.2, 1.0])
@pytest.mark.parametrize("M,C", [(131072, 128), (32768, 256), (30752, 512)])
def test_batchnorm_real_sizes(ops, M, C, slope):
    """config 5's PatchGAN: 2 048 / 512 / 481 slabs of 64 rows through bn_sum_partials"""
    run_batchnorm(ops, M, C, slope, seed=M + C)


@pytest.mark.parametrize("ratio,scale", [(8, 1.0), (32, 1.0), (0, 1e3), (0, 1e-3)])
def test_batchnorm_mean_offset_and_scale(ops, ratio, scale):
    run_batchnorm(ops, 131072, 128, 0.2, ratio=ratio, scale=scale, seed=9)


@pytest.mark.parametrize("M,C", [(131072, 128), (30752, 512)])
def test_batchnorm_exact(ops, M, C):
    run_batchnorm(ops, M, C, 1.0, ternary=True, seed=13)


def test_batchnorm_reproducible(ops):
    _same("batchnorm 131072 x 128", run_batchnorm(ops, 131072, 128, 0.2, ratio=2, seed=4, check=False),
          run_batchnorm(ops, 131072, 128, 0.2, ratio=2, seed=4, check=False))
