"""The four kernels of csrc/gumbel.hip against the float64 yardstick of tests/gumbel_reference.py (which derives every bound used here).

Shapes (N, h, n): the seams of the 32-row workgroup (63, 65, 257), the 16-row MFMA group (33), the 16-code tile (17, 1000, 1025), k = 4 (3, 4),
the 256 limit of the latent width, and the three row-width paths of the row passes (n <= 1024, n <= 8192, wider).  Data: N(0, 1), and a badly
scaled set (|z| ~ 100, |w| ~ 0.01).  Each case's inputs and float64 results are computed once and shared by the tests."""
import functools

import pytest
import torch

from tests import gumbel_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 1), (63, 4, 17), (65, 8, 1025), (257, 32, 1000), (33, 256, 512), (64, 16, 8192), (2, 8, 65536)]
DATA = ["normal", "scaled"]
TAU, W_KL = 0.9, 0.37
BF16 = torch.bfloat16


@functools.lru_cache(maxsize=None)
def case(shape, data):
    """inputs (CPU fp32), what the kernels returned for them (one run, shared), and the float64 restatement"""
    from neurosis_amd import ops

    N, h, n = shape
    gen = torch.Generator().manual_seed(1000 * N + 10 * h + n + (7 if data == "scaled" else 0))
    zs, ws = (100.0, 0.01) if data == "scaled" else (1.0, 1.0)
    wide = zs * torch.randn(N, h + 5, generator=gen)
    z = wide[:, 2:2 + h]                                    # a strided column slice
    W = ws * torch.randn(n, h, generator=gen)
    b = 0.3 * torch.randn(n, generator=gen)
    u = torch.rand(N, n, generator=gen).clamp_(2.0 ** -24, 1.0 - 2.0 ** -24)
    g = -torch.log(-torch.log(u))                           # fp32 Gumbel values, injected
    G = torch.randn(N, n, generator=gen).to(BF16)
    c = dict(N=N, h=h, n=n, z=z, W=W, b=b, g=g, G=G)
    dz = wide.cuda()[:, 2:2 + h]
    assert dz.stride() == (h + 5, 1)
    c["logits"] = ops.gumbel_logits(dz, W.cuda(), b.cuda())
    c["logits_dense"] = ops.gumbel_logits(dz.contiguous(), W.cuda(), b.cuda())
    y, idx, kl = ops.gumbel_softmax_fwd(c["logits"], TAU, noise=g.cuda())
    d = ops.gumbel_softmax_bwd(c["logits"], y, G.cuda().clone(), TAU, W_KL)
    torch.cuda.synchronize()
    c.update(y=y.cpu(), idx=idx.cpu(), kl=float(kl), d=d.cpu(), l32=c["logits"].cpu())
    return c


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", SHAPES)
def test_logits_within_the_chain_bound(shape, data):
    c = case(shape, data)
    l64 = R.logits64(c["z"], c["W"], c["b"])
    bound = R.logit_bound(c["z"], c["W"], c["b"])
    ratio = float(((c["l32"].double() - l64).abs() / bound).max())
    print(f"logits {shape} {data}: worst error / bound = {ratio:.3f}")
    assert c["l32"].shape == (c["N"], c["n"]) and ratio <= 1.0
    assert torch.equal(c["logits"], c["logits_dense"])                 # the strided slice is read as it is


@pytest.mark.parametrize("shape", SHAPES)
def test_logits_exact_on_small_integers(shape):
    from neurosis_amd import ops

    N, h, n = shape
    gen = torch.Generator().manual_seed(N + h + n)
    z = torch.randint(-4, 5, (N, h), generator=gen).float()
    W = torch.randint(-3, 4, (n, h), generator=gen).float()
    b = torch.randint(-9, 10, (n,), generator=gen).float()
    got = ops.gumbel_logits(z.cuda(), W.cuda(), b.cuda()).cpu()
    assert torch.equal(got.double(), R.logits64(z, W, b))              # every partial sum is an integer below 2^24: no rounding anywhere


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_against_the_restatement(shape):
    from neurosis_amd import ops

    N, _, n = shape
    site = 3
    ops.dropout_seed(0x0BAD_5EED_1234_5678 + n)
    with ops.dropout_token_scope(None):
        tok = ops.dropout_draw()
        g = ops.gumbel_noise(N, n, site, tok)
        again = ops.gumbel_noise(N, n, site, tok)
        other = ops.gumbel_noise(N, n, site, ops.dropout_draw())
    seed, step = tok.tolist()
    g64 = R.noise64(N, n, seed, step, site)
    ratio = float(((g.cpu().double() - g64).abs() / R.noise_tol(g64)).max())
    print(f"noise {shape}: worst error / tolerance = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(g, again) and not torch.equal(g, other)
    if N * n >= 64:
        assert not torch.equal(g, ops.gumbel_noise(N, n, site + 1, tok))


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_indices_softmax_and_kl(shape, data):
    c = case(shape, data)
    N, n = c["N"], c["n"]
    ok, jmax, decided = R.acceptable(c["z"], c["W"], c["b"], c["g"])
    undecided = int((~decided).sum())
    print(f"forward {shape} {data}: {undecided} undecided rows of {N}")
    assert undecided <= 0.01 * N                                       # a condition on the inputs
    assert bool(ok[torch.arange(N), c["idx"]].all())
    assert torch.equal(c["idx"][decided], jmax[decided])
    # y and kl against float64 of the kernel's own inputs (its fp32 logits and the injected noise)
    a64 = (c["l32"].double() + c["g"].double()) * R.inv_tau32(TAU)
    y64 = torch.softmax(a64, dim=1)
    ratio = float(((c["y"].double() - y64).abs() / R.softmax_tol(a64, y64)).max())
    kl64 = float(R.kl64(c["l32"].double()))
    print(f"   y worst error / tolerance = {ratio:.3f}; kl {c['kl']!r} float64 {kl64!r} allowed {R.kl_tol(kl64, n):.3e}")
    assert c["y"].dtype == BF16 and ratio <= 1.0
    assert abs(c["kl"] - kl64) <= R.kl_tol(kl64, n)


@pytest.mark.parametrize("n", [1, 24, 1000, 1025, 8192, 8200])
def test_equal_scores_take_index_zero(n):
    from neurosis_amd import ops

    logits = torch.full((3, n), 0.25, device="cuda")
    y, idx, kl = ops.gumbel_softmax_fwd(logits, 1.0, noise=torch.full((3, n), 0.5, device="cuda"))
    assert idx.tolist() == [0, 0, 0]
    assert float((y.float() - 1.0 / n).abs().max()) <= 2.0 ** -8 / n and abs(float(kl)) <= R.kl_tol(0.0, n)
    logits[1, n - 1] = float("nan")                                    # a NaN is never taken
    logits[2, n // 2] = 1.0
    _, idx, _ = ops.gumbel_softmax_fwd(logits, 1.0, noise=torch.full((3, n), 0.5, device="cuda"))
    assert idx.tolist() == [0, 0, n // 2]


@pytest.mark.parametrize("shape", SHAPES)
def test_token_route_equals_the_noise_route_bitwise(shape):
    from neurosis_amd import ops

    c = case(shape, "normal")
    N, n = c["N"], c["n"]
    ops.dropout_seed(77 + n)
    with ops.dropout_token_scope(None):
        tok = ops.dropout_draw()
    y1, i1, k1 = ops.gumbel_softmax_fwd(c["logits"], TAU, token=tok, site=2)
    y2, i2, k2 = ops.gumbel_softmax_fwd(c["logits"], TAU, noise=ops.gumbel_noise(N, n, 2, tok))
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)) and torch.equal(i1, i2) and torch.equal(k1.view(torch.int32), k2.view(torch.int32))
    y3, i3, k3 = ops.gumbel_softmax_fwd(c["logits"], TAU, token=tok, site=2)
    assert torch.equal(y1.view(torch.int16), y3.view(torch.int16)) and torch.equal(i1, i3) and torch.equal(k1, k3)     # and run to run
    with pytest.raises(ValueError, match="exactly one of"):
        ops.gumbel_softmax_fwd(c["logits"], TAU)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_against_float64_on_the_same_bf16_operands(shape, data):
    c = case(shape, data)
    d64 = R.softmax_bwd64(c["l32"], c["y"], c["G"], TAU, W_KL)
    tol = R.softmax_bwd_tol(c["l32"], c["y"], c["G"], TAU, W_KL, d64)
    ratio = float(((c["d"].double() - d64).abs() / tol).max())
    print(f"backward {shape} {data}: worst error / tolerance = {ratio:.3f}")
    assert c["d"].dtype == BF16 and ratio <= 1.0
