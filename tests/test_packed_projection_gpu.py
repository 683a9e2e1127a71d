"""transformer.Packed, the text towers' packed projection: its forward, input gradient, weight and bias gradients bit for bit against the
single ops it is made of on hand-made operands, and the life of its bf16 copy.  M = 154 rows (B = 2, L = 77: a multiple of no tile), K = 128."""
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
M, K = 154, 128
CASES = {"clip-3x128-biased": ((128, 128, 128), True), "t5-192+64-bias-free": ((192, 64), False)}


def _projections(rows, bias, seed):
    g = torch.Generator().manual_seed(seed)
    layers = [nn.Linear(K, n, bias=bias) for n in rows]
    with torch.no_grad():
        for lin in layers:
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * K ** -0.5)
            if bias:
                lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return [lin.cuda() for lin in layers]


@pytest.mark.parametrize("case", list(CASES))
def test_forward_and_gradients_equal_the_single_ops(case):
    from neurosis_amd import ops
    from neurosis_amd.models.text_encoder.transformer import Packed

    rows, bias = CASES[case]
    layers = _projections(rows, bias, 1)
    N = sum(rows)
    g = torch.Generator().manual_seed(2)
    h = torch.randn(M, K, generator=g).cuda().to(BF16)
    dy = torch.randn(M, N, generator=g).cuda().to(BF16)
    weight = torch.cat([ops.cast_bf16(lin.weight.detach()) for lin in layers])
    fp32_bias = torch.cat([lin.bias.detach() for lin in layers]) if bias else None

    packed = Packed(*layers)
    y, bwd = packed.train(h)
    assert torch.equal(y, ops.gemm_nt(h, weight, fp32_bias))
    assert torch.equal(packed.forward(h), y)
    dh = bwd(dy)
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    assert torch.equal(dh, ops.gemm_nn(dy, weight))
    first, off = [], 0
    for lin, n in zip(layers, rows):
        dw = torch.full((n, K), float("nan"), device="cuda")
        db = torch.full((n,), float("nan"), device="cuda") if bias else None
        ops.gemm_tn_f32(dy[:, off:off + n], h, dw, 0, dbias=db)      # the projection's own launch, on its own column slice
        assert torch.equal(lin.weight.grad, dw), f"{case}: weight gradient of rows {off}:{off + n}"
        assert not bias or torch.equal(lin.bias.grad, db), f"{case}: bias gradient of rows {off}:{off + n}"
        first.append((lin.weight.grad.clone(), lin.bias.grad.clone() if bias else None))
        off += n

    # a second backward in accumulate mode doubles every gradient exactly
    ops.state.grad_accumulate = True
    try:
        packed.train(h)[1](dy)
        ops.join_wgrad_stream()
        torch.cuda.synchronize()
    finally:
        ops.state.grad_accumulate = False
    for lin, (dw, db) in zip(layers, first):
        assert torch.equal(lin.weight.grad, 2 * dw)
        assert db is None or torch.equal(lin.bias.grad, 2 * db)


def test_bias_gradients_equal_colsum_of_their_slices():
    """Each bias.grad against ops.colsum of its column slice, bit for bit.

    The bias gradient comes out of the weight-gradient launch (gemm_tn_f32's dbias=, nk_linear_wgrad_bias), which adds a column up in the
    order of its MFMA row tiles; nk_colsum adds it up in its fixed-order reducer's.  On normal random values the two fp32 sums of the same 154
    bf16 numbers differ by one unit in the last place in about 1 entry of 128 (measured on an MI355X: 4.768e-07 at |sum| 36.7, 9.537e-07 at
    26.8; tests/test_kernels_gpu.py holds the two kernels to each other within a tolerance for that reason), which says nothing about the
    packed projection.  So dy here holds multiples of 1 / 8 in [-4, 4], as the bit-for-bit GEMM tests use integers: every partial sum of 154
    of them is a multiple of 1 / 8 below 2^10 and exact in fp32 in ANY order, and torch.equal then holds exactly when each bias received
    the sum of its own columns and of nothing else.  (On random values the bias gradients are pinned bit for bit by the test above, to the
    dbias of each projection's own launch.)"""
    from neurosis_amd import ops
    from neurosis_amd.models.text_encoder.transformer import Packed

    rows, _ = CASES["clip-3x128-biased"]
    layers = _projections(rows, True, 1)
    g = torch.Generator().manual_seed(2)
    h = torch.randn(M, K, generator=g).cuda().to(BF16)
    dy = ((torch.randn(M, sum(rows), generator=g) * 16).round().clamp(-32, 32) / 8).cuda().to(BF16)
    assert len(dy.float().sum(0).unique()) > sum(rows) // 2, "the column sums must tell the columns apart"
    Packed(*layers).train(h)[1](dy)
    ops.join_wgrad_stream()
    torch.cuda.synchronize()
    off = 0
    for lin, n in zip(layers, rows):
        db = torch.full((n,), float("nan"), device="cuda")
        ops.colsum(dy[:, off:off + n], db, False)
        print(f"[packed] bias gradient of rows {off}:{off + n}: {int((lin.bias.grad != db).sum())} of {n} entries differ from colsum, "
              f"max |difference| {float((lin.bias.grad - db).abs().max()):.3e} at max |sum| {float(db.abs().max()):.3e}")
        assert torch.equal(db, dy[:, off:off + n].float().sum(0)), "colsum itself must be exact on these values"
        assert torch.equal(lin.bias.grad, db), f"bias gradient of rows {off}:{off + n}"
        off += n


@pytest.mark.parametrize("case", list(CASES))
def test_the_copy_is_kept_until_a_parameter_changes(case):
    from neurosis_amd.models.text_encoder.transformer import Packed

    rows, bias = CASES[case]
    layers = _projections(rows, bias, 3)
    packed = Packed(*layers)
    weight, fp32_bias = packed.matrices()
    assert weight.dtype == BF16 and weight.shape == (sum(rows), K) and (fp32_bias is None) == (not bias)
    again = packed.matrices()
    assert again[0].data_ptr() == weight.data_ptr() and (not bias or again[1].data_ptr() == fp32_bias.data_ptr())
    before = weight.clone()
    with torch.no_grad():
        layers[1].weight.mul_(2.0)
    after = packed.matrices()[0]
    lo, hi = rows[0], rows[0] + rows[1]
    assert torch.equal(after[lo:hi].float(), 2 * before[lo:hi].float()) and bool((after[lo:hi] != before[lo:hi]).any())
    assert torch.equal(after[:lo], before[:lo]) and torch.equal(after[hi:], before[hi:])
