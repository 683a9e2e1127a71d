"""The fixed-order partial-row reducer (csrc/nk_reduce.h: nk_reduce_rows) behind the parameter gradients, the GroupNorm sums and the bias
gradients, through every entry point that instantiates it, on inputs whose sums are exact.

Every input is an integer in {-2 .. 2} and the backward entry points get mean = 0, rstd = 1, silu = 0, so x-hat = x and every term dy,
dy * x-hat, (1 + scale) * a is an integer; every sum stays far below 2^24 (the largest here: 3 * 4 * 3 * 1056 < 2^16), so each fp32 partial
and total is exact whatever the order and must EQUAL the float64 sum: a dropped, doubled or misplaced partial row, a wrong row-group
stride or a wrong workspace offset shows as a wrong integer.  dmod is stored as bf16, which holds integers exactly up to 256: its case
keeps dy to 21 non-zero rows per (image, channel), spread over all row splits, so |gamma * b + beta * a| <= 2 * 84 + 2 * 42 = 252.
The sizes are the smallest that cross each edge: one row, one short of / exactly / one over a row group (16, 32, 8 rows) and a block's
rows (64), several blocks, channel counts that fill no block and more than one, one and two channel slabs, one and two reduction levels."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


def _ints(seed, *shape, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=g).to(dtype).cuda()


def _exact(label, got, ref):
    got, ref = got.to(F64), ref.to(F64)
    assert got.shape == ref.shape and torch.equal(got, ref), (
        f"{label}: {int((got != ref).sum())} of {got.numel()} differ; first at {int((got != ref).flatten().nonzero()[0])}: "
        f"got {got.flatten()[(got != ref).flatten()][:4].tolist()}, want {ref.flatten()[(got != ref).flatten()][:4].tolist()}")


@pytest.mark.parametrize("accumulate", [0, 1])
def test_colpart_reduce_batch_sums_exactly(ops, accumulate):
    from neurosis_amd.lib import NkColpartBatch

    cases = [(rows, c) for rows in (1, 31, 32, 33, 67) for c in (8, 24, 40)]
    b = NkColpartBatch()
    b.n = len(cases)
    keep = []
    for z, (rows, c) in enumerate(cases):
        part, dg, db = _ints(100 + z, rows, 2, c), _ints(200 + z, c), _ints(300 + z, c)
        keep.append((part, dg, db, dg.clone(), db.clone()))
        b.part[z], b.dgamma[z], b.dbeta[z], b.nrows[z], b.C[z], b.accumulate[z] = part.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, c, accumulate
    ops.call("nk_colpart_reduce_batch", C.byref(b), ops._stream())
    torch.cuda.synchronize()
    for (rows, c), (part, dg, db, dg0, db0) in zip(cases, keep):
        s = part.to(F64).sum(0)
        _exact(f"colpart batch dgamma rows={rows} C={c}", dg, s[0] + accumulate * dg0.to(F64))
        _exact(f"colpart batch dbeta rows={rows} C={c}", db, s[1] + accumulate * db0.to(F64))


@pytest.mark.parametrize("G", [1, 32])
@pytest.mark.parametrize("nparts", [1, 7, 8, 9, 128, 129, 300])
def test_groupnorm_sums_from_parts_sums_exactly(ops, nparts, G):
    N = 2
    part = _ints(nparts * 64 + G, N, nparts, 2 * G)
    sums = torch.full((N, 2 * G), 7.0, device="cuda")
    ws = ops._ws(ops.query("nk_groupnorm_sums_ws_floats", N, nparts, G), part.device)
    ops.call("nk_groupnorm_sums_from_parts", part.data_ptr(), sums.data_ptr(), ws.data_ptr(), N, nparts, G, ops._stream())
    _exact(f"sums from {nparts} partial rows, G={G}", sums, part.to(F64).sum(1))


@pytest.mark.parametrize("nbatch", [1, 3])
@pytest.mark.parametrize("N", [8, 72, 136])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1093])
def test_colsum_sums_exactly(ops, M, N, nbatch):
    dy = _ints(M * 1000 + N + nbatch, nbatch * M, N, dtype=BF16)
    ref = dy.to(F64).view(nbatch, M, N).sum(1)
    ws = torch.empty(nbatch * ops.query("nk_colsum_ws_floats", M, N), device="cuda")
    for accumulate in (0, 1):
        out = _ints(M + N, nbatch, N)
        want = ref + accumulate * out.to(F64)
        if nbatch == 1:
            ops.call("nk_colsum", dy.data_ptr(), out.data_ptr(), ws.data_ptr(), M, N, N, accumulate, ops._stream())
            _exact(f"colsum {M}x{N} accumulate={accumulate}", out, want)
            out = _ints(M + N, nbatch, N)
        ops.call("nk_colsum_batched", dy.data_ptr(), out.data_ptr(), ws.data_ptr(), M, N, N, nbatch, accumulate, ops._stream())
        _exact(f"colsum_batched {nbatch}x{M}x{N} accumulate={accumulate}", out, want)


@pytest.mark.parametrize("Cc", [8, 72, 136])
@pytest.mark.parametrize("M", [1, 63, 65, 1093])
def test_layernorm_parameter_gradients_sum_exactly(ops, M, Cc):
    dy, x = _ints(M * 7 + Cc, M, Cc, dtype=BF16), _ints(M * 11 + Cc, M, Cc, dtype=BF16)
    gamma = _ints(5, Cc)
    mean, rstd = torch.zeros(M, device="cuda"), torch.ones(M, device="cuda")
    want_g, want_b = (dy.to(F64) * x.to(F64)).sum(0), dy.to(F64).sum(0)
    ws = ops._ws(ops.query("nk_layernorm_ws_floats", M, Cc), dy.device)
    for accumulate in (0, 1):
        dg, db = _ints(1, Cc), _ints(2, Cc)
        dg0, db0 = dg.to(F64), db.to(F64)
        ops.call("nk_layernorm_bwd_params", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(),
                 M, Cc, accumulate, ops._stream())
        _exact(f"layernorm_bwd_params dgamma {M}x{Cc}", dg, want_g + accumulate * dg0)
        _exact(f"layernorm_bwd_params dbeta {M}x{Cc}", db, want_b + accumulate * db0)
        dg, db, dx = _ints(1, Cc), _ints(2, Cc), torch.empty_like(x)
        ops.call("nk_layernorm_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(), dg.data_ptr(),
                 db.data_ptr(), ws.data_ptr(), M, Cc, accumulate, ops._stream())
        _exact(f"layernorm_bwd dgamma {M}x{Cc}", dg, want_g + accumulate * dg0)
        _exact(f"layernorm_bwd dbeta {M}x{Cc}", db, want_b + accumulate * db0)


GN_SHAPES = [(1, 32, 8, 1), (2, 1056, 72, 3), (3, 64, 2304, 3)]      # (N, HW, C, G): one block; 33 row splits; two channel slabs


def _gn_bwd(ops, shape, dy, x, gamma, beta, mod, accumulate):
    N, HW, Cc, G = shape
    mean, rstd = torch.zeros(N, G, device="cuda"), torch.ones(N, G, device="cuda")
    dg, db, dx = _ints(1, Cc), _ints(2, Cc), torch.empty_like(x)
    dg0, db0 = dg.to(F64), db.to(F64)
    ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, Cc, G), x.device)
    if mod is None:
        ops.call("nk_groupnorm_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None, dx.data_ptr(),
                 dg.data_ptr(), db.data_ptr(), ws.data_ptr(), N, HW, Cc, G, 0, accumulate, ops._stream())
        return dg, db, None, dg0, db0
    dmod = torch.empty_like(mod)
    ops.call("nk_groupnorm_mod_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), mod.data_ptr(), mean.data_ptr(), rstd.data_ptr(), None,
             dx.data_ptr(), dg.data_ptr(), db.data_ptr(), dmod.data_ptr(), ws.data_ptr(), N, HW, Cc, G, 0, accumulate, ops._stream())
    return dg, db, dmod, dg0, db0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm_parameter_and_modulation_gradients_sum_exactly(ops, shape, accumulate):
    N, HW, Cc, G = shape
    x, dense = _ints(sum(shape), N * HW, Cc, dtype=BF16), _ints(sum(shape) + 1, N * HW, Cc, dtype=BF16)
    gamma, beta, mod = _ints(3, Cc), _ints(4, Cc), _ints(6, N, 2 * Cc, dtype=BF16)
    # 21 non-zero rows per (image, channel), a different set per channel, spread over the image's rows
    K = min(21, HW)
    rows = (torch.arange(Cc)[None, :] * 7 + (torch.arange(K) * max(HW // K, 1))[:, None]) % HW
    keep = torch.zeros(HW, Cc).scatter_(0, rows, 1.0).cuda().to(BF16)
    sparse = (dense.view(N, HW, Cc) * keep).view(N * HW, Cc)
    for label, dy in (("dense", dense), ("sparse", sparse)):
        d, xd = dy.to(F64).view(N, HW, Cc), x.to(F64).view(N, HW, Cc)
        a, b = d.sum(1), (d * xd).sum(1)                                   # per image: sum dz, sum dz * xhat
        dg, db, _, dg0, db0 = _gn_bwd(ops, shape, dy, x, gamma, beta, None, accumulate)
        _exact(f"groupnorm_bwd dgamma {shape} {label}", dg, b.sum(0) + accumulate * dg0)
        _exact(f"groupnorm_bwd dbeta {shape} {label}", db, a.sum(0) + accumulate * db0)
        s1 = 1 + mod[:, :Cc].to(F64)
        dg, db, dmod, dg0, db0 = _gn_bwd(ops, shape, dy, x, gamma, beta, mod, accumulate)
        _exact(f"groupnorm_mod_bwd dgamma {shape} {label}", dg, (s1 * b).sum(0) + accumulate * dg0)
        _exact(f"groupnorm_mod_bwd dbeta {shape} {label}", db, (s1 * a).sum(0) + accumulate * db0)
        if label == "sparse":
            want = torch.cat([gamma.to(F64) * b + beta.to(F64) * a, a], 1)
            assert float(want.abs().max()) <= 256, "dmod must stay within bf16's exact integers"
            _exact(f"groupnorm_mod_bwd dmod {shape}", dmod, want)


@pytest.mark.parametrize("shape", GN_SHAPES)
def test_zero_modulation_equals_the_plain_entry_points_bit_for_bit(ops, shape):
    N, HW, Cc, G = shape
    g = torch.Generator(device="cpu").manual_seed(sum(shape))
    rnd = lambda *s: torch.randn(*s, generator=g)
    x, dy, add = (rnd(N * HW, Cc).cuda().to(BF16) for _ in range(3))
    gamma, beta = (rnd(Cc) * 0.5 + 1).cuda(), (rnd(Cc) * 0.1).cuda()
    mod = torch.zeros(N, 2 * Cc, dtype=BF16, device="cuda")
    ws = ops._ws(ops.query("nk_groupnorm_ws_floats", N, HW, Cc, G), x.device)
    outs = []
    for m in (None, mod):
        y, dx = torch.empty_like(x), torch.empty_like(x)
        mean, rstd = torch.empty(N, G, device="cuda"), torch.empty(N, G, device="cuda")
        dg, db = torch.full((Cc,), 0.5, device="cuda"), torch.full((Cc,), -0.25, device="cuda")
        mp = () if m is None else (m.data_ptr(),)
        ops.call("nk_groupnorm_fwd" if m is None else "nk_groupnorm_mod_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *mp, y.data_ptr(),
                 mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), N, HW, Cc, G, 1e-5, 1, ops._stream())
        extra = () if m is None else (torch.empty_like(mod),)
        ops.call("nk_groupnorm_bwd" if m is None else "nk_groupnorm_mod_bwd", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), *mp,
                 mean.data_ptr(), rstd.data_ptr(), add.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), *(e.data_ptr() for e in extra),
                 ws.data_ptr(), N, HW, Cc, G, 1, 1, ops._stream())
        torch.cuda.synchronize()
        outs.append({"y": y, "mean": mean, "rstd": rstd, "dx": dx, "dgamma": dg, "dbeta": db})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), f"{shape}: {k} of the modulated entry point with mod = 0 differs from the plain one"
