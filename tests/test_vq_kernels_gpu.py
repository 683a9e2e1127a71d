"""The three kernels of csrc/vq.hip against float64: nk_vq_search (ops.vq_search), nk_vq_code_stats, nk_vq_quantize.

Search.  With d64_j = sum e_j^2 - 2 z . e_j in float64 and bound_j of tests/vq_reference.py, EVERY row must return an acceptable index, a
decided row float64's argmin itself; at most 1 % of a case's rows may be undecided (a condition on the inputs: a plain fp32 evaluation
stays inside it on N(0,1), trained-like and badly scaled data).  On small-integer data every score is exact in fp32 and the result must
be float64's argmin with the lowest-index tie rule on all rows.  Shapes: the smallest at which a seam can break -- D around the MFMA's
k = 4 and at the 256 limit, N around the 32-row workgroup and the 16-row MFMA group, n_e around the 16-code tile and the 4-wave split."""
import pytest
import torch

from tests.vq_reference import U, acceptable, scores64

pytestmark = pytest.mark.gpu


def _data(kind: str, N: int, D: int, n_e: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(n_e, D, generator=g)
    if kind == "normal":
        z = torch.randn(N, D, generator=g)
    elif kind == "trained":       # codes plus 0.3 sigma noise
        z = E[torch.randint(0, n_e, (N,), generator=g)] + 0.3 * torch.randn(N, D, generator=g)
    else:                         # badly scaled: |z| ~ 100, |e| ~ 0.01
        z, E = 100.0 * torch.randn(N, D, generator=g), 0.01 * E
    return z, E


CASES = [
    ("normal", 1, 3, 1), ("trained", 4096, 3, 1000), ("normal", 63, 4, 17), ("normal", 257, 4, 16384), ("scaled", 64, 8, 512),
    ("normal", 65, 8, 1025), ("trained", 257, 32, 1025), ("normal", 4096, 32, 512), ("normal", 65, 256, 1000), ("scaled", 257, 256, 17),
    ("trained", 63, 256, 1025), ("normal", 64, 32, 1000), ("scaled", 1, 256, 512),
]


def _check_search(idx: torch.Tensor, z: torch.Tensor, E: torch.Tensor):
    ok, jmin, decided = acceptable(z, E)
    idx = idx.cpu()
    assert idx.dtype == torch.int64 and idx.shape == (z.shape[0],)
    assert bool(((idx >= 0) & (idx < E.shape[0])).all())
    undecided = float((~decided).float().mean())
    print(f"undecided share {undecided:.4%}, disagreeing with float64 on {int((idx != jmin).sum())} rows")
    assert undecided <= 0.01
    assert bool(ok.gather(1, idx[:, None]).all()), "a row returned an index outside its acceptable set"
    assert torch.equal(idx[decided], jmin[decided])


@pytest.mark.parametrize("kind,N,D,n_e", CASES)
def test_search_returns_an_acceptable_index_on_every_row(kind, N, D, n_e):
    from neurosis_amd import ops

    z, E = _data(kind, N, D, n_e, seed=N * 31 + D * 7 + n_e)
    _check_search(ops.vq_search(z.cuda(), E.cuda()), z, E)


def test_the_cases_cover_the_direct_search_and_the_one_cut_across_workgroups():
    """with few rows the code tiles are cut across workgroups and merged in a second launch; the workspace size tells how many cuts"""
    from neurosis_amd.lib import query

    cuts = {(N, n_e): (query("nk_vq_search_ws_floats", N, n_e) - n_e) // (2 * N) for _, N, _, n_e in CASES}
    assert cuts[(63, 17)] == 0 and cuts[(1, 1)] == 0                 # one cut: no partial results
    assert cuts[(4096, 1000)] == 3 and cuts[(257, 16384)] == 64 and cuts[(65, 1025)] == 4
    assert query("nk_vq_search_ws_floats", 32768, 8192) == 8192       # enough rows: the direct path


@pytest.mark.parametrize("N,D,n_e,off,width", [(257, 3, 512, 2, 8), (65, 32, 1000, 5, 41)])
def test_search_takes_a_strided_column_slice(N, D, n_e, off, width):
    from neurosis_amd import ops

    z, E = _data("normal", N, D, n_e, seed=5)
    wide = torch.full((N, width), float("nan"))
    wide[:, off:off + D] = z
    view = wide.cuda()[:, off:off + D]
    assert not view.is_contiguous()
    _check_search(ops.vq_search(view, E.cuda()), z, E)


def _lowest_argmin64(z, E):
    d64, _ = scores64(z, E)
    ties = d64 == d64.min(1, keepdim=True).values
    first = torch.where(ties, torch.arange(E.shape[0])[None], E.shape[0]).min(1).values
    return first, ties


@pytest.mark.parametrize("N,D,n_e,dups", [(257, 3, 1000, ()), (4096, 8, 17, (0, 16)), (65, 32, 1025, (0, 117, 600, 1024)),
                                          (64, 256, 512, (0, 100, 511)), (63, 4, 1025, (3, 1009, 1024))])
def test_search_is_exact_on_integers_with_the_lowest_index_tie_rule(N, D, n_e, dups):
    """small integers: every score is exact in fp32, so the result is float64's argmin on all rows, the lowest index among the many ties.
    `dups`: one codebook row copied to indices in different 16-code tiles (different waves' shares), the last partial tile, 0 and n_e - 1;
    the first rows of z equal it, so exactly its copies tie for the minimum."""
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(n_e + D)
    E = torch.randint(-2, 3, (n_e, D), generator=g).float()
    z = torch.randint(-3, 4, (N, D), generator=g).float()
    z[N // 2] = 0.0                       # scores = the norms: ties between all codes of the smallest norm
    if dups:
        E[list(dups)] = E[dups[0]].clone()
        z[:8] = E[dups[0]]               # d_j = |e_j - z|^2 - |z|^2: exactly the copies reach the minimum
    want, ties = _lowest_argmin64(z, E)
    assert int((ties.sum(1) > 1).sum()) >= min(N, 8), "the case must hold genuine ties"
    if dups:
        assert bool(ties[:8][:, list(dups)].all()) and bool((want[:8] <= min(dups)).all())
    got = ops.vq_search(z.cuda(), E.cuda()).cpu()
    assert torch.equal(got, want)


def test_a_rows_result_does_not_depend_on_N():
    """a row searched alone, as the last row of shorter matrices, and inside the full matrix gives one index; the codebook holds near-ties
    (pairs of codes one ulp-scale step apart)"""
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(11)
    D, n_e, N = 32, 1000, 200
    E = torch.randn(n_e, D, generator=g)
    E[1::2] = E[0::2] * (1.0 + 2.0 ** -22)
    z = E[torch.randint(0, n_e, (N,), generator=g)] + 0.05 * torch.randn(N, D, generator=g)
    zc, Ec = z.cuda(), E.cuda()
    full = ops.vq_search(zc, Ec)
    for r in (0, 15, 16, 31, 32, 63, 64, 100, 199):
        alone = ops.vq_search(zc[r:r + 1], Ec)
        last = ops.vq_search(zc[:r + 1], Ec)
        assert int(alone[0]) == int(last[-1]) == int(full[r]), r
        assert torch.equal(last, full[:r + 1])


def test_nan_scores_are_never_chosen_and_an_all_nan_row_gives_zero():
    from neurosis_amd import ops

    z, E = _data("normal", 70, 8, 100, seed=3)
    E[0, 3] = float("nan")                # index 0: what a careless "all NaN" fallback would return
    E[37, 0] = float("nan")
    z[5] = float("nan")                   # every score of row 5 is NaN
    got = ops.vq_search(z.cuda(), E.cuda()).cpu()
    assert int(got[5]) == 0
    rest = torch.ones(70, dtype=torch.bool)
    rest[5] = False
    assert not bool(((got[rest] == 0) | (got[rest] == 37)).any())
    keep = torch.ones(100, dtype=torch.bool)
    keep[[0, 37]] = False
    ok, jmin, decided = acceptable(z[rest], E[keep])
    back = torch.arange(100)[keep]
    assert bool(decided.all()) and torch.equal(got[rest], back[jmin])


def test_rows_whose_scores_are_all_infinite_take_the_first_of_them():
    """fp32 overflow: z . e = -inf for every code gives d = +inf everywhere; argmin's first index, skipping a NaN code"""
    from neurosis_amd import ops

    E = -torch.ones(40, 4)
    z = torch.full((3, 4), 3.0e38)
    z[1] = 1.0                            # an ordinary row between them
    assert int(ops.vq_search(z.cuda(), E.cuda())[0]) == 0
    E[0, 0] = float("nan")
    got = ops.vq_search(z.cuda(), E.cuda()).cpu()
    assert got.tolist() == [1, 1, 1]


def test_limits_are_refused_with_their_message():
    from neurosis_amd import ops
    from neurosis_amd.lib import NkError

    with pytest.raises(NkError, match="1 <= D <= 256"):
        ops.vq_search(torch.zeros(4, 257).cuda(), torch.zeros(8, 257).cuda())
    with pytest.raises(NkError, match="1 <= n_e <= 65536"):
        ops.vq_search(torch.zeros(4, 1).cuda(), torch.zeros(65537, 1).cuda())
    with pytest.raises(NkError, match="1 <= D <= 256"):
        ops.vq_code_stats(torch.zeros(4, dtype=torch.int64).cuda(), torch.zeros(4, 257).cuda(), 8)
    with pytest.raises(NkError, match="1 <= n_e <= 65536"):
        ops.vq_quantize(torch.zeros(4, dtype=torch.int64).cuda(), torch.zeros(65537, 2).cuda(), torch.zeros(4, 2).cuda())


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def _stats_case(name: str):
    g = torch.Generator().manual_seed(len(name))
    if name == "random":
        N, D, n_e = 1000, 5, 37
        idx = torch.randint(0, n_e, (N,), generator=g)
    elif name == "one_code":          # all rows map to one code: the longest chain
        N, D, n_e = 300, 256, 40
        idx = torch.full((N,), 7)
    elif name == "own_code":          # every row maps to its own code
        N, D, n_e = 64, 65, 64
        idx = torch.randperm(n_e, generator=g)
    elif name == "more_codes_than_rows":
        N, D, n_e = 10, 3, 1000
        idx = torch.randint(0, n_e, (N,), generator=g)
    else:                             # strided z, rows past one 64-row chunk, codes past one 32-code workgroup
        N, D, n_e = 513, 33, 100
        idx = torch.randint(0, n_e, (N,), generator=g) // 2 * 2          # odd codes stay unused
    return idx, torch.randn(N, D, generator=g), n_e


@pytest.mark.parametrize("name", ["random", "one_code", "own_code", "more_codes_than_rows", "strided"])
def test_code_stats_counts_exactly_and_sums_in_a_fixed_order(name):
    from neurosis_amd import ops

    idx, z, n_e = _stats_case(name)
    zc = z.cuda()
    if name == "strided":
        wide = torch.full((z.shape[0], z.shape[1] + 7), float("nan")).cuda()
        wide[:, 4:4 + z.shape[1]] = zc
        zc = wide[:, 4:4 + z.shape[1]]
    count, total = ops.vq_code_stats(idx.cuda(), zc, n_e)
    count2, total2 = ops.vq_code_stats(idx.cuda(), zc, n_e)
    assert torch.equal(count, count2) and torch.equal(total, total2)                      # two runs are bit-identical
    want_count = torch.bincount(idx, minlength=n_e)
    assert count.dtype == torch.int64 and torch.equal(count.cpu(), want_count)
    want = torch.zeros(n_e, z.shape[1], dtype=torch.float64).index_add_(0, idx, z.double())
    sum_abs = torch.zeros(n_e, z.shape[1], dtype=torch.float64).index_add_(0, idx, z.double().abs())
    # sum[j] is one chain of c_j = count_j additions in row order (csrc/vq.hip): |error| <= c_j U sum|z_i|, safety factor 2
    bound = 2.0 * want_count.double()[:, None] * U * sum_abs
    err = (total.cpu().double() - want).abs()
    print(f"{name}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    unused = want_count == 0
    if name in ("one_code", "more_codes_than_rows", "strided"):
        assert bool(unused.any())
    assert not bool(total.cpu()[unused].any()) and not bool(torch.signbit(total.cpu()[unused]).any())     # exact (positive) zeros


def test_code_stats_own_code_rows_are_copies():
    from neurosis_amd import ops

    idx, z, n_e = _stats_case("own_code")
    count, total = ops.vq_code_stats(idx.cuda(), z.cuda(), n_e)
    assert bool((count == 1).all()) and torch.equal(total.cpu()[idx], z)


# ---- quantize -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,n_e,hw", [(70, 4, 37, 1), (70, 4, 37, 35), (1000, 37, 50, 250), (70000, 3, 1000, 1), (257, 256, 17, 257)])
def test_quantize_gathers_bit_exactly_and_sums_the_squared_error(N, D, n_e, hw):
    from neurosis_amd import ops

    g = torch.Generator().manual_seed(N + D)
    E, z = torch.randn(n_e, D, generator=g), torch.randn(N, D, generator=g)
    idx = torch.randint(0, n_e, (N,), generator=g)
    out = torch.full((N // hw, D, hw) if hw > 1 else (N, D), float("nan")).cuda()          # every element must be written
    z_q, sumsq = ops.vq_quantize(idx.cuda(), E.cuda(), z.cuda(), hw, out=out)
    assert z_q.data_ptr() == out.data_ptr()
    rows = E[idx]
    want = rows.view(N // hw, hw, D).permute(0, 2, 1) if hw > 1 else rows
    assert torch.equal(z_q.cpu(), want.contiguous())
    s64 = float(((rows.double() - z.double()) ** 2).sum())
    # longest addition chain D + ceil(ceil(N / 256) / 256) + 16 (csrc/vq.hip), every term non-negative and itself two roundings (the
    # difference, squared) from exact: relative error <= (chain + 3) U, safety factor 2
    blocks = -(-N // 256)
    chain = D + -(-blocks // 256) + 16
    err = abs(float(sumsq) - s64) / s64
    print(f"sumsq relative error {err:.3e}, bound {2 * (chain + 3) * U:.3e}")
    assert sumsq.shape == () and err <= 2 * (chain + 3) * U
    fresh, s2 = ops.vq_quantize(idx.cuda(), E.cuda(), z.cuda(), hw)
    assert torch.equal(fresh, z_q) and torch.equal(s2, sumsq)


def test_quantize_writes_nan_for_an_index_outside_the_codebook():
    from neurosis_amd import ops

    E, z = torch.randn(5, 4).cuda(), torch.randn(3, 4).cuda()
    z_q, _ = ops.vq_quantize(torch.tensor([0, 5, -1]).cuda(), E, z)
    assert torch.equal(z_q[0], E[0]) and bool(z_q[1:].isnan().all())
