"""GumbelQuantizer on the GPU against the reference's fixture (tests/golden/gumbel_tiny: z [2, 8, 3, 5], 24 codes of width 8) and the
float64 restatement of tests/gumbel_reference.py, at the fixture's widths and at h = 32, d = 16, n = 1000 on z [2, 32, 5, 7]; and its wiring
into AutoencodingEngine.  Indices are compared exactly on decided rows; gradients (bf16 GEMM operands, fp32 accumulation) by the floors of
tests/util.check_grad_cosines, 0.999 for matrices and 0.99 for vectors, the project's standing figure for bf16 gradient paths.

Bounds used below, with U = 2^-24:
  hard z_q     the gather returns E[idx] exactly; the reference's (1 - y + y) E differs from it by one rounding at the chosen code: 2 U |E|_max.
  soft z_q     y @ E on bf16 y and E with fp32 accumulation over n terms (any order: (n + 8) U sum |y E|, safety 2) and a bf16 store (2^-8);
               against the fp32 reference the operands' own roundings come on top: 2^-8 each on y and E, so 3 * 2^-8 sum_j |y_j E_jk|.
  loss         kl_weight * (kl bound 2 (n + 8) U max(|kl|, 1) + the logits' chain bound carried through dKL/dl to first order,
               max_j logit_bound * sum_j |q_j (h_j - sum q h)|, maximised over rows).
  hard dE      row j is the sum of the count_j rows of dz that chose j, added in row order: (count_j + 2) U sum |dz| (columnwise)."""
import pytest
import torch

from tests import gumbel_reference as R
from tests.golden.fixture_io import load_fixture
from tests.util import check_grad_cosines

pytestmark = pytest.mark.gpu
U = R.U
CASES = ["hard1_train1", "hard0_train1", "hard1_train0", "hard0_train0"]


@pytest.fixture(scope="module")
def fx():
    return load_fixture("gumbel_tiny")


def _cls():
    from neurosis_amd.modules.autoencoding.regularizers import GumbelQuantizer

    return GumbelQuantizer


def _quantizer(fx, c, **kw):
    q = _cls()(fx["num_hiddens"], fx["embedding_dim"], fx["n_embed"], straight_through=c["hard"], kl_weight=fx["kl_weight"], temp_init=fx["temp"], **kw)
    q.load_state_dict({"proj.weight": fx["proj_w"], "proj.bias": fx["proj_b"], "embed.weight": fx["embed"]})
    return q.train(c["train"]).cuda()


def _loss_tol(rows, W, b, kl_weight):
    l64 = R.logits64(rows, W, b)
    q = torch.softmax(l64, dim=1)
    h = R.h_of(q)
    sens = (q * (h - (q * h).sum(1, keepdim=True))).abs().sum(1).max()
    return kl_weight * (R.kl_tol(float(R.kl64(l64)), W.shape[0]) + float(R.logit_bound(rows, W, b).max() * sens))


def _check_forward(q, z, W, b, E, noise, tau, hard, kl_weight, z_q, log, want, label):
    from neurosis_amd import ops

    n, h, d = W.shape[0], W.shape[1], E.shape[1]
    rows, g = R.rows_of(z, h), R.rows_of(noise, n)
    _, jmax, decided = R.acceptable(rows, W, b, g)
    idx = log["indices"].reshape(-1).cpu()
    assert log["indices"].shape == (z.shape[0], z.shape[2], z.shape[3]) and torch.equal(idx[decided], jmax[decided]) and bool(decided.all())
    zq_rows = R.rows_of(z_q.cpu(), d)
    if hard:
        assert torch.equal(zq_rows, E[idx])                                                  # the codebook's rows, bit for bit
        assert float((zq_rows.double() - R.rows_of(want["z_q"], d)).abs().max()) <= 2 * U * float(E.abs().max())
    else:
        logits = ops.gumbel_logits(rows.contiguous().cuda(), W.cuda(), b.cuda())
        y = ops.gumbel_softmax_fwd(logits, tau, noise=g.contiguous().cuda())[0].cpu().double()
        Eb = E.to(torch.bfloat16).double()
        z64, mag = y @ Eb, y @ Eb.abs()
        err = (zq_rows.double() - z64).abs()
        assert bool((err <= 2.0 ** -8 * z64.abs() + 2 * (n + 8) * U * mag + 2.0 ** -126).all()), label
        assert bool(((zq_rows.double() - R.rows_of(want["z_q"], d)).abs() <= 3 * 2.0 ** -8 * (want["y"] @ E.double().abs()) + 2 * (n + 8) * U * mag).all()), label
    loss = float(log["loss/vq"])
    tol = _loss_tol(rows, W, b, kl_weight)
    print(f"{label}: loss {loss!r} float64 {float(want['loss'])!r} allowed {tol:.3e}")
    assert abs(loss - float(want["loss"])) <= tol
    return idx


@pytest.mark.parametrize("case", CASES)
def test_reproduces_the_reference(fx, case):
    c = fx["cases"][case]
    n, h, d = fx["n_embed"], fx["num_hiddens"], fx["embedding_dim"]
    W, b, E = fx["proj_w"].view(n, h), fx["proj_b"], fx["embed"]
    hard = c["hard"] if c["train"] else True
    q = _quantizer(fx, c)
    z_q, log, bwd = q.regularize(fx["z"].cuda(), c["noise"].cuda())
    want = R.restate64(fx["z"], W, b, E, R.rows_of(c["noise"], n), fx["temp"], hard, fx["kl_weight"], fx["upstream"])
    idx = _check_forward(q, fx["z"], W, b, E, c["noise"], fx["temp"], hard, fx["kl_weight"], z_q, log, want, case)
    assert torch.equal(idx, c["indices"].reshape(-1)) and set(log) == {"loss/vq", "indices"}
    assert abs(float(log["loss/vq"]) - float(c["loss"])) <= 2 * _loss_tol(R.rows_of(fx["z"], h), W, b, fx["kl_weight"])
    if hard:
        assert float((z_q.cpu() - c["z_q"]).abs().max()) <= 2 * U * float(E.abs().max())
    # gradients: NaN-filled slots show that overwrite mode writes every element
    for p in q.parameters():
        p.grad = torch.full_like(p, float("nan"))
    dz = bwd(fx["upstream"].cuda(), 1.0).cpu()
    got = {"dz": dz, "dW": q.proj.weight.grad.cpu().view(n, h), "db": q.proj.bias.grad.cpu(), "dE": q.embed.weight.grad.cpu()}
    assert dz.shape == fx["z"].shape and all(bool(torch.isfinite(t).all()) for t in got.values())
    check_grad_cosines(f"gumbel {case} vs float64", got, {k: want[k].float() for k in got})
    check_grad_cosines(f"gumbel {case} vs reference", got, {"dz": c["dz"], "dW": c["d_proj_w"].view(n, h), "db": c["d_proj_b"], "dE": c["d_embed"]})
    if hard:
        up = R.rows_of(fx["upstream"], d).double()
        count = torch.bincount(idx, minlength=n).double()
        bound = (count[:, None] + 2) * U * up.abs().sum(0)[None, :]
        assert bool(((got["dE"].double() - want["dE"]).abs() <= bound).all())
        assert not bool(got["dE"][count == 0].any())
    # forward(): the same through the public surface, logits on request
    z_q2, log2 = q(fx["z"].cuda(), return_logits=True)
    assert z_q2.shape == z_q.shape and log2["logits"].shape == (2, n, 3, 5) and log2["indices"].shape == (2, 3, 5)
    lb = R.logit_bound(R.rows_of(fx["z"], h), W, b)
    assert bool(((R.rows_of(log2["logits"].cpu(), n).double() - want["logits"]).abs() <= lb).all())


@pytest.fixture(scope="module")
def wide():
    """h = 32, d = 16, n = 1000 on z [2, 32, 5, 7]"""
    gen = torch.Generator().manual_seed(31)
    n, h, d = 1000, 32, 16
    t = dict(n=n, h=h, d=d, W=0.4 * torch.randn(n, h, generator=gen), b=0.2 * torch.randn(n, generator=gen), E=torch.randn(n, d, generator=gen),
             z=torch.randn(2, h, 5, 7, generator=gen), upstream=torch.randn(2, d, 5, 7, generator=gen))
    u = torch.rand(2, n, 5, 7, generator=gen).clamp_(2.0 ** -24, 1 - 2.0 ** -24)
    t["noise"] = -torch.log(-torch.log(u))
    return t


@pytest.mark.parametrize("hard", [True, False])
def test_wider_shapes_against_float64(wide, hard):
    t = wide
    n, h, d = t["n"], t["h"], t["d"]
    q = _cls()(h, d, n, straight_through=hard, kl_weight=0.05, temp_init=0.7)
    q.load_state_dict({"proj.weight": t["W"].view(n, h, 1, 1), "proj.bias": t["b"], "embed.weight": t["E"]})
    q = q.cuda().train()
    z_q, log, bwd = q.regularize(t["z"].cuda(), t["noise"].cuda())
    want = R.restate64(t["z"], t["W"], t["b"], t["E"], R.rows_of(t["noise"], n), 0.7, hard, 0.05, t["upstream"], w=0.5)
    _check_forward(q, t["z"], t["W"], t["b"], t["E"], t["noise"], 0.7, hard, 0.05, z_q, log, want, f"wide hard={hard}")
    dz = bwd(t["upstream"].cuda(), 0.5).cpu()
    got = {"dz": dz, "dW": q.proj.weight.grad.cpu().view(n, h), "db": q.proj.bias.grad.cpu(), "dE": q.embed.weight.grad.cpu()}
    check_grad_cosines(f"gumbel wide hard={hard} vs float64", got, {k: want[k].float() for k in got})


def test_gradients_accumulate_in_the_engine_mode(fx):
    """the first micro-batch overwrites, the second adds (as test_codebook_gradient_accumulates_in_the_engine_mode)"""
    from neurosis_amd import ops

    for case in ("hard1_train1", "hard0_train1"):
        c = fx["cases"][case]
        q = _quantizer(fx, c)
        _, _, bwd = q.regularize(fx["z"].cuda(), c["noise"].cuda())
        params = list(q.parameters())
        for p in params:
            p.grad = torch.full_like(p, 7.0)
        bwd(fx["upstream"].cuda(), 0.5)
        once = [p.grad.clone() for p in params]
        assert all(bool(g.any()) and not bool((g == 7.0).any()) for g in once)
        st = ops.state_of(q.embed.weight)
        st.grad_accumulate = True
        try:
            bwd(fx["upstream"].cuda(), 0.5)
        finally:
            st.grad_accumulate = False
        for p, g in zip(params, once):
            assert torch.equal(p.grad, g + g)
        bwd(fx["upstream"].cuda(), 0.5)
        for p, g in zip(params, once):
            assert torch.equal(p.grad, g)


@pytest.mark.parametrize("case", ["hard1_train1", "hard0_train1"])
def test_torch_op_matches_the_closure(fx, case):
    import neurosis_amd.torch_ops  # noqa: F401

    c = fx["cases"][case]
    n, h, d = fx["n_embed"], fx["num_hiddens"], fx["embedding_dim"]
    w = 0.5
    q = _quantizer(fx, c)
    z_q, log, bwd = q.regularize(fx["z"].cuda(), c["noise"].cuda())
    dz_closure = R.rows_of(bwd(fx["upstream"].cuda(), w), h)
    z = R.rows_of(fx["z"], h).contiguous().cuda().requires_grad_(True)
    W = fx["proj_w"].view(n, h).cuda().requires_grad_(True)
    b = fx["proj_b"].cuda().requires_grad_(True)
    E = fx["embed"].cuda().requires_grad_(True)
    g = R.rows_of(c["noise"], n).contiguous().cuda()
    up = R.rows_of(fx["upstream"], d).contiguous().cuda()
    zq, loss, idx = torch.ops.neurosis_hip.gumbel_quantize(z, W, b, E, g, fx["temp"], c["hard"], fx["kl_weight"])
    assert not idx.requires_grad and torch.equal(idx, log["indices"].reshape(-1))
    assert torch.equal(zq.detach(), R.rows_of(z_q, d)) and torch.equal(loss.detach(), log["loss/vq"])
    dz, dW, db, dE = torch.autograd.grad((zq * up).sum() + w * loss, (z, W, b, E))
    # the same kernels on the same operands: the same bits
    assert torch.equal(dz, dz_closure) and torch.equal(dW, q.proj.weight.grad.view(n, h)) and torch.equal(db, q.proj.bias.grad) and torch.equal(dE, q.embed.weight.grad)


def test_noise_route_draws_and_repeats(fx):
    from neurosis_amd import ops

    c = fx["cases"]["hard0_train1"]
    q = _quantizer(fx, c)
    z = fx["z"].cuda()
    ops.dropout_seed(4242)
    with ops.dropout_token_scope(None):                  # no draw open: the quantizer draws its own, one per call
        a, la, _ = q.regularize(z)
        b, lb, _ = q.regularize(z)
        assert ops.dropout_token(required=False) is None
        assert not torch.equal(a, b)
        ops.dropout_seed(4242)
        a2, la2, _ = q.regularize(z)
        b2, lb2, _ = q.regularize(z)
        assert torch.equal(a, a2) and torch.equal(b, b2) and torch.equal(la["indices"], la2["indices"]) and torch.equal(lb["indices"], lb2["indices"])
        assert torch.equal(la["loss/vq"], lb["loss/vq"])                     # the KL term does not see the noise
        tok = ops.dropout_draw()                                                 # an open draw is used as it is: the same noise twice
        c1, _, _ = q.regularize(z)
        c2, _, _ = q.regularize(z)
        assert torch.equal(c1, c2) and ops.dropout_token() is tok
        # and it is the generator's noise: the injected route with ops.gumbel_noise gives the same bits
        g = ops.gumbel_noise(30, fx["n_embed"], ops.dropout_site(q), tok)
        c3, _, _ = q.regularize(z, g)
        assert torch.equal(c1, c3)
    q.eval()                                                                     # eval quantizes hard, with noise, as the reference
    with ops.dropout_token_scope(None):
        e1, le1 = q(z)
        assert torch.equal(R.rows_of(e1.cpu(), 8), fx["embed"][le1["indices"].reshape(-1).cpu()])


# ---- engine wiring ----------------------------------------------------------------------------------------------------------------
def _engine():
    from neurosis_amd.models.autoencoder import AutoencodingEngine
    from neurosis_amd.modules.diffusion.model import Decoder, Encoder

    torch.manual_seed(0)
    cfg = dict(ch=32, out_ch=3, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[], dropout=0.0, in_channels=3, resolution=32, double_z=False,
               attn_type="vanilla", standalone=True)
    q = _cls()(32, 16, 64, straight_through=False, kl_weight=0.05, temp_init=1.0)
    eng = AutoencodingEngine(encoder=Encoder(**cfg, z_channels=32, embed_dim=32), decoder=Decoder(**cfg, z_channels=16, embed_dim=16), regularizer=q,
                             regularization_weights={"loss/vq": 1.0}).cuda()
    eng.setup_flat_params()
    seen = {}
    inner = q.regularize

    def recording(z_e, noise=None, *more):
        z_q, log, bwd = inner(z_e, noise, *more)

        def bwd_rec(dz, weight_=0.0):
            seen["dz"], seen["w"] = dz.detach().clone(), weight_
            return bwd(dz, weight_)

        seen.update(z_e=z_e.detach().clone(), W=q.proj.weight.detach().clone().view(64, 32), b=q.proj.bias.detach().clone(), E=q.embed.weight.detach().clone())
        return z_q, log, bwd_rec

    q.regularize = recording
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).cuda() * 2 - 1
    return eng, q, seen, x


def test_engine_trains_a_gumbel_autoencoder():
    eng, q, seen, x = _engine()
    params = [q.proj.weight, q.proj.bias, q.embed.weight]
    assert all(p._nk_store is eng.store for p in params)
    gen = torch.Generator().manual_seed(9)
    u = torch.rand(2, 64, 16, 16, generator=gen).clamp_(2.0 ** -24, 1 - 2.0 ** -24)
    noise = (-torch.log(-torch.log(u))).cuda()
    before = eng.store.master.clone()
    loss = eng.training_step({"image": x}, 0, lr=1e-3, noise=noise)
    assert bool(torch.isfinite(loss)) and seen["w"] == 1.0 and seen["dz"].shape == (2, 16, 16, 16) and seen["z_e"].shape == (2, 32, 16, 16)
    # the first step's regularizer gradients against float64 on what the regularizer saw
    want = R.restate64(seen["z_e"].cpu(), seen["W"].cpu(), seen["b"].cpu(), seen["E"].cpu(), R.rows_of(noise.cpu(), 64), 1.0, False, 0.05, seen["dz"].cpu(), w=1.0)
    got = {"dW": q.proj.weight.grad.cpu().view(64, 32), "db": q.proj.bias.grad.cpu(), "dE": q.embed.weight.grad.cpu()}
    check_grad_cosines("gumbel engine step 0 vs float64", got, {k: want[k].float() for k in got})
    for p in params:
        assert p.grad.data_ptr() == eng.store.grad[p._nk_offset:p._nk_offset + p.numel()].data_ptr()
    for i in (1, 2):                                      # the generator's noise from here on
        loss = eng.training_step({"image": x}, i, lr=1e-3)
        assert bool(torch.isfinite(loss))
    moved = eng.store.master != before
    for p in params:
        assert bool(moved[p._nk_offset:p._nk_offset + p.numel()].all()), tuple(p.shape)
    assert "train/loss/vq" in eng.last_log and eng.last_log["train/indices"].shape == (2, 16, 16)
    zz, xr, reg_log = eng(x)
    assert zz.shape == (2, 16, 16, 16) and xr.shape == x.shape and "loss/vq" in reg_log
