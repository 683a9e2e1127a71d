"""VectorQuantizer / EMAVectorQuantizer on the GPU against the reference's fixture (tests/golden/vq_tiny) and float64, and their wiring
into AutoencodingEngine.  The fixture's rows are decided (tests/test_vq_cpu.py recomputes that), so indices are compared exactly and z_q
bit for bit with the codebook rows; loss, gradients and EMA buffers are held to the bounds of tests/vq_reference.py (operation counts on top
of the statistics kernel's chain bound, safety factor 2), which the CPU test shows the reference's own fp32 values to satisfy as well."""
import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.vq_reference import U, ema_bound, ema_step64, perplexity_tol, rows_of, tiny_vq_engine, vq_bounds, vq_restate64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_fixture("vq_tiny")


def _quantizers():
    from neurosis_amd.modules.autoencoding.regularizers.quantize import EMAVectorQuantizer, VectorQuantizer

    return VectorQuantizer, EMAVectorQuantizer


def _vq(fx, **kw):
    vq = _quantizers()[0](fx["n_e"], fx["dim"], beta=fx["vq"]["beta"], **kw)
    vq.load_state_dict({"embedding.weight": fx["vq"]["codebook"]})
    return vq.cuda()


def _nchw(rows, shape):
    return rows.reshape(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)


def test_vector_quantizer_reproduces_the_reference(fx):
    v = fx["vq"]
    vq = _vq(fx, log_perplexity=True)
    z_q, log, bwd = vq.regularize(v["z"].cuda())
    want = vq_restate64(v["z"], v["codebook"], v["indices"], v["upstream"], v["beta"])
    bounds = vq_bounds(v["z"], v["codebook"], v["indices"], v["upstream"])
    assert torch.equal(log["min_encoding_indices"].cpu(), v["indices"])
    assert torch.equal(z_q.cpu(), _nchw(v["codebook"][v["indices"]], v["z"].shape))           # the codebook's rows, bit for bit
    loss = float(log["loss/vq"])
    print(f"loss {loss!r} float64 {float(want['loss'])!r} reference {float(v['loss'])!r}")
    assert abs(loss - float(want["loss"])) <= bounds["loss"] * float(want["loss"])
    assert abs(loss - float(v["loss"])) <= 2 * bounds["loss"] * float(want["loss"])
    ppl_tol = perplexity_tol(float(v["perplexity"]), fx["n_e"])
    assert abs(float(log["perplexity"]) - float(v["perplexity"])) <= ppl_tol and int(log["cluster_usage"]) == int(v["cluster_usage"])
    vq.embedding.weight.grad = torch.full_like(vq.embedding.weight, float("nan"))       # overwrite mode must write every row
    dz = bwd(v["upstream"].cuda(), 1.0).cpu()
    dE = vq.embedding.weight.grad.cpu()
    assert float((dz.double() - want["dz"]).abs().max()) <= bounds["dz"]
    assert float((dz - v["dz"]).abs().max()) <= 2 * bounds["dz"]
    assert bool(((dE.double() - want["dE"]).abs() <= bounds["dE"]).all())
    assert bool(((dE - v["d_codebook"]).abs() <= 2 * bounds["dE"]).all())
    unused = torch.bincount(v["indices"], minlength=fx["n_e"]) == 0
    assert bool(unused.any()) and not bool(dE[unused].any())


def test_vector_quantizer_forward_and_input_routes(fx):
    v = fx["vq"]
    z_q, log = _vq(fx)(v["z"].cuda())
    assert set(log) == {"loss/vq", "min_encoding_indices"} and log["min_encoding_indices"].shape == (70,)
    z_q2, log2 = _vq(fx, sane_index_shape=True, log_perplexity=True, loss_key="loss/codebook")(v["z"].cuda())
    assert set(log2) == {"loss/codebook", "min_encoding_indices", "perplexity", "cluster_usage"}
    assert log2["min_encoding_indices"].shape == (2, 5, 7) and torch.equal(log2["min_encoding_indices"].reshape(-1), log["min_encoding_indices"])
    assert torch.equal(z_q, z_q2) and torch.equal(log["loss/vq"], log2["loss/codebook"])
    rows = rows_of(v["z"], fx["dim"]).contiguous()
    q2, l2 = _vq(fx)(rows.cuda())                                   # 2-D input: taken as it is
    q3, l3 = _vq(fx, sane_index_shape=True)(rows.reshape(2, 35, 4).cuda())
    assert torch.equal(q2.cpu(), v["codebook"][v["indices"]]) and torch.equal(q3.reshape(70, 4), q2)
    assert torch.equal(l2["min_encoding_indices"].cpu(), v["indices"]) and l3["min_encoding_indices"].shape == (2, 35)
    vq = _vq(fx)
    entry = vq.get_codebook_entry(v["indices"].cuda(), (2, 5, 7, 4))
    assert torch.equal(entry, z_q) and vq.get_codebook_entry(v["indices"].cuda()).shape == (70, 4)


def test_codebook_gradient_accumulates_in_the_engine_mode(fx):
    """overwrite mode zeroes the rows nobody chose; a second bwd in add mode doubles the gradient"""
    from neurosis_amd import ops

    v = fx["vq"]
    vq = _vq(fx)
    _, _, bwd = vq.regularize(v["z"].cuda())
    vq.embedding.weight.grad = torch.full_like(vq.embedding.weight, 7.0)
    bwd(v["upstream"].cuda(), 0.5)
    once = vq.embedding.weight.grad.clone()
    unused = (torch.bincount(v["indices"], minlength=fx["n_e"]) == 0).cuda()
    assert not bool(once[unused].any()) and bool(once[~unused].any())
    st = ops.state_of(vq.embedding.weight)
    st.grad_accumulate = True
    try:
        bwd(v["upstream"].cuda(), 0.5)
    finally:
        st.grad_accumulate = False
    assert torch.equal(vq.embedding.weight.grad, once + once)
    bwd(v["upstream"].cuda(), 0.5)
    assert torch.equal(vq.embedding.weight.grad, once)


def test_torch_ops_match_the_closure(fx):
    import neurosis_amd.torch_ops  # noqa: F401

    v = fx["vq"]
    w = 0.5
    vq = _vq(fx)
    _, log, bwd = vq.regularize(v["z"].cuda())
    dz_closure = rows_of(bwd(v["upstream"].cuda(), w), 4)
    z = rows_of(v["z"], 4).contiguous().cuda().requires_grad_(True)
    E = v["codebook"].cuda().requires_grad_(True)
    g = rows_of(v["upstream"], 4).contiguous().cuda()
    idx = torch.ops.neurosis_hip.vq_search(z, E)
    assert not idx.requires_grad and torch.equal(idx.cpu(), v["indices"])
    z_q, loss = torch.ops.neurosis_hip.vq_quantize(z, E, idx, v["beta"])
    assert torch.equal(z_q.detach().cpu(), v["codebook"][v["indices"]]) and torch.equal(loss.detach(), log["loss/vq"])
    dz, dE = torch.autograd.grad((z_q * g).sum() + w * loss, (z, E))
    bounds = vq_bounds(v["z"], v["codebook"], v["indices"], v["upstream"])
    assert float((dz - dz_closure).abs().max()) <= 2 * bounds["dz"]
    assert bool(((dE - vq.embedding.weight.grad).abs().cpu() <= 2 * w * bounds["dE"]).all())
    m = torch.ops.neurosis_hip.vq_search(torch.empty(9, 4, device="meta"), torch.empty(5, 4, device="meta"))
    assert m.shape == (9,) and m.dtype == torch.int64 and m.device.type == "meta"


def _ema(fx, **kw):
    e = fx["ema"]
    q = _quantizers()[1](fx["n_e"], fx["dim"], beta=e["beta"], decay=e["decay"], eps=e["eps"], **kw)
    q.load_state_dict({"embedding.weight": e["weight0"], "embedding.cluster_size": torch.zeros(fx["n_e"]), "embedding.embed_avg": e["weight0"].clone()})
    return q.cuda()


def test_ema_quantizer_reproduces_the_reference(fx):
    e = fx["ema"]
    q = _ema(fx, return_encodings=True).eval()
    before = {k: t.clone() for k, t in q.state_dict().items()}
    z_q, log = q(e["z"].cuda())
    assert all(torch.equal(t, before[k]) for k, t in q.state_dict().items())                # eval(): bit-unchanged
    assert set(log) == {"loss/vq", "encoding_indices", "perplexity", "encodings"}
    assert torch.equal(log["encoding_indices"].cpu(), e["indices"])
    assert torch.equal(log["encodings"].cpu(), torch.nn.functional.one_hot(e["indices"], fx["n_e"]).float())
    assert torch.equal(z_q.cpu(), _nchw(e["weight0"][e["indices"]], e["z"].shape))
    rows = rows_of(e["z"], 4).double()
    mse = float(((e["weight0"].double()[e["indices"]] - rows) ** 2).mean())
    tol = 2.0 * (rows.numel() + 8) * U
    assert abs(float(log["loss/vq"]) - e["beta"] * mse) <= tol * e["beta"] * mse and abs(float(log["loss/vq"]) - float(e["loss"])) <= 2 * tol * float(e["loss"])
    assert abs(float(log["perplexity"]) - float(e["perplexity"])) <= perplexity_tol(float(e["perplexity"]), fx["n_e"])
    q.train()
    q.embedding.update = False
    q(e["z"].cuda())
    assert all(torch.equal(t, before[k]) for k, t in q.state_dict().items())                # embedding.update = False: bit-unchanged
    assert "encodings" not in _ema(fx)(e["z"].cuda())[1]


def test_ema_buffers_after_three_training_steps(fx):
    e = fx["ema"]
    q = _ema(fx).train()
    w, cs, avg = e["weight0"].double(), torch.zeros(fx["n_e"], dtype=torch.float64), e["weight0"].double()
    for step in e["steps"]:
        _, log = q(step["z"].cuda())
        assert torch.equal(log["encoding_indices"].cpu(), step["indices"])
        rows = rows_of(step["z"], 4)
        w, cs, avg = ema_step64(w, cs, avg, rows, step["indices"], e["decay"], e["eps"])
    bound = ema_bound(rows.shape[0])
    for key, want in (("embedding.weight", w), ("embedding.cluster_size", cs), ("embedding.embed_avg", avg)):
        got = q.state_dict()[key].cpu().double()
        scale = want.abs().amax(1, keepdim=True) if want.ndim == 2 else want.abs().max()       # normwise per code
        print(key, "worst error / bound", float(((got - want).abs() / (bound * scale)).max()))
        assert bool(((got - want).abs() <= bound * scale).all()), key
        assert bool(((got - e["after"][key].double()).abs() <= 2 * bound * scale).all()), key


# ---- engine wiring ----------------------------------------------------------------------------------------------------------------
W_VQ = 0.5


def _engine(loss="l2", **kw):
    torch.manual_seed(0)
    vq = _quantizers()[0](64, 4)
    with torch.no_grad():
        vq.embedding.weight.copy_(0.5 * torch.randn(64, 4))          # codes on the scale of the untrained encoder's output
    eng = tiny_vq_engine(vq, loss=loss, **kw).cuda()
    eng.setup_flat_params()
    seen = {}
    inner = vq.regularize

    def recording(z_e, noise=None):
        z_q, log, bwd = inner(z_e, noise)
        seen.update(z_e=z_e.detach().clone(), idx=log["min_encoding_indices"].clone(), codebook=vq.embedding.weight.detach().clone())
        return z_q, log, bwd

    vq.regularize = recording
    x = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).cuda() * 2 - 1
    return eng, vq, seen, x


def _vq64(seen, beta=0.25):
    rows = rows_of(seen["z_e"].cpu(), 4).double()
    return (1.0 + beta) * float(((seen["codebook"].cpu().double()[seen["idx"].cpu()] - rows) ** 2).mean())


def test_engine_trains_a_vq_autoencoder():
    eng, vq, seen, x = _engine(regularization_weights={"loss/vq": W_VQ})
    weight = vq.embedding.weight
    assert weight._nk_store is eng.store and weight._nk_offset == max(p._nk_offset for p in eng.store.params)       # the codebook goes last
    loss, z, xrec, log = eng.loss_and_backward(x)
    assert z.shape == (2, 4, 16, 16) and xrec.shape == x.shape and log["min_encoding_indices"].shape == (512,)
    assert torch.equal(z.cpu(), _nchw(seen["codebook"].cpu()[seen["idx"].cpu()], z.shape))
    rec64 = float(((xrec.double() - x.double()) ** 2).mean())
    vq64 = _vq64(seen)
    # fp32 sums of non-negative terms over x (rec) and z (vq) in whatever order, a few scalar operations behind them
    tol = 2.0 * (x.numel() + z.numel() + 16) * U
    print(f"loss {float(loss)!r}, rec {rec64!r} + {W_VQ} * vq {vq64!r}")
    assert abs(float(loss) - (rec64 + W_VQ * vq64)) <= tol * (rec64 + W_VQ * vq64)
    assert abs(float(log["loss/vq"]) - vq64) <= tol * vq64
    # the codebook's slot of the flat store holds the regularizer-level gradient
    z_e = seen["z_e"].cpu()
    want = vq_restate64(z_e, seen["codebook"].cpu(), seen["idx"].cpu(), torch.zeros_like(z_e), 0.25, w=W_VQ)
    bounds = vq_bounds(z_e, seen["codebook"].cpu(), seen["idx"].cpu(), torch.zeros_like(z_e))
    slot = eng.store.grad[weight._nk_offset:weight._nk_offset + weight.numel()].view(64, 4)
    assert slot.data_ptr() == weight.grad.data_ptr()
    assert bool(((slot.cpu().double() - want["dE"]).abs() <= W_VQ * bounds["dE"]).all()) and bool(slot.any())
    lo, hi = eng.store.param_range(eng.encoder)
    enc_grad = eng.store.grad[lo:hi]
    assert bool(torch.isfinite(enc_grad).all()) and float(enc_grad.abs().max()) > 0
    # forward-only surfaces work with a quantizer
    zz, xr, reg_log = eng(x)
    assert torch.equal(zz.cpu(), _nchw(seen["codebook"].cpu()[seen["idx"].cpu()], z.shape)) and xr.shape == x.shape and "loss/vq" in reg_log
    assert eng.encode(x).shape == z.shape and eng._reconstruct(x, None)[1].shape == x.shape
    # one step moves both the codebook and the encoder; twenty on one batch lower the loss
    before = eng.store.master.clone()
    first = float(eng.training_step({"image": x}, 0, lr=1e-3))
    moved = eng.store.master != before
    assert bool(moved[weight._nk_offset:weight._nk_offset + weight.numel()].any()) and bool(moved[lo:hi].any())
    for i in range(1, 20):
        last = float(eng.training_step({"image": x}, i, lr=1e-3))
    print(f"loss at step 0 {first:.5f}, at step 19 {last:.5f}")
    assert last < first
    assert "train/loss/vq" in eng.last_log


def test_engine_takes_the_weight_from_a_loss_class():
    """GeneralLPIPSWithDiscriminator(perceptual_weight=0, regularization_weights={"loss/vq": w}) as loss=: one generator step (the
    discriminator has not started: loss = nll + w * vq with nll = sum((xrec - x)^2) / B)"""
    from neurosis_amd.modules.autoencoding.losses import GeneralLPIPSWithDiscriminator

    loss_cfg = GeneralLPIPSWithDiscriminator(disc_start=1000, perceptual_weight=0.0, disc_num_layers=2, regularization_weights={"loss/vq": W_VQ})
    eng, vq, seen, x = _engine(loss=loss_cfg)
    assert eng.regularization_weights == {"loss/vq": W_VQ}
    loss, z, xrec, log = eng.loss_and_backward(x)
    nll64 = float(((xrec.double() - x.double()) ** 2).sum()) / x.shape[0]
    vq64 = _vq64(seen)
    tol = 2.0 * (x.numel() + z.numel() + 16) * U
    assert abs(float(loss) - (nll64 + W_VQ * vq64)) <= tol * (nll64 + W_VQ * vq64)
    weight = vq.embedding.weight
    assert bool(weight.grad.any())
    before = eng.store.master.clone()
    eng.training_step({"image": x}, 0, lr=1e-3)
    moved = eng.store.master != before
    lo, hi = eng.store.param_range(eng.encoder)
    assert bool(moved[weight._nk_offset:weight._nk_offset + weight.numel()].any()) and bool(moved[lo:hi].any())
