"""GumbelQuantizer without a GPU: the class and its refusals, the op surface, and the float64 yardstick of tests/gumbel_reference.py proved
against the reference's own fp32 results (tests/golden/gumbel_tiny, made by tests/golden/make_golden_gumbel.py).

Tolerance of the yardstick against the fixture: the reference computes in fp32 with torch's CPU kernels, in no particular order.  Its z_q,
loss and gradients are sums of at most OPS = n_embed + num_hiddens + rows = 24 + 8 + 30 products behind a softmax (an exp and a quotient:
a handful of roundings, amplified by the scores' size, below 16 here), so every compared tensor is held to 2 * (OPS + 64) * U * its own
largest magnitude -- about 1.9e-5 relative, normwise."""
import numpy as np
import pytest
import torch

from tests import dropout_ref
from tests import gumbel_reference as R
from tests.golden.fixture_io import load_fixture

OPS_COUNT = 24 + 8 + 30
TOL = 2.0 * (OPS_COUNT + 64) * R.U


@pytest.fixture(scope="module")
def fx():
    return load_fixture("gumbel_tiny")


def _cls():
    from neurosis_amd.modules.autoencoding.regularizers import GumbelQuantizer

    return GumbelQuantizer


def test_class_constructs_with_the_reference_keys_and_defaults(fx):
    q = _cls()(fx["num_hiddens"], fx["embedding_dim"], fx["n_embed"])
    assert {k: list(v.shape) for k, v in q.state_dict().items()} == fx["state_dict_shapes"]
    assert list(q.state_dict()) == list(fx["state_dict_shapes"])
    assert (q.straight_through, q.kl_weight, q.temperature, q.loss_key, q.unknown_index, q.re_embed) == (True, 5e-4, 1.0, "loss/vq", "random", fx["n_embed"])
    assert isinstance(q.proj, torch.nn.Conv2d) and isinstance(q.embed, torch.nn.Embedding)
    assert [tuple(p.shape) for p in q.get_trainable_parameters()] == [(24, 8, 1, 1), (24,), (24, 8)]
    q.load_state_dict({"proj.weight": fx["proj_w"], "proj.bias": fx["proj_b"], "embed.weight": fx["embed"]})
    entry = q.get_codebook_entry(torch.arange(30) % 24, (2, 3, 5, 8))
    assert entry.shape == (2, 8, 3, 5) and torch.equal(entry[1, :, 2, 4], fx["embed"][29 % 24])


def test_refusals_are_by_name(tmp_path):
    G = _cls()
    with pytest.raises(NotImplementedError, match="GumbelQuantizer: remap="):
        G(8, 8, 24, remap=str(tmp_path / "used.npy"))
    with pytest.raises(NotImplementedError, match='GumbelQuantizer: unknown_index="extra"'):
        G(8, 8, 24, unknown_index="extra")
    with pytest.raises(ValueError, match="GumbelQuantizer: unknown_index"):
        G(8, 8, 24, unknown_index="nearest")
    for kw, name in ((dict(num_hiddens=12, embedding_dim=8, n_embed=24), "num_hiddens = 12"), (dict(num_hiddens=8, embedding_dim=4, n_embed=24), "embedding_dim = 4"),
                     (dict(num_hiddens=8, embedding_dim=8, n_embed=100), "n_embed = 100"), (dict(num_hiddens=264, embedding_dim=8, n_embed=24), "num_hiddens = 264"),
                     (dict(num_hiddens=8, embedding_dim=8, n_embed=65544), "n_embed = 65544")):
        with pytest.raises(NotImplementedError, match=f"GumbelQuantizer: {name}"):
            G(**kw)
    q = G(8, 8, 24)
    with pytest.raises(NotImplementedError, match="CPU tensor"):
        q(torch.zeros(1, 8, 2, 2))


def test_ops_are_registered():
    from neurosis_amd import torch_ops

    for name in ("gumbel_logits", "gumbel_noise", "gumbel_softmax_fwd", "gumbel_softmax_bwd", "gumbel_quantize"):
        assert name in torch_ops.OPS and hasattr(torch.ops.neurosis_hip, name)
    y, idx, kl = torch.ops.neurosis_hip.gumbel_softmax_fwd(torch.empty(9, 40, device="meta"), 1.0, torch.empty(9, 40, device="meta"))
    assert y.shape == (9, 40) and y.dtype == torch.bfloat16 and idx.shape == (9,) and idx.dtype == torch.int64 and kl.shape == ()
    z_q, loss, idx = torch.ops.neurosis_hip.gumbel_quantize(torch.empty(9, 8, device="meta"), torch.empty(40, 8, device="meta"), torch.empty(40, device="meta"),
                                                            torch.empty(40, 16, device="meta"), torch.empty(9, 40, device="meta"), 1.0, True, 5e-4)
    assert z_q.shape == (9, 16) and loss.shape == () and idx.dtype == torch.int64


def _close(got, want, what):
    err = float((got.double() - want.double()).abs().max())
    scale = float(want.double().abs().max())
    print(f"{what}: worst error {err:.3e}, allowed {TOL * scale:.3e}")
    assert err <= TOL * scale, what


@pytest.mark.parametrize("case", ["hard1_train1", "hard0_train1", "hard1_train0", "hard0_train0"])
def test_float64_restatement_reproduces_the_fixture(fx, case):
    c = fx["cases"][case]
    n, h = fx["n_embed"], fx["num_hiddens"]
    W = fx["proj_w"].view(n, h)
    g = R.rows_of(c["noise"], n)
    hard = c["hard"] if c["train"] else True
    _, jmax, decided = R.acceptable(R.rows_of(fx["z"], h), W, fx["proj_b"], g)
    assert bool(decided.all())
    want = R.restate64(fx["z"], W, fx["proj_b"], fx["embed"], g, fx["temp"], hard, fx["kl_weight"], fx["upstream"])
    assert torch.equal(want["indices"], c["indices"].reshape(-1)) and torch.equal(jmax, c["indices"].reshape(-1))
    _close(c["logits"], want["logits"].view(2, 3, 5, n).permute(0, 3, 1, 2), "logits")
    _close(c["z_q"], want["z_q"], "z_q")
    _close(c["loss"], want["loss"], "loss")
    _close(c["dz"], want["dz"], "dz")
    _close(c["d_proj_w"].view(n, h), want["dW"], "d proj.weight")
    _close(c["d_proj_b"], want["db"], "d proj.bias")
    _close(c["d_embed"], want["dE"], "d embed.weight")


def test_restated_noise_is_a_gumbel_draw_from_the_open_interval():
    seed, step, site = 0x1234_5678_9ABC_DEF0, 3, 5
    words = R.noise_words(1 << 16, seed, step, site)
    for v in (0, 1, 777, (1 << 14) - 1):                 # the vectorised rounds against the plain-Python generator, keyed as the kernel keys it
        ctr, key = dropout_ref.counter_key(v, seed ^ (R.KEY_XOR << 32), step, site)
        assert tuple(int(w) for w in words[4 * v:4 * v + 4]) == dropout_ref.philox4x32_10(ctr, key)
    assert not np.array_equal(words[:64], dropout_ref.philox_words(16, seed, step, site).reshape(-1))        # not the dropout stream
    u = R.uniform_of(words)
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)                # exactly fp32 values
    # the extreme words: never 0 or 1
    ends = R.uniform_of(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert ends[0] == 2.0 ** -24 and ends[1] == 1.0 - 2.0 ** -24
    g = R.noise64(1 << 8, 1 << 8, seed, step, site)
    assert bool(torch.isfinite(g).all())
    # a Gumbel(0, 1) sample: mean = Euler's constant, variance = pi^2 / 6 (standard error of the mean of 65536 draws: 0.005)
    assert abs(float(g.mean()) - 0.5772156649) < 0.03 and abs(float(g.var()) - np.pi ** 2 / 6) < 0.08


def test_kl_gradient_formula_matches_finite_differences():
    """d kl / d l_m = (1 / N) q_m (h_m - sum_k q_k h_k), the second term of nk_gumbel_softmax_bwd, against central differences in float64"""
    gen = torch.Generator().manual_seed(5)
    l = 2.0 * torch.randn(3, 11, generator=gen, dtype=torch.float64)
    zero = torch.zeros(3, 11, dtype=torch.float64)
    d = R.softmax_bwd64(l, zero, zero, 1.0, 1.0)
    eps = 1e-6
    for i, m in ((0, 0), (1, 4), (2, 10), (0, 7)):
        e = torch.zeros_like(l)
        e[i, m] = eps
        fd = float(R.kl64(l + e) - R.kl64(l - e)) / (2 * eps)
        assert abs(fd - float(d[i, m])) <= 1e-8 * max(1.0, abs(fd)), (i, m, fd, float(d[i, m]))
    l.requires_grad_(True)
    (auto,) = torch.autograd.grad(R.kl64(l), l)
    assert float((auto - d).abs().max()) <= 1e-14
