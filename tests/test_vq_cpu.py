"""Vector quantizers without a GPU: constructors, state_dict surface and class paths against the reference's fixture
(tests/golden/vq_tiny, made by tests/golden/make_golden_vq.py), every refusal, the engine's parameter list, and the fixture's own
side of the numerical contract: its inputs are decided rows in float64, and its fp32 values lie inside the bounds the GPU tests use."""
import importlib

import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.vq_reference import U, acceptable, ema_bound, ema_step64, perplexity_tol, rows_of, tiny_vq_engine, vq_bounds, vq_restate64

Q = "neurosis.modules.autoencoding.regularizers.quantize."


@pytest.fixture(scope="module")
def fx():
    return load_fixture("vq_tiny")


def _resolve(path: str):
    module, _, cls = path.replace("neurosis.", "neurosis_amd.", 1).rpartition(".")
    return getattr(importlib.import_module(module), cls)


def test_class_paths_resolve_under_the_prefix_swap():
    from neurosis_amd.models.autoencoder import DiagonalGaussianRegularizer

    for name in ("VectorQuantizer", "EMAVectorQuantizer"):
        assert isinstance(_resolve(Q + name), type)
    for name in ("AbstractRegularizer", "IdentityRegularizer", "measure_perplexity"):
        assert _resolve("neurosis.modules.autoencoding.regularizers.base." + name) is not None
    assert _resolve("neurosis.modules.autoencoding.regularizers.DiagonalGaussianRegularizer") is DiagonalGaussianRegularizer
    assert DiagonalGaussianRegularizer.loss_key == "kl_loss"


def test_constructors_and_state_dict_surface(fx):
    vq = _resolve(Q + "VectorQuantizer")(fx["n_e"], fx["dim"])
    assert {k: list(v.shape) for k, v in vq.state_dict().items()} == fx["vq"]["state_dict_shapes"]
    assert float(vq.embedding.weight.detach().abs().max()) <= 1.0 / fx["n_e"] and vq.embedding.weight.requires_grad
    assert (vq.beta, vq.loss_key, vq.sane_index_shape, vq.log_perplexity) == (0.25, "loss/vq", False, False)
    assert [p is vq.embedding.weight for p in vq.get_trainable_parameters()] == [True]
    vq.load_state_dict({"embedding.weight": fx["vq"]["codebook"]})
    ema = _resolve(Q + "EMAVectorQuantizer")(fx["n_e"], fx["dim"], beta=0.25)
    assert {k: list(v.shape) for k, v in ema.state_dict().items()} == fx["ema"]["state_dict_shapes"]
    assert not any(p.requires_grad for p in ema.parameters()) and list(ema.get_trainable_parameters()) == []
    assert (ema.embedding.decay, ema.embedding.eps, ema.embedding.update, ema.loss_key) == (0.99, 1e-5, True, "loss/vq")
    assert torch.equal(ema.embedding.weight, ema.embedding.embed_avg) and not ema.embedding.cluster_size.any()
    ema.load_state_dict(fx["ema"]["after"])


def test_refusals_name_the_argument():
    VQ, EMA = _resolve(Q + "VectorQuantizer"), _resolve(Q + "EMAVectorQuantizer")
    with pytest.raises(NotImplementedError, match="remap"):
        VQ(8, 4, remap="used.npy")
    with pytest.raises(NotImplementedError, match="unknown_index"):
        VQ(8, 4, unknown_index="extra")
    with pytest.raises(NotImplementedError, match="embedding_weight_norm"):
        VQ(8, 4, embedding_weight_norm=True)
    with pytest.raises(NotImplementedError, match="remap"):
        EMA(8, 4, 0.25, remap="used.npy")
    with pytest.raises(NotImplementedError, match="unknown_index"):
        EMA(8, 4, 0.25, unknown_index="extra")
    for missing in ("GumbelQuantizer", "VectorQuantizerWithInputProjection"):
        with pytest.raises(AttributeError):
            _resolve(Q + missing)


def test_cpu_tensors_are_refused(fx):
    import neurosis_amd.torch_ops  # noqa: F401  (registers torch.ops.neurosis_hip.*)
    from neurosis_amd import ops

    z, E = torch.zeros(6, 4), torch.zeros(5, 4)
    idx = torch.zeros(6, dtype=torch.int64)
    for call in (lambda: ops.vq_search(z, E), lambda: ops.vq_code_stats(idx, z, 5), lambda: ops.vq_quantize(idx, E, z),
                 lambda: torch.ops.neurosis_hip.vq_search(z, E), lambda: torch.ops.neurosis_hip.vq_quantize(z, E, idx, 0.25)):
        with pytest.raises(NotImplementedError, match="CPU"):
            call()
    with pytest.raises(NotImplementedError, match="CPU"):
        _resolve(Q + "VectorQuantizer")(fx["n_e"], fx["dim"])(fx["vq"]["z"])


def test_torch_ops_are_registered_with_meta_kernels():
    import neurosis_amd.torch_ops as T

    assert {"vq_search", "vq_code_stats", "vq_quantize"} <= set(T.OPS)
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    idx = torch.ops.neurosis_hip.vq_search(m(70, 4), m(37, 4))
    assert idx.shape == (70,) and idx.dtype == torch.int64
    z_q, loss = torch.ops.neurosis_hip.vq_quantize(m(70, 4), m(37, 4), m(70, dtype=torch.int64), 0.25)
    assert z_q.shape == (70, 4) and loss.shape == ()
    count, total = torch.ops.neurosis_hip.vq_code_stats(m(70, dtype=torch.int64), m(70, 4), 37)
    assert count.shape == (37,) and count.dtype == torch.int64 and total.shape == (37, 4)


def test_measure_perplexity_against_the_fixture(fx):
    from neurosis_amd.modules.autoencoding.regularizers import measure_perplexity

    p, used = measure_perplexity(fx["vq"]["indices"], fx["n_e"])
    assert abs(float(p) - float(fx["vq"]["perplexity"])) <= perplexity_tol(float(p), fx["n_e"])
    assert int(used) == int(fx["vq"]["cluster_usage"])
    p, _ = measure_perplexity(fx["ema"]["indices"], fx["n_e"])
    assert abs(float(p) - float(fx["ema"]["perplexity"])) <= perplexity_tol(float(p), fx["n_e"])


def test_fixture_inputs_are_decided_in_float64(fx):
    """every row of every fixture input has exactly one acceptable code, and it is the one the reference chose"""
    ok, jmin, decided = acceptable(rows_of(fx["vq"]["z"], fx["dim"]), fx["vq"]["codebook"])
    assert bool(decided.all()) and torch.equal(jmin, fx["vq"]["indices"])
    ok, jmin, decided = acceptable(rows_of(fx["ema"]["z"], fx["dim"]), fx["ema"]["weight0"])
    assert bool(decided.all()) and torch.equal(jmin, fx["ema"]["indices"])
    # the EMA training steps: replay the three buffers in float64 along the reference's indices; each step's input is decided
    # against the weights of that step
    e = fx["ema"]
    w, cs, avg = e["weight0"].double(), torch.zeros(fx["n_e"], dtype=torch.float64), e["weight0"].double()
    for step in e["steps"]:
        rows = rows_of(step["z"], fx["dim"])
        ok, jmin, decided = acceptable(rows, w)
        assert bool(decided.all()) and torch.equal(jmin, step["indices"])
        w, cs, avg = ema_step64(w, cs, avg, rows, jmin, e["decay"], e["eps"])
    for key, want in (("embedding.weight", w), ("embedding.cluster_size", cs), ("embedding.embed_avg", avg)):
        got = e["after"][key].double()
        scale = want.abs().amax(1, keepdim=True) if want.ndim == 2 else want.abs().max()       # normwise per code
        assert bool(((got - want).abs() <= ema_bound(rows.shape[0]) * scale).all()), key


def test_fixture_values_lie_inside_the_float64_bounds(fx):
    """the reference's fp32 loss / gradients against a float64 restatement, inside the bounds tests/test_vq_gpu.py holds the kernels to"""
    v = fx["vq"]
    want = vq_restate64(v["z"], v["codebook"], v["indices"], v["upstream"], v["beta"])
    bounds = vq_bounds(v["z"], v["codebook"], v["indices"], v["upstream"])
    # the reference returns z + (z_q - z): two roundings away from the codebook rows themselves (which is what the kernels write)
    assert float((v["z_q"].double() - want["z_q"]).abs().max()) <= 2 * 2 * U * float(v["z"].abs().max() + v["codebook"].abs().max())
    assert abs(float(v["loss"]) - float(want["loss"])) <= bounds["loss"] * float(want["loss"])
    assert float((v["dz"].double() - want["dz"]).abs().max()) <= bounds["dz"]
    assert bool(((v["d_codebook"].double() - want["dE"]).abs() <= bounds["dE"]).all())


def test_engine_parameter_list_puts_the_codebook_last():
    from neurosis_amd.models.autoencoder import DiagonalGaussianRegularizer

    vq = _resolve(Q + "VectorQuantizer")(64, 4)
    eng = tiny_vq_engine(vq, regularization_weights={"loss/vq": 1.0})
    params = eng.get_autoencoder_params()
    assert params[-1] is vq.embedding.weight and sum(p is vq.embedding.weight for p in params) == 1
    gauss = tiny_vq_engine(DiagonalGaussianRegularizer())
    want = list(gauss.decoder.parameters()) + list(gauss.encoder.parameters())
    got = gauss.get_autoencoder_params()
    assert len(got) == len(want) and all(a is b for a, b in zip(got, want))
    assert all(a is b for a, b in zip(eng.get_autoencoder_params(decoder_only=True), eng.decoder.parameters()))
    ema = tiny_vq_engine(_resolve(Q + "EMAVectorQuantizer")(64, 4, 0.25))
    assert len(ema.get_autoencoder_params()) == len(want)
