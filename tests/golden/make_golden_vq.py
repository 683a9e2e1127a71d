"""Fixtures of the vector quantizers: the reference's own VectorQuantizer / EMAVectorQuantizer run on the CPU in fp32.

    python -m tests.golden.make_golden_vq        ->  tests/golden/vq_tiny.{json,safetensors}

Per class: state_dict keys and shapes, one forward on z [2, 4, 5, 7] against 37 codes (outputs, loss, indices, perplexity / cluster
usage); for VectorQuantizer autograd's dz and d embedding.weight of <g, z_q> + loss for a fixed g; for the EMA class the three buffers
after three training forwards on three different inputs.  Every input row is DECIDED (tests/vq_reference.py): its nearest code is the
same under any fp32 evaluation order, so the indices are facts, not accidents of a BLAS.  The generator asserts that and fails otherwise.
"""
from __future__ import annotations

import torch

from tests.golden.fixture_io import save_fixture
from tests.golden.make_golden import import_reference
from tests.vq_reference import acceptable, rows_of

N_E, DIM, SHAPE = 37, 4, (2, 4, 5, 7)


def _assert_decided(z, E, what):
    _, _, decided = acceptable(rows_of(z, DIM), E)
    assert bool(decided.all()), f"{what}: {int((~decided).sum())} undecided rows; change the seed"


def main() -> None:
    import_reference()
    from neurosis.modules.autoencoding.regularizers.quantize import EMAVectorQuantizer, VectorQuantizer

    g = torch.Generator().manual_seed(20240607)
    out = {"n_e": N_E, "dim": DIM}

    # -- VectorQuantizer ------------------------------------------------------------------------------------------
    vq = VectorQuantizer(N_E, DIM, beta=0.25, log_perplexity=True)
    init = vq.embedding.weight.detach().clone()
    assert float(init.abs().max()) <= 1.0 / N_E
    codebook = 0.7 * torch.randn(N_E, DIM, generator=g)
    vq.load_state_dict({"embedding.weight": codebook})
    z = torch.randn(*SHAPE, generator=g).requires_grad_(True)
    upstream = torch.randn(*SHAPE, generator=g)
    _assert_decided(z, codebook, "VectorQuantizer")
    z_q, log = vq(z)
    ((z_q * upstream).sum() + log["loss/vq"]).backward()
    out["vq"] = {
        "state_dict_shapes": {k: list(v.shape) for k, v in vq.state_dict().items()},
        "codebook": codebook, "z": z.detach(), "upstream": upstream, "z_q": z_q.detach(), "loss": log["loss/vq"].detach(),
        "indices": log["min_encoding_indices"], "perplexity": log["perplexity"], "cluster_usage": log["cluster_usage"],
        "dz": z.grad, "d_codebook": vq.embedding.weight.grad, "beta": 0.25,
    }

    # -- EMAVectorQuantizer -----------------------------------------------------------------------------------------
    ema = EMAVectorQuantizer(N_E, DIM, beta=0.25, decay=0.9, eps=1e-5)
    weight0 = 0.7 * torch.randn(N_E, DIM, generator=g)
    ema.load_state_dict({"embedding.weight": weight0, "embedding.cluster_size": torch.zeros(N_E), "embedding.embed_avg": weight0.clone()})
    ze = torch.randn(*SHAPE, generator=g)
    _assert_decided(ze, weight0, "EMAVectorQuantizer eval")
    ema.eval()
    q, elog = ema(ze)
    case = {
        "state_dict_shapes": {k: list(v.shape) for k, v in ema.state_dict().items()},
        "weight0": weight0, "z": ze, "z_q": q.detach(), "loss": elog["loss/vq"].detach(), "indices": elog["encoding_indices"],
        "perplexity": elog["perplexity"], "beta": 0.25, "decay": 0.9, "eps": 1e-5, "steps": [],
    }
    ema.train()
    for step in range(3):
        zs = torch.randn(*SHAPE, generator=g) * (1.0 + 0.5 * step)
        _assert_decided(zs, ema.embedding.weight.detach(), f"EMAVectorQuantizer step {step}")
        _, slog = ema(zs)
        case["steps"].append({"z": zs, "indices": slog["encoding_indices"], "loss": slog["loss/vq"].detach()})
    case["after"] = {k: v.detach().clone() for k, v in ema.state_dict().items()}
    out["ema"] = case
    save_fixture(out, "vq_tiny")


if __name__ == "__main__":
    main()
