"""Fixture of the Gumbel-softmax quantizer: the reference's own GumbelQuantizer run on the CPU in fp32.

    python -m tests.golden.make_golden_gumbel        ->  tests/golden/gumbel_tiny.{json,safetensors}

z [2, 8, 3, 5] against 24 codes of width 8, in the four mode combinations (straight_through or not, train or eval).  F.gumbel_softmax draws
its noise as -empty_like(logits).exponential_().log() from the global generator; each case seeds it, and the generator of this file replays
the seeded draw to record the noise [B, n, H, W] next to the outputs.  Per case: z_q, loss, indices, and autograd's dz, d proj.weight,
d proj.bias, d embed.weight of <upstream, z_q> + loss for a fixed upstream.  Every row is DECIDED (tests/gumbel_reference.py): its argmax
is the same under any fp32 evaluation order.  The generator asserts that and fails otherwise.
"""
from __future__ import annotations

import torch

from tests.golden.fixture_io import save_fixture
from tests.golden.make_golden import import_reference
from tests.gumbel_reference import acceptable, rows_of

H_DIM, E_DIM, N_EMBED, SHAPE = 8, 8, 24, (2, 8, 3, 5)
KL_WEIGHT, TEMP = 5e-2, 0.8


def main() -> None:
    import_reference()
    from neurosis.modules.autoencoding.regularizers.quantize import GumbelQuantizer

    g = torch.Generator().manual_seed(20240921)
    proj_w = 0.6 * torch.randn(N_EMBED, H_DIM, 1, 1, generator=g)
    proj_b = 0.2 * torch.randn(N_EMBED, generator=g)
    embed = torch.randn(N_EMBED, E_DIM, generator=g)
    z0 = torch.randn(*SHAPE, generator=g)
    upstream = torch.randn(SHAPE[0], E_DIM, SHAPE[2], SHAPE[3], generator=g)
    out = {"num_hiddens": H_DIM, "embedding_dim": E_DIM, "n_embed": N_EMBED, "kl_weight": KL_WEIGHT, "temp": TEMP, "proj_w": proj_w, "proj_b": proj_b,
           "embed": embed, "z": z0, "upstream": upstream, "cases": {}}
    for seed, (hard, train) in enumerate(((True, True), (False, True), (True, False), (False, False)), start=101):
        q = GumbelQuantizer(H_DIM, E_DIM, N_EMBED, straight_through=hard, kl_weight=KL_WEIGHT, temp_init=TEMP)
        if seed == 101:
            out["state_dict_shapes"] = {k: list(v.shape) for k, v in q.state_dict().items()}
        q.load_state_dict({"proj.weight": proj_w, "proj.bias": proj_b, "embed.weight": embed})
        q.train(train)
        z = z0.clone().requires_grad_(True)
        torch.manual_seed(seed)
        z_q, log = q(z, return_logits=True)
        torch.manual_seed(seed)
        noise = -torch.empty_like(log["logits"], memory_format=torch.legacy_contiguous_format).exponential_().log()
        _, _, decided = acceptable(rows_of(z0, H_DIM), proj_w.view(N_EMBED, H_DIM), proj_b, rows_of(noise, N_EMBED))
        assert bool(decided.all()), f"hard={hard} train={train}: {int((~decided).sum())} undecided rows; change the seed"
        ((z_q * upstream).sum() + log["loss/vq"]).backward()
        # the recorded noise is the draw the forward used: the soft one-hot rebuilt from it reproduces the indices
        replay = torch.softmax((log["logits"].detach() + noise) / TEMP, dim=1).argmax(1)
        assert torch.equal(replay, log["indices"])
        out["cases"][f"hard{int(hard)}_train{int(train)}"] = {
            "hard": hard, "train": train, "noise": noise, "z_q": z_q.detach(), "loss": log["loss/vq"].detach(), "indices": log["indices"],
            "logits": log["logits"].detach(), "dz": z.grad, "d_proj_w": q.proj.weight.grad, "d_proj_b": q.proj.bias.grad, "d_embed": q.embed.weight.grad,
        }
    save_fixture(out, "gumbel_tiny")


if __name__ == "__main__":
    main()
