"""Shared by tests/golden/make_golden_dreamsim.py and the DreamSim tests: the tiny towers' seeded weights.  They are a pure function of
each tensor's name and shape (6 MB as a file, so they are rebuilt, not stored); the fixture records a checksum per tensor, which
`seeded_state` callers compare so that a torch whose CPU generator draws differently fails loudly instead of quietly testing other weights."""
from __future__ import annotations

import zlib

import torch

TINY = dict(embed_dim=128, depth=2, num_heads=2, img_size=32)
HEAD_WIDTH, PATCH = 16, 16
GAIN, TABLE_STD = 1.5, 0.2      # matrices ~ GAIN / sqrt(fan_in) (the default 0.02 init gives embeddings that barely depend on the image)


def seeded_tensor(name: str, shape) -> torch.Tensor:
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    shape = tuple(shape)
    if name.endswith("weight") and len(shape) >= 2:
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        return GAIN * torch.randn(shape, generator=g) / fan_in ** 0.5
    if name.endswith("weight"):                        # LayerNorm
        return 1.0 + 0.1 * torch.randn(shape, generator=g)
    if name.endswith("bias"):
        return 0.1 * torch.randn(shape, generator=g)
    return TABLE_STD * torch.randn(shape, generator=g)   # cls_token, pos_embed


def seeded_state(shapes: dict) -> dict:
    """{name: tensor} for {name: shape}"""
    return {k: seeded_tensor(k, v) for k, v in shapes.items()}


def checksums(state: dict) -> dict:
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in state.items()}


def checked_state(fixture: dict) -> dict:
    """the fixture's towers' weights, rebuilt and compared with the recorded checksums"""
    state = seeded_state(fixture["state_shapes"])
    for k, (s, a) in fixture["state_checksums"].items():
        got = checksums({k: state[k]})[k]
        assert abs(got[0] - s) <= 1e-6 * max(1.0, a) and abs(got[1] - a) <= 1e-6 * max(1.0, a), f"seeded weight {k} differs from the fixture's: {got} vs {[s, a]}"
    return state
