"""Reads the T5 fixtures that tests/golden/make_golden_t5.py writes (shared by tests/test_t5_cpu.py and tests/test_t5_gpu.py)."""
from __future__ import annotations

import functools

from tests.golden.fixture_io import load_fixture


@functools.lru_cache(maxsize=None)
def index() -> dict:
    """{"variants": {name: weight shards}, "lengths", "batch", "byt5": {"texts", "max_length", "ids"}}"""
    return load_fixture("t5_tiny")


@functools.lru_cache(maxsize=None)
def variant(name: str) -> dict:
    """{"config", "keys", "cases": {str(L): {"ids", "out", "floor_rms", "floor_max", "mutations"}}, "state": transformers' state_dict}
    (+ "compute_bias": {str(L): [H, L, L]} on v11).  Loaded once and shared: treat it as read-only."""
    entry = dict(load_fixture(f"t5_tiny_{name}"))
    state = {}
    for i in range(index()["variants"][name]):
        state.update({k.replace("|", "."): v for k, v in load_fixture(f"t5_tiny_{name}_w{i}").items()})
    state["encoder.embed_tokens.weight"] = state["shared.weight"]
    entry["state"] = state
    return entry


def names() -> list:
    return list(index()["variants"])
