"""`bench.py --dump-outputs DIR`: what the last timed step computed, written so that two builds can be compared output for output.
CPU only: the dump of a stand-in flat parameter store (the same three fields the engine's FlatParamStore has)."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _store(n):
    """every element holds its own flat index (negated in the gradients), so a sample names the indices it was taken at"""
    master = torch.arange(n, dtype=torch.float32)
    return SimpleNamespace(numel=n, master=master, grad=-master)


def test_dump_writes_float32_arrays_at_fixed_indices(tmp_path):
    shapes = bench.dump_outputs(tmp_path / "a", torch.tensor(0.25, dtype=torch.bfloat16), _store(10_000), sample=512)
    assert shapes == {"loss": (1,), "master_sample": (512,), "grad_sample": (512,)}
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == set(shapes) and all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].tolist() == [0.25]
    assert np.array_equal(got["grad_sample"], -got["master_sample"])          # the same indices into both buffers
    assert len(np.unique(got["master_sample"])) > 400                         # spread over the buffer, not one element
    bench.dump_outputs(tmp_path / "b", torch.tensor(1.0), _store(10_000), sample=512)
    assert np.array_equal(np.load(tmp_path / "b" / "master_sample.npy"), got["master_sample"])     # and the same ones on every run


def test_dump_of_the_flagship_size_stays_within_64_mb():
    assert 2 * bench.DUMP_SAMPLE * 4 + 4 <= 64 << 20


def test_steps_must_be_positive():
    assert bench.parse_args(["--steps", "3", "--dump-outputs", "d"]).steps == 3
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
