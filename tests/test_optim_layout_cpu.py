"""The tensor tables, work items and chunk lists of the fused optimizers, pinned without a GPU or the HIP library: the kernels
read these bytes through C structs, so a planner change that moves one of them changes the launch arguments of every step.

`FlatAdafactor` and `FlatCAME` are built over a stub store (parameters on the meta device) with `neurosis_amd.optim.query`
answering the table dtype's own size, and sha256 digests of what they lay out are compared with EXPECTED.  The digests were
recorded at commit 2b11a1c (the parent of the commit that folded both planners into one) by running this file as a script
there: `python tests/test_optim_layout_cpu.py` prints the dict.  They are this project's own tables, not reference data.
"""
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

EXPECTED = {
    'adafactor/sdxl': {'tensors': 'b32f8d5cf17563525b98838aff07ac46687973c73faff326204eacecd9342b97',
                       'items': '8f8e570014001472f32428d0ef9ed502fbd1e2d06534dffe5a19cf6c24c7df8a',
                       'chunks': '3665e8080e039216884546fbdbcae435b28f4cb9ea5cee23c99fb23feeec5498',
                       'nchunks': 85,
                       'ntensors': 1680,
                       'nitems': 187163,
                       'sizes': [244330560, 646400, 26969, 5740, 187163]},
    'adafactor/sdxl/restricted': {'chunks': '394a605a9c7e3c1b9fa892bf70b667fbfa95bb1aef1f463ac7b6011dedd66c6d', 'nchunks': 88},
    'adafactor/small': {'tensors': 'a1219dd6b6702850dea918a042c5438e2fb3cc73e22ec3652f8989192bf7ddaf',
                        'items': 'dd228fb2d7ae6ce82561bfce16f4d7ae0cfa856237b6e851f3fe2616c99b6ba0',
                        'chunks': '46249a87dbdf322dab6becf128744fd7d8432ca5f559402aca28acb76300872c',
                        'nchunks': 5,
                        'ntensors': 9,
                        'nitems': 25,
                        'sizes': [12864, 1280, 28, 7, 25]},
    'came/sdxl': {'tensors': 'e77ba115303e8b6d4bfe54c46b4cf727922d5c1a9825850236837a1fc639d078',
                  'items': '8f8e570014001472f32428d0ef9ed502fbd1e2d06534dffe5a19cf6c24c7df8a',
                  'chunks': '3665e8080e039216884546fbdbcae435b28f4cb9ea5cee23c99fb23feeec5498',
                  'nchunks': 85,
                  'ntensors': 1680,
                  'nitems': 187163,
                  'sizes': [3054541440, 646400, 26969, 11480, 187163]},
    'came/small': {'tensors': '96fc4ca9f7aa531a2653e5600ad0621bc769a6f470861b67bf78cc96527dfed7',
                   'items': 'dd228fb2d7ae6ce82561bfce16f4d7ae0cfa856237b6e851f3fe2616c99b6ba0',
                   'chunks': '46249a87dbdf322dab6becf128744fd7d8432ca5f559402aca28acb76300872c',
                   'nchunks': 5,
                   'ntensors': 9,
                   'nitems': 25,
                   'sizes': [172160, 1280, 28, 14, 25]},
    'adafactor/sdxl/blocks': {'tensors': 'f83f29e5a50cffc241a6f1548659ffa74b6c27d15ca00df1bf743892b8315ee2',
                              'items': '8f8e570014001472f32428d0ef9ed502fbd1e2d06534dffe5a19cf6c24c7df8a',
                              'chunks': 'c031e258076eb5ce6a6eab0b098d484cc59c896eca377cc4cb456e7ad9afde74',
                              'nchunks': 97,
                              'ntensors': 1680,
                              'nitems': 187163,
                              'sizes': [244330560, 646400, 26969, 5740, 187163],
                              'nboundaries': 22},
    'adafactor/sdxl/blocks/restricted': {'chunks': '418f7817eca1459ca6a1c882c1c8583f2f7b1193dc5af3bb722e2daa5ab4ef54', 'nchunks': 100},
    'adafactor/small/bounds': {'tensors': 'a1219dd6b6702850dea918a042c5438e2fb3cc73e22ec3652f8989192bf7ddaf',
                               'items': 'dd228fb2d7ae6ce82561bfce16f4d7ae0cfa856237b6e851f3fe2616c99b6ba0',
                               'chunks': 'a7ad051d72da1bb84cb1b554e815ad35fdba431712914708c7badecefc42ec89',
                               'nchunks': 7,
                               'ntensors': 9,
                               'nitems': 25,
                               'sizes': [12864, 1280, 28, 7, 25]},
    'adamw8bit/sdxl': {'arrays': 'e29272a93d2606f092b0c43bac8105d911b7ee10e842d421dffb4ed039db084d', 'nblocks': 10029262, 'small': 917824},
}

# a vector, a vector shorter than one item, a matrix with d0 not a multiple of 256, a wide matrix, a 1x1 and a 3x3 conv, a 3x1 conv
SMALL_SHAPES = [(1500,), (7,), (300, 128), (64, 520), (48, 40, 1, 1), (32, 24, 3, 3), (16, 8, 3, 1), (1024, 64), (96,)]
SMALL_CHUNK_BYTES = 160 << 10


def _sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class _Store:
    """What the flat optimizers touch of a FlatParamStore at construction, with FlatParamStore's 64-element alignment."""

    def __init__(self, params):
        self.params = list(params)
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 63) // 64 * 64
        self.master = SimpleNamespace(device=torch.device("meta"))
        self.listeners = []

    def add_listener(self, obj) -> None:
        self.listeners.append(obj)


def _sdxl_unet():
    import bench
    import neurosis_amd.modules.diffusion as D

    with torch.device("meta"):
        return D.UNetModel(**bench.SDXL_UNET)


def _block_boundaries(unet, store) -> list:
    from neurosis_amd.models.diffusion import DiffusionEngine

    return DiffusionEngine._block_boundaries(SimpleNamespace(model=SimpleNamespace(diffusion_model=unet), store=store))


def _planned(monkeypatch, cls, store, dtype, **kwargs) -> tuple:
    """(optimizer, digests): the table and item bytes are taken where they are handed to the device (`torch.from_numpy`)."""
    import neurosis_amd.optim as optim

    uploads = []
    real = torch.from_numpy

    def from_numpy(a):
        uploads.append(a.copy())
        return real(a)

    monkeypatch.setattr(optim, "query", lambda name: dtype.itemsize)
    monkeypatch.setattr(torch, "from_numpy", from_numpy)
    opt = cls(store, **kwargs)
    monkeypatch.setattr(torch, "from_numpy", real)
    assert len(uploads) == 2 and uploads[0].tobytes() == opt._tens_np.tobytes()
    assert uploads[1].size == opt.nitems * optim.AF_ITEM_DTYPE.itemsize
    return opt, {"tensors": _sha(opt._tens_np), "items": _sha(uploads[1]), "chunks": _sha(np.array(opt.chunks, dtype=np.int64)),
                 "nchunks": len(opt.chunks), "ntensors": opt.ntensors, "nitems": opt.nitems,
                 "sizes": [t.numel() for t in (opt.state, opt.ws, opt.counters, opt.mean_row, opt.u2_part)]}


def measure(monkeypatch) -> dict:
    import neurosis_amd.optim as optim
    from neurosis_amd.optim import FlatAdafactor, FlatAdamW8bit, FlatCAME

    monkeypatch.delenv("NK_AF_CHUNK_MB", raising=False)
    monkeypatch.delenv("NK_AF_STREAMS", raising=False)
    unet = _sdxl_unet()
    store = _Store(p for p in unet.parameters() if p.requires_grad)
    with torch.device("meta"):
        small = _Store(torch.nn.Parameter(torch.empty(s)) for s in SMALL_SHAPES)
    out = {}
    for name, cls, dtype in (("adafactor", FlatAdafactor, optim.AF_TENSOR_DTYPE), ("came", FlatCAME, optim.CAME_TENSOR_DTYPE)):
        opt, out[f"{name}/sdxl"] = _planned(monkeypatch, cls, store, dtype)
        if cls is FlatAdafactor:
            opt.restrict_ranges([(0, 400), (900, 1300)])
            out["adafactor/sdxl/restricted"] = {"chunks": _sha(np.array(opt.chunks, dtype=np.int64)), "nchunks": len(opt.chunks)}
        _, out[f"{name}/small"] = _planned(monkeypatch, cls, small, dtype, chunk_bytes=SMALL_CHUNK_BYTES)
    bounds = _block_boundaries(unet, store)
    opt, out["adafactor/sdxl/blocks"] = _planned(monkeypatch, FlatAdafactor, store, optim.AF_TENSOR_DTYPE, boundaries=bounds)
    out["adafactor/sdxl/blocks"]["nboundaries"] = len(bounds)
    opt.restrict_ranges([(0, 400), (900, 1300)])
    out["adafactor/sdxl/blocks/restricted"] = {"chunks": _sha(np.array(opt.chunks, dtype=np.int64)), "nchunks": len(opt.chunks)}
    _, out["adafactor/small/bounds"] = _planned(monkeypatch, FlatAdafactor, small, optim.AF_TENSOR_DTYPE, chunk_bytes=SMALL_CHUNK_BYTES,
                                                boundaries=[1, 6])
    lay = FlatAdamW8bit.layout([tuple(p.shape) for p in store.params])
    out["adamw8bit/sdxl"] = {"arrays": _sha(*(lay[k] for k in ("numel", "is8", "blk_start", "soff"))), "nblocks": lay["nblocks"],
                             "small": lay["small"]}
    return out


def test_layout_matches_the_recorded_tables(monkeypatch):
    got = measure(monkeypatch)
    assert sorted(got) == sorted(EXPECTED)
    for case in EXPECTED:
        assert got[case] == EXPECTED[case], case


def test_shape_refusals_name_the_calling_class(monkeypatch):
    import neurosis_amd.optim as optim

    for cls, dtype in ((optim.FlatAdafactor, optim.AF_TENSOR_DTYPE), (optim.FlatCAME, optim.CAME_TENSOR_DTYPE)):
        monkeypatch.setattr(optim, "query", lambda name, n=dtype.itemsize: n)
        for shape, words in (((4, 4, 4), "3-d parameters"), ((8, 6), "rows must be a multiple of 4"), ((4, 4, 5, 1), "larger than 3x3")):
            with torch.device("meta"):
                store = _Store([torch.nn.Parameter(torch.empty(shape))])
            with pytest.raises(NotImplementedError, match=f"{cls.__name__}: .*{words}"):
                cls(store)


if __name__ == "__main__":
    import pprint
    import sys
    from pathlib import Path

    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    with pytest.MonkeyPatch.context() as mp:
        pprint.pprint(measure(mp), width=140, sort_dicts=False)
