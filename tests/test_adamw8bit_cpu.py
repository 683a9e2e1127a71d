"""neurosis_amd.optimizers.AdamW8bit without a GPU: bitsandbytes' AdamW8bit constructor, the refusals of what is not built, torch.optim.AdamW's
validation, no CPU path, the quantization maps, the pure-torch restatement against its committed fixture (tests/golden/adamw8bit_steps,
written by make_golden_adamw8bit.py), the engine, and the state memory of the SDXL UNet's parameter shapes."""
import inspect
from functools import partial
from types import SimpleNamespace

import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.golden.make_golden_adamw8bit import (A8_BLOCK, SHAPES, ZERO_BLOCK, dynamic_map, init_state, nearest, phys, restated_step,
                                                unphys)

BNB_SIGNATURE = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, optim_bits=32, args=None, min_8bit_size=4096,
                     percentile_clipping=100, block_wise=True, is_paged=False)


def load_adamw8bit_case(tag: str) -> dict:
    """One case of the adamw8bit_steps fixture with the shared inputs (stored once, bf16-exact) attached in fp32: kwargs, init, grads
    (four steps), after (four steps), states (after the last step; codes / fp32 moments in the parameters' shapes), step."""
    fx = load_fixture("adamw8bit_steps")
    return {**fx[tag], "init": [t.float() for t in fx["init"]], "grads": [[t.float() for t in gs] for gs in fx["grads"]],
            "qmap1": fx["qmap1"], "qmap2": fx["qmap2"]}


def test_class_path_resolves_with_the_bitsandbytes_signature():
    import importlib

    mod, name = "neurosis_amd.optimizers.AdamW8bit".rsplit(".", 1)
    cls = getattr(importlib.import_module(mod), name)
    assert issubclass(cls, torch.optim.Optimizer)
    sig = inspect.signature(cls.__init__)
    mine = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params")}
    assert list(mine) == list(BNB_SIGNATURE), "argument order differs from bitsandbytes.optim.AdamW8bit's"
    assert mine == BNB_SIGNATURE
    from neurosis_amd.optimizers.adamw8bit import AdamW8bit

    assert AdamW8bit is cls
    import neurosis_amd.optimizers as O

    assert "AdamW8bit" in O.__all__ and "neurosis_amd.optimizers.AdamW8bit" in O.__doc__


@pytest.mark.parametrize("kw,what", [(dict(amsgrad=True), "amsgrad"), (dict(block_wise=False), "block_wise"),
                                     (dict(percentile_clipping=95), "percentile_clipping"), (dict(args=object()), "args"),
                                     (dict(is_paged=True), "is_paged")])
def test_refuses_what_is_not_built(kw, what):
    from neurosis_amd.optimizers import AdamW8bit

    with pytest.raises(NotImplementedError, match=what) as e:
        AdamW8bit([torch.nn.Parameter(torch.zeros(8, 8))], **kw)
    assert "not implemented" in str(e.value)


@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(-0.1, 0.999)),
                                dict(eps=-1e-8), dict(weight_decay=-0.1)])
def test_adamw_validation(kw):
    from neurosis_amd.optimizers import AdamW8bit

    with pytest.raises(ValueError):
        AdamW8bit([torch.nn.Parameter(torch.zeros(4, 4))], **kw)
    with pytest.raises(ValueError):                       # the same arguments torch.optim.AdamW refuses
        torch.optim.AdamW([torch.nn.Parameter(torch.zeros(4, 4))], **kw)


def test_no_cpu_path():
    from neurosis_amd.optimizers import AdamW8bit

    p = torch.nn.Parameter(torch.zeros(8, 8))
    p.grad = torch.ones(8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        AdamW8bit([p]).step()


def test_quantization_maps():
    from neurosis_amd.optim import create_dynamic_map

    q1, q2 = create_dynamic_map(signed=True), create_dynamic_map(signed=False)
    fx = load_fixture("adamw8bit_steps")
    assert torch.equal(q1, fx["qmap1"]) and torch.equal(q2, fx["qmap2"])
    assert torch.equal(q1, dynamic_map(True)) and torch.equal(q2, dynamic_map(False))
    for q in (q1, q2):
        assert q.dtype == torch.float32 and q.numel() == 256
        assert bool((q[1:] > q[:-1]).all()), "not sorted into 256 distinct entries"
        assert float(q[-1]) == 1.0 and int((q == 0).sum()) == 1
    assert abs(float(q1[0]) + 0.99297) < 1e-5 and float(q1[0]) > -1.0      # asymmetric: -0.99297 .. 1.0
    assert float(q2[0]) == 0.0
    assert int((q1 < 0).sum()) == 127 and int((q1 > 0).sum()) == 128


def test_nearest_is_the_lowest_argmin():
    """The restatement's neighbour form of `nearest` is argmin |q - x| over all 256 entries, first index on a tie: on random values, on
    the map entries themselves, on the exact midpoints between neighbours, and outside [-1, 1]."""
    g = torch.Generator().manual_seed(3)
    for q in (dynamic_map(True), dynamic_map(False)):
        mids = (q[1:] + q[:-1]) / 2
        x = torch.cat([torch.rand(20000, generator=g) * 2 - 1, torch.randn(2000, generator=g) * 1e-4, q, mids,
                       torch.tensor([-1.0, -2.0, 1.5, 0.0])])
        brute = (q[None, :] - x[:, None]).abs().argmin(dim=1).to(torch.uint8)
        assert torch.equal(nearest(q, x), brute)


def test_fixture_is_self_consistent():
    fx = load_fixture("adamw8bit_steps")
    assert [tuple(s) for s in fx["shapes"]] == SHAPES and fx["block"] == A8_BLOCK == 256 and fx["min_8bit_size"] == 4096
    assert all(t.dtype == torch.bfloat16 for t in fx["init"]) and all(t.dtype == torch.bfloat16 for gs in fx["grads"] for t in gs)
    small = [int(torch.tensor(s).prod()) < 4096 for s in SHAPES]
    assert any(small) and not all(small)
    assert {len(s) for s in SHAPES} >= {1, 2, 4} and any(int(torch.tensor(s).prod()) % 256 for s, sm in zip(SHAPES, small) if not sm)
    for tag in ("sdxl_te", "decay"):
        c = load_adamw8bit_case(tag)
        assert c["step"] == 4 and len(c["after"]) == 4
        for s in range(4):
            assert [tuple(t.shape) for t in c["after"][s]] == SHAPES
        for shape, sm, st in zip(SHAPES, small, c["states"]):
            n = int(torch.tensor(shape).prod())
            if sm:
                assert {k: (tuple(v.shape), v.dtype) for k, v in st.items()} == {k: (shape, torch.float32) for k in ("state1", "state2")}
            else:
                nb = -(-n // 256)
                assert st["state1"].dtype == st["state2"].dtype == torch.uint8 and tuple(st["state1"].shape) == shape
                assert tuple(st["absmax1"].shape) == tuple(st["absmax2"].shape) == (nb,)
        ti, b = ZERO_BLOCK
        st = c["states"][ti]
        assert float(st["absmax1"][b]) == 0.0 and float(st["absmax2"][b]) == 0.0
        assert bool((phys(st["state1"])[b * 256:(b + 1) * 256] == 127).all()) and bool((phys(st["state2"])[b * 256:(b + 1) * 256] == 0).all())
    assert load_adamw8bit_case("decay")["kwargs"]["weight_decay"] > 0
    assert load_adamw8bit_case("sdxl_te")["kwargs"] == dict(lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


@pytest.mark.parametrize("tag", ["sdxl_te", "decay"])
def test_restatement_reproduces_the_fixture(tag):
    c = load_adamw8bit_case(tag)
    params = [phys(t) for t in c["init"]]
    states = [init_state(p.numel()) for p in params]
    for s in range(4):
        params = [restated_step(p, phys(g), st, s + 1, **c["kwargs"]) for p, g, st in zip(params, c["grads"][s], states)]
        for p, want, shape in zip(params, c["after"][s], SHAPES):
            assert torch.equal(unphys(p, shape), want), (s, shape)
    for st, want, shape in zip(states, c["states"], SHAPES):
        for k, v in want.items():
            assert torch.equal(unphys(st[k], shape) if k.startswith("state") else st[k], v), (shape, k)


def test_fp64_restatement_stays_close_to_fp32():
    """The fp64 variant (the GPU tests' oracle on larger shapes) against the fp32 fixture: a code differs only where fp32 rounding moved
    a value across a decision boundary (one adjacent code, rarely), and such a flip moves a parameter by lr times about one map gap --
    hence 1e-5 relative on the parameters (lr 1e-3 here), not the last-bit agreement of the fp32 restatement."""
    c = load_adamw8bit_case("decay")
    params = [phys(t) for t in c["init"]]
    states = [init_state(p.numel(), dtype=torch.float64) for p in params]
    for s in range(4):
        params = [restated_step(p, phys(g), st, s + 1, dtype=torch.float64, **c["kwargs"]) for p, g, st in zip(params, c["grads"][s], states)]
    for p, want, shape in zip(params, c["after"][3], SHAPES):
        assert p.dtype == torch.float64
        assert float((unphys(p, shape) - want).abs().max() / want.abs().max()) <= 1e-5, shape
    total = flips = 0
    for st, want, shape in zip(states, c["states"], SHAPES):
        for k in ("state1", "state2"):
            if want[k].dtype == torch.uint8:
                d = (unphys(st[k], shape).int() - want[k].int()).abs()
                assert int(d.max()) <= 1, (shape, k)
                total, flips = total + d.numel(), flips + int((d > 0).sum())
    assert flips <= 1e-3 * total, (flips, total)


def _engine(**kw):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models import DiffusionEngine
    from tests.golden.make_golden import UNET_TINY

    return DiffusionEngine(model=D.UNetModel(**UNET_TINY), denoiser=D.Denoiser(preconditioning=D.EpsPreconditioning()), first_stage_model=None,
                           loss_fn=None, **kw)


def test_engine_accepts_adamw8bit():
    from neurosis_amd.optimizers import AdamW8bit

    eng = _engine(optimizer=partial(AdamW8bit, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0))
    opt = eng.configure_optimizers()
    assert isinstance(opt, AdamW8bit)
    g = opt.param_groups[0]
    assert g["name"] == "UNet" and g["lr"] == 3e-5 and g["weight_decay"] == 0.0


def test_engine_refuses_adamw8bit_with_the_streamed_update():
    from neurosis_amd.optimizers import AdamW8bit

    eng = _engine(optimizer=partial(AdamW8bit, lr=1e-4))
    eng.stream_optimizer = True
    with pytest.raises(NotImplementedError, match="stream_optimizer"):
        eng.configure_optimizers()
    eng = _engine(optimizer=partial(AdamW8bit, lr=1e-4))
    eng.configure_optimizers()
    with pytest.raises(NotImplementedError, match="stream_optimizer"):
        eng.stream_optimizer = True


def test_engine_refuses_adamw8bit_with_the_sharded_exchange():
    """NK_DP_MODE=rs_ag restricts the chunked Adafactor to a shard; the 8-bit update is refused before anything runs."""
    from neurosis_amd.optimizers import AdamW8bit

    eng = _engine(optimizer=partial(AdamW8bit, lr=1e-4))
    eng.configure_optimizers()
    eng.store = SimpleNamespace()                  # stands in for the flat store: the refusal comes before it is touched
    with pytest.raises(NotImplementedError, match="rs_ag"):
        eng.optimizer_step(dp=SimpleNamespace(sharded=True))


def test_sdxl_unet_state_is_at_most_2_05_bytes_per_parameter():
    """bench.py's SDXL UNet (2.57 G parameters) on the meta device: codes, absmax and the small tensors' fp32 moments, per parameter."""
    import bench
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.optim import FlatAdamW8bit

    with torch.device("meta"):
        unet = D.UNetModel(**bench.SDXL_UNET)
    shapes = [tuple(p.shape) for p in unet.parameters() if p.requires_grad]
    n = sum(int(torch.tensor(s).prod()) for s in shapes)
    assert n > 2.5e9
    per_param = FlatAdamW8bit.state_bytes(shapes) / n
    assert per_param <= 2.05, per_param
    assert FlatAdamW8bit.state_bytes(shapes, min_8bit_size=1 << 62) == 8 * n          # all fp32: AdamW's 8 B/param
