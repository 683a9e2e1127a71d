"""neurosis_amd.optimizers.came.CAME without a GPU: the class path the reference's configs name resolves, with the reference's
constructor, defaults and validation; the options the fused update does not implement are refused; the engine accepts it.
Also the golden fixture (tests/golden/came_steps, written by make_golden_came.py from the reference class) and the fp64
restatement of the reference step that the GPU tests use as their oracle on larger shapes."""
import inspect
from functools import partial

import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.util import rel_err

SHAPES = [(48, 32), (40, 64), (300, 8), (16, 8, 3, 3), (8, 16, 1, 1), (32,), (7,), (1200,)]


def load_came_case(tag: str) -> dict:
    """One case of the came_steps fixture with the shared inputs (stored once, bf16-exact) attached in fp32: kwargs, init, grads
    (four steps), after (four steps), states (after the last step), step."""
    fx = load_fixture("came_steps")
    return {**fx[tag], "init": [t.float() for t in fx["init"]], "grads": [[t.float() for t in gs] for gs in fx["grads"]]}


def came_ref_step(p, g, st: dict, lr: float, betas=(0.9, 0.999, 0.9999), weight_decay: float = 0.0, weight_decouple: bool = True,
                  fixed_decay: bool = False, clip_threshold: float = 1.0, eps1: float = 1e-30, eps2: float = 1e-16):
    """One CAME step of one tensor (reference optimizers/came.py:136-224) in fp64; `st` holds the reference's state keys and is
    updated in place.  Returns the new parameter."""
    assert weight_decouple or weight_decay == 0.0
    p, g = p.double(), g.double()
    b1, b2, b3 = betas
    factored = p.dim() >= 2
    if not st:
        st["exp_avg"] = torch.zeros_like(p)
        if factored:
            for k in ("exp_avg_sq", "exp_avg_res"):
                st[k + "_row"] = torch.zeros(p.shape[:-1], dtype=torch.float64)
                st[k + "_col"] = torch.zeros(p.shape[:-2] + p.shape[-1:], dtype=torch.float64)
        else:
            st["exp_avg_sq"] = torch.zeros_like(p)
    st.update({k: v.double() for k, v in st.items()})

    def factor(row, col):
        return (row / row.mean(dim=-1, keepdim=True)).rsqrt().unsqueeze(-1) * col.unsqueeze(-2).rsqrt()

    q = g * g + eps1
    if factored:
        st["exp_avg_sq_row"] = b2 * st["exp_avg_sq_row"] + (1 - b2) * q.mean(dim=-1)
        st["exp_avg_sq_col"] = b2 * st["exp_avg_sq_col"] + (1 - b2) * q.mean(dim=-2)
        u = factor(st["exp_avg_sq_row"], st["exp_avg_sq_col"]) * g
    else:
        st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1 - b2) * q
        u = st["exp_avg_sq"].rsqrt() * g
    rms = u.norm() / u.numel() ** 0.5
    u = u / max(1.0, float(rms) / clip_threshold)
    st["exp_avg"] = b1 * st["exp_avg"] + (1 - b1) * u
    m = st["exp_avg"]
    if factored:
        res = (u - m) ** 2 + eps2
        st["exp_avg_res_row"] = b3 * st["exp_avg_res_row"] + (1 - b3) * res.mean(dim=-1)
        st["exp_avg_res_col"] = b3 * st["exp_avg_res_col"] + (1 - b3) * res.mean(dim=-2)
        upd = factor(st["exp_avg_res_row"], st["exp_avg_res_col"]) * m
    else:
        upd = m
    return p * (1.0 - weight_decay * (1.0 if fixed_decay else lr)) - lr * upd


def test_class_path_resolves_with_the_reference_signature():
    import importlib

    fx = load_fixture("came_steps")
    mod, name = "neurosis.optimizers.came.CAME".replace("neurosis.", "neurosis_amd.", 1).rsplit(".", 1)
    cls = getattr(importlib.import_module(mod), name)
    assert issubclass(cls, torch.optim.Optimizer)
    sig = inspect.signature(cls.__init__)
    mine = {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params")}
    assert list(mine) == list(fx["signature"]), "argument order differs from the reference's"
    assert mine == fx["signature"]
    from neurosis_amd.optimizers import CAME

    assert CAME is cls


def test_refuses_what_the_fused_update_does_not_implement():
    from neurosis_amd.optimizers.came import CAME

    p = [torch.nn.Parameter(torch.zeros(8, 8))]
    with pytest.raises(NotImplementedError, match="ams_bound"):
        CAME(p, ams_bound=True)
    with pytest.raises(NotImplementedError, match="weight_decouple"):
        CAME(p, weight_decouple=False, weight_decay=0.01)
    CAME(p, weight_decouple=False, weight_decay=0.0)      # nothing to decay: nothing refused


@pytest.mark.parametrize("kw", [dict(lr=-1e-3), dict(betas=(1.0, 0.999, 0.9999)), dict(betas=(0.9, -0.1, 0.9999)), dict(betas=(0.9, 0.999, 1.5)),
                                dict(eps1=-1e-30), dict(eps2=-1e-16), dict(weight_decay=-0.1)])
def test_reference_validation(kw):
    from neurosis_amd.optimizers.came import CAME

    with pytest.raises(ValueError):
        CAME([torch.nn.Parameter(torch.zeros(4, 4))], **kw)


def test_no_cpu_path():
    from neurosis_amd.optimizers.came import CAME

    p = torch.nn.Parameter(torch.zeros(8, 8))
    p.grad = torch.ones(8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CAME([p]).step()


def _engine(**kw):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models import DiffusionEngine
    from tests.golden.make_golden import UNET_TINY

    return DiffusionEngine(model=D.UNetModel(**UNET_TINY), denoiser=D.Denoiser(preconditioning=D.EpsPreconditioning()), first_stage_model=None,
                           loss_fn=None, **kw)


def test_engine_accepts_came():
    from neurosis_amd.optimizers.came import CAME

    eng = _engine(optimizer=partial(CAME, lr=1e-4, weight_decay=0.01))
    opt = eng.configure_optimizers()
    assert isinstance(opt, CAME)
    g = opt.param_groups[0]
    assert g["name"] == "UNet" and g["lr"] == 1e-4 and g["weight_decay"] == 0.01


def test_engine_refuses_came_with_the_streamed_update():
    from neurosis_amd.optimizers.came import CAME

    eng = _engine(optimizer=partial(CAME, lr=1e-4))
    eng.stream_optimizer = True
    with pytest.raises(NotImplementedError, match="stream_optimizer"):
        eng.configure_optimizers()
    eng = _engine(optimizer=partial(CAME, lr=1e-4))
    eng.configure_optimizers()
    with pytest.raises(NotImplementedError, match="stream_optimizer"):
        eng.stream_optimizer = True


def test_fixture_is_self_consistent():
    fx = load_fixture("came_steps")
    assert [tuple(s) for s in fx["shapes"]] == SHAPES
    assert "stand_in" in fx
    assert all(t.dtype == torch.bfloat16 for t in fx["init"]) and all(t.dtype == torch.bfloat16 for gs in fx["grads"] for t in gs)
    for tag in ("default", "decay", "fixed"):
        c = load_came_case(tag)
        assert all(t.dtype == torch.float32 for a in c["after"] for t in a)
        assert c["step"] == 4 and len(c["grads"]) == 4 and len(c["after"]) == 4
        assert [tuple(t.shape) for t in c["init"]] == SHAPES
        for s in range(4):
            assert [tuple(t.shape) for t in c["grads"][s]] == SHAPES and [tuple(t.shape) for t in c["after"][s]] == SHAPES
        for shape, st in zip(SHAPES, c["states"]):
            if len(shape) >= 2:
                want = {"exp_avg": shape, "exp_avg_sq_row": shape[:-1], "exp_avg_sq_col": shape[:-2] + shape[-1:],
                        "exp_avg_res_row": shape[:-1], "exp_avg_res_col": shape[:-2] + shape[-1:]}
            else:
                want = {"exp_avg": shape, "exp_avg_sq": shape}
            assert {k: tuple(v.shape) for k, v in st.items()} == want


@pytest.mark.parametrize("tag", ["default", "decay", "fixed"])
def test_fp64_restatement_follows_the_reference(tag):
    """The oracle of the GPU tests' larger shapes reproduces the reference's own steps (and update clipping is exercised)."""
    c = load_came_case(tag)
    params = [t.clone() for t in c["init"]]
    states = [{} for _ in params]
    for s in range(4):
        params = [came_ref_step(p, g, st, **c["kwargs"]) for p, g, st in zip(params, c["grads"][s], states)]
        for p, want in zip(params, c["after"][s]):
            assert rel_err(p, want) <= 1e-5, (s, tuple(p.shape))
    for st, want in zip(states, c["states"]):
        for k, v in want.items():
            assert rel_err(st[k], v) <= 1e-5, k
