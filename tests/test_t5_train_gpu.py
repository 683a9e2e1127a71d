"""The T5 / ByT5 towers trained with the UNet: every parameter gradient of T5EncoderTower.train_outputs against float64 autograd of the
pure-torch restatement (tests/t5_train_ref.py, held to transformers by test_t5_train_cpu.py), and one training step of a small SDXL-shaped
engine whose conditioner is a trainable FrozenByT5Embedder.

Criterion of the tower gradients, that of test_text_encoder_train_gpu.py: the same restatement run as a bf16 step runs it (fp32 weights under
torch's bf16 autocast) against float64 gives, per parameter, a normalised max error e_bf16 and a cosine c_bf16; the HIP gradient must reach
e <= 4 e_bf16 + 2^-8 and 1 - c <= 4 (1 - c_bf16) + 1e-5.

Condition on the oracle: the fixture state is loaded with every SelfAttention.q.weight times 1 / 8.  Unscaled, these random towers
saturate their softmaxes and bf16 autocast alone is off by e_bf16 = 0.12-0.37, so the criterion would admit anything; with the factor the
v11 and wide variants give e_bf16 <= 0.021 and 1 - c_bf16 <= 2e-4, and the test asserts e_bf16 <= 0.05 and 1 - c_bf16 <= 5e-4 for every
parameter of those two before it judges the HIP gradient.  The relu variant keeps e_bf16 up to 0.27 (ReLU sign flips near zero) and is
held to the cosine criterion only (c_bf16 0.997-0.999; asserted 1 - c_bf16 <= 5e-3); its mask is pinned exactly by
test_t5_train_kernels_gpu.py."""
from functools import partial

import pytest
import torch

from tests import t5_fixture as F
from tests import t5_train_ref as ref
from tests.util import cosine, rel_err

pytestmark = pytest.mark.gpu
F64, BF16, UB = torch.float64, torch.bfloat16, 2.0 ** -8
Q_FACTOR = 0.125


def _oracle(fx, ids, up, bf16):
    dtype = torch.float32 if bf16 else F64
    state = ref.trainable_state(fx["state"], dtype, "cuda", Q_FACTOR)
    with torch.autocast("cuda", dtype=BF16, enabled=bf16):
        out = ref.encode(state, fx["config"], ids)
    out.to(dtype).backward(up.to(dtype))
    return {k: v.grad.to(F64) for k, v in state.items()}


def _tower(fx):
    from neurosis_amd.models.text_encoder.t5 import T5EncoderTower
    from neurosis_amd.nn import FlatParamStore

    tower = T5EncoderTower(**fx["config"])
    tower.load_state_dict({k: (v * Q_FACTOR if k.endswith("SelfAttention.q.weight") else v) for k, v in fx["state"].items()})
    tower = tower.cuda()
    return tower, FlatParamStore(list(tower.parameters()))


@pytest.mark.parametrize("L", [20, 200])
@pytest.mark.parametrize("name", ["v11", "wide", "relu"])
def test_tower_gradients_against_float64(name, L):
    fx = F.variant(name)
    ids = fx["cases"][str(L)]["ids"].cuda()
    up = torch.randn(*ids.shape, fx["config"]["d_model"], generator=torch.Generator().manual_seed(L)).cuda()
    ref64, ref16 = _oracle(fx, ids, up, False), _oracle(fx, ids, up, True)
    tower, store = _tower(fx)
    names = {k: p for k, p in tower.named_parameters()}
    assert "shared.weight" in names and "encoder.embed_tokens.weight" not in names, "the tied embedding is one parameter"
    assert sorted(names) == sorted(ref64)

    out = tower.train_outputs(ids)
    assert out.requires_grad and out.dtype == torch.float32 and tuple(out.shape) == tuple(up.shape)
    assert torch.equal(out.detach(), tower(ids)["last_hidden_state"]), "the training forward differs from the frozen forward"
    store.grad.fill_(float("nan"))
    out.backward(up)
    torch.cuda.synchronize()
    rows, failures = [], []
    for key, p in names.items():
        got, r = p.grad.to(F64), ref64[key]
        assert torch.isfinite(got).all(), f"{key}: non-finite gradient (an element was not written?)"
        e, c, e16, c16 = rel_err(got, r), cosine(got, r), rel_err(ref16[key], r), cosine(ref16[key], r)
        if name == "relu":
            assert 1 - c16 <= 5e-3, (key, c16)
            ratio = (1 - c) / (4 * (1 - c16) + 1e-5)
        else:
            assert e16 <= 0.05 and 1 - c16 <= 5e-4, f"{key}: the bf16 oracle itself is off by e {e16:.3g}, 1 - c {1 - c16:.3g}: the criterion would admit anything"
            ratio = max(e / (4 * e16 + UB), (1 - c) / (4 * (1 - c16) + 1e-5))
        rows.append((ratio, key, e, e16, c, c16))
        if not ratio <= 1.0:
            failures.append(key)
    rows.sort(reverse=True)
    print(f"[tower] t5 {name} L={L}: {len(rows)} parameters, worst ratio to the floor {rows[0][0]:.3g}")
    for ratio, key, e, e16, c, c16 in rows[:6]:
        print(f"[tower]   {key}: ratio {ratio:.3g}  error {e:.3e} (oracle bf16 {e16:.3e})  1-cos {1 - c:.3e} (oracle bf16 {1 - c16:.3e})")
    assert not failures, f"t5 {name} L={L}: {len(failures)} parameters beyond the floor, e.g. {failures[:6]}"


def test_tower_gradients_accumulate_and_repeat_bitwise():
    fx = F.variant("v11")
    tower, store = _tower(fx)
    ids = [fx["cases"][str(L)]["ids"].cuda() for L in (20, 77)]
    ups = [torch.randn(*i.shape, 64, generator=torch.Generator().manual_seed(n)).cuda() for n, i in enumerate(ids)]

    def grads(n, accumulate):
        store.state.grad_accumulate = accumulate
        tower.train_outputs(ids[n]).backward(ups[n])
        torch.cuda.synchronize()
        store.state.grad_accumulate = False
        return store.grad.clone()

    store.grad.fill_(float("nan"))
    a = grads(0, False)
    assert torch.isfinite(a).all() and torch.equal(grads(0, False), a), "the same micro-batch twice: the same bits"
    b = grads(1, False)
    grads(0, False)
    both = grads(1, True)
    assert torch.allclose(both, a + b, rtol=1e-6, atol=1e-6 * float((a.abs() + b.abs()).max()))
    grads(0, False)
    assert torch.equal(grads(1, True), both), "two accumulated micro-batches repeat bitwise"
    assert tower.shared.weight.grad is tower.encoder.embed_tokens.weight.grad and len(store.params) == len(list(tower.parameters()))


# ================================================================================================================================
# engine
# ================================================================================================================================
def _engine(optimizer, trainable=True):
    """a small SDXL-shaped engine whose conditioner is a FrozenByT5Embedder over the v11 fixture (vocabulary 384, crossattn width 64)"""
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models.diffusion import DiffusionEngine
    from neurosis_amd.models.text_encoder import FrozenByT5Embedder
    from neurosis_amd.modules.encoders.embedding import GeneralConditioner

    fx = F.variant("v11")
    torch.manual_seed(0)
    cfg = dict(in_channels=4, model_channels=32, out_channels=4, num_res_blocks=1, attention_resolutions=[2], channel_mult=[1, 2], num_head_channels=16,
               use_linear_in_transformer=True, transformer_depth=1, context_dim=64, use_checkpoint=False)
    flags = dict(is_trainable=True, freeze=False, base_lr=1.0) if trainable else {}
    byt5 = FrozenByT5Embedder(config=fx["config"], max_length=20, input_key="caption", **flags)
    byt5.model.load_state_dict({k: (v * Q_FACTOR if k.endswith("SelfAttention.q.weight") else v) for k, v in fx["state"].items()})
    net = D.UNetModel(**cfg)
    with torch.no_grad():
        for p in net.parameters():                   # (zero_module'd outputs would give the conditioning no gradient at all)
            if p.dim() >= 2 and not p.abs().sum():
                p.normal_(std=0.05)
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=None, conditioner=GeneralConditioner([byt5]), optimizer=optimizer,
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting()))
    eng = eng.cuda()
    eng.setup_flat_params()
    return eng


def _step(eng, seed):
    g = torch.Generator().manual_seed(seed)
    ids = F.variant("v11")["cases"]["20"]["ids"].cuda()
    x, noise = torch.randn(2, 4, 16, 16, generator=g).cuda(), torch.randn(2, 4, 16, 16, generator=g).cuda()
    eng.accumulate(0)
    loss = eng(x, {"caption": ids}, sigmas=torch.tensor([0.5, 3.0]).cuda(), noise=noise)
    loss.mean().backward()
    torch.cuda.synchronize()
    return loss.detach()


def test_engine_step_trains_the_byt5_tower():
    """one step of AdamW8bit over two groups (UNet, ByT5): the tower's store gets finite nonzero gradients from the UNet's d(context), the
    update moves every trained parameter of tower and UNet, and the same step from the same state repeats bitwise"""
    from neurosis_amd.optimizers import AdamW8bit

    results = []
    for _ in range(2):
        eng = _engine(partial(AdamW8bit, lr=1e-3, weight_decay=0.01))
        opt = eng._torch_optimizer
        assert [g["name"] for g in opt.param_groups] == ["UNet", "FrozenByT5Embedder"]
        tower_store, = eng.embedder_stores
        byt5, = eng.conditioner.embedders
        assert len(tower_store.params) == len(list(byt5.model.parameters())) == len(byt5.trained_parameters())
        tower_store.grad.fill_(float("nan"))
        loss = _step(eng, 40)
        assert torch.isfinite(tower_store.grad).all() and float(tower_store.grad.abs().max()) > 0
        for p, o in zip(tower_store.params, tower_store.offsets):
            assert float(tower_store.grad[o:o + p.numel()].abs().max()) > 0, "a tower parameter without a gradient"
        stores = [eng.store, tower_store]
        before = [s.master.clone() for s in stores]
        eng.optimizer_step()
        eng.join_optimizer()
        torch.cuda.synchronize()
        for s, m in zip(stores, before):
            moved = [not torch.equal(p.detach(), m[o:o + p.numel()].view(p.shape)) for p, o in zip(s.params, s.offsets)]
            assert all(moved), "a trained parameter did not move"
        results.append((loss.clone(), [s.grad.clone() for s in stores], [s.master.clone() for s in stores]))
    (l0, g0, m0), (l1, g1, m1) = results
    assert torch.equal(l0, l1) and all(torch.equal(a, b) for a, b in zip(g0 + m0, g1 + m1)), "the same step from the same state differs"


def test_frozen_byt5_embedder_in_the_engine_behaves_as_before():
    """freeze=True and no is_trainable: no tower store, no tower group, the conditioning carries no gradient and the tower does not move"""
    from neurosis_amd.optimizers import AdamW8bit

    eng = _engine(partial(AdamW8bit, lr=1e-3, weight_decay=0.01), trainable=False)
    byt5, = eng.conditioner.embedders
    assert eng.embedder_stores == [] and eng.trainable_embedders() == []
    assert [g["name"] for g in eng._torch_optimizer.param_groups] == ["UNet"]
    before = [p.detach().clone() for p in byt5.parameters()]
    ids = F.variant("v11")["cases"]["20"]["ids"].cuda()
    z = byt5(ids)
    assert not z.requires_grad and torch.equal(z, byt5.model(ids)["last_hidden_state"])
    _step(eng, 40)
    assert all(p.grad is None for p in byt5.parameters())
    eng.optimizer_step()
    eng.join_optimizer()
    torch.cuda.synchronize()
    assert all(torch.equal(p.detach(), b) for p, b in zip(byt5.parameters(), before))
