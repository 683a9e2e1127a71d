"""Class-conditional UNets on the GPU: the label kernels (nk_label_rows_fwd / _bwd, nk_linear1_fwd / _bwd) per element against float64, the
three tiny UNets and the ClassEmbedder engine step against fixtures captured from the reference (tests/golden/make_golden_labels.py).

Bounds.  The lookups copy (fp32 out) or add once and round once (bf16 out): bit-equal to the same two torch operations.  A class's gradient
row is an fp32 sum of its n_v samples' rows in a fixed order: |err| <= n_v * 2^-24 * sum |terms| (the summation bound; one term is exact).
linear1: the forward is one bf16 rounding (2^-9 relative) plus fp32 noise on a sum of three terms, held to 2^-8 * (|y w| + |b| + |add|); the
sums over b (dw, db) and over j (dy) to B resp. D times 2^-23 of their sum of absolute terms (product rounding and summation together).
The UNets are held to what tests/test_adm_gpu.py holds its tiny UNets to."""
import os
from functools import partial

import pytest
import torch

from tests.golden.fixture_io import load_fixture
from tests.golden.make_golden import block_upstream, synth_state_dict
from tests.golden.make_golden_labels import LABEL_KINDS, class_engine_inputs, label_inputs
from tests.util import check_grad_cosines, cosine, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
ROW_CASES = [(1, 1, 8), (6, 10, 40), (64, 1000, 1280)]
LIN_CASES = [(1, 8), (5, 40), (64, 1280)]


@pytest.fixture(scope="module")
def ops():
    from neurosis_amd import ops as o

    return o


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t


def _param(ops, t, accumulate=False, prefill=float("nan")):
    """a free parameter with an engine state of its own and garbage in its gradient"""
    p = torch.nn.Parameter(t.cuda())
    p._nk_state = ops.EngineState()
    p._nk_state.grad_accumulate = accumulate
    p.grad = torch.full_like(p, prefill)
    return p


# ------------------------------------------------------------------------------------------------
# 1. label_rows
# ------------------------------------------------------------------------------------------------
_rows = {}


def _row_case(B, V, D):
    key = (B, V, D)
    if key not in _rows:
        g = torch.Generator().manual_seed(B * 7 + V * 3 + D)
        if key == (6, 10, 40):
            ids = torch.tensor([3, 0, 3, 9, 3, 0])
        elif B == 1:
            ids = torch.zeros(1, dtype=torch.int64)
        else:
            ids = torch.randint(0, V, (B,), generator=g)
            ids[:6] = torch.tensor([0, V - 1, 17, 17, V - 1, 17])
        c = dict(ids=ids.cuda(), table=torch.randn(V, D, generator=g).cuda(), add=torch.randn(B, D, generator=g).to(BF).cuda())
        for tag in ("d", "d2"):
            c[tag] = torch.randn(B, D, generator=g).cuda()
        c["ids2"] = ids.flip(0).roll(1).cuda() if B > 1 else ids.cuda()
        for tag, i in (("d", "ids"), ("d2", "ids2")):
            for dt in (torch.float32, BF):
                dd = c[tag].to(dt).double()
                ref = torch.zeros(V, D, dtype=F64, device="cuda").index_add_(0, c[i], dd)
                mag = torch.zeros(V, D, dtype=F64, device="cuda").index_add_(0, c[i], dd.abs())
                c[(tag, dt)] = (ref, mag, torch.bincount(c[i], minlength=V))
        _rows[key] = c
    return _rows[key]


@pytest.mark.parametrize("B,V,D", ROW_CASES)
def test_label_rows_forward_is_the_lookup_bit_for_bit(ops, B, V, D):
    c = _row_case(B, V, D)
    ids, table, add = c["ids"], c["table"], c["add"]
    if B > 1:
        assert 0 in ids.tolist() and V - 1 in ids.tolist() and len(set(ids.tolist())) < B
    out = ops.label_rows(table, ids)
    assert out.dtype == torch.float32 and torch.equal(out, table[ids])
    got = ops.label_rows(table, ids, add=add, out_dtype=BF)
    assert got.dtype == BF and torch.equal(bits(got), bits((table[ids] + add.float()).bfloat16()))
    for bad in (V, -1):        # an id outside the table: never an address, a NaN row, the others untouched
        for pos in {0, B - 1}:
            wrong = ids.clone()
            wrong[pos] = bad
            keep = torch.arange(B, device="cuda") != pos
            for o, want in ((ops.label_rows(table, wrong), out), (ops.label_rows(table, wrong, add=add, out_dtype=BF), got)):
                assert bool(torch.isnan(o[pos]).all()) and torch.equal(bits(o[keep]), bits(want[keep]))


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,V,D", ROW_CASES)
def test_label_rows_backward_against_float64(ops, B, V, D, dtype):
    c = _row_case(B, V, D)
    ids, d = c["ids"], c["d"].to(dtype)
    ref, mag, count = c[("d", dtype)]
    table = _param(ops, c["table"])
    ops.label_rows_bwd(ids, d, table)
    first = table.grad.clone()
    err = (first.double() - ref).abs()
    bound = count[:, None].double() * 2.0 ** -24 * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"[label_rows_bwd B {B} V {V} D {D} {dtype}] worst error / bound {worst:.3f}, most samples on one class {int(count.max())}")
    assert bool((err <= bound).all())
    assert torch.count_nonzero(first[count == 0]) == 0 and not torch.isnan(first).any()
    table.grad.fill_(float("nan"))
    ops.label_rows_bwd(ids, d, table)
    assert torch.equal(table.grad, first), "the same call twice: the same bits"
    # accumulate: the second batch's sums are formed first and added once -- the fp32 sum of the two overwrite results
    ids2, d2 = c["ids2"], c["d2"].to(dtype)
    other = _param(ops, c["table"])
    ops.label_rows_bwd(ids2, d2, other)
    table._nk_state.grad_accumulate = True
    ops.label_rows_bwd(ids2, d2, table)
    assert torch.equal(table.grad, first + other.grad)
    with pytest.raises(NotImplementedError, match="at most 8192 samples"):
        ops.label_rows_bwd(torch.zeros(8193, dtype=torch.int64, device="cuda"), torch.zeros(8193, D, dtype=dtype, device="cuda"), table)


# ------------------------------------------------------------------------------------------------
# 2. linear1
# ------------------------------------------------------------------------------------------------
_lins = {}


def _lin_case(B, D):
    if (B, D) not in _lins:
        g = torch.Generator().manual_seed(B * 5 + D)
        r = lambda *s: torch.randn(*s, generator=g)
        c = dict(y=r(B, 1), w=r(D, 1), b=r(D) * 0.3, add=r(B, D).to(BF), d=r(B, D).to(BF), y2=r(B, 1), d2=r(B, D).to(BF))
        c = {k: v.cuda() for k, v in c.items()}
        y, w, b, add = c["y"].double(), c["w"].double(), c["b"].double(), c["add"].double()
        c["out"], c["out_mag"] = y * w.t() + b + add, (y * w.t()).abs() + b.abs() + add.abs()
        c["out_plain"], c["plain_mag"] = y * w.t() + b, (y * w.t()).abs() + b.abs()
        for t, (yy, dd) in (("", (y, c["d"].double())), ("2", (c["y2"].double(), c["d2"].double()))):
            c["dw" + t], c["dw_mag" + t] = (yy * dd).sum(0)[:, None], (yy * dd).abs().sum(0)[:, None]
            c["db" + t], c["db_mag" + t] = dd.sum(0), dd.abs().sum(0)
            c["dy" + t], c["dy_mag" + t] = (dd * w.t()).sum(1, keepdim=True), (dd * w.t()).abs().sum(1, keepdim=True)
        _lins[(B, D)] = c
    return _lins[(B, D)]


def _lin_run(ops, c, w, b, second=False, add=True, need_dy=True):
    y, d = (c["y2"], c["d2"]) if second else (c["y"], c["d"])
    out, bwd = ops.linear1_fwd(y, w, b, add=c["add"] if add else None, need_dy=need_dy)
    return out, bwd(d)


@pytest.mark.parametrize("B,D", LIN_CASES)
def test_linear1_against_float64(ops, B, D):
    c = _lin_case(B, D)
    w, b = _param(ops, c["w"]), _param(ops, c["b"])
    b._nk_state = w._nk_state
    out, dy = _lin_run(ops, c, w, b)
    plain, none = _lin_run(ops, c, w, b, add=False, need_dy=False)
    assert none is None and out.dtype == BF and dy.dtype == torch.float32 and tuple(dy.shape) == (B, 1)
    checks = [("out", out, c["out"], 2.0 ** -8 * c["out_mag"]), ("out without add", plain, c["out_plain"], 2.0 ** -8 * c["plain_mag"]),
              ("dw", w.grad, c["dw"], B * 2.0 ** -23 * c["dw_mag"]), ("db", b.grad, c["db"], B * 2.0 ** -23 * c["db_mag"]),
              ("dy", dy, c["dy"], D * 2.0 ** -23 * c["dy_mag"])]
    for name, got, ref, bound in checks:
        err = (got.double() - ref).abs()
        print(f"[linear1 B {B} D {D}] {name}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert got.shape == ref.shape and bool((err <= bound).all()), name
    first = (out.clone(), dy.clone(), w.grad.clone(), b.grad.clone())
    w.grad.fill_(float("nan"))
    b.grad.fill_(float("nan"))
    again = _lin_run(ops, c, w, b) + (w.grad, b.grad)
    assert all(torch.equal(bits(u), bits(v)) for u, v in zip(first, again)), "the same call twice: the same bits"
    # accumulate: the fp32 sum of the two overwrite results
    w2, b2 = _param(ops, c["w"]), _param(ops, c["b"])
    b2._nk_state = w2._nk_state
    _lin_run(ops, c, w2, b2, second=True)
    w._nk_state.grad_accumulate = True
    _lin_run(ops, c, w, b, second=True)
    assert torch.equal(w.grad, first[2] + w2.grad) and torch.equal(b.grad, first[3] + b2.grad)


# ------------------------------------------------------------------------------------------------
# 3. the three tiny UNets
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unets():
    return {kind: load_fixture(f"unet_labels_tiny_{kind}") for kind in LABEL_KINDS}


def _unet(fx, store=False):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.nn import FlatParamStore

    net = D.UNetModel(**fx["cfg"])
    res = net.load_state_dict(synth_state_dict(fx["shapes"]))
    assert not res.missing_keys and not res.unexpected_keys
    net = net.cuda()
    return net, (FlatParamStore(net.parameters()) if store else None)


@pytest.mark.parametrize("store", [True, False], ids=["flat_store", "free_params"])
@pytest.mark.parametrize("kind", list(LABEL_KINDS))
def test_tiny_unets_against_the_reference(unets, kind, store):
    """tests/test_adm_gpu.py::_check_unet_against_the_reference's bounds: output rel <= 3e-2 and cosine >= 0.999, gradient cosines >= 0.9985
    (matrices) / 0.997 (vectors), gradient norms within 5e-2 relative + 5e-4, the analytically-zero gradients within twice the bf16 rounding
    noise the fixture holds for them.  Every label_emb.* gradient is compared whole."""
    fx = unets[kind]
    net, st = _unet(fx, store)
    if st is not None:
        st.grad.fill_(float("nan"))
    ins = {k: v.cuda() for k, v in label_inputs(kind).items()}
    if kind == "continuous":
        ins["y"].requires_grad_(True)
    f = net(ins["x"], ins["timesteps"], ins["context"], ins["y"])
    print(f"[labels unet {kind}] output rel {rel_err(f, fx['F_out']):.3e} cosine {cosine(f, fx['F_out']):.6f}")
    assert f.shape == fx["F_out"].shape and rel_err(f, fx["F_out"]) <= 3e-2 and cosine(f, fx["F_out"]) >= 0.999
    f.backward(block_upstream("unet_adm_tiny", f.shape).cuda())
    torch.cuda.synchronize()
    grads = dict(net.named_parameters())
    zero = fx["bf16_zero_grad_noise"]
    refs = {**fx["grads"], **fx["label_grads"]}
    assert all(k in refs for k in grads if k.startswith("label_emb."))
    check_grad_cosines(f"labels unet {kind}", grads, refs, floor_matrix=0.9985, floor_vector=0.997, keep=lambda k, g: k not in zero)
    bad, worst_rel, worst_zero = [], 0.0, 0.0
    for k, n in fx["grad_norms"].items():
        mine = float(grads[k].grad.float().norm())
        if k in zero:
            worst_zero = max(worst_zero, mine / zero[k])
            if mine > 2.0 * zero[k]:
                bad.append((k, mine, n, zero[k]))
            continue
        worst_rel = max(worst_rel, abs(mine - n) / n)
        if abs(mine - n) > 5e-2 * n + 5e-4:
            bad.append((k, mine, n))
    print(f"[labels unet {kind}] gradient norms: worst relative deviation {worst_rel:.3e}; analytically-zero gradients: at most {worst_zero:.2f} x "
          f"the bf16 rounding noise of the reference's gradient")
    assert not bad, bad[:8]
    if kind == "int":
        g = net.label_emb.weight.grad
        absent = [v for v in range(10) if v != 3]
        assert torch.count_nonzero(g[absent]) == 0 and float(g[3].abs().max()) > 0
        assert ins["y"].grad is None
    if kind == "continuous":
        dy = ins["y"].grad
        print(f"[labels unet continuous] d_y {dy.flatten().tolist()} reference {fx['d_y'].flatten().tolist()} cosine {cosine(dy, fx['d_y']):.6f}")
        assert dy.shape == fx["d_y"].shape and cosine(dy, fx["d_y"]) >= 0.997


def _need_dy_of(kind):
    """what the chain's backward returns for y when asked (need_dy): dy [B, 1] for the continuous kind, None for ids and the timestep kind"""
    return kind == "continuous"


@pytest.mark.parametrize("kind", list(LABEL_KINDS))
def test_need_dy_of_the_chain(ops, unets, kind):
    from neurosis_amd.nn import as_tokens

    net, _ = _unet(unets[kind])
    ins = {k: v.cuda() for k, v in label_inputs(kind).items()}
    fired = []
    net.grad_ready_hook = fired.append
    img = ops.Img(ops.nchw_to_tokens(ins["x"], 8), 2, 16, 24)
    out, bwd = net.fwd(img, ins["timesteps"], as_tokens(ins["context"]), ins["y"], need_dy=True)
    dx, dctx, dy = bwd(ops.nchw_to_tokens(block_upstream("unet_adm_tiny", (2, 4, 16, 24)).cuda(), out.C))
    torch.cuda.synchronize()
    assert dctx is None
    if _need_dy_of(kind):
        assert dy.dtype == torch.float32 and tuple(dy.shape) == (2, 1) and cosine(dy, unets[kind]["d_y"]) >= 0.997
    else:
        assert dy is None
    assert sum(m is net.label_emb for m in fired) == 1 and fired.index(net.label_emb) + 1 == fired.index(net.time_embed)


def _step_labels(kind, i):
    """the label input of step i: another one every step, so that a replay which kept the captured y is caught"""
    if kind == "int":
        return torch.tensor([[3, 3], [1, 7], [0, 9], [7, 1]][i])
    g = torch.Generator().manual_seed(100 + i)
    return torch.randn(2, 1, generator=g) if kind == "continuous" else torch.rand(2, generator=g) * 900.0


def _graph_steps(fx, kind, graph: bool, n=4):
    import neurosis_amd.modules.diffusion as D

    os.environ["NK_GRAPH"] = "1" if graph else "0"
    try:
        net, store = _unet(fx, store=True)
        store.state.wgrad_stream = torch.cuda.Stream()
        den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
        lossfn = D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())
        ins = label_inputs(kind)
        g = torch.Generator().manual_seed(7)
        losses, grads, replays = [], [], []
        for i in range(n):
            x, noise = torch.randn(ins["x"].shape, generator=g).cuda(), torch.randn(ins["x"].shape, generator=g).cuda()
            loss = lossfn._forward(D.OpenAIWrapper(net), den, {"crossattn": ins["context"].cuda(), "vector": _step_labels(kind, i).cuda()}, x, {},
                                   sigmas=torch.tensor([0.5, 3.0]).cuda(), noise=noise)
            loss.mean().backward()
            torch.cuda.synchronize()
            losses.append(loss.detach().clone())
            grads.append(store.grad.clone())
            replays.append(net._nk_graphs.replays if net._nk_graphs is not None else 0)
            store.adamw_step(1e-3, (0.9, 0.999), 1e-8, 0.0, 1.0)
        return losses, grads, replays
    finally:
        os.environ.pop("NK_GRAPH", None)


@pytest.mark.parametrize("kind", list(LABEL_KINDS))
def test_graph_replay_equals_the_eager_chain_with_y_changing(unets, kind):
    """tests/test_adm_gpu.py::test_tiny_unet_graph_replay_equals_the_eager_chain with another y at every step: y is a graph input"""
    fx = unets[kind]
    loss_g, grad_g, replays = _graph_steps(fx, kind, True)
    loss_e, grad_e, replays_e = _graph_steps(fx, kind, False)
    assert replays_e == [0] * 4 and replays[0] == 0 and replays[2] > replays[1] > 0 and replays[3] > replays[2]
    for i in range(4):
        assert torch.equal(loss_g[i], loss_e[i]), (i, loss_g[i].tolist(), loss_e[i].tolist())
        d = float((grad_g[i] - grad_e[i]).norm() / grad_e[i].norm())
        print(f"[labels unet {kind} graphs] step {i + 1}: loss {loss_g[i].tolist()} flat gradient relative distance to the eager chain {d:.3e}")
        assert d <= 1e-5 and float(grad_e[i].norm()) > 0, (i, d)
    assert not torch.equal(loss_e[2], loss_e[3])


@pytest.mark.parametrize("kind", list(LABEL_KINDS))
def test_two_micro_batches_accumulate_into_the_label_parameters(unets, kind):
    net, store = _unet(unets[kind], store=True)
    ins = {k: v.cuda() for k, v in label_inputs(kind).items()}
    dout = block_upstream("unet_adm_tiny", (2, 4, 16, 24)).cuda()
    labels = [net.label_emb.weight] if kind != "timestep" else list(net.label_emb.parameters())
    if kind == "continuous":
        labels.append(net.label_emb.bias)

    def micro(i, accumulate):
        store.state.grad_accumulate = accumulate
        net(ins["x"], ins["timesteps"], ins["context"], _step_labels(kind, i + 1).cuda()).backward(dout)
        torch.cuda.synchronize()
        return [p.grad.clone() for p in labels]

    store.grad.fill_(float("nan"))
    a, b = micro(0, False), micro(1, False)
    micro(0, False)
    both = micro(1, True)
    store.state.grad_accumulate = False
    for p, ga, gb, gab in zip(labels, a, b, both):
        scale = float((ga.abs() + gb.abs()).max())
        assert scale > 0 and float((gab - (ga + gb)).abs().max()) <= 1e-5 * scale, "the second micro-batch must add"
        assert float((gab - gb).abs().max()) > 1e-3 * scale, "the second micro-batch overwrote the first"
    if kind == "int":     # classes 1, 7 (first), 0, 9 (second): every other row stays exactly zero
        assert torch.count_nonzero(both[0][[2, 3, 4, 5, 6, 8]]) == 0


# ------------------------------------------------------------------------------------------------
# 4. the fused route against the generic route, and the captured sampler step
# ------------------------------------------------------------------------------------------------
def test_fused_loss_route_against_the_generic_route(unets):
    import neurosis_amd.modules.diffusion as D

    class Generic(D.OpenAIWrapper):          # the denoiser's own route: UNetModel.forward behind Denoiser.forward
        def fused_unet(self, *a, **k):
            return None

    net, _ = _unet(unets["int"])
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
    lossfn = D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())
    ins = label_inputs("int")
    g = torch.Generator().manual_seed(3)
    x, noise = torch.randn(ins["x"].shape, generator=g).cuda(), torch.randn(ins["x"].shape, generator=g).cuda()
    cond = {"crossattn": ins["context"].cuda(), "vector": torch.tensor([3, 8]).cuda()}
    res = {}
    for name, wrapper in (("fused", D.OpenAIWrapper), ("generic", Generic)):
        for p in net.parameters():
            p.grad = None
        loss = lossfn._forward(wrapper(net), den, cond, x, {}, sigmas=torch.tensor([0.5, 3.0]).cuda(), noise=noise)
        loss.mean().backward()
        torch.cuda.synchronize()
        res[name] = (loss.detach().clone(), net.label_emb.weight.grad.clone())
    (lf, gf), (lg, gg) = res["fused"], res["generic"]
    print(f"[labels routes] loss fused {lf.tolist()} generic {lg.tolist()} rel {rel_err(lf, lg):.3e}; label gradient cosine {cosine(gf, gg):.6f}")
    assert rel_err(lf, lg) <= 3e-2 and cosine(lf, lg) >= 0.999
    assert cosine(gf, gg) >= 0.9985 and torch.count_nonzero(gf[[0, 1, 2, 4, 5, 6, 7, 9]]) == 0


def test_captured_euler_step_reloads_the_class_ids(unets):
    import neurosis_amd.modules.diffusion as D
    import neurosis_amd.modules.diffusion.sampling as S
    from neurosis_amd.modules.guidance import VanillaCFG

    net, _ = _unet(unets["int"])
    wrapped = D.OpenAIWrapper(net.eval())
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization()).cuda()
    ins = label_inputs("int")
    ctx = ins["context"].cuda()
    cond, uc = {"crossattn": ctx, "vector": torch.tensor([3, 8]).cuda()}, {"crossattn": torch.zeros_like(ctx), "vector": torch.tensor([9, 9]).cuda()}
    cond2 = dict(cond, vector=torch.tensor([5, 0]).cuda())
    guider = VanillaCFG(3.0)
    x = ins["x"].cuda()
    sig = [torch.full((2,), v, device="cuda") for v in (2.5, 1.4, 0.7)]
    res = {}
    with torch.no_grad():
        for use_graph in (False, True):
            fused = S.FusedDenoiser(wrapped, den, use_graph=use_graph)
            assert fused.supports(x, guider, cond)
            x1 = fused.euler(x, sig[0], sig[1], cond, uc, guider).clone()
            x2 = fused.euler(x1.clone(), sig[1], sig[2], cond2, uc, guider).clone()
            stale = fused.euler(x1.clone(), sig[1], sig[2], cond, uc, guider).clone()
            res[use_graph] = (x1, x2, stale)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res[False], res[True]))
    assert not torch.equal(res[True][1], res[True][2]), "the second step's class ids must matter"


# ------------------------------------------------------------------------------------------------
# 5. ClassEmbedder through the engine
# ------------------------------------------------------------------------------------------------
def _engine(fx, trainable=True):
    import neurosis_amd.modules.diffusion as D
    from neurosis_amd.models.diffusion import DiffusionEngine
    from neurosis_amd.modules.encoders import ClassEmbedder, GeneralConditioner, PrecomputedEmbedder
    from neurosis_amd.optimizers import AdamW

    net = D.UNetModel(**fx["unet_cfg"])
    net.load_state_dict(synth_state_dict(fx["unet_shapes"]))
    emb = ClassEmbedder(**{**fx["embedder"], "is_trainable": trainable})
    emb.load_state_dict(synth_state_dict(fx["embedder_shapes"]))
    den = D.DiscreteDenoiser(preconditioning=D.EpsPreconditioning(), num_idx=1000, discretization=D.LegacyDDPMDiscretization())
    eng = DiffusionEngine(model=net, denoiser=den, first_stage_model=None, conditioner=GeneralConditioner([emb, PrecomputedEmbedder(input_key="crossattn")]),
                          optimizer=partial(AdamW, lr=1e-2, weight_decay=0.0),
                          loss_fn=D.StandardDiffusionLoss(sigma_generator=D.InjectedSigmaGenerator(), loss_weighting=D.EpsWeighting())).cuda()
    eng.setup_flat_params()
    return eng, emb


def _engine_loss(eng, fx):
    ins = class_engine_inputs()
    eng.accumulate(0)
    return eng(ins["x"].cuda(), {"cls": fx["cls"].cuda(), "crossattn": ins["context"].cuda()}, sigmas=fx["sigma"].cuda(), noise=fx["noise"].cuda())


def test_class_embedder_trains_through_the_engine():
    fx = load_fixture("class_engine_tiny")
    eng, emb = _engine(fx)
    store, = eng.embedder_stores
    assert [g["name"] for g in eng._torch_optimizer.param_groups] == ["UNet", "ClassEmbedder"]
    assert len(store.params) == 1 and store.params[0] is emb.embedding.weight
    out = emb(fx["cls"].cuda())
    assert out.requires_grad and out.dtype == torch.float32 and torch.equal(out.detach(), emb.embedding.weight.detach()[fx["cls"].cuda()])
    store.grad.fill_(float("nan"))
    loss = _engine_loss(eng, fx)
    loss.mean().backward()
    torch.cuda.synchronize()
    print(f"[class engine] loss {loss.tolist()} reference {fx['loss'].tolist()} rel {rel_err(loss, fx['loss']):.3e}")
    assert rel_err(loss, fx["loss"]) <= 3e-2
    g, ref = emb.embedding.weight.grad, fx["d_embedding"]
    hit = sorted(set(fx["cls"].tolist()))
    absent = [v for v in range(fx["embedder"]["n_classes"]) if v not in hit]
    assert hit == [2, 7, 10]
    for v in hit:
        print(f"[class engine] d embedding row {v}: cosine {cosine(g[v], ref[v]):.6f} norm {float(g[v].norm()):.5f} reference {float(ref[v].norm()):.5f}")
        assert cosine(g[v], ref[v]) >= 0.997
    assert torch.count_nonzero(g[absent]) == 0 and not torch.isnan(g).any()
    before = emb.embedding.weight.detach().clone()
    unet_before = eng.store.master.clone()
    eng.optimizer_step()
    eng.join_optimizer()
    torch.cuda.synchronize()
    after = emb.embedding.weight.detach()
    assert torch.equal(after[absent], before[absent]), "rows of absent classes must not move"
    assert all(not torch.equal(after[v], before[v]) for v in hit) and not torch.equal(eng.store.master, unet_before)

    # the same embedder frozen: the same loss bits, no store, no group
    frozen, femb = _engine(fx, trainable=False)
    assert frozen.embedder_stores == [] and [g["name"] for g in frozen._torch_optimizer.param_groups] == ["UNet"]
    floss = _engine_loss(frozen, fx)
    assert not femb(fx["cls"].cuda()).requires_grad
    assert torch.equal(floss.detach(), loss.detach())
    floss.mean().backward()
    assert femb.embedding.weight.grad is None


def test_class_embedder_sequence_dim_and_dispatcher_ops(ops):
    import neurosis_amd.torch_ops  # noqa: F401  (registers the namespace)
    from neurosis_amd.modules.encoders import ClassEmbedder, GeneralConditioner

    emb = ClassEmbedder(embed_dim=48, n_classes=11, input_key="cls", add_sequence_dim=True, is_trainable=True).cuda()
    ids = torch.tensor([7, 2, 7, 10]).cuda()
    cond = GeneralConditioner([emb])({"cls": ids})
    assert list(cond) == ["crossattn"] and tuple(cond["crossattn"].shape) == (4, 1, 48)
    up = torch.randn(4, 1, 48, generator=torch.Generator().manual_seed(1)).cuda()
    cond["crossattn"].backward(up)
    want = torch.zeros(11, 48, device="cuda").index_add_(0, ids[[1, 3]], up[[1, 3], 0])
    want[7] = up[0, 0] + up[2, 0]
    assert torch.equal(emb.embedding.weight.grad, want)
    o = torch.ops.neurosis_hip
    table = emb.embedding.weight.detach().clone().requires_grad_(True)
    y = o.label_rows(table, ids)
    y.backward(up[:, 0].contiguous())
    assert torch.equal(y.detach(), table.detach()[ids]) and torch.equal(table.grad, want)
    c = _lin_case(5, 40)
    yy, w, b = c["y"].clone().requires_grad_(True), c["w"].clone().requires_grad_(True), c["b"].clone().requires_grad_(True)
    out = o.linear1(yy, w, b, c["add"])
    out.backward(c["d"])
    ref, _ = ops.linear1_fwd(c["y"], _param(ops, c["w"]), _param(ops, c["b"]), add=c["add"])
    assert torch.equal(bits(out.detach()), bits(ref))
    for got, key, terms in ((w.grad, "dw", 5), (b.grad, "db", 5), (yy.grad, "dy", 40)):
        assert got.shape == c[key].shape and bool(((got.double() - c[key]).abs() <= terms * 2.0 ** -23 * c[key + "_mag"]).all()), key
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        t, i = torch.empty(11, 48, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")
        assert o.label_rows(t, i).shape == (4, 48) and o.label_rows(t, i, None, False).dtype == BF
        assert o.linear1(torch.empty(4, 1, device="cuda"), torch.empty(48, 1, device="cuda"), torch.empty(48, device="cuda")).shape == (4, 48)
