"""conv3x3(nearest_upsample_2x(x)) as four 2 x 2 phase convolutions (ops.conv2d_fwd(upsample=True) with NK_UP2_PHASES=1: nk_up2_phase_weights,
nk_conv2d_up2_fwd / _dgrad / _wgrad_bias) against the fused-upsample gather it replaces (NK_UP2_PHASES=0) and against float64.  The shapes are
small, below the size from which the default (NK_UP2_PHASES=1) takes the phase path, so the tests ask for it with NK_UP2_PHASES=2 (every
qualifying call); tests/test_up2_phases_cpu.py checks what the default selects:

  (a) small-integer inputs: every phase sum is exact in bf16 and every product sum exact in fp32, so y, dx, dw and dbias of the two paths are
      bit-equal (and equal to the rounded float64 result), with accumulate 0 and 1;
  (b) random inputs: the phase path's largest error against float64 is at most twice the fused path's own on the same inputs (the one extra
      bf16 rounding per summed weight is the size of the shadow's rounding of the weight itself);
  (c) the Upsample module forward and backward replayed from hipGraphs, with the switch at 2 and at 0.

The index formulas of the three identities are checked in float64 on the CPU in tests/test_up2_phases_cpu.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout): one pixel; odd sizes with channel counts that are no multiple of a tile; H > W; 320 channels (whole 64-deep slabs: the
# kernels the UNet's layers run on) at 6 x 10
SHAPES = [(1, 1, 1, 8, 8), (2, 5, 7, 24, 40), (1, 9, 4, 16, 8), (1, 6, 10, 320, 320)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def tok(t):
    """NCHW -> channels-last token matrix [N*H*W, C] (bf16, on the device)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda().bfloat16()


def untok(t, N, H, W):
    return t.view(N, H, W, -1).permute(0, 3, 1, 2).double().cpu()


def cl_param(w):
    """fp32 OIHW parameter stored [O][KH][KW][I], the layout the kernels read"""
    return torch.nn.Parameter(w.float().permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2))


def reference(x, w, b, dy):
    """float64: y, dx, dw, dbias, and the input gradient on the 2x grid (what the fused path rounds before its 2 x 2 sum)"""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    b = b.double().requires_grad_(True)
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    up.retain_grad()
    y = F.conv2d(up, w, b, padding=1)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, b.grad, up.grad


def run_path(monkeypatch, phases, shape, x, w, b, dy, accumulate=False, prefill=None):
    from neurosis_amd import ops

    N, H, W, Cin, Cout = shape
    monkeypatch.setenv("NK_UP2_PHASES", phases)
    weight, bias = cl_param(w), torch.nn.Parameter(b.float().cuda())
    st = ops.EngineState()
    st.grad_accumulate = accumulate
    weight._nk_state = bias._nk_state = st
    if prefill is not None:
        weight.grad = prefill[0].float().permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
        bias.grad = prefill[1].float().cuda()
    ops.lib.launch_log(1)
    try:
        out, bwd = ops.conv2d_fwd(ops.Img(tok(x), N, H, W), weight, bias, upsample=True)
        dx, _ = bwd(tok(dy))
        names = ops.lib.launched()
    finally:
        ops.lib.launch_log(0)
    torch.cuda.synchronize()
    took = any(n == "up2_phase_weights_kernel" for n in names)
    assert took == (phases == "2"), f"NK_UP2_PHASES={phases} launched {sorted(set(names))}"
    assert (out.H, out.W, dx.H, dx.W) == (2 * H, 2 * W, H, W)
    return untok(out.t, N, 2 * H, 2 * W), untok(dx.t, N, H, W), weight.grad.double().cpu(), bias.grad.double().cpu()


def int_case(shape, seed):
    """integers: x in [-2, 2]; w and dy in {-1, 0, 1}, sparse, so that the input gradient on the 2x grid stays an integer bf16 holds (the fused
    path rounds it there); bias in [-8, 8]"""
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    sparse = lambda keep, *s: ri(-1, 1, *s) * (torch.rand(*s, generator=g) < keep)
    return ri(-2, 2, N, Cin, H, W), sparse(0.25, Cout, Cin, 3, 3), ri(-8, 8, Cout), sparse(0.125 if Cout > 64 else 1.0, N, Cout, 2 * H, 2 * W)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_integer_inputs_are_bit_equal_to_the_fused_gather(shape, accumulate, monkeypatch):
    N, H, W, Cin, Cout = shape
    x, w, b, dy = int_case(shape, 11)
    y64, dx64, dw64, db64, dup64 = reference(x, w, b, dy)
    # the exactness conditions, from the reference: the 2x-grid input gradient is exact in bf16, every sum exact in fp32
    assert float(dup64.abs().max()) <= 256 and max(float(t.abs().max()) for t in (y64, dx64, dw64, db64)) < 2 ** 23
    prefill = None
    if accumulate:
        g = torch.Generator().manual_seed(12)
        prefill = (torch.randint(-256, 257, (Cout, Cin, 3, 3), generator=g).double(), torch.randint(-256, 257, (Cout,), generator=g).double())
        dw64, db64 = dw64 + prefill[0], db64 + prefill[1]
    old = run_path(monkeypatch, "0", shape, x, w, b, dy, bool(accumulate), prefill)
    new = run_path(monkeypatch, "2", shape, x, w, b, dy, bool(accumulate), prefill)
    want = (y64.bfloat16().double(), dx64.bfloat16().double(), dw64, db64)
    for name, o, n, r in zip(("y", "dx", "dw", "dbias"), old, new, want):
        assert torch.equal(n, o), f"{name}: the phase path differs from the fused gather in {int((n != o).sum())} of {n.numel()} elements"
        assert torch.equal(n, r), f"{name}: differs from the float64 result in {int((n != r).sum())} of {n.numel()} elements"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_inputs_err_at_most_twice_the_fused_gather(shape, monkeypatch):
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(21)
    rb = lambda *s: torch.randn(*s, generator=g).bfloat16().double()       # activations: bf16 values, as the layers see them
    x, dy = rb(N, Cin, H, W), rb(N, Cout, 2 * H, 2 * W)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5).float().double()      # fp32 master weights: both paths read their bf16 shadow
    b = torch.randn(Cout, generator=g).float().double()
    ref = reference(x, w, b, dy)[:4]
    old = run_path(monkeypatch, "0", shape, x, w, b, dy)
    new = run_path(monkeypatch, "2", shape, x, w, b, dy)
    errs = {name: (float((o - r).abs().max()), float((n - r).abs().max())) for name, o, n, r in zip(("y", "dx", "dw", "dbias"), old, new, ref)}
    print("up2 max |error| against float64 (fused gather, phases)", shape, {k: (f"{a:.3e}", f"{c:.3e}") for k, (a, c) in errs.items()})
    for name, (e_old, e_new) in errs.items():
        assert e_new <= 2 * e_old, f"{name}: phases {e_new:.3e} > 2 x fused gather {e_old:.3e}"


@pytest.mark.parametrize("phases", ["2", "0"])
def test_upsample_module_replays_from_graphs(phases, monkeypatch):
    """Upsample.fwd and its backward through neurosis_amd.graphs.ChainGraphs (weight gradient on the side stream, its workspace from the side
    graph's pool): warm-up, capture and two replays with fresh inputs and moved weights, each against the eager launch of the same path"""
    from neurosis_amd import ops
    from neurosis_amd.graphs import ChainGraphs
    from neurosis_amd.modules.diffusion.openaimodel import Upsample
    from neurosis_amd.nn import FlatParamStore

    monkeypatch.setenv("NK_UP2_PHASES", phases)
    N, H, W, Cc = 2, 6, 10, 64
    torch.manual_seed(0)
    mods = []
    for _ in range(2):      # [0] replayed, [1] eager, same weights
        m = Upsample(Cc, True).cuda()
        if mods:
            m.load_state_dict(mods[0][0].state_dict())
        else:
            with torch.no_grad():
                m.conv.weight.normal_(0, (9 * Cc) ** -0.5)
                m.conv.bias.normal_()
        store = FlatParamStore(m.parameters())
        store.state.wgrad_stream = torch.cuda.Stream()
        mods.append((m, store))
    (mg, sg), (me, se) = mods
    cg = ChainGraphs(mg.conv.weight)

    def chain(m):
        def fwd(xt):
            out, b = m.fwd(ops.Img(xt, N, H, W))

            def bwd(dy):
                est = ops.state_of(m.conv.weight)
                dx, _ = b(dy)
                if est.segment_hook is not None:
                    est.segment_hook(m)
                ops.join_wgrad_stream(m.conv.weight)
                return dx.t

            return out.t, bwd

        return fwd

    g = torch.Generator().manual_seed(5)
    for step in range(4):
        xt = torch.randn(N * H * W, Cc, generator=g).cuda().bfloat16()
        dy = torch.randn(N * 4 * H * W, Cc, generator=g).cuda().bfloat16()
        for s in (sg, se):
            s.grad.fill_(float("nan"))
        y_g, bwd_g = cg.run(chain(mg), [xt])
        dx_g = bwd_g(dy)
        y_e, bwd_e = chain(me)(xt)
        dx_e = bwd_e(dy)
        torch.cuda.synchronize()
        assert torch.equal(y_g, y_e) and torch.equal(dx_g, dx_e), step
        assert torch.isfinite(sg.grad).all() and float((sg.grad - se.grad).norm() / se.grad.norm()) <= 1e-5, step
        for s in (sg, se):
            s.adamw_step(1e-2, (0.9, 0.999), 1e-8, 0.0, 1.0)        # the weights move: a replay must rebuild the phase weights from the new ones
    assert not cg.broken and next(iter(cg.pairs.values())).segments is not None and int(cg.ticks) == 3
