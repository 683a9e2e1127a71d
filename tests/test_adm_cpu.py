"""The ADM block family without a GPU: the float64 restatement (tests/adm_ref.py) against fixtures captured from the reference's own ResBlock
(tests/golden/make_golden_adm.py), its closed-form backward against autograd, and the mirrored classes' constructors and state_dict keys.

Bounds of (a) are those of test_blocks_real_width.py::test_oracle_matches_the_reference_blocks: 2e-5 on outputs, 2e-4 on gradients."""
import pytest
import torch

from tests import adm_ref as R
from tests.golden.fixture_io import load_fixture
from tests.golden.make_golden import BLOCK_SAMPLE_ROWS, block_inputs, block_upstream, synth_state_dict
from tests.golden.make_golden_adm import ADM_BLOCK_CASES, CONV_SAMPLE_CIN
from tests.util import rel_err


@pytest.fixture(scope="module")
def blocks():
    return load_fixture("adm_blocks")


@pytest.fixture(scope="module")
def unets():
    return load_fixture("unet_adm_tiny")


@pytest.mark.parametrize("name", list(ADM_BLOCK_CASES))
def test_restatement_matches_the_reference_blocks(blocks, name):
    fx = blocks[name]
    kw, in_shapes = ADM_BLOCK_CASES[name]
    sd = {k: v.double().requires_grad_(True) for k, v in synth_state_dict(fx["shapes"]).items()}
    ins = {k: v.double().requires_grad_(True) for k, v in block_inputs(name, in_shapes).items()}
    out = R.resblock(sd, ins["x"], ins["emb"], kw.get("use_scale_shift_norm", False), kw.get("up", False), kw.get("down", False))
    assert list(out.shape) == fx["out_shape"]
    out.backward(block_upstream(name, out.shape).double())
    got, want = R.stored_view(fx["out"], out)
    assert rel_err(got, want) <= 2e-5
    assert abs(float(out.detach().norm()) - fx["out"]["norm"]) <= 2e-5 * fx["out"]["norm"]
    got, want = R.stored_view(fx["d_x"], ins["x"].grad)
    assert rel_err(got, want) <= 2e-4
    assert abs(float(ins["x"].grad.norm()) - fx["d_x"]["norm"]) <= 2e-4 * fx["d_x"]["norm"]
    assert rel_err(ins["emb"].grad, fx["d_emb"]) <= 2e-4
    nmax = max(fx["grad_norms"].values())
    for k in fx["params"]:
        g, n = sd[k].grad, fx["grad_norms"][k]
        if n <= 1e-5 * nmax:                 # a bias in front of a GroupNorm: an analytic zero computed in floating point
            assert float(g.norm()) <= 1e-3 * nmax, k
            continue
        assert abs(float(g.norm()) - n) <= 2e-4 * n + 1e-12, k
        assert rel_err(R.stored_rows(g, BLOCK_SAMPLE_ROWS, CONV_SAMPLE_CIN), fx["g"][k]) <= 2e-4, k


@pytest.mark.parametrize("silu", [True, False])
def test_closed_form_backward_is_autograd_of_the_forward(silu):
    g = torch.Generator().manual_seed(5)
    N, C, H, W = 3, 64, 5, 7
    x = (torch.randn(N, C, H, W, generator=g, dtype=R.F64) * 2 + 0.5).requires_grad_(True)
    gamma = (1 + 0.5 * torch.randn(C, generator=g, dtype=R.F64)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g, dtype=R.F64)).requires_grad_(True)
    scale = torch.randn(N, C, generator=g, dtype=R.F64).requires_grad_(True)
    shift = torch.randn(N, C, generator=g, dtype=R.F64).requires_grad_(True)
    dy = torch.randn(N, C, H, W, generator=g, dtype=R.F64)
    R.gn_mod_fwd(x, gamma, beta, scale, shift, 32, 1e-5, silu).backward(dy)
    with torch.no_grad():
        got = R.gn_mod_bwd(dy, x, gamma, beta, scale, shift, 32, 1e-5, silu)
    for name, a, b in zip(("dx", "dgamma", "dbeta", "d_scale", "d_shift"), got, (x.grad, gamma.grad, beta.grad, scale.grad, shift.grad)):
        assert rel_err(a, b) <= 1e-11, name
    # with no modulation it is nn.GroupNorm
    ref = torch.nn.functional.group_norm(x, 32, gamma, beta, 1e-5)
    zero = torch.zeros(N, C, dtype=R.F64)
    assert rel_err(R.gn_mod_fwd(x, gamma, beta, zero, zero, 32, 1e-5, silu=False), ref) <= 1e-12


@pytest.mark.parametrize("H,W", [(7, 10), (16, 16), (5, 5)])
def test_resamplers_are_torch_and_their_adjoints(H, W):
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randn(2, 8, H, W, generator=g, dtype=R.F64).requires_grad_(True)
    y = R.avgpool2x(x)
    assert rel_err(y, torch.nn.functional.avg_pool2d(x, 2, 2)) <= 1e-15
    dy = torch.randn(y.shape, generator=g, dtype=R.F64)
    y.backward(dy)
    dx = R.avgpool2x_bwd(dy, H, W)
    assert rel_err(dx, x.grad) <= 1e-15
    if H % 2:
        assert float(dx[:, :, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(dx[:, :, :, W - 1].abs().max()) == 0.0
    x.grad = None
    up = R.upsample2x(x)
    assert torch.equal(up, torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"))
    dup = torch.randn(up.shape, generator=g, dtype=R.F64)
    up.backward(dup)
    assert rel_err(R.upsample2x_bwd(dup), x.grad) <= 1e-15


# ---- (c) the mirrored classes: constructors, module trees, state_dict keys ----
def _shapes(m):
    return {k: list(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", list(ADM_BLOCK_CASES))
def test_resblock_constructs_with_the_reference_keys(blocks, name):
    from neurosis_amd.modules.diffusion.openaimodel import Downsample, ResBlock, Upsample

    kw, _ = ADM_BLOCK_CASES[name]
    blk = ResBlock(**kw)
    assert _shapes(blk) == blocks[name]["shapes"]
    assert [k for k, _ in blk.named_parameters()] == blocks[name]["params"]
    assert blk.updown == bool(kw.get("up") or kw.get("down"))
    if kw.get("use_scale_shift_norm"):
        assert list(blk.emb_layers[1].weight.shape) == [2 * kw["out_channels"], kw["emb_channels"]]
    want = Upsample if kw.get("up") else Downsample if kw.get("down") else torch.nn.Identity
    assert type(blk.h_upd) is want and type(blk.x_upd) is want
    if blk.updown:
        assert not blk.h_upd.use_conv and not list(blk.h_upd.parameters())


def test_parameter_free_resamplers_construct():
    from neurosis_amd.modules.diffusion.openaimodel import Downsample, Upsample

    assert _shapes(Upsample(8, False)) == {} and _shapes(Downsample(8, False)) == {}
    assert not hasattr(Upsample(8, False), "conv")
    assert sorted(_shapes(Upsample(8, True))) == ["conv.bias", "conv.weight"] and sorted(_shapes(Downsample(8, True))) == ["op.bias", "op.weight"]
    with pytest.raises(AssertionError):
        Downsample(8, False, out_channels=16)


@pytest.mark.parametrize("case", ["updown_ssn", "plain_resample"])
def test_unet_constructs_with_the_reference_keys(unets, case):
    from neurosis_amd.modules.diffusion.openaimodel import Downsample, ResBlock, UNetModel, Upsample

    fx = unets[case]
    net = UNetModel(**fx["cfg"])
    assert _shapes(net) == fx["shapes"]
    assert list(_shapes(net)) == list(fx["shapes"])          # registration order too: the flat parameter store lays out by it
    if case == "updown_ssn":
        assert isinstance(net.input_blocks[2][0], ResBlock) and net.input_blocks[2][0].updown
        assert isinstance(net.output_blocks[1][1], ResBlock) and net.output_blocks[1][1].updown
        assert all(m.use_scale_shift_norm for m in net.modules() if isinstance(m, ResBlock))
    else:
        assert isinstance(net.input_blocks[2][0], Downsample) and not net.input_blocks[2][0].use_conv
        assert isinstance(net.output_blocks[1][1], Upsample) and not net.output_blocks[1][1].use_conv


# ---- (d) what stays refused ----
@pytest.mark.parametrize("opt", ["exchange_temb_dims", "skip_t_emb"])
def test_video_options_stay_refused(opt):
    from neurosis_amd.modules.diffusion.openaimodel import ResBlock

    with pytest.raises(NotImplementedError, match="video"):
        ResBlock(64, 128, 0.0, **{opt: True})
