"""The autoencoder loss classes' resize options and AutoencoderPerceptual (reference modules/autoencoding/losses/vae_lpips_discr.py:25-137):
construction, names, state-dict keys, class-path resolution.  No GPU: the arithmetic is the engine's (tests/test_mixed_resolution_gpu.py)."""
import inspect
import logging

import pytest
import torch

from neurosis_amd.modules.autoencoding import losses as L

LP = dict(lpips_kwargs=dict(pnet_type="vgg", pretrained=False))
DISC = dict(n_layers=1, ndf=8)


def test_autoencoder_perceptual_constructor_is_the_references():
    sig = inspect.signature(L.AutoencoderPerceptual.__init__)
    want = dict(perceptual_type="lpips", perceptual_weight=1.0, lpips_type="alex", recon_type="l1", recon_weight=1.0, resize_input=False,
                resize_target=False, loss_ema_steps=64, extra_log_keys=[], delay_setup=False, compile=False, lpips_kwargs=None)
    got = {k: p.default for k, p in sig.parameters.items() if k != "self"}
    assert list(got) == list(want) and got == want
    loss = L.AutoencoderPerceptual(lpips_type="vgg", lpips_kwargs=dict(pretrained=False))
    assert loss.forward_keys == ["split"]
    assert isinstance(loss.perceptual_loss, L.LPIPS) and loss.perceptual_loss.pnet_type == "vgg" and not loss.perceptual_loss.training
    keys = list(loss.state_dict())
    assert keys and all(k.startswith("perceptual_loss.") for k in keys)
    assert list(loss.get_trainable_parameters()) == []
    cfg = loss.engine_settings()
    assert cfg["perceptual_only"] and cfg["discriminator"] is None and cfg["resize"] is None and cfg["rec_loss_type"] == "l1"
    assert L.AutoencoderPerceptual(recon_type="mse", resize_target=True, **LP).engine_settings()["rec_loss_type"] == "l2"
    with pytest.raises(ValueError):
        L.AutoencoderPerceptual(recon_type="huber", **LP)
    with pytest.raises(NotImplementedError):
        L.AutoencoderPerceptual(perceptual_type="dreamsim", **LP)


def test_delay_setup_and_compile(caplog):
    with caplog.at_level(logging.INFO, logger=L.__name__):
        loss = L.AutoencoderPerceptual(delay_setup=True, compile=True, **LP)
    assert loss.perceptual_loss is None and list(loss.state_dict()) == []
    assert any("compile" in r.getMessage() and "ignored" in r.getMessage() for r in caplog.records)
    loss.configure_model()
    first = loss.perceptual_loss
    assert isinstance(first, L.LPIPS) and any(k.startswith("perceptual_loss.") for k in loss.state_dict())
    loss.configure_model()
    assert loss.perceptual_loss is first                         # idempotent, as in the reference


def test_resolves_under_the_prefix_swap_and_refuses_a_standalone_call():
    from tests.test_config_classpaths import resolve, swap

    assert resolve(swap("neurosis.modules.autoencoding.losses.AutoencoderPerceptual")) is L.AutoencoderPerceptual
    assert "AutoencoderPerceptual" in L.__all__
    loss = L.AutoencoderPerceptual(**LP)
    with pytest.raises(RuntimeError, match="AutoencodingEngine"):
        loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), split="train")


def test_both_resize_options_at_once_are_a_value_error():
    with pytest.raises(ValueError, match="resize_input and resize_target"):
        L.AutoencoderPerceptual(resize_input=True, resize_target=True, **LP)
    with pytest.raises(ValueError, match="resize_input and resize_target"):
        L.AutoencoderLPIPSWithDiscr(resize_input=True, resize_target=True, perceptual_weight=0.0, disc_kwargs=DISC)


def test_the_formerly_refused_resize_options_construct():
    a = L.AutoencoderLPIPSWithDiscr(resize_input=True, perceptual_weight=0.0, disc_kwargs=DISC)
    assert a.resize_input_to_target and not a.resize_target_to_input and a.engine_settings()["resize"] == "input"
    b = L.AutoencoderLPIPSWithDiscr(resize_target=True, perceptual_weight=0.0, disc_kwargs=DISC)
    assert b.resize_target_to_input and b.engine_settings()["resize"] == "target"
    c = L.GeneralLPIPSWithDiscriminator(disc_start=0, scale_input_to_tgt_size=True, perceptual_weight=0.0, disc_num_layers=1)
    assert c.scale_input_to_tgt_size and c.engine_settings()["resize"] == "input"
    assert L.AutoencoderPerceptual(resize_input=True, **LP).engine_settings()["resize"] == "input"
    # the defaults are unchanged
    assert L.AutoencoderLPIPSWithDiscr(perceptual_weight=0.0, disc_kwargs=DISC).engine_settings()["resize"] is None
    assert L.GeneralLPIPSWithDiscriminator(disc_start=0, perceptual_weight=0.0, disc_num_layers=1).engine_settings()["resize"] is None


def test_engine_reads_the_resize_option_from_the_loss_or_the_keyword():
    from neurosis_amd.models.autoencoder import AutoencodingEngine
    from neurosis_amd.modules.diffusion.model import Decoder, Encoder
    from tests.golden.fixture_io import load_fixture

    cfg = load_fixture("vae_train_tiny")["cfg"]
    enc, dec = Encoder(**cfg), Decoder(**cfg)
    assert AutoencodingEngine(encoder=enc, decoder=dec, loss="l2").resize is None
    assert AutoencodingEngine(encoder=enc, decoder=dec, loss="l1", resize="target").resize == "target"
    with pytest.raises(ValueError):
        AutoencodingEngine(encoder=enc, decoder=dec, loss="l2", resize="both")
    eng = AutoencodingEngine(encoder=enc, decoder=dec, loss=L.AutoencoderPerceptual(resize_input=True, delay_setup=True, perceptual_weight=0.7, **LP))
    assert eng.resize == "input" and eng.perceptual_only and eng.discriminator is None and eng.perceptual_weight == 0.7
    assert eng.loss.perceptual_loss is None
    eng.loss.configure_model()
    assert any(k.startswith("loss.perceptual_loss.") for k in eng.state_dict())
    assert not any(k.startswith("perceptual_loss.") for k in eng.state_dict())          # registered once, under the loss
    eng = AutoencodingEngine(encoder=enc, decoder=dec, loss=L.AutoencoderLPIPSWithDiscr(resize_target=True, perceptual_weight=0.0, disc_kwargs=DISC))
    assert eng.resize == "target" and not eng.perceptual_only
