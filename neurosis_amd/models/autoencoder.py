"""AutoencoderKL holder: the slice of neurosis.models.autoencoder (autoencoder.py:429-522) the diffusion engine
touches -- construction, weight layout (encoder.*, decoder.*, quant_conv.*, post_quant_conv.*), freeze()/eval(),
encode() and decode().  The training step only runs the ENCODER forward (DiffusionEngine.encode_first_stage,
models/diffusion.py:186-197); the decoder forward serves sampling / log_images.  The VAE's own
training step (row N2) is not built.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..lib import call
from ..modules.diffusion.model import Decoder, Encoder
from ..nn import Conv2d, FlatParamStore
from ..ops import BF16, Img


class AutoencoderKL(nn.Module):
    def __init__(self, *, embed_dim: int, ddconfig: dict, loss=None, ckpt_path: Optional[str] = None, monitor: Optional[str] = None, **kwargs):
        super().__init__()
        dd = dict(ddconfig)
        dd.pop("standalone", None)
        self.embed_dim = embed_dim
        self.encoder = Encoder(**dd, embed_dim=embed_dim, standalone=False)
        self.decoder = Decoder(**dd, embed_dim=embed_dim, standalone=False)
        z = dd["z_channels"]
        double_z = dd.get("double_z", True)
        self.quant_conv = Conv2d((1 + double_z) * z, (1 + double_z) * embed_dim, 1)
        self.post_quant_conv = Conv2d(embed_dim, z, 1)
        self.monitor = monitor
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path)

    def init_from_ckpt(self, path: str) -> None:
        from safetensors.torch import load_file

        sd = load_file(path) if str(path).endswith(".safetensors") else torch.load(path, map_location="cpu")
        sd = sd.get("state_dict", sd)
        own = self.state_dict()
        self.load_state_dict({k: v for k, v in sd.items() if k in own}, strict=False)

    def freeze(self) -> None:
        for p in self.parameters():
            p.requires_grad = False

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> torch.Tensor:
        """moments -> DiagonalGaussian mode (mean), fp32 NCHW."""
        enc = self.encoder
        prev = (enc.standalone, enc.quant_conv)
        enc.standalone, enc.quant_conv = True, self.quant_conv
        try:
            return enc(x, regularize=True)
        finally:
            enc.standalone, enc.quant_conv = prev

    @torch.no_grad()
    def decode(self, z: torch.Tensor, **kwargs) -> torch.Tensor:
        """post_quant_conv + decoder (autoencoder.py:505-508), fp32 NCHW."""
        dec = self.decoder
        prev = (dec.standalone, dec.post_quant_conv)
        dec.standalone, dec.post_quant_conv = True, self.post_quant_conv
        try:
            return dec(z, **kwargs)
        finally:
            dec.standalone, dec.post_quant_conv = prev


class DiagonalGaussianRegularizer(nn.Module):
    """`neurosis.modules.regularizers.DiagonalGaussianRegularizer` (:23-42) over `DiagonalGaussianDistribution`
    (modules/distributions.py:28-72): moments = [mean | logvar] on the channel axis, logvar clamped to [-30, 20],
    z = mean + exp(logvar / 2) * eps (or the mode with sample=False), log["kl_loss"] = sum_b KL(b) / B.
    `regularize` also returns the backward of the map moments -> (z, kl_loss): the tensors are latent-sized
    ([B, 2*z, H/8, W/8] fp32), plain torch arithmetic on the device."""

    loss_key = "kl_loss"      # the entry of the log that `regularization_weights` weighs (the quantizers' is "loss/vq")

    def __init__(self, sample: bool = True) -> None:
        super().__init__()
        self.sample = sample

    def get_trainable_parameters(self):
        yield from ()

    def regularize(self, moments: torch.Tensor, noise: Optional[torch.Tensor] = None):
        mean, raw_logvar = torch.chunk(moments, 2, dim=1)
        logvar = raw_logvar.clamp(-30.0, 20.0)
        std, var = torch.exp(0.5 * logvar), torch.exp(logvar)
        if self.sample:
            eps = torch.randn(mean.shape).to(mean.device) if noise is None else noise.to(mean)
            z = mean + std * eps
        else:
            eps, z = None, mean
        kl = 0.5 * torch.sum(mean * mean + var - 1.0 - logvar, dim=[1, 2, 3])
        batch = moments.shape[0]
        log = {"kl_loss": kl.sum() / batch}

        def bwd(dz: torch.Tensor, d_kl_loss: float = 0.0) -> torch.Tensor:
            """gradient w.r.t. the moments of  <dz, z> + d_kl_loss * kl_loss"""
            d_mean = dz + (d_kl_loss / batch) * mean
            d_logvar = (d_kl_loss / batch) * 0.5 * (var - 1.0)
            if eps is not None:
                d_logvar = d_logvar + dz * eps * 0.5 * std
            inside = (raw_logvar >= -30.0) & (raw_logvar <= 20.0)
            return torch.cat((d_mean, d_logvar * inside), dim=1)

        return z, log, bwd

    def forward(self, z: torch.Tensor):
        out, log, _ = self.regularize(z)
        return out, log


class AutoencodingEngine(nn.Module):
    """The reconstruction part of `neurosis.models.autoencoder.AutoencodingEngine` (autoencoder.py:131-293) without Lightning:
    encode -> regularize -> decode, a "simple" reconstruction loss (the branch of inner_training_step where `self.loss(x, xrec)`
    returns a tensor, :247-256), manual optimisation.  The adversarial / perceptual loss (GeneralLPIPSWithDiscriminator: LPIPS
    feature nets, PatchGAN, adaptive weighting, second optimizer) is the part of SURVEY 8(f) N2 that is not built.

    MI355X shape of it: images enter as fp32 NCHW and leave the same way, everything between is channels-last bf16 tokens
    through `Encoder.fwdb` / `Decoder.fwdb` (explicit backward closures, weight gradients on the side stream as in the UNet),
    the l2 loss and its gradient come from one kernel over the decoder's output tokens, parameters / gradients / AdamW state
    live in one FlatParamStore across encoder and decoder."""

    def __init__(self, *, encoder: Encoder, decoder: Decoder, loss="l2", regularizer: Optional[nn.Module] = None, input_key: str = "image",
                 regularization_weights: Optional[dict] = None, discriminator: Optional[nn.Module] = None, disc_loss: str = "hinge", disc_start: int = 0,
                 disc_factor: float = 1.0, disc_weight: float = 1.0, rec_weight: float = 1.0, logvar_init: float = 0.0, learn_logvar: bool = False,
                 perceptual_loss: Optional[nn.Module] = None, perceptual_weight: float = 1.0, resize: Optional[str] = None, **kwargs):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder
        self.perceptual_only, self.perceptual_kind = False, "lpips"
        self.disc_store: Optional[FlatParamStore] = None
        self.regularization = regularizer if regularizer is not None else DiagonalGaussianRegularizer()
        if hasattr(loss, "engine_settings"):
            # a loss CLASS of the reference's surface (neurosis_amd.modules.autoencoding.losses.GeneralLPIPSWithDiscriminator /
            # AutoencoderLPIPSWithDiscr, as a config-5 YAML names it): registered as `self.loss` like the reference engine does
            # (models/autoencoder.py:161), so its submodules checkpoint under `loss.*`; the fused arithmetic below reads its settings.
            # The discriminator / LPIPS / logvar it owns are referenced WITHOUT registering them a second time.
            self.loss = loss
            cfg = loss.engine_settings()
            self.__dict__["discriminator"] = cfg["discriminator"]
            self.__dict__["perceptual_loss"] = cfg["perceptual_loss"]
            self.perceptual_weight = cfg["perceptual_weight"] if cfg["perceptual_loss"] is not None else 0.0
            disc_loss, disc_factor, disc_weight, rec_weight = cfg["disc_loss"], cfg["disc_factor"], cfg["disc_weight"], cfg["rec_weight"]
            disc_start = disc_start if disc_start else cfg["disc_start"]
            learn_logvar = cfg["learn_logvar"]
            lv = cfg["logvar"]
            if lv is None:
                self.logvar = nn.Parameter(torch.zeros(size=()), requires_grad=False)
            else:
                self.__dict__["logvar"] = lv
            if regularization_weights is None:
                regularization_weights = cfg["regularization_weights"]
            loss = cfg["rec_loss_type"]
            resize = resize if resize is not None else cfg.get("resize")
            # AutoencoderPerceptual: clamped images, per-sample means, no discriminator (_perceptual_loss); its LPIPS is read from the loss
            # object at each step, so that `delay_setup` / `configure_model()` work as in the reference
            self.perceptual_only = bool(cfg.get("perceptual_only", False))
            self.perceptual_kind = cfg.get("perceptual_kind", "lpips")          # "dreamsim": AutoencoderDreamsim, read from `loss.dreamsim_loss`
            if self.perceptual_only:
                self.perceptual_weight = cfg["perceptual_weight"]
        else:
            # adversarial part as keyword arguments (GeneralLPIPSWithDiscriminator's, discriminator_loss.py:23-40)
            self.discriminator = discriminator
            self.perceptual_loss = perceptual_loss            # neurosis_amd.modules.losses.LPIPS (frozen), or None
            self.perceptual_weight = perceptual_weight if perceptual_loss is not None else 0.0
            # the output log-variance of the nll (discriminator_loss.py:56-58): a scalar parameter, trained with the autoencoder when
            # learn_logvar (get_trainable_autoencoder_parameters, :90-93)
            self.logvar = nn.Parameter(torch.ones(size=()) * logvar_init, requires_grad=learn_logvar)
        if self.discriminator is not None:
            from ..modules.losses import get_discr_loss_fn

            self.disc_loss = get_discr_loss_fn(disc_loss)
        self.disc_start, self.disc_factor, self.discriminator_weight = disc_start, disc_factor, disc_weight
        self.rec_weight = rec_weight
        self.learn_logvar = learn_logvar
        if isinstance(loss, nn.MSELoss) or loss in ("l2", "mse"):
            self.rec_loss_type = "l2"
        elif isinstance(loss, nn.L1Loss) or loss in ("l1", "mae"):
            self.rec_loss_type = "l1"
        else:
            raise NotImplementedError("loss must be 'l2' / 'l1' (or nn.MSELoss / nn.L1Loss), or one of the loss classes of "
                                      "neurosis_amd.modules.autoencoding.losses; got " + type(loss).__name__)
        # decoder output of another size than the input (an autoencoder whose decoder has more or fewer levels than its encoder): "input"
        # resamples the input to the reconstruction's size, "target" the reconstruction to the input's (resize_input / resize_target of the
        # loss classes; antialiased bicubic, ops.resize_bicubic_aa); None refuses such a pair
        if resize not in (None, "input", "target"):
            raise ValueError(f"resize must be None, 'input' or 'target', got {resize!r}")
        self.resize = resize
        self.input_key = input_key
        self.regularization_weights = dict(regularization_weights or {})     # e.g. {"kl_loss": 1e-6}; the reference's simple branch uses none
        self.global_step = 0
        self.store: Optional[FlatParamStore] = None
        self.last_log: dict = {}

    # -- reference surface -------------------------------------------------------------------------
    def get_input(self, batch: dict) -> torch.Tensor:
        return batch[self.input_key]

    def get_autoencoder_params(self, decoder_only: bool = False) -> list:
        params = ([self.logvar] if self.learn_logvar else []) + list(self.decoder.parameters())
        if decoder_only:
            return params
        # the regularizer's own parameters (a VectorQuantizer's codebook) go last: nothing for the Gaussian one, whose layout is unchanged
        reg = getattr(self.regularization, "get_trainable_parameters", None)
        return params + list(self.encoder.parameters()) + (list(reg()) if reg is not None else [])

    def get_last_layer(self):
        return self.decoder.get_last_layer()

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_reg_log: bool = False, unregularized: bool = False):
        z = self.encoder(x)
        if unregularized:
            return z, dict()
        z, reg_log = self.regularization(z)
        return (z, reg_log) if return_reg_log else z

    @torch.no_grad()
    def decode(self, z: torch.Tensor, **kwargs) -> torch.Tensor:
        return self.decoder(z, **kwargs)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, **kwargs):
        z, reg_log = self.encode(x, return_reg_log=True)
        return z, self.decode(z, **kwargs), reg_log

    # -- training ----------------------------------------------------------------------------------
    def setup_flat_params(self) -> FlatParamStore:
        self.store = FlatParamStore(self.get_autoencoder_params())
        if self.discriminator is not None:
            self.disc_store = FlatParamStore(list(self.discriminator.parameters()))
        if self.store.master.is_cuda:   # one side stream for both stores: their steps alternate, they never run together
            side = torch.cuda.Stream(device=self.store.master.device)
            self.store.state.wgrad_stream = side
            if self.discriminator is not None:
                self.disc_store.state.wgrad_stream = side
        return self.store

    @torch.no_grad()
    def loss_and_backward(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None):
        """forward + backward of  rec_loss(x, decode(regularize(encode(x)))) + sum_k w_k * reg_log[k]  into the parameters'
        gradients.  Returns (loss, z, xrec, reg_log); xrec fp32 NCHW, the decoder's own output.  `noise` may be injected (parity tests).
        When the decoder's output has another size than x, `self.resize` says which of the two the loss resamples (_resized); with equal
        sizes nothing of that runs."""
        B, C, H, W = x.shape
        x = x.float().contiguous()
        cpad = (C + 7) // 8 * 8
        moments_img, b_enc = self.encoder.fwdb(Img(ops.nchw_to_tokens(x, cpad), B, H, W))
        mc = self.encoder.quant_conv.out_channels if self.encoder.standalone else self.encoder.conv_out.out_channels
        moments = ops.tokens_to_nchw(moments_img.t, B, mc, moments_img.H, moments_img.W, dtype=torch.float32)
        z, reg_log, b_reg = self.regularization.regularize(moments, noise)
        zc = z.shape[1]
        out_img, b_dec = self.decoder.fwdb(Img(ops.nchw_to_tokens(z.contiguous(), (zc + 7) // 8 * 8), B, z.shape[2], z.shape[3]))
        xrec_out = xrec = ops.tokens_to_nchw(out_img.t, B, C, out_img.H, out_img.W, dtype=torch.float32)
        dev = x.device
        # the images the loss terms see: x, xrec and the reconstruction's tokens as they are when the sizes agree; otherwise the resized input,
        # or the resized reconstruction with `pull`, which takes a token gradient w.r.t. it back to the decoder's output resolution
        x, xrec, out_img, pull = self._loss_view(x, xrec, out_img)
        H, W = x.shape[2:]
        adversarial = self.discriminator is not None or self.perceptual_loss is not None
        log = {}
        if self.perceptual_only:
            loss, d_out, log = self._perceptual_loss(x, xrec, out_img)
        elif adversarial:
            loss, d_out, log = self._generator_loss(x, xrec, out_img, b_dec, pull)
            pull = None                                   # (already at the decoder's resolution: the adaptive weight needed it there)
        elif self.rec_loss_type == "l2":
            # mean((xrec - x)^2) over everything = sum_b (1/B) * mean_chw: the edm loss kernel with c_out = 1, c_skip = 0, w = 1/B
            one, zero = torch.ones(B, device=dev), torch.zeros(B, device=dev)
            weight = torch.full((B,), 1.0 / B, device=dev)
            per_sample = torch.empty(B, dtype=torch.float32, device=dev)
            d_out = torch.empty_like(out_img.t)
            call("nk_edm_loss", out_img.t.data_ptr(), x.data_ptr(), x.data_ptr(), one.data_ptr(), zero.data_ptr(), weight.data_ptr(), per_sample.data_ptr(),
                 d_out.data_ptr(), B, C, H * W, out_img.C, 1.0, ops._stream())
            loss = per_sample.sum()
        else:
            diff = xrec - x
            loss = diff.abs().mean()
            d_out = ops.nchw_to_tokens((torch.sign(diff) / diff.numel()).contiguous(), out_img.C)
        for key, w in self.regularization_weights.items():
            loss = loss + w * reg_log[key]
        reg_log = {**reg_log, **log}
        if pull is not None:
            d_out = pull(d_out)
        dz = ops.tokens_to_nchw(b_dec(d_out), B, zc, z.shape[2], z.shape[3], dtype=torch.float32)
        d_moments = b_reg(dz, float(self.regularization_weights.get(getattr(self.regularization, "loss_key", "kl_loss"), 0.0)))
        b_enc(ops.nchw_to_tokens(d_moments.contiguous(), moments_img.C))
        ops.join_wgrad_stream()
        return loss, z, xrec_out, reg_log

    def _resized(self, x: torch.Tensor, xrec: torch.Tensor):
        """(x, xrec, backward of the reconstruction's resize or None) at one common size, by `self.resize`"""
        if x.shape[2:] == xrec.shape[2:]:
            return x, xrec, None
        if self.resize is None:
            raise ValueError(f"the decoder's output is {tuple(xrec.shape[2:])} and the input {tuple(x.shape[2:])}: the loss needs resize='input' (resize_input / "
                             "scale_input_to_tgt_size of the loss classes: the input is resampled to the reconstruction's size) or resize='target' "
                             "(resize_target: the reconstruction is resampled to the input's size)")
        if self.resize == "input":
            return ops.resize_bicubic_aa(x, tuple(xrec.shape[2:]))[0], xrec, None          # no gradient flows to the input
        xrec_t, b_resize = ops.resize_bicubic_aa(xrec, tuple(x.shape[2:]))
        return x, xrec_t, b_resize

    def _loss_view(self, x: torch.Tensor, xrec: torch.Tensor, out_img: Img):
        x, xrec_t, b_resize = self._resized(x, xrec)
        if b_resize is None:
            return x, xrec_t, out_img, None
        B, C, H, W = xrec_t.shape
        cpad = out_img.C

        def pull(d_tokens: torch.Tensor) -> torch.Tensor:
            return ops.nchw_to_tokens(b_resize(ops.tokens_to_nchw(d_tokens, B, C, H, W, dtype=torch.float32)), cpad)

        return x, xrec_t, Img(ops.nchw_to_tokens(xrec_t, cpad), B, H, W), pull

    def _perceptual_loss(self, x: torch.Tensor, xrec: torch.Tensor, out_img: Img):
        """AutoencoderPerceptual (vae_lpips_discr.py:97-137):  loss = mean_b(recon_weight * rec_b + perceptual_weight * relu(LPIPS_b)),  rec_b the
        per-sample mean of |x - xrec| or (x - xrec)^2, both images clamped to [-1, 1]; no gradient where xrec was clamped.  (The reference
        adds a [B] to a [B, 1, 1, 1] tensor, which backpropagates only at B = 1, where it is this formula.)  AutoencoderDreamsim shares everything
        but the perceptual term, which is dreamsim_weight * relu(sum_b' d_b') for every sample (below).
        Returns (loss, d loss / d reconstruction tokens, log); every log entry is a device scalar."""
        B, C, H, W = x.shape
        inside = (xrec >= -1.0) & (xrec <= 1.0)
        xc, rc = x.clamp(-1.0, 1.0), xrec.clamp(-1.0, 1.0)
        diff = rc - xc
        rec = diff * diff if self.rec_loss_type == "l2" else diff.abs()
        rec_term = self.rec_weight * rec.mean(dim=(1, 2, 3))                                 # [B]
        d_rec = (2.0 * diff if self.rec_loss_type == "l2" else torch.sign(diff)) * (self.rec_weight / (B * C * H * W))
        p_term = torch.zeros(B, device=x.device)
        if self.perceptual_weight > 0 and self.perceptual_kind == "dreamsim":
            # AutoencoderDreamsim (losses/dreamsim.py:101-140): the distances are summed over the batch BEFORE the relu and that scalar joins every
            # sample's term:  loss = mean_b(recon_weight * rec_b + dreamsim_weight * relu(sum_b' d_b')),  d loss / d d_b' = dreamsim_weight * [sum > 0]
            dreamsim = self.loss.dreamsim_loss
            if dreamsim is None:
                raise RuntimeError("AutoencoderDreamsim(delay_setup=True): call configure_model() on the loss before the first training step")
            d, b_dreamsim = dreamsim.fwdb(xc, rc, rescale=self.loss.rescale_input)
            d_sum = d.sum()
            p_term = (self.perceptual_weight * torch.relu(d_sum)).expand(B)
            d_rec = d_rec + b_dreamsim(((d_sum > 0) * self.perceptual_weight).expand(B).contiguous())
        elif self.perceptual_weight > 0:
            lpips = self.loss.perceptual_loss
            if lpips is None:
                raise RuntimeError("AutoencoderPerceptual(delay_setup=True): call configure_model() on the loss before the first training step")
            p_loss, b_lpips = lpips.fwdb(xc, Img(ops.nchw_to_tokens(rc, out_img.C), B, H, W))
            p_term = self.perceptual_weight * torch.relu(p_loss)
            d_p = ops.tokens_to_nchw(b_lpips(((p_loss > 0) * (self.perceptual_weight / B)).contiguous()), B, C, H, W, dtype=torch.float32)
            d_rec = d_rec + d_p
        total = rec_term + p_term
        loss = total.mean()
        log = {"loss/total": loss.detach(), "loss/rec": rec_term.mean(), "loss/p": p_term.mean()}
        return loss, ops.nchw_to_tokens((d_rec * inside).contiguous(), out_img.C), log

    def _generator_loss(self, x: torch.Tensor, xrec: torch.Tensor, out_img: Img, b_dec, pull=None):
        """The autoencoder's side of the adversarial loss with perceptual_weight = 0:
            nll   = sum(rec_weight * rec(x, xrec) / exp(logvar) + logvar) / B                  (get_nll_loss, :219-233)
            g     = -mean(D(xrec))                                                             (:268-270)
            d_w   = clamp(||d nll / dW|| / (||d g / dW|| + 1e-4), 0, 1e4) * disc_weight         W = decoder.conv_out.weight (:205-217)
            loss  = nll + disc_factor * d_w * g          (0 adversarial weight before disc_start)
        With a perceptual loss, rec(x, xrec) becomes rec_weight * rec + perceptual_weight * LPIPS(x, xrec) (the per-sample distance
        broadcast over the image, :254-259).
        The reference's forward for this branch does not run as written (it evaluates `weights > 0` with weights = None, and
        sums the un-reduced p_rec_loss tensor into a loss that is then passed to backward()); this is the formula its terms
        spell out -- the one of the taming-transformers / generative-models loss it was reworked from.
        `x`, `xrec` and `out_img` are the images the terms see (_loss_view); with a resized reconstruction `pull` takes each token gradient
        back to the decoder's output resolution, which is where the last layer's gradient norms and the returned gradient live (the adjoint
        is linear: the sum of the two pulled gradients is the pulled sum, so the total passes through it once).
        Returns (loss, d loss / d decoder-output tokens, log)."""
        B, C, H, W = x.shape
        diff = xrec - x
        rec = diff * diff if self.rec_loss_type == "l2" else diff.abs()
        lv = self.logvar.detach().float()
        inv_var = torch.exp(-lv)                    # (device scalars: no host sync)
        weighted_rec = (rec * self.rec_weight).sum()
        nll = (weighted_rec * inv_var + lv * rec.numel()) / B
        d_nll = (2.0 * diff if self.rec_loss_type == "l2" else torch.sign(diff)) * (self.rec_weight * inv_var / B)
        d_nll_tok = ops.nchw_to_tokens(d_nll.contiguous(), out_img.C)
        log = {}
        if self.perceptual_loss is not None and self.perceptual_weight > 0:
            # p_rec_loss = rec_weight * rec + perceptual_weight * p_loss[b] broadcast over the image (:258-259): every element of
            # sample b carries the LPIPS distance once, so nll gains perceptual_weight * C*H*W * p_loss[b] / exp(logvar) / B
            p_loss, b_lpips = self.perceptual_loss.fwdb(x, out_img)
            per_sample = self.perceptual_weight * (C * H * W) * inv_var / B
            nll = nll + per_sample * p_loss.sum()
            weighted_rec = weighted_rec + self.perceptual_weight * (C * H * W) * p_loss.sum()
            d_nll_tok = ops.add(d_nll_tok, b_lpips(per_sample.expand(B).contiguous()))
            log["p_loss"] = p_loss.mean().detach()
        if self.learn_logvar:
            # d nll / d logvar = (-sum(p_rec) / exp(logvar) + numel) / B; the adversarial term does not depend on it
            g = ((rec.numel() - weighted_rec * inv_var) / B).reshape(())
            flat = ops.grad_flat(self.logvar)
            flat.copy_(g.reshape(flat.shape)) if not ops.state_of(self.logvar).grad_accumulate else flat.add_(g.reshape(flat.shape))
        active = self.discriminator is not None and self.global_step >= self.disc_start
        log["nll_loss"] = nll.detach()
        if pull is not None:
            d_nll_tok = pull(d_nll_tok)
        if not active:
            log.update(g_loss=torch.zeros((), device=x.device), d_weight=torch.zeros((), device=x.device))
            return nll, d_nll_tok, log
        logits, b_disc = self.discriminator.fwdb(out_img)
        vals = ops.tokens_to_nchw(logits.t, B, 1, logits.H, logits.W, dtype=torch.float32)
        g_loss = -vals.mean()
        d_logits = torch.full_like(vals, -1.0 / vals.numel())
        d_g_tok = b_disc(ops.nchw_to_tokens(d_logits, logits.C))       # also writes the discriminator's weight gradients: unused here,
        ops.join_wgrad_stream()                                          # overwritten by its own step
        if pull is not None:
            d_g_tok = pull(d_g_tok)
        d_weight = (b_dec.last_layer_grad_norm(d_nll_tok) / (b_dec.last_layer_grad_norm(d_g_tok) + 1e-4)).clamp(0.0, 1e4) * self.discriminator_weight
        factor = d_weight * self.disc_factor
        log.update(g_loss=g_loss.detach(), d_weight=d_weight.detach())
        return nll + factor * g_loss, ops.add(d_nll_tok, ops.cast_bf16((d_g_tok.float() * factor).contiguous())), log

    @torch.no_grad()
    def discriminator_step_loss(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None):
        """optimizer_idx == 1 of the reference's loss (discriminator_loss.py:303-320): d_loss = disc_factor * disc_loss(D(x), D(xrec))
        with the reconstruction detached; forward + backward into the discriminator's gradients.  Returns (d_loss, log)."""
        B, C, H, W = x.shape
        x = x.float().contiguous()
        _, xrec, _ = self._reconstruct(x, noise)
        x, xrec, _ = self._resized(x, xrec)          # (the reconstruction is detached here: no backward through the resize)
        H, W = x.shape[2:]
        cpad = (C + 7) // 8 * 8
        lr_img, b_real = self.discriminator.fwdb(Img(ops.nchw_to_tokens(x, cpad), B, H, W), need_dx=False)
        lf_img, b_fake = self.discriminator.fwdb(Img(ops.nchw_to_tokens(xrec.contiguous(), cpad), B, H, W), need_dx=False)
        real = ops.tokens_to_nchw(lr_img.t, B, 1, lr_img.H, lr_img.W, dtype=torch.float32)
        fake = ops.tokens_to_nchw(lf_img.t, B, 1, lf_img.H, lf_img.W, dtype=torch.float32)
        log = {"logits_real": real.mean(), "logits_fake": fake.mean()}
        if self.global_step < self.disc_start:
            return torch.zeros((), device=x.device), log
        loss, d_real, d_fake = self.disc_loss.with_grad(real, fake)
        dstate = self.disc_store.state if getattr(self, "disc_store", None) is not None else ops.state_of(next(self.discriminator.parameters()))
        dstate.grad_accumulate = False
        b_real(ops.nchw_to_tokens((d_real * self.disc_factor).contiguous(), lr_img.C))
        dstate.grad_accumulate = True            # the fake pass adds to the real pass's weight gradients
        try:
            b_fake(ops.nchw_to_tokens((d_fake * self.disc_factor).contiguous(), lf_img.C))
        finally:
            dstate.grad_accumulate = False
        ops.join_wgrad_stream()
        return loss * self.disc_factor, log

    def _reconstruct(self, x: torch.Tensor, noise: Optional[torch.Tensor]):
        """forward only: (z, xrec, reg_log) with the posterior sampled (or `noise` injected)"""
        moments = self.encoder(x)
        z, reg_log, _ = self.regularization.regularize(moments, noise)
        return z, self.decoder(z), reg_log

    def training_step(self, batch: dict, batch_idx: int = 0, lr: float = 4.5e-6, betas=(0.5, 0.9), weight_decay: float = 0.0, noise=None) -> torch.Tensor:
        """autoencoder.py:280-293: with a discriminator the two optimizers alternate by batch index (the autoencoder's until
        disc_start); gradients are overwritten by each backward, then one fused AdamW step over that optimizer's flat buffers."""
        if self.store is None:
            raise RuntimeError("call setup_flat_params() first")
        n_opts = 2 if self.discriminator is not None else 1
        optimizer_idx = batch_idx % n_opts if self.global_step >= self.disc_start else 0
        x = self.get_input(batch)
        if optimizer_idx == 0:
            loss, _, _, log = self.loss_and_backward(x, noise)
            self.store.adamw_step(lr, betas, 1e-8, weight_decay)
            self.last_log = {"train/loss/rec": loss.detach(), **{f"train/{k}": v.detach() for k, v in log.items()}}
        else:
            loss, log = self.discriminator_step_loss(x, noise)
            if self.global_step >= self.disc_start:
                self.disc_store.adamw_step(lr, betas, 1e-8, weight_decay)
            self.last_log = {"train/loss/disc": loss.detach(), **{f"train/{k}": v.detach() for k, v in log.items()}}
        self.global_step += 1
        return loss
