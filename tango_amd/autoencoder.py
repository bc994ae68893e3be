"""`AutoencoderKL` -- drop-in for audioldm/variational_autoencoder/autoencoder.py:9-135 of the reference:
`decode_first_stage`, `decode`, `decode_to_waveform`, `device()` (a METHOD there, autoencoder.py:108) and, with
`with_encoder=True`, `encode` / `encode_first_stage` / `get_first_stage_encoding` with the
`DiagonalGaussianDistribution` posterior of distributions.py:24-41.  The mel front-end (STFT) is not part of this class.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import HIFIGAN_CONFIG, Engine, _stream_ptr
from .inpaint import check_latent_h

#: AudioLDM style_transfer's guard against blown-up encodings (audioldm/pipeline.py:209-210): above the trigger, clamp to the range
EDIT_CLIP_TRIGGER, EDIT_CLIP_RANGE = 1e2, 10.0


class DiagonalGaussianDistribution:
    """distributions.py:24-41 of the reference: `parameters` = [mean | logvar] along dim 1, logvar clamped to [-30, 20];
    `sample()` draws from torch's global generator on the parameters' device, like the reference."""

    def __init__(self, parameters, deterministic=False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self):
        return self.mean + self.std * torch.randn(self.mean.shape).to(device=self.parameters.device)

    def mode(self):
        return self.mean


class AutoencoderKL:
    def __init__(self, ddconfig=None, lossconfig=None, image_key="fbank", embed_dim=None, time_shuffle=1, subband=1,
                 ckpt_path=None, reload_from_ckpt=None, ignore_keys=[], colorize_nlabels=None, monitor=None, base_learning_rate=1e-5,
                 scale_factor=1, *, hifigan_config=None, dtype: str = "fp16", device="cuda:0", with_encoder: bool = False, **_):
        assert subband == 1, "freq_merge_subband is the identity only for subband == 1 (autoencoder.py:126-135)"
        dd = dict(ddconfig)
        self.vae_cfg = dict(ch=dd["ch"], ch_mult=list(dd["ch_mult"]), num_res_blocks=dd["num_res_blocks"],
                            z_channels=dd["z_channels"], out_ch=dd["out_ch"], embed_dim=embed_dim or dd["z_channels"],
                            scale_factor=scale_factor, in_channels=dd.get("in_channels", 1))
        assert not dd.get("attn_resolutions"), "attn_resolutions must be empty (released Tango VAE)"
        self.scale_factor = scale_factor
        self.embed_dim = self.vae_cfg["embed_dim"]
        self._device = torch.device(device)
        self.with_encoder = bool(with_encoder)
        self.engine = Engine(vae=self.vae_cfg, hifigan=hifigan_config or HIFIGAN_CONFIG, dtype=dtype, device=device,
                             vae_encoder=self.with_encoder)

    def load_state_dict(self, sd, strict=True):
        missing = self.engine.load_state_dict(sd, strict=strict)
        self.engine.finalize()
        return missing

    def eval(self):
        return self

    def to(self, device):
        return self

    def device(self):
        return self._device

    @torch.no_grad()
    def encode(self, x):
        """autoencoder.py:52-58: Encoder + quant_conv on the engine -> posterior (subband == 1: no frequency split).  The mel's
        frame count names the clip length: [B, 1, 4H, 64] for a latent height H of the duration grid."""
        return DiagonalGaussianDistribution(self.engine.vae_encode(x, latent_h=self._mel_h(x)))

    def _mel_h(self, x):
        f = 1 << (len(self.vae_cfg["ch_mult"]) - 1)
        if not torch.is_tensor(x) or x.dim() != 4 or x.shape[2] % f:
            raise ValueError("mel must be [B, 1, %d H, %d], got %s" % (f, 16 * f, tuple(getattr(x, "shape", ()))))
        return check_latent_h(x.shape[2] // f)

    def _latent_h(self, z):
        if not torch.is_tensor(z) or z.dim() != 4:
            raise ValueError("latents must be [B, %d, H, 16], got %s" % (self.embed_dim, tuple(getattr(z, "shape", ()))))
        return check_latent_h(z.shape[2])

    def encode_first_stage(self, x):
        """autoencoder.py:112-113"""
        return self.encode(x)

    def get_first_stage_encoding(self, encoder_posterior):
        """autoencoder.py:126-135: scale_factor * posterior.sample() (or the tensor itself)"""
        if isinstance(encoder_posterior, DiagonalGaussianDistribution):
            z = encoder_posterior.sample()
        elif isinstance(encoder_posterior, torch.Tensor):
            z = encoder_posterior
        else:
            raise NotImplementedError(f"encoder_posterior of type '{type(encoder_posterior)}' not yet implemented")
        return self.scale_factor * z

    @torch.no_grad()
    def encode_start_latents(self, moments, sa, sb, samples, posterior="sample", eps=None, noise=None, seed=0, sample_offset=0,
                             want_clean=False):
        """The start latents of an audio-to-audio edit in one fused launch (tango_op_latent_encode, include/tango_engine.h): from
        the encoder's `moments` [K, 2C, H, W] (K = `samples`, or 1: one clip fans out to `samples` draws) the posterior sample
        (`posterior="mode"`: its mean), times scale_factor, clamped to +-10 when a sample's largest magnitude exceeds 100
        (pipeline.py:209-210), then the forward noising `sa * z + sb * n` with the scheduler's add_noise scalars at the encode
        timestep (a row of blend_table(); sa = 1, sb = 0: no noising).  `eps` / `noise` [samples, C, H, W] inject the two draws;
        by default both come from the device Philox generator under `seed` at global sample index `sample_offset` + row, so an
        edit does not depend on how a batch is split.  Returns x_t [samples, C, H, W] fp32, or `(x_t, z)` with `want_clean`
        (z: the clean scaled latents, the `known_latents` of a regional edit).  Asynchronous on the current stream."""
        if posterior not in ("sample", "mode"):
            raise ValueError("posterior must be 'sample' or 'mode', got %r" % (posterior,))
        if not torch.is_tensor(moments) or moments.dim() != 4 or moments.shape[1] % 2:
            raise ValueError("moments must be [K, 2C, H, W]")
        B = int(samples)
        if B < 1 or moments.shape[0] not in (1, B):
            raise ValueError("moments hold %d clips: need 1 or samples = %d" % (moments.shape[0], B))
        dev = self._device
        mom = moments.detach().to(device=dev, dtype=torch.float32).contiguous()
        Cc, H, Wd = mom.shape[1] // 2, mom.shape[2], mom.shape[3]
        shape = (B, Cc, H, Wd)
        given = []
        for what, t in (("eps", eps), ("noise", noise)):
            if t is not None:
                if tuple(t.shape) != shape:
                    raise ValueError("%s must be %s, got %s" % (what, shape, tuple(t.shape)))
                t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
            given.append(t)
        eps, noise = given
        if (noise is None or (eps is None and posterior == "sample")) and Cc % 4:
            raise ValueError("the device Philox generator draws four channels at a time: C = %d needs injected eps / noise" % Cc)
        xt = torch.empty(shape, device=dev, dtype=torch.float32)
        z0 = torch.empty(shape, device=dev, dtype=torch.float32) if want_clean else None
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(self.engine.lib.tango_op_latent_encode(
                p(mom), mom.shape[0], p(z0), p(xt), p(eps), p(noise), B, Cc, H * Wd, float(self.scale_factor), EDIT_CLIP_TRIGGER,
                EDIT_CLIP_RANGE, float(sa), float(sb), 1 if posterior == "mode" else 0, int(seed) & (2 ** 64 - 1), int(sample_offset),
                _stream_ptr()), "latent_encode")
        return (xt, z0) if want_clean else xt

    @torch.no_grad()
    def decode(self, z):
        """autoencoder.py:60-64 (post_quant_conv + Decoder); note: no 1/scale_factor here."""
        return self.engine.vae_decode(z * self.scale_factor, latent_h=self._latent_h(z))

    @torch.no_grad()
    def decode_first_stage(self, z):
        """autoencoder.py:116-124: z / scale_factor -> decode -> mel [B,1,1024,64] ([B,1,4H,64] for latents of height H)."""
        return self.engine.vae_decode(z, latent_h=self._latent_h(z))

    @torch.no_grad()
    def decode_to_waveform(self, dec) -> np.ndarray:
        """autoencoder.py:66-69 -> vocoder_infer (hifigan/utilities.py:76-86): np.int16 [B, 163872] (160 * frames + 32 samples for a mel of any frame count).
        The int16 cast (C truncation of wav*32768) happens on the device; only int16 crosses PCIe."""
        wav = self.engine.vocode(dec)
        return wav.cpu().numpy()
