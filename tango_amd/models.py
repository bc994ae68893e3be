"""`AudioDiffusion` -- drop-in for the inference-side surface of the reference class
(models.py:55-305 of declare-lab/tango): `inference`, `prepare_latents`, `encode_text`,
`encode_text_classifier_free`, `.unet.config.in_channels`.  Training (`forward`, `compute_snr`) is
out of scope.

The denoise loop (models.py:233-249) runs inside the HIP engine; the frozen FLAN-T5 encoder stays a
PyTorch-ROCm module (its output is the engine's input).
"""
import json
import os
from types import SimpleNamespace
from typing import List, Optional

import torch

from .engine import Engine, normalize_unet_config
from .inpaint import check_latent_h, duration_geometry, long_geometry, loop_geometry, timeline_geometry, window_taper
from .scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler  # noqa: F401  (re-exported like `from models import DDPMScheduler`)
from .scheduler import DDIMInverseScheduler, cfg_enabled, check_guidance_rescale, from_diffusers, guidance_table

_TEXT_BUCKETS = (16, 32, 64, 128, 256, 512)


def build_pretrained_models(ckpt, vae_config=None, dtype="fp16", device="cuda:0", autoencoder_cls=None, stft_config=None, stft_cls=None):
    """models.py:27-52 of the reference: build the mel-VAE (+ vocoder) and the TacotronSTFT wave->mel front-end from an AudioLDM
    `.ckpt` (`{"state_dict": {"first_stage_model.*": ..., "scale_factor": ...}}`); `ckpt` is a path or an already loaded dict.
    Returns `(vae, fn_STFT)` like the reference.  `vae_config` defaults to the AudioLDM first-stage config
    (audioldm/utils.py:158-181 == mustango/configs/vae_config.json), `stft_config` to its preprocessing block
    (audioldm/utils.py:104-118: n_fft 1024, hop 160, 64 mels, 16 kHz, 0-8000 Hz)."""
    if autoencoder_cls is None:
        from .autoencoder import AutoencoderKL as autoencoder_cls
    if stft_cls is None:
        from .stft import TacotronSTFT as stft_cls
    checkpoint = torch.load(ckpt, map_location="cpu") if isinstance(ckpt, (str, os.PathLike)) else ckpt
    sd = checkpoint["state_dict"]
    scale_factor = float(sd["scale_factor"].item() if hasattr(sd["scale_factor"], "item") else sd["scale_factor"])
    vae_state_dict = {k[len("first_stage_model."):]: v for k, v in sd.items() if k.startswith("first_stage_model.")}
    cfg = dict(vae_config) if vae_config is not None else dict(
        image_key="fbank", subband=1, embed_dim=8, time_shuffle=1,
        ddconfig=dict(double_z=True, z_channels=8, resolution=256, downsample_time=False, in_channels=1, out_ch=1, ch=128,
                      ch_mult=[1, 2, 4], num_res_blocks=2, attn_resolutions=[], dropout=0.0))
    cfg["scale_factor"] = scale_factor
    vae = autoencoder_cls(**cfg, dtype=dtype, device=device)
    vae.load_state_dict(vae_state_dict)
    sc = dict(stft_config) if stft_config is not None else dict(filter_length=1024, hop_length=160, win_length=1024, n_mel_channels=64,
                                                                 sampling_rate=16000, mel_fmin=0, mel_fmax=8000)
    fn_STFT = stft_cls(sc["filter_length"], sc["hop_length"], sc["win_length"], sc["n_mel_channels"], sc["sampling_rate"],
                       sc["mel_fmin"], sc["mel_fmax"], device=device)
    vae.eval()
    fn_STFT.eval()
    return vae, fn_STFT


def _hf_classes():
    """(AutoTokenizer, T5EncoderModel) of models.py:98-100, imported on first use"""
    from transformers import AutoTokenizer, T5EncoderModel
    return AutoTokenizer, T5EncoderModel


class _UNetHandle:
    """What callers read off `model.unet` (models.py:227)."""

    def __init__(self, cfg, engine):
        self.config = SimpleNamespace(**cfg)
        self.in_channels = cfg["in_channels"]
        self._engine = engine

    def __call__(self, sample, timestep, encoder_hidden_states=None, encoder_attention_mask=None, beat_features=None,
                 chord_features=None, beat_attention_mask=None, chord_attention_mask=None, **_):
        out = self._engine.unet_forward(sample, int(timestep), encoder_hidden_states, encoder_attention_mask, beat_features,
                                        chord_features, beat_attention_mask, chord_attention_mask)
        return SimpleNamespace(sample=out)


class AudioDiffusion:
    def __init__(self, text_encoder_name=None, scheduler_name=None, unet_model_name=None, unet_model_config_path=None,
                 snr_gamma=None, freeze_text_encoder=True, uncondition=False, *, unet_config: Optional[dict] = None,
                 dtype: str = "fp16", device="cuda:0", text_encoder=None, tokenizer=None, bucket_text_len: bool = True,
                 attn_fp8: bool = False):
        assert unet_model_name is None, "released Tango checkpoints take the set_from == 'random' branch (models.py:83-86)"
        if unet_config is None:
            if unet_model_config_path is None:
                raise ValueError("Either UNet pretrain model name or a config file path is required")
            unet_config = json.load(open(unet_model_config_path))
        self.unet_config = normalize_unet_config({k: v for k, v in unet_config.items() if not k.startswith("_")})
        self.text_encoder_name = text_encoder_name
        self.scheduler_name = scheduler_name
        self.set_from = "random"
        self.device = torch.device(device)
        self.engine = Engine(unet=self.unet_config, dtype=dtype, device=device, attn_fp8=attn_fp8)
        self.unet = _UNetHandle(self.unet_config, self.engine)
        self.text_encoder = text_encoder
        self.tokenizer = tokenizer
        self.bucket_text_len = bucket_text_len
        self.use_graph = True
        self.seed = None          # None: every call draws its Philox key from torch's default generator (torch.manual_seed rules)
        self._calls = 0
        self._text_sd = None      # `text_encoder.*` tensors of pytorch_model_main.bin, applied when the encoder exists

    # ---- state dict --------------------------------------------------------------------------
    def load_state_dict(self, sd, strict=True):
        """pytorch_model_main.bin: `unet.*` goes to the engine, `text_encoder.*` to the torch T5."""
        missing = self.engine.load_state_dict(sd, strict=strict)
        self.engine.finalize()
        # The reference loads the checkpoint's text encoder through the same call (tango.py:28 -> nn.Module.load_state_dict,
        # strict): checkpoints trained with freeze_text_encoder=False carry tuned T5 weights.  The encoder may not exist yet
        # (it is built lazily), so the sub-dict is kept and applied by _ensure_text().
        te = {k[len("text_encoder."):]: v for k, v in sd.items() if k.startswith("text_encoder.")}
        self._text_sd = te or None
        if isinstance(self.text_encoder, str):
            # text_encoder="engine": run FLAN-T5 on the HIP engine too (tango_amd/text_encoder.py), built from the checkpoint's
            # own tensors -- no hub access, no PyTorch compute left in generate()
            if self.text_encoder != "engine":
                raise ValueError("text_encoder must be a module, None or the string 'engine'")
            if not te:
                raise RuntimeError("text_encoder='engine' needs the checkpoint's text_encoder.* tensors")
            from .text_encoder import T5EncoderOnEngine
            self.text_encoder = T5EncoderOnEngine.from_state_dict(sd, "text_encoder.", device=self.device)
            self._text_sd = None
        elif self.text_encoder is not None:
            self._apply_text_sd()
        return missing

    def _apply_text_sd(self):
        if self._text_sd is None:
            return
        res = self.text_encoder.load_state_dict(self._text_sd, strict=False)
        # `shared.weight` and `encoder.embed_tokens.weight` are one tied tensor: either name alone is complete
        tied = {"shared.weight", "encoder.embed_tokens.weight"}
        miss = [k for k in res.missing_keys if not (k in tied and tied & set(self._text_sd))]
        if miss or res.unexpected_keys:
            raise RuntimeError("text_encoder state_dict mismatch: missing %s unexpected %s" % (miss[:4], list(res.unexpected_keys)[:4]))
        self._text_sd = None

    def eval(self):
        return self

    def to(self, device):
        return self

    # ---- text --------------------------------------------------------------------------------
    def _ensure_text(self):
        if isinstance(self.text_encoder, str):
            raise RuntimeError("text_encoder='engine' is built by load_state_dict(); no checkpoint has been loaded yet")
        # each component is loaded only if IT is missing (models.py:98-100): an encoder that load_state_dict() already built
        # from the checkpoint (text_encoder="engine") or that the caller supplied must never be replaced by stock hub
        # weights just because no tokenizer was passed
        if self.tokenizer is None:
            self.tokenizer = _hf_classes()[0].from_pretrained(self.text_encoder_name)
        if self.text_encoder is None:
            self.text_encoder = _hf_classes()[1].from_pretrained(self.text_encoder_name).to(self.device).eval()
        self._apply_text_sd()

    def encode_text(self, prompt: List[str]):
        """models.py:129-147"""
        self._ensure_text()
        batch = self.tokenizer(prompt, max_length=self.tokenizer.model_max_length, padding=True, truncation=True,
                               return_tensors="pt")
        ids, am = batch.input_ids.to(self.device), batch.attention_mask.to(self.device)
        with torch.no_grad():
            hs = self.text_encoder(input_ids=ids, attention_mask=am)[0]
        return hs, (am == 1).to(self.device)

    def encode_text_classifier_free(self, prompt: List[str], num_samples_per_prompt: int, negative_prompt=None):
        """models.py:266-305: returns [uncond; cond] embeddings and the boolean mask.  `negative_prompt`: as in
        _encode_text_classifier_free."""
        pe, pm, _ = self._encode_text_classifier_free(prompt, num_samples_per_prompt, negative_prompt)
        return pe, pm

    def _encode_text_classifier_free(self, prompt: List[str], num_samples_per_prompt: int, negative_prompt=None):
        """the same, plus the tokenizer's own HOST copy of the mask (third value): `inference` hands it to the engine beside the device
        mask, so that the plan is chosen without a device -> host read-back.

        `negative_prompt`: None -- the unconditional half is T5("") padded to the prompt's length (models.py:282-289), one valid key
        per row; a str -- that text against every prompt; or a list of len(prompt) strings.  Both halves are then tokenised to one
        common length, the longer of the two (padded keys are masked, which is exact: _pad_text); a negative prompt longer than
        the prompt is NOT cut to the prompt's length, as the reference's max_length=pe.shape[1], truncation=True would.  The order
        stays [negative; cond]."""
        self._ensure_text()
        dev = self.device
        if negative_prompt is not None:
            if isinstance(negative_prompt, str):
                negative_prompt = [negative_prompt] * len(prompt)
            negative_prompt = list(negative_prompt)
            if len(negative_prompt) != len(prompt):
                raise ValueError("negative_prompt holds %d strings for %d prompts" % (len(negative_prompt), len(prompt)))
            return self._encode_text_pair(prompt, negative_prompt, num_samples_per_prompt)
        batch = self.tokenizer(prompt, max_length=self.tokenizer.model_max_length, padding=True, truncation=True,
                               return_tensors="pt")
        ids, am = batch.input_ids.to(dev), batch.attention_mask.to(dev)
        with torch.no_grad():
            pe = self.text_encoder(input_ids=ids, attention_mask=am)[0]
        pe = pe.repeat_interleave(num_samples_per_prompt, 0)
        am = am.repeat_interleave(num_samples_per_prompt, 0)
        ub = self.tokenizer([""] * len(prompt), max_length=pe.shape[1], padding="max_length", truncation=True,
                            return_tensors="pt")
        uids, uam = ub.input_ids.to(dev), ub.attention_mask.to(dev)
        with torch.no_grad():
            ne = self.text_encoder(input_ids=uids, attention_mask=uam)[0]
        ne = ne.repeat_interleave(num_samples_per_prompt, 0)
        uam = uam.repeat_interleave(num_samples_per_prompt, 0)
        host = torch.cat([ub.attention_mask.repeat_interleave(num_samples_per_prompt, 0),
                          batch.attention_mask.repeat_interleave(num_samples_per_prompt, 0)]) == 1      # tokenizer outputs: CPU tensors
        return torch.cat([ne, pe]), (torch.cat([uam, am]) == 1).to(dev), host.cpu()

    def _encode_prompts(self, prompt, samples_per_prompt, guidance_scale, negative_prompt):
        """what every string-level entry point hands its *_from_embeddings form: fp32 embeddings and the mask, [uncond; cond] with the
        tokenizer's HOST mask when guidance is on (`negative_prompt` is read only then), the conditional rows alone and None
        otherwise; each prompt's rows repeated `samples_per_prompt` times"""
        if cfg_enabled(guidance_scale):
            pe, pm, host = self._encode_text_classifier_free(prompt, samples_per_prompt, negative_prompt)
            return pe.float(), pm, host
        pe, pm = self.encode_text(prompt)
        return pe.repeat_interleave(samples_per_prompt, 0).float(), pm.repeat_interleave(samples_per_prompt, 0), None

    def _encode_text_pair(self, prompt, negative_prompt, num_samples_per_prompt):
        """[negative; cond] with both halves at one length: each is tokenised on its own (padding=True: its longest row), then the
        shorter one again with padding="max_length" at the longer one's length -- no row of either is truncated below the
        tokenizer's model_max_length"""
        dev = self.device
        tok = lambda texts, **kw: self.tokenizer(texts, truncation=True, return_tensors="pt", **kw)   # noqa: E731
        limit = self.tokenizer.model_max_length
        cb, nb = tok(list(prompt), max_length=limit, padding=True), tok(negative_prompt, max_length=limit, padding=True)
        L = max(cb.input_ids.shape[1], nb.input_ids.shape[1])
        if cb.input_ids.shape[1] < L:
            cb = tok(list(prompt), max_length=L, padding="max_length")
        if nb.input_ids.shape[1] < L:
            nb = tok(negative_prompt, max_length=L, padding="max_length")
        halves = []
        for b in (nb, cb):
            with torch.no_grad():
                e = self.text_encoder(input_ids=b.input_ids.to(dev), attention_mask=b.attention_mask.to(dev))[0]
            halves.append((e.repeat_interleave(num_samples_per_prompt, 0), b.attention_mask.repeat_interleave(num_samples_per_prompt, 0)))
        host = (torch.cat([halves[0][1], halves[1][1]]) == 1).cpu()
        return torch.cat([halves[0][0], halves[1][0]]), host.to(dev), host

    # ---- latents -----------------------------------------------------------------------------
    def prepare_latents(self, batch_size, inference_scheduler, num_channels_latents, dtype, device, latent_h=256, long_h=None):
        """models.py:259-264 (global torch generator on `device`, like the reference).  `latent_h`: the latent height of the clip
        length, tango_amd.inpaint.duration_geometry(duration)[0] (256 = 10 s).  `long_h`: the canvas height of a long clip
        (tango_amd.inpaint.long_geometry(duration)[0]) instead, which is not on that grid; `latent_h` is then not read."""
        if long_h is not None:
            if int(long_h) != long_h or long_h < 1:
                raise ValueError("long_h must be a positive number of latent rows, got %r" % (long_h,))
            shape = (batch_size, num_channels_latents, int(long_h), 16)
        else:
            shape = (batch_size, num_channels_latents, check_latent_h(latent_h), 16)
        latents = torch.randn(shape, device=device, dtype=dtype)
        return latents * inference_scheduler.init_noise_sigma

    # ---- the hot path ------------------------------------------------------------------------
    def _pad_text(self, embeds, mask, mask_host=None):
        """Static plan shapes: pad L up to a bucket with masked tokens.  Numerically exact: a masked
        key's weight is exp(-10000) == 0 in fp32 (SURVEY.md section 4 differential check).  No mask: every key is valid."""
        if mask is None:
            mask = torch.ones(embeds.shape[:2], dtype=torch.bool, device=embeds.device)
        L = embeds.shape[1]
        if not self.bucket_text_len:
            return embeds, mask, mask_host
        tgt = next((b for b in _TEXT_BUCKETS if b >= L), L)
        if tgt == L:
            return embeds, mask, mask_host
        pe = torch.zeros((embeds.shape[0], tgt, embeds.shape[2]), device=embeds.device, dtype=embeds.dtype)
        pe[:, :L] = embeds
        pm = torch.zeros((mask.shape[0], tgt), device=mask.device, dtype=torch.bool)
        pm[:, :L] = mask
        if mask_host is not None:
            ph = torch.zeros((mask.shape[0], tgt), dtype=torch.bool)
            ph[:, :L] = mask_host
            mask_host = ph
        return pe, pm, mask_host

    def _philox_seed(self, seed):
        """the Philox key of one engine call; counts the call.  The reference draws step noise from torch's global generator
        (randn_tensor in scheduler.step): with no seed given the key is drawn from that generator, so torch.manual_seed() fixes the
        whole trajectory and calls differ -- after the call's latents, which prepare_latents draws from the same generator."""
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if self.seed is None else (int(self.seed) << 20) + self._calls
        self._calls += 1
        return seed

    def _denoise(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale, latents, noise, seed,
                 sample_offset, mask_host=None, known_latents=None, latent_mask=None, blend_noise=None, start=0, count=None,
                 latent_h=256, guidance_rescale=0.0, **extra_conditions):
        """the shared body of the loop of models.py:224-249 / mustango/models.py:563-598: seed derivation, text bucketing, scheduler
        tables, one engine call (`extra_conditions`: the Music UNet's beat / chord streams; `known_latents` / `latent_mask` /
        `blend_noise`: the masked loop of audioldm/ldm.py:724-818, Engine.denoise).  `start` > 0: the truncated loop of an edit over
        `timesteps[start:]` with the scheduler's truncated tables; `count`: the first `count` steps of a DDIMInverseScheduler.
        The clip length is the height of `latents` (a height of the duration grid); `latent_h` sizes the latents drawn here when
        none are given.  `guidance_scale`: a scalar, or a per-sample [B] / per-step [N, B] table (scheduler.guidance_table; N counts
        the EXECUTED steps of a truncated loop); `guidance_rescale`: phi of Engine.denoise."""
        cfg_on = cfg_enabled(guidance_scale)
        guidance_rescale = check_guidance_rescale(guidance_scale, guidance_rescale)
        B = prompt_embeds.shape[0] // 2 if cfg_on else prompt_embeds.shape[0]
        inference_scheduler = _own_scheduler(inference_scheduler)
        inference_scheduler.set_timesteps(num_steps, device=self.device)
        if count is not None:
            timesteps, coef, window = inference_scheduler.timesteps[:count], inference_scheduler.coef_table(count=count), {}
        elif start:
            timesteps, coef, window = inference_scheduler.timesteps[start:], inference_scheduler.coef_table(start=start), dict(start=start)
        else:
            timesteps, coef, window = inference_scheduler.timesteps, inference_scheduler.coef_table(), {}
        if latents is None:
            if known_latents is not None and torch.is_tensor(known_latents) and known_latents.dim() == 4:
                latent_h = known_latents.shape[2]             # a masked loop runs at the known clip's length
            latents = self.prepare_latents(B, inference_scheduler, self.unet.config.in_channels, torch.float32, self.device,
                                           latent_h=latent_h)
        latents = latents.to(self.device, torch.float32).contiguous().clone()
        if latents.dim() != 4:
            raise ValueError("latents must be [B, C, H, W], got %s" % (tuple(latents.shape),))
        # (the mask is NOT moved here: a host mask reaches the engine as a host pointer too, which spares the call its only host sync)
        pe, pm, mask_host = self._pad_text(prompt_embeds.to(self.device), boolean_prompt_mask, mask_host)
        c = inference_scheduler.config
        seed = self._philox_seed(seed)
        masking = {}
        if known_latents is not None or latent_mask is not None:
            masking = dict(known_latents=known_latents, latent_mask=latent_mask, blend_coef=inference_scheduler.blend_table(**window),
                           blend_noise=blend_noise)
        elif blend_noise is not None:
            raise ValueError("blend_noise needs known_latents and latent_mask")
        table = guidance_table(guidance_scale, len(timesteps), latents.shape[0])
        self.engine.denoise(latents, pe, pm, timesteps.cpu().numpy(), coef, 1.0 if table is not None else guidance_scale,
                            guidance_table=table, guidance_rescale=guidance_rescale,
                            prediction_type=c.prediction_type, rule=inference_scheduler.rule, clip_sample=c.clip_sample,
                            clip_sample_range=getattr(c, "clip_sample_range", 1.0), noise=noise, seed=seed,
                            sample_offset=sample_offset, use_graph=self.use_graph, prompt_mask_host=mask_host,
                            latent_h=check_latent_h(latents.shape[2]), **masking, **extra_conditions)
        return latents

    @torch.no_grad()
    def inference_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20,
                                  guidance_scale=3, latents=None, noise=None, seed=None, sample_offset=0, mask_host=None, duration=10,
                                  guidance_rescale=0.0):
        """Loop of models.py:224-249 given the encoder outputs ([uncond; cond] when guidance > 1).  `mask_host`: optional CPU copy of
        a device-resident `boolean_prompt_mask` (see Engine.denoise).  `duration` (seconds, 2.5 .. 20 on the 2.5 s grid) sizes the
        initial latents when `latents` is None; given latents carry their own height.  `guidance_scale` may be a per-sample [B] or
        per-step [N, B] table and `guidance_rescale` the rescale factor phi (_denoise)."""
        return self._denoise(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale, latents, noise, seed,
                             sample_offset, mask_host=mask_host, latent_h=duration_geometry(duration)[0],
                             guidance_rescale=guidance_rescale)

    @torch.no_grad()
    def inference(self, prompt, inference_scheduler, num_steps=20, guidance_scale=3, num_samples_per_prompt=1,
                  disable_progress=True, duration=10, negative_prompt=None, guidance_rescale=0.0):
        """models.py:210-257 (same signature, same return: latents [B*S, 8, 256, 16]); `duration` seconds of audio instead of 10:
        latents [B*S, 8, int(duration * 25.6), 16] (audioldm/pipeline.py:94-95,113-126).  `negative_prompt` (None, a str or one str per
        prompt) replaces the empty unconditional text; it is read only when guidance is on."""
        pe, pm, host = self._encode_prompts(prompt, num_samples_per_prompt, guidance_scale, negative_prompt)
        return self.inference_from_embeddings(pe, pm, inference_scheduler, num_steps, guidance_scale, mask_host=host,
                                              duration=duration, guidance_rescale=guidance_rescale)

    # ---- clips longer than 20 s: MultiDiffusion windows in time (the fork's pipeline_stable_diffusion_panorama.py:442-456, 614-652) ----
    @torch.no_grad()
    def inference_long_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3,
                                       duration=30, window=10, hop=5, latents=None, noise=None, seed=None, sample_offset=0,
                                       mask_host=None):
        """inference_from_embeddings for a clip of `duration` > `window` seconds: the canvas [B, 8, H, 16] (H = int(duration * 25.6))
        is denoised as V overlapping windows of `window` seconds every `hop` seconds (tango_amd.inpaint.long_geometry), every window
        under its sample's text, the per-view updates averaged on the canvas at every step (Engine.denoise_windows).
        `prompt_embeds` / `boolean_prompt_mask` as in inference_from_embeddings ([uncond; cond] with guidance): their rows are repeated
        per window here.  `noise` [N, B, 8, H, 16] is canvas-shaped.  DDPM and DDIM schedulers; a DPM-Solver scheduler, a guidance
        table and a rescale are refused."""
        return self._windowed_from_embeddings(False, long_geometry(duration, window, hop), prompt_embeds, boolean_prompt_mask,
                                              inference_scheduler, num_steps, guidance_scale, duration, latents, noise, seed,
                                              sample_offset, mask_host)

    def _windowed_from_embeddings(self, ring, geometry, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale,
                                  duration, latents, noise, seed, sample_offset, mask_host, window_prompt=None, num_samples=1,
                                  view_weights=None):
        """inference_long_from_embeddings (ring False: Engine.denoise_windows) and inference_loop_from_embeddings (ring True:
        Engine.denoise_ring) once the geometry is known.  `window_prompt` (inference_timeline_from_embeddings): the embedding rows
        are per SEGMENT, window v of each of the `num_samples` samples takes row window_prompt[v] of its half; `view_weights` goes to
        the engine."""
        H, hw, stride, V = geometry
        how = "on a ring" if ring else "with windows"
        if not isinstance(guidance_scale, (int, float)):
            raise ValueError("a guidance table is not supported %s: guidance_scale must be a scalar" % how)
        inference_scheduler = _own_scheduler(inference_scheduler)
        if inference_scheduler.rule == "dpmsolver":
            raise ValueError("the multistep DPM-Solver rule is not supported on a ring: use DDPM or DDIM" if ring else
                             "the multistep DPM-Solver rule is not supported with windows (a per-view history has no reference "
                             "behaviour): use DDPM or DDIM")
        cfg_on = guidance_scale > 1.0
        B = prompt_embeds.shape[0] // 2 if cfg_on else prompt_embeds.shape[0]
        if window_prompt is not None:
            S, B = B, int(num_samples)                # B counted the segments
            window_prompt = [int(i) for i in window_prompt]
            if len(window_prompt) != V or not all(0 <= i < S for i in window_prompt):
                raise ValueError("window_prompt must hold %d segment indices below %d (one per window), got %r" % (V, S, window_prompt))
            if B < 1:
                raise ValueError("num_samples must be positive, got %r" % (num_samples,))
        inference_scheduler.set_timesteps(num_steps, device=self.device)
        if latents is None:
            latents = self.prepare_latents(B, inference_scheduler, self.unet.config.in_channels, torch.float32, self.device, long_h=H)
        latents = latents.to(self.device, torch.float32).contiguous().clone()
        if latents.dim() != 4 or latents.shape[0] != B or latents.shape[2] != H:
            raise ValueError("latents must be [%d, C, %d, W] for %r s, got %s" % (B, H, duration, tuple(latents.shape)))
        pe, pm, mask_host = self._pad_text(prompt_embeds.to(self.device), boolean_prompt_mask, mask_host)
        if window_prompt is None:
            # one row per window, row half * B * V + b * V + v: each half's rows repeated V times in place
            pe, pm = pe.repeat_interleave(V, 0), pm.repeat_interleave(V, 0)
            mask_host = mask_host.repeat_interleave(V, 0) if mask_host is not None else None
        else:
            # the same row order, gathered from the per-segment rows: row half * S + window_prompt[v] for every sample
            idx = torch.tensor([half * S + i for half in range(2 if cfg_on else 1) for _ in range(B) for i in window_prompt])
            pe, pm = pe.index_select(0, idx.to(pe.device)), pm.index_select(0, idx.to(pm.device))
            mask_host = mask_host.index_select(0, idx) if mask_host is not None else None
        c = inference_scheduler.config
        seed = self._philox_seed(seed)
        run = self.engine.denoise_ring if ring else self.engine.denoise_windows
        run(latents, pe, pm, inference_scheduler.timesteps.cpu().numpy(), inference_scheduler.coef_table(), guidance_scale, window_h=hw,
            stride=stride, prediction_type=c.prediction_type, rule=inference_scheduler.rule, clip_sample=c.clip_sample,
            clip_sample_range=getattr(c, "clip_sample_range", 1.0), noise=noise, seed=seed, sample_offset=sample_offset,
            use_graph=self.use_graph, prompt_mask_host=mask_host, view_weights=view_weights)
        return latents

    @torch.no_grad()
    def inference_long(self, prompt, inference_scheduler, num_steps=20, guidance_scale=3, num_samples_per_prompt=1, duration=30,
                       window=10, hop=5, negative_prompt=None, seed=None, sample_offset=0):
        """inference() for a clip longer than `window` seconds (inference_long_from_embeddings): latents [B*S, 8, int(duration * 25.6), 16]"""
        long_geometry(duration, window, hop)
        pe, pm, host = self._encode_prompts(prompt, num_samples_per_prompt, guidance_scale, negative_prompt)
        return self.inference_long_from_embeddings(pe, pm, inference_scheduler, num_steps, guidance_scale, duration, window, hop,
                                                   seed=seed, sample_offset=sample_offset, mask_host=host)

    # ---- seamless loops: the same windows on a ring in time (include/tango_engine.h tango_engine_denoise_ring) ----------------------
    @torch.no_grad()
    def inference_loop_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3,
                                       duration=10, window=None, hop=None, latents=None, noise=None, seed=None, sample_offset=0,
                                       mask_host=None):
        """inference_long_from_embeddings for a clip that is played in a loop: the canvas [B, 8, H, 16] (H = duration * 25.6) is a ring
        in time, denoised as V = H / stride windows that wrap round it (tango_amd.inpaint.loop_geometry; Engine.denoise_ring), so row
        H - 1 joins row 0 as any two neighbouring rows join.  `duration` >= `window`; by default one window of the clip's own length
        (up to 10 s) every half window.  The other arguments and the refusals are inference_long_from_embeddings'."""
        return self._windowed_from_embeddings(True, loop_geometry(duration, window, hop), prompt_embeds, boolean_prompt_mask,
                                              inference_scheduler, num_steps, guidance_scale, duration, latents, noise, seed,
                                              sample_offset, mask_host)

    @torch.no_grad()
    def inference_loop(self, prompt, inference_scheduler, num_steps=20, guidance_scale=3, num_samples_per_prompt=1, duration=10,
                       window=None, hop=None, negative_prompt=None, seed=None, sample_offset=0):
        """inference() for a seamless loop (inference_loop_from_embeddings): ring latents [B*S, 8, duration * 25.6, 16]"""
        loop_geometry(duration, window, hop)
        pe, pm, host = self._encode_prompts(prompt, num_samples_per_prompt, guidance_scale, negative_prompt)
        return self.inference_loop_from_embeddings(pe, pm, inference_scheduler, num_steps, guidance_scale, duration, window, hop,
                                                   seed=seed, sample_offset=sample_offset, mask_host=host)

    # ---- timed prompts: a prompt per window and tapered view weights (include/tango_engine.h tango_engine_denoise_windows_weighted) ----
    @torch.no_grad()
    def inference_timeline_from_embeddings(self, prompt_embeds, boolean_prompt_mask, window_prompt, inference_scheduler, num_steps=20,
                                           guidance_scale=3, duration=30, window=10, hop=5, loop=False, taper=True, num_samples=1,
                                           latents=None, noise=None, seed=None, sample_offset=0, mask_host=None):
        """inference_long_from_embeddings (`loop` False) or inference_loop_from_embeddings (`loop` True) with a prompt per window: the
        region-based half of MultiDiffusion (Bar-Tal et al. 2023, section 4.2) in time.  `prompt_embeds` / `boolean_prompt_mask` hold
        one row per SEGMENT ([uncond; cond] with guidance: 2 S rows), `window_prompt` the segment index of each of the V windows
        (tango_amd.inpaint.timeline_geometry); each of the `num_samples` samples runs the same timeline.  `taper` True: the per-view
        updates are averaged with tango_amd.inpaint.window_taper's weights, so a view fades out towards its edges and the prompts
        cross-fade over the overlaps; False: the equal weights of the long clip and the loop.  The refusals are theirs."""
        geometry = loop_geometry(duration, window, hop) if loop else long_geometry(duration, window, hop)
        weights = window_taper(geometry[1], geometry[2]) if taper else None
        return self._windowed_from_embeddings(bool(loop), geometry, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps,
                                              guidance_scale, duration, latents, noise, seed, sample_offset, mask_host,
                                              window_prompt=window_prompt, num_samples=num_samples, view_weights=weights)

    @torch.no_grad()
    def inference_timeline(self, segments, inference_scheduler, num_steps=20, guidance_scale=3, num_samples=1, duration=30, window=10,
                           hop=5, loop=False, taper=True, negative_prompt=None, seed=None, sample_offset=0):
        """inference() for a timeline of prompts: `segments` = [(prompt, start_seconds), ...] (tango_amd.inpaint.timeline_geometry).
        `negative_prompt`: None, one str, or one str per segment.  Latents [num_samples, 8, duration * 25.6, 16]."""
        window_prompt = timeline_geometry(segments, duration, window, hop, loop)[4]
        prompts = [p for p, _ in segments]
        pe, pm, host = self._encode_prompts(prompts, 1, guidance_scale, negative_prompt)
        return self.inference_timeline_from_embeddings(pe, pm, window_prompt, inference_scheduler, num_steps, guidance_scale,
                                                       duration, window, hop, loop, taper, num_samples, seed=seed,
                                                       sample_offset=sample_offset, mask_host=host)

    # ---- masked-latent inpainting (audioldm/pipeline.py:249-301, ldm.py:724-818, ddim.py:207-233) ------------------------------
    @torch.no_grad()
    def inpaint_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3, *,
                                known_latents, latent_mask, latents=None, noise=None, blend_noise=None, seed=None, sample_offset=0,
                                mask_host=None, guidance_rescale=0.0):
        """The loop of inference_from_embeddings with the region where `latent_mask` [B, 1, 256, 16] is 1 held to the known latents
        `known_latents` [B, 8, 256, 16] (scale_factor * posterior sample of the encoded mel): before every UNet call the latents
        become inference_scheduler.add_noise(known, n_i, t_i) * m + (1 - m) * latents (ddim.py:210-217), none after the last step.
        `blend_noise` [N, B, 8, 256, 16] injects the n_i; by default they come from the engine's Philox generator under `seed`."""
        return self._denoise(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale, latents, noise, seed,
                             sample_offset, mask_host=mask_host, known_latents=known_latents, latent_mask=latent_mask,
                             blend_noise=blend_noise, guidance_rescale=guidance_rescale)

    @torch.no_grad()
    def inpaint(self, prompt, known_latents, latent_mask, inference_scheduler, num_steps=20, guidance_scale=3, num_samples_per_prompt=1,
                negative_prompt=None, guidance_rescale=0.0):
        """inference() with masking: `known_latents` [K, 8, 256, 16] and `latent_mask` [K, 1, 256, 16] for the K prompts; with
        num_samples_per_prompt = S > 1, row k * S + j of the result pairs with clip k (the repeat_interleave order of the text
        embeddings, not ldm.py:791's candidate-major cat).  Returns latents [K * S, 8, 256, 16]."""
        S = num_samples_per_prompt
        if known_latents.shape[0] != len(prompt) or latent_mask.shape[0] != len(prompt):
            raise ValueError("known_latents and latent_mask need one row per prompt (%d), got %d and %d"
                             % (len(prompt), known_latents.shape[0], latent_mask.shape[0]))
        pe, pm, host = self._encode_prompts(prompt, S, guidance_scale, negative_prompt)
        return self.inpaint_from_embeddings(pe, pm, inference_scheduler, num_steps, guidance_scale,
                                            known_latents=known_latents.repeat_interleave(S, 0),
                                            latent_mask=latent_mask.repeat_interleave(S, 0), mask_host=host,
                                            guidance_rescale=guidance_rescale)

    # ---- audio-to-audio editing (audioldm/pipeline.py:145-247 style_transfer; latent_diffusion/ddim.py:246-304) ------------------
    @torch.no_grad()
    def edit_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3, *,
                             start_latents, strength, known_latents=None, latent_mask=None, noise=None, blend_noise=None, seed=None,
                             sample_offset=0, mask_host=None, guidance_rescale=0.0, **conditions):
        """The last k = int(strength * num_steps) steps of the loop of inference_from_embeddings, from `start_latents` [B, 8, 256,
        16]: an existing clip's latents noised (AutoencoderKL.encode_start_latents) or inverted (invert_from_embeddings) to the
        level `inference_scheduler.edit_plan(num_steps, strength)` names.  The engine runs `timesteps[start:]` with the scheduler's
        truncated tables; the multistep DPM-Solver restarts its order ramp at the first executed step.  `noise` / `blend_noise`
        hold one entry per EXECUTED step ([k, B, 8, 256, 16]).  With `known_latents` / `latent_mask` it is a regional edit: the
        region where the mask is 1 keeps the clip's audio (the masked loop of inpaint_from_embeddings), the rest is edited.
        `conditions`: what a subclass's UNet takes beside the text (_extra_conditions)."""
        inference_scheduler = _own_scheduler(inference_scheduler)
        if start_latents is None:
            raise ValueError("an edit starts from start_latents")
        start, _ = inference_scheduler.edit_plan(num_steps, strength)
        return self._denoise(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale, start_latents, noise,
                             seed, sample_offset, mask_host=mask_host, known_latents=known_latents, latent_mask=latent_mask,
                             blend_noise=blend_noise, start=start, guidance_rescale=guidance_rescale,
                             **self._extra_conditions(**conditions))

    @torch.no_grad()
    def edit(self, prompt, start_latents, inference_scheduler, num_steps=20, guidance_scale=3, strength=0.5, num_samples_per_prompt=1,
             known_latents=None, latent_mask=None, seed=None, negative_prompt=None, guidance_rescale=0.0):
        """edit_from_embeddings() for prompt strings, encoded like inference() / inpaint(): `start_latents` (and `known_latents`
        / `latent_mask` when given) hold one row per prompt and sample, row k * S + j for sample j of prompt k."""
        S = num_samples_per_prompt
        if start_latents.shape[0] != len(prompt) * S:
            raise ValueError("start_latents need one row per prompt and sample (%d), got %d" % (len(prompt) * S, start_latents.shape[0]))
        pe, pm, host = self._encode_prompts(prompt, S, guidance_scale, negative_prompt)
        return self.edit_from_embeddings(pe, pm, inference_scheduler, num_steps, guidance_scale, start_latents=start_latents,
                                         strength=strength, known_latents=known_latents, latent_mask=latent_mask, seed=seed,
                                         mask_host=host, guidance_rescale=guidance_rescale)

    @torch.no_grad()
    def invert_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, *, latents, count,
                               guidance_scale=1.0, mask_host=None, **conditions):
        """DDIM inversion, the deterministic encoder of an edit: `count` steps of DDIMInverseScheduler (ascending timesteps, the
        inverse coefficient table, no step noise) from clean `latents` through the same fused loop, under the text the clip is
        described by (`guidance_scale` 1: no CFG, `prompt_embeds` hold the B conditional rows only).  `inference_scheduler`: a
        DDIMInverseScheduler, or a sampler: the inverse scheduler is then built on its noise schedule and walks its timesteps
        upward (DDIMInverseScheduler.from_scheduler), so that after `count` = k steps the latents sit exactly on the sampler's
        `edit_plan(num_steps, k / num_steps)` encode timestep `timesteps[num_steps - k - 1]`, DDIM and DPM-Solver alike.  A bare
        DDIMInverseScheduler keeps the fork's grid `arange(0, n) * ratio + steps_offset` and lands on its own `timesteps[k]`."""
        inv = _inverse_scheduler(inference_scheduler)
        if latents is None:
            raise ValueError("inversion starts from the clip's clean latents")
        return self._denoise(prompt_embeds, boolean_prompt_mask, inv, num_steps, guidance_scale, latents, None, 0, 0,
                             mask_host=mask_host, count=int(count), **self._extra_conditions(**conditions))

    def _extra_conditions(self):
        """the engine's keywords for what the UNet takes beside the text: nothing here (a keyword given is a TypeError)"""
        return {}


def _own_scheduler(scheduler):
    """a diffusers / fork scheduler object (the reference's loop takes any) -> the engine's class of the same name and config"""
    return scheduler if hasattr(scheduler, "coef_table") else from_diffusers(scheduler)


def _inverse_scheduler(scheduler):
    scheduler = _own_scheduler(scheduler)
    if isinstance(scheduler, DDIMInverseScheduler):
        return scheduler
    return DDIMInverseScheduler.from_scheduler(scheduler)


class MusicAudioDiffusion(AudioDiffusion):
    """Inference side of Mustango's `MusicAudioDiffusion` (mustango/models.py:312-740) on the engine: the UNet is
    UNet2DConditionModelMusic (mustango/configs/music_diffusion_model_config.json -- every cross-attention site attends to the
    text, then the beat, then the chord embeddings) and the loop of mustango/models.py:563-598 runs as the same captured
    hipGraph step with three condition tensors bound.

    What stays with the caller, exactly like the T5 encoder of `AudioDiffusion`: the symbolic front-end that turns beat / chord
    annotations into embeddings -- `beat_tokenizer`, `chord_tokenizer`, `Beat_Embedding`, `Chord_Embedding`,
    `Fundamental_Music_Embedding`, `Music_PositionalEncoding` (mustango/layers/layers.py, mustango/models.py:376-388,433-467):
    small trainable torch modules whose outputs ([B, 50, 1024] beats, [B, 20, 1024] chords and their masks,
    `encode_beats_classifier_free` / `encode_chords_classifier_free` ordered [uncond; cond]) are this class's inputs."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if not self.unet_config.get("music"):
            raise ValueError("MusicAudioDiffusion needs a UNet config with *Music blocks (mustango/configs/music_diffusion_model_config.json)")

    @torch.no_grad()
    def inference_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3,
                                  latents=None, noise=None, seed=None, sample_offset=0, *, encoded_beats=None, beat_mask=None,
                                  encoded_chords=None, chord_mask=None, known_latents=None, latent_mask=None, blend_noise=None,
                                  duration=10, guidance_rescale=0.0):
        """mustango/models.py:540-598 given the three encoder outputs ([uncond; cond] when guidance > 1); with `known_latents` /
        `latent_mask` (/ `blend_noise`) the masked loop of AudioDiffusion.inpaint_from_embeddings.  `duration` sizes the initial
        latents when none are given, as in AudioDiffusion.inference_from_embeddings."""
        conditions = self._extra_conditions(encoded_beats, beat_mask, encoded_chords, chord_mask)
        return self._denoise(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale, latents, noise, seed,
                             sample_offset, known_latents=known_latents, latent_mask=latent_mask, blend_noise=blend_noise,
                             latent_h=duration_geometry(duration)[0], guidance_rescale=guidance_rescale, **conditions)

    @torch.no_grad()
    def inpaint_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3, *,
                                known_latents, latent_mask, latents=None, noise=None, blend_noise=None, seed=None, sample_offset=0,
                                encoded_beats=None, beat_mask=None, encoded_chords=None, chord_mask=None, guidance_rescale=0.0):
        """AudioDiffusion.inpaint_from_embeddings with the beat / chord streams of inference_from_embeddings"""
        return self.inference_from_embeddings(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale,
                                              latents, noise, seed, sample_offset, encoded_beats=encoded_beats, beat_mask=beat_mask,
                                              encoded_chords=encoded_chords, chord_mask=chord_mask, known_latents=known_latents,
                                              latent_mask=latent_mask, blend_noise=blend_noise, guidance_rescale=guidance_rescale)

    def _extra_conditions(self, encoded_beats=None, beat_mask=None, encoded_chords=None, chord_mask=None):
        if encoded_beats is None or encoded_chords is None:
            raise ValueError("encoded_beats and encoded_chords are required (mustango/models.py:548-550)")
        return dict(beat_embeds=encoded_beats, beat_mask=beat_mask, chord_embeds=encoded_chords, chord_mask=chord_mask)

    @torch.no_grad()
    def edit_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, guidance_scale=3, *,
                             start_latents, strength, known_latents=None, latent_mask=None, noise=None, blend_noise=None, seed=None,
                             sample_offset=0, encoded_beats=None, beat_mask=None, encoded_chords=None, chord_mask=None,
                             guidance_rescale=0.0):
        """AudioDiffusion.edit_from_embeddings with the beat / chord streams of inference_from_embeddings"""
        return super().edit_from_embeddings(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, guidance_scale,
                                            start_latents=start_latents, strength=strength, known_latents=known_latents,
                                            latent_mask=latent_mask, noise=noise, blend_noise=blend_noise, seed=seed,
                                            sample_offset=sample_offset, guidance_rescale=guidance_rescale, encoded_beats=encoded_beats,
                                            beat_mask=beat_mask, encoded_chords=encoded_chords, chord_mask=chord_mask)

    @torch.no_grad()
    def invert_from_embeddings(self, prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps=20, *, latents, count,
                               guidance_scale=1.0, encoded_beats=None, beat_mask=None, encoded_chords=None, chord_mask=None):
        """AudioDiffusion.invert_from_embeddings with the beat / chord streams of inference_from_embeddings"""
        return super().invert_from_embeddings(prompt_embeds, boolean_prompt_mask, inference_scheduler, num_steps, latents=latents,
                                              count=count, guidance_scale=guidance_scale, encoded_beats=encoded_beats,
                                              beat_mask=beat_mask, encoded_chords=encoded_chords, chord_mask=chord_mask)

    def edit(self, *a, **k):
        raise NotImplementedError("strings / beat and chord annotations are encoded by the caller's Mustango front-end modules; "
                                  "pass their outputs to edit_from_embeddings()")

    def inpaint(self, *a, **k):
        raise NotImplementedError("strings / beat and chord annotations are encoded by the caller's Mustango front-end modules; "
                                  "pass their outputs to inpaint_from_embeddings()")

    def inference(self, *a, **k):
        raise NotImplementedError("strings / beat and chord annotations are encoded by the caller's Mustango front-end modules; "
                                  "pass their outputs to inference_from_embeddings()")
