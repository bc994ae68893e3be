"""`Tango` -- drop-in for tango.py:9-64 of the reference: same constructor, `generate`,
`generate_for_batch`; the three hot calls (inference -> decode_first_stage -> decode_to_waveform) run
on the HIP engine.  `name` may be a local directory holding the HF snapshot files
(vae_config.json, main_config.json, pytorch_model_{vae,main}.bin); hub download is attempted otherwise.
"""
import json
import os

import numpy as np
import torch

from .autoencoder import AutoencoderKL
from .inpaint import clip_duration, duration_geometry, latent_mask, long_geometry, loop_geometry, prepare_waveform, timeline_geometry
from .models import AudioDiffusion
from .scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
from .scheduler import cfg_enabled, check_guidance_rescale, guidance_is_table
from .stft import wav_to_fbank

_CONFIG_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")


class Tango:
    def __init__(self, name="declare-lab/tango", device="cuda:0", dtype="fp16", scheduler_config=None, text_encoder=None,
                 tokenizer=None, with_encoder=False):
        """`text_encoder` / `tokenizer` (optional): already-built T5EncoderModel / tokenizer, e.g. from a local directory
        on a box without hub access; the checkpoint's `text_encoder.*` tensors are loaded into it like the reference does.
        `with_encoder`: also build the mel-VAE encoder (the checkpoint holds its weights), which `inpaint` needs."""
        if os.path.isdir(name):
            path = name
        else:
            from huggingface_hub import snapshot_download   # tango.py:12
            path = snapshot_download(repo_id=name)
        vae_config = json.load(open("{}/vae_config.json".format(path)))
        main_config = json.load(open("{}/main_config.json".format(path)))
        self.vae = AutoencoderKL(**vae_config, dtype=dtype, device=device, with_encoder=with_encoder)
        # tango.py:17-27: the wave -> mel front-end and its buffers (generation never calls it; training / evaluation callers
        # reach it as `tango.stft`, inference.py:81).  Snapshots without the two files simply have no `stft`.
        self.stft = None
        if os.path.exists("{}/stft_config.json".format(path)) and os.path.exists("{}/pytorch_model_stft.bin".format(path)):
            from .stft import TacotronSTFT
            self.stft = TacotronSTFT(**json.load(open("{}/stft_config.json".format(path))), device=device)
            self.stft.load_state_dict(torch.load("{}/pytorch_model_stft.bin".format(path), map_location="cpu"))
            self.stft.eval()
        cfg_path = main_config.get("unet_model_config_path")
        if cfg_path is None or not os.path.exists(cfg_path):
            # the reference resolves configs/diffusion_model_config.json relative to the cwd (models.py:83-85)
            base = os.path.basename(cfg_path) if cfg_path else "diffusion_model_config.json"
            cfg_path = os.path.join(_CONFIG_DIR, base)
        main_config = dict(main_config, unet_model_config_path=cfg_path)
        self.model = AudioDiffusion(**main_config, dtype=dtype, device=device, text_encoder=text_encoder, tokenizer=tokenizer)
        vae_weights = torch.load("{}/pytorch_model_vae.bin".format(path), map_location="cpu")
        main_weights = torch.load("{}/pytorch_model_main.bin".format(path), map_location="cpu")
        self.vae.load_state_dict(vae_weights)
        self.model.load_state_dict(main_weights)
        print("Successfully loaded checkpoint from:", name)
        self.vae.eval()
        self.model.eval()
        # tango.py:36 pulls stabilityai/stable-diffusion-2-1's scheduler JSON from the hub; config is data here
        self.scheduler = DDPMScheduler.from_config(_ddpm_keys(scheduler_config or SD21_SCHEDULER_CONFIG))

    @classmethod
    def from_components(cls, model: AudioDiffusion, vae: AutoencoderKL, scheduler=None, stft=None):
        """Assemble from already-built components (synthetic-weight benchmarks, tests)."""
        self = cls.__new__(cls)
        self.model, self.vae, self.stft = model, vae, stft
        self.scheduler = scheduler or DDPMScheduler.from_config(_ddpm_keys(SD21_SCHEDULER_CONFIG))
        return self

    def chunks(self, lst, n):
        """ Yield successive n-sized chunks from a list. """
        for i in range(0, len(lst), n):
            yield lst[i:i + n]

    @staticmethod
    def _check_guidance(guidance, guidance_rescale):
        """the guidance argument checks that need no device: guidance_rescale in [0, 1], and > 0 only with guidance on"""
        return check_guidance_rescale(guidance, guidance_rescale)

    @staticmethod
    def _slice_per_batch(value, k, n, rows_per_prompt=1):
        """prompts k .. k + n - 1 of a per-prompt list, or their latents rows (the last axis) of a guidance table; anything else as it is"""
        if isinstance(value, (list, tuple)) and all(isinstance(v, str) for v in value):
            return list(value[k:k + n])
        if value is not None and guidance_is_table(value):
            value = value if torch.is_tensor(value) else np.asarray(value)
            return value[..., k * rows_per_prompt:(k + n) * rows_per_prompt]
        return value

    def generate(self, prompt, steps=100, guidance=3, samples=1, disable_progress=True, duration=10, negative_prompt=None,
                 guidance_rescale=0.0):
        """ Generate audio for a single prompt string. (tango.py:43-49)  `duration`: seconds of audio, 2.5 .. 20 on the 2.5 s grid
        (audioldm/pipeline.py:113-126 text_to_audio); a ValueError for anything else.

        `negative_prompt`: text the result is steered away from (the unconditional half of the guidance batch; None: the empty
        text, as the reference).  `guidance`: a scalar, or one scale per sample ([samples]) or per step and sample ([steps,
        samples]).  `guidance_rescale` in [0, 1]: Lin et al. 2023, pulls the guided output back to the conditional output's
        per-sample standard deviation (0 = off). """
        self._check_guidance(guidance, guidance_rescale)
        with torch.no_grad():
            latents = self.model.inference([prompt], self.scheduler, steps, guidance, samples, disable_progress=disable_progress,
                                           duration=duration, negative_prompt=negative_prompt, guidance_rescale=guidance_rescale)
            mel = self.vae.decode_first_stage(latents)
            wave = self.vae.decode_to_waveform(mel)
        return wave[0]

    #: UNet rows of one engine call of generate_long: the benchmarked batch, which is known to fit
    LONG_MAX_ROWS = 64

    def generate_long(self, prompt, duration, steps=100, guidance=3, samples=1, window=10, hop=5, negative_prompt=None, seed=None):
        """ Generate `duration` > `window` seconds of audio for a single prompt string: MultiDiffusion in time.  The clip is denoised as
        V overlapping windows of `window` seconds (a length of generate()'s grid) every `hop` seconds, averaged on one latent canvas at
        every step (AudioDiffusion.inference_long), decoded window by window with a cross-fade of the overlaps
        (Engine.vae_decode_tiled) and vocoded in one piece.  `duration` must be window + k * hop (tango_amd.inpaint.long_geometry names
        the neighbours otherwise), at most 32 windows.  Works with the configured DDPM or a DDIM scheduler; a DPM-Solver scheduler is
        refused.  `seed`: the Philox key of the step noise (None: from torch's generator); the canvas noise comes from torch's
        generator, like generate()'s.  Samples are chunked so that one engine call runs at most 64 UNet rows.
        Returns np.int16 [samples, vocoder_samples(4 * H)]. """
        H, hw, stride, V = long_geometry(duration, window, hop)
        if not isinstance(guidance, (int, float)):
            raise ValueError("a guidance table is not supported with windows: guidance must be a scalar")
        if getattr(self.scheduler, "rule", None) == "dpmsolver":
            raise ValueError("the multistep DPM-Solver rule is not supported with windows (a per-view history has no reference "
                             "behaviour): use DDPM or DDIM")
        per_call = max(1, self.LONG_MAX_ROWS // ((2 if cfg_enabled(guidance) else 1) * V))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        waves = []
        with torch.no_grad():
            for k in range(0, samples, per_call):
                n = min(per_call, samples - k)
                latents = self.model.inference_long([prompt], self.scheduler, steps, guidance, n, duration, window, hop,
                                                    negative_prompt=negative_prompt, seed=seed, sample_offset=k)
                mel = self.vae.engine.vae_decode_tiled(latents, hw, stride)
                waves.append(self.vae.decode_to_waveform(mel))
        return np.concatenate(waves)

    def generate_loop(self, prompt, duration, steps=100, guidance=3, samples=1, window=None, hop=None, negative_prompt=None, seed=None):
        """ Generate `duration` seconds of audio that plays in a loop without a click or a jump at the wrap: MultiDiffusion on a ring in
        time.  The latent canvas is a ring, denoised as V windows of `window` seconds every `hop` seconds that wrap round it
        (AudioDiffusion.inference_loop), decoded window by window with every tile cross-faded into both neighbours
        (Engine.vae_decode_ring) and vocoded with circular context (Engine.vocode_ring).  `window` defaults to `duration` when that is
        a length of generate()'s grid of at most 10 s, else to 10; `hop` to window / 2; `duration` must be a whole number of hops
        (tango_amd.inpaint.loop_geometry names the neighbours otherwise), at most 32 windows.  DDPM or DDIM scheduler; a DPM-Solver
        scheduler and a guidance table are refused.  `seed` and the chunking of samples as in generate_long.
        Returns np.int16 [samples, 640 * H]: exactly the ring's samples (163 840 for 10 s, where generate() returns 163 872). """
        H, hw, stride, V = loop_geometry(duration, window, hop)
        if not isinstance(guidance, (int, float)):
            raise ValueError("a guidance table is not supported on a ring: guidance must be a scalar")
        if getattr(self.scheduler, "rule", None) == "dpmsolver":
            raise ValueError("the multistep DPM-Solver rule is not supported on a ring: use DDPM or DDIM")
        per_call = max(1, self.LONG_MAX_ROWS // ((2 if cfg_enabled(guidance) else 1) * V))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        waves = []
        with torch.no_grad():
            for k in range(0, samples, per_call):
                n = min(per_call, samples - k)
                latents = self.model.inference_loop([prompt], self.scheduler, steps, guidance, n, duration, window, hop,
                                                    negative_prompt=negative_prompt, seed=seed, sample_offset=k)
                mel = self.vae.engine.vae_decode_ring(latents, hw, stride)
                waves.append(self.vae.engine.vocode_ring(mel).cpu().numpy())
        return np.concatenate(waves)

    def generate_timeline(self, segments, duration, steps=100, guidance=3, samples=1, window=10, hop=5, loop=False, taper=True,
                          negative_prompt=None, seed=None):
        """ Generate `duration` seconds of audio that follows a timeline of prompts, e.g. [("rain", 0), ("thunder rolls in", 12.5),
        ("birds after the storm", 22)]: `segments` is a list of (prompt, start_seconds) with ascending starts, the first at 0.  The
        clip is cut into windows as generate_long cuts it (`loop` False: tiled decode, then the vocoder) or as generate_loop does
        (`loop` True: ring decode, then the ring vocoder); every window runs under the prompt of the segment that holds its centre
        (tango_amd.inpaint.timeline_geometry refuses a segment that holds none), and with `taper` the per-view updates are averaged
        with weights that fall off towards a window's edges (tango_amd.inpaint.window_taper), so that neighbouring prompts cross-fade
        over the overlap instead of meeting in a step.  `negative_prompt`: None, one string, or one per segment.  One segment with
        taper=False is generate_long / generate_loop, bit for bit.  The scheduler rules, `seed` and the chunking of samples are theirs.
        Returns np.int16 [samples, n]: generate_long's or generate_loop's length. """
        H, hw, stride, V, _ = timeline_geometry(segments, duration, window, hop, loop)
        how = "on a ring" if loop else "with windows"
        if not isinstance(guidance, (int, float)):
            raise ValueError("a guidance table is not supported %s: guidance must be a scalar" % how)
        if getattr(self.scheduler, "rule", None) == "dpmsolver":
            raise ValueError("the multistep DPM-Solver rule is not supported on a ring: use DDPM or DDIM" if loop else
                             "the multistep DPM-Solver rule is not supported with windows (a per-view history has no reference "
                             "behaviour): use DDPM or DDIM")
        per_call = max(1, self.LONG_MAX_ROWS // ((2 if cfg_enabled(guidance) else 1) * V))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        waves = []
        with torch.no_grad():
            for k in range(0, samples, per_call):
                n = min(per_call, samples - k)
                latents = self.model.inference_timeline(segments, self.scheduler, steps, guidance, n, duration, window, hop, loop, taper,
                                                        negative_prompt=negative_prompt, seed=seed, sample_offset=k)
                if loop:
                    mel = self.vae.engine.vae_decode_ring(latents, hw, stride)
                    waves.append(self.vae.engine.vocode_ring(mel).cpu().numpy())
                else:
                    mel = self.vae.engine.vae_decode_tiled(latents, hw, stride)
                    waves.append(self.vae.decode_to_waveform(mel))
        return np.concatenate(waves)

    def generate_for_batch(self, prompts, steps=100, guidance=3, samples=1, batch_size=8, disable_progress=True, duration=10,
                           negative_prompt=None, guidance_rescale=0.0):
        """ Generate audio for a list of prompt strings. (tango.py:51-64)  `duration`: as in generate(), one length for all.
        `negative_prompt` (None, a str, or one str per prompt), `guidance` (a scalar, or a table over all len(prompts) * samples
        latents rows: [rows] or [steps, rows]) and `guidance_rescale` as in generate(); a list and a table are sliced per batch
        like the prompts. """
        duration_geometry(duration)
        self._check_guidance(guidance, guidance_rescale)
        if isinstance(negative_prompt, (list, tuple)) and len(negative_prompt) != len(prompts):
            raise ValueError("negative_prompt holds %d strings for %d prompts" % (len(negative_prompt), len(prompts)))
        if guidance_is_table(guidance) and np.shape(guidance)[-1] != len(prompts) * samples:
            raise ValueError("a guidance table holds one entry per prompt and sample (%d), got %d"
                             % (len(prompts) * samples, np.shape(guidance)[-1]))
        outputs = []
        for k in range(0, len(prompts), batch_size):
            batch = prompts[k: k + batch_size]
            with torch.no_grad():
                latents = self.model.inference(batch, self.scheduler, steps, self._slice_per_batch(guidance, k, len(batch), samples),
                                               samples, disable_progress=disable_progress, duration=duration,
                                               negative_prompt=self._slice_per_batch(negative_prompt, k, len(batch)),
                                               guidance_rescale=guidance_rescale)
                mel = self.vae.decode_first_stage(latents)
                wave = self.vae.decode_to_waveform(mel)
                outputs += [item for item in wave]
        if samples == 1:
            return outputs
        return list(self.chunks(outputs, samples))

    def generate_for_batch_dp(self, prompts, steps=100, guidance=3, samples=1, batch_size=8, group=None, duration=10,
                              negative_prompt=None, guidance_rescale=0.0):
        """Data-parallel `generate_for_batch` over the ranks of the default (or given) torch.distributed group: one
        process per GPU, each holding a full `Tango`.  Every rank makes this call; rank 0's `prompts` are used, the text
        encoder runs on rank 0 only, embeddings travel by one RCCL broadcast per pass of `batch_size * world` prompts,
        int16 waveforms come back by one gather.  Returns the `generate_for_batch` result on rank 0, None elsewhere.
        `duration`: as in generate(); every rank passes the same value.  `negative_prompt` (rank 0's is used: rank 0 encodes, nothing
        new travels) and `guidance_rescale` (every rank passes the same value) as in generate_for_batch(); a guidance TABLE is
        refused with a ValueError: sharding it over the ranks is not implemented."""
        from .parallel import generate_for_batch_dp
        if guidance_is_table(guidance):
            raise ValueError("generate_for_batch_dp takes a scalar guidance: a guidance table is not sharded over the ranks")
        self._check_guidance(guidance, guidance_rescale)
        if isinstance(negative_prompt, (list, tuple)) and prompts is not None and len(negative_prompt) != len(prompts):
            raise ValueError("negative_prompt holds %d strings for %d prompts" % (len(negative_prompt), len(prompts)))
        latent_h, frames, _ = duration_geometry(duration)
        done = [0]            # prompts encoded so far: passes are encoded in order, each once

        def encode(batch, n_per_prompt, g):
            if g > 1.0:
                neg = self._slice_per_batch(negative_prompt, done[0], len(batch))
                done[0] += len(batch)
                pe, pm = self.model.encode_text_classifier_free(batch, n_per_prompt, neg)
            else:
                pe, pm = self.model.encode_text(batch)
                pe, pm = pe.repeat_interleave(n_per_prompt, 0), pm.repeat_interleave(n_per_prompt, 0)
            return pe.float(), pm

        def compute(pe, pm, offset, seed):
            # initial latents keyed by (broadcast seed, GLOBAL sample index), like the step noise: ranks that share a
            # torch.manual_seed must not start their samples from identical noise, and the result must not depend on the
            # number of ranks (parallel.py docstring)
            b = pe.shape[0] // 2 if guidance > 1.0 else pe.shape[0]
            ecfg = self.model.engine._cfg
            lat = dp_initial_latents(seed, offset, b, self.model.unet.config.in_channels, latent_h, ecfg.latent_w) * self.scheduler.init_noise_sigma
            latents = self.model.inference_from_embeddings(pe, pm, self.scheduler, steps, guidance, latents=lat, seed=seed,
                                                           sample_offset=offset, guidance_rescale=guidance_rescale)
            return self.vae.engine.vocode(self.vae.decode_first_stage(latents))      # int16 stays on the device

        with torch.no_grad():
            return generate_for_batch_dp(prompts, encode, compute, self.vae.engine.vocoder_samples(frames), self.model.device,
                                         guidance=guidance, samples=samples, batch_size=batch_size, group=group)

    def generate_from_embeddings(self, prompt_embeds, boolean_prompt_mask, steps=100, guidance=3, duration=10, **kw):
        """Same three calls given the text-encoder outputs (benchmarks / data-parallel workers); `duration` as in generate().
        `guidance` may be a table over the latents rows, and `guidance_rescale=` goes through `kw` (AudioDiffusion.inference_from_embeddings);
        a negative prompt is the first half of `prompt_embeds`."""
        with torch.no_grad():
            latents = self.model.inference_from_embeddings(prompt_embeds, boolean_prompt_mask, self.scheduler, steps, guidance,
                                                           duration=duration, **kw)
            mel = self.vae.decode_first_stage(latents)
            return self.vae.decode_to_waveform(mel)

    # ---- masked-latent inpainting (audioldm/pipeline.py:249-301 super_resolution_and_inpainting) ------------------------------
    def inpaint(self, prompt, audio, time_range=(0.10, 0.15), freq_range=(1.0, 1.0), steps=100, guidance=3, samples=1, duration=10,
                negative_prompt=None, guidance_rescale=0.0):
        """Regenerate the time span `time_range` and the mel band `freq_range` (fractions of the clip, ldm.py:773-777) of one 16 kHz
        clip `audio` (1-D; reading and resampling are the caller's) under the text `prompt`; the rest keeps the clip's audio.
        Returns np.int16 [samples, 163872].

        `duration`: seconds the clip is cut or zero-padded to (2.5 .. 20 on the 2.5 s grid; 10 -> 163872 samples, else
        duration_geometry(duration)[2]).  None: the smallest grid duration that holds the clip (tango_amd.inpaint.clip_duration; a 3 s
        clip runs as 5 s, a quarter of the latent rows of the default), 20 s for longer clips.  AudioLDM's round_up_duration
        (pipeline.py:49-50) always adds one more 2.5 s block instead; that is not reproduced.
        `negative_prompt`, table `guidance` and `guidance_rescale`: as in generate()."""
        self._check_guidance(guidance, guidance_rescale)
        with torch.no_grad():
            known = self.encode_audio(audio, duration)
            mask = latent_mask(1, time_range, freq_range, known.shape[2], known.shape[3])
            latents = self.model.inpaint([prompt], known, mask, self.scheduler, steps, guidance, samples,
                                         negative_prompt=negative_prompt, guidance_rescale=guidance_rescale)
            mel = self.vae.decode_first_stage(latents)
            return self.vae.decode_to_waveform(mel)

    def inpaint_from_embeddings(self, prompt_embeds, boolean_prompt_mask, audio, time_range=(0.10, 0.15), freq_range=(1.0, 1.0),
                                steps=100, guidance=3, samples=1, duration=10, **kw):
        """`inpaint` given the text-encoder outputs for the `samples` rows ([uncond; cond] when guidance > 1, like
        generate_from_embeddings); `kw` goes to AudioDiffusion.inpaint_from_embeddings (latents, noise, blend_noise, seed, ...)."""
        with torch.no_grad():
            known = self.encode_audio(audio, duration)
            rows = prompt_embeds.shape[0] // 2 if cfg_enabled(guidance) else prompt_embeds.shape[0]
            if rows != samples:
                raise ValueError("prompt_embeds hold %d rows, `samples` is %d" % (rows, samples))
            mask = latent_mask(samples, time_range, freq_range, known.shape[2], known.shape[3])
            latents = self.model.inpaint_from_embeddings(prompt_embeds, boolean_prompt_mask, self.scheduler, steps, guidance,
                                                         known_latents=known.repeat_interleave(samples, 0), latent_mask=mask, **kw)
            mel = self.vae.decode_first_stage(latents)
            return self.vae.decode_to_waveform(mel)

    # ---- audio-to-audio editing (audioldm/pipeline.py:145-247 style_transfer) -----------------------------------------------------
    def edit(self, prompt, audio, strength=0.5, steps=100, guidance=3, samples=1, mode="noise", source_prompt="", time_range=None,
             freq_range=None, seed=None, duration=10, negative_prompt=None, guidance_rescale=0.0):
        """Edit one 16 kHz clip `audio` (1-D; reading and resampling are the caller's) towards the text `prompt`: the clip's latents
        are moved part of the way into the noise and the last k = int(strength * steps) of `steps` denoise steps run from there.
        Returns np.int16 [samples, 163872].

        mode="noise" is AudioLDM's style_transfer: a posterior sample of the encoded clip, noised to the encode level (one fused
        launch; the draws are the device Philox generator's under `seed`, so an edit reproduces across batch splits).
        mode="invert" is deterministic: the posterior mode, then k DDIM-inversion steps under `source_prompt` (the text that
        describes the clip as it is; no CFG) up the sampler's own timesteps, which end exactly on the encode timestep of
        mode="noise" (DDIMInverseScheduler.from_scheduler); `self.scheduler` must be a DDIMScheduler with eta = 0 or a
        DPMSolverMultistepScheduler (a stochastic sampler would not retrace an inverted trajectory).
        With `time_range` / `freq_range` (fractions of the clip, tango_amd.inpaint.latent_mask) only that region is edited;
        the rest keeps the clip's audio through the masked loop.

        `duration`: seconds the clip is cut or zero-padded to, as in inpaint() (None: the smallest grid duration that holds the
        clip, without round_up_duration's extra 2.5 s block); the result has duration_geometry(duration)[2] samples.

        `negative_prompt` and `guidance_rescale`: as in generate(); a `guidance` table counts the k EXECUTED steps ([k, samples]).

        Not reproduced from AudioLDM: the `samples[:, :, :-3, :]` crop of the decoded mel (pipeline.py:241)."""
        with torch.no_grad():
            self._check_edit(mode, steps, strength)
            self._check_guidance(guidance, guidance_rescale)
            host = None
            if cfg_enabled(guidance):
                pe, pm, host = self.model._encode_text_classifier_free([prompt], samples, negative_prompt)
            else:
                pe, pm = self.model.encode_text([prompt])
                pe, pm = pe.repeat_interleave(samples, 0), pm.repeat_interleave(samples, 0)
            src = None
            if mode == "invert":
                se, sm = self.model.encode_text([source_prompt])
                src = (se.repeat_interleave(samples, 0).float(), sm.repeat_interleave(samples, 0))
            return self._edit(pe.float(), pm, audio, strength, steps, guidance, samples, mode, src, time_range, freq_range, seed,
                              dict(mask_host=host, guidance_rescale=guidance_rescale), duration)

    def edit_from_embeddings(self, prompt_embeds, boolean_prompt_mask, audio, strength=0.5, steps=100, guidance=3, samples=1,
                             mode="noise", source_embeds=None, source_mask=None, time_range=None, freq_range=None, seed=None,
                             duration=10, **kw):
        """`edit` given the text-encoder outputs for the `samples` rows ([uncond; cond] when guidance > 1, like
        generate_from_embeddings); mode="invert" takes the source prompt's `source_embeds` [samples, L, d] / `source_mask`
        (conditional rows only).  `kw` goes to AudioDiffusion.edit_from_embeddings (noise, blend_noise, sample_offset)."""
        with torch.no_grad():
            self._check_edit(mode, steps, strength)
            rows = prompt_embeds.shape[0] // 2 if cfg_enabled(guidance) else prompt_embeds.shape[0]
            if rows != samples:
                raise ValueError("prompt_embeds hold %d rows, `samples` is %d" % (rows, samples))
            src = None
            if mode == "invert":
                if source_embeds is None or source_embeds.shape[0] != samples:
                    raise ValueError("mode='invert' needs source_embeds with %d rows" % samples)
                src = (source_embeds, source_mask)
            return self._edit(prompt_embeds, boolean_prompt_mask, audio, strength, steps, guidance, samples, mode, src, time_range,
                              freq_range, seed, kw, duration)

    def _check_edit(self, mode, steps, strength):
        """the argument checks of edit() that need no device"""
        if mode not in ("noise", "invert"):
            raise ValueError("mode must be 'noise' or 'invert', got %r" % (mode,))
        k = int(strength * steps)
        if not 1 <= k <= steps - 1:
            raise ValueError("strength %r of %d steps runs k = %d steps; an edit needs 1 <= k <= %d" % (strength, steps, k, steps - 1))
        if mode == "invert":
            s = self.scheduler
            ok = isinstance(s, DPMSolverMultistepScheduler) or (isinstance(s, DDIMScheduler) and s.eta == 0)
            if not ok:
                raise ValueError("mode='invert' needs a deterministic sampler: set Tango.scheduler to a DDIMScheduler (eta = 0) or a "
                                 "DPMSolverMultistepScheduler, not %s" % type(s).__name__)

    def _edit(self, pe, pm, audio, strength, steps, guidance, samples, mode, src, time_range, freq_range, seed, kw, duration=10):
        moments = self.encode_moments(audio, duration)
        if seed is None:
            # like the loop's step noise: the Philox key comes from torch's global generator, so torch.manual_seed() fixes the edit
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        offset = kw.get("sample_offset", 0)
        regional = time_range is not None or freq_range is not None
        start, t_enc = self.scheduler.edit_plan(steps, strength)
        if mode == "noise":
            sa, sb = self.scheduler.blend_table(start=start - 1)[0]
            out = self.vae.encode_start_latents(moments, float(sa), float(sb), samples, seed=seed, sample_offset=offset,
                                                want_clean=regional)
            x, known = out if regional else (out, None)
        else:
            # sa = 1, sb = 0: the scaled posterior mode itself, the same clip in every row (with sb = 0 the kernel draws no n)
            z = self.vae.encode_start_latents(moments, 1.0, 0.0, samples, posterior="mode", seed=seed, sample_offset=offset)
            known = z if regional else None
            x = self.model.invert_from_embeddings(src[0], src[1], self.scheduler, steps, latents=z, count=steps - start)
        masking = {}
        if regional:
            # latent_mask(): 1 keeps the known audio, 0 regenerates the named region -- the region of the edit
            m = latent_mask(samples, time_range or (0.0, 0.0), freq_range or (1.0, 1.0), x.shape[2], x.shape[3])
            masking = dict(known_latents=known, latent_mask=m)
        latents = self.model.edit_from_embeddings(pe, pm, self.scheduler, steps, guidance, start_latents=x, strength=strength,
                                                  seed=seed, **masking, **kw)
        mel = self.vae.decode_first_stage(latents)
        return self.vae.decode_to_waveform(mel)

    def _need_encoder(self, what):
        if self.stft is None or not getattr(self.vae, "with_encoder", False):
            raise RuntimeError("%s needs the mel front-end and the VAE encoder: build Tango(..., with_encoder=True) from a "
                               "snapshot with stft_config.json / pytorch_model_stft.bin, or pass stft= and an AutoencoderKL(with_encoder=True) "
                               "to from_components" % what)

    def _clip_fbank(self, audio, duration):
        """prepare_waveform -> wav_to_fbank at `duration` seconds (None: clip_duration() of the clip): fbank [1, frames, 64]"""
        if duration is None:
            duration = clip_duration(len(audio))
        frames = duration_geometry(duration)[1]
        wav = prepare_waveform(audio, duration=duration)[None].to(self.model.device)
        fbank, _, _ = wav_to_fbank(wav, frames, fn_STFT=self.stft)
        return fbank

    def encode_moments(self, audio, duration=10):
        """one 1-D 16 kHz clip -> the posterior's moments [1, 16, 256, 16] = [mean | logvar]: prepare_waveform -> wav_to_fbank ->
        the VAE encoder, before any draw (AutoencoderKL.encode_start_latents takes them).  `duration` as in inpaint(): the moments
        are [1, 16, int(duration * 25.6), 16]."""
        self._need_encoder("editing")
        fbank = self._clip_fbank(audio, duration)
        return self.vae.engine.vae_encode(fbank.unsqueeze(1), latent_h=fbank.shape[1] // 4)

    def encode_audio(self, audio, duration=10):
        """one 1-D 16 kHz clip -> known latents [1, 8, 256, 16]: prepare_waveform -> wav_to_fbank -> encode_first_stage ->
        get_first_stage_encoding (one posterior sample from torch's global generator, ldm.py:180-181).  `duration` as in
        inpaint(): the latents are [1, 8, int(duration * 25.6), 16]."""
        self._need_encoder("inpainting")
        fbank = self._clip_fbank(audio, duration)
        return self.vae.get_first_stage_encoding(self.vae.encode_first_stage(fbank.unsqueeze(1)))


def dp_initial_latents(seed, offset, count, channels=8, height=256, width=16):
    """Initial latents [count, channels, height, width] (fp32, CPU; the engine's latent size) of the samples with GLOBAL indices
    offset .. offset+count-1 under the pass seed: one torch generator per sample, so a shard of a batch draws exactly what the
    unsharded batch would.  NOT the draw of `prepare_latents` (models.py:259-264: one randn of the whole batch from torch's global
    generator): `generate_for_batch_dp` at world size 1 and `generate_for_batch` under the same torch.manual_seed give different
    (equally distributed) samples -- the price of results that do not depend on the number of ranks."""
    out = []
    for i in range(count):
        g = torch.Generator(device="cpu").manual_seed((int(seed) * 1000003 + offset + i) % (2 ** 63 - 1))
        out.append(torch.randn(channels, height, width, generator=g))
    return torch.stack(out) if out else torch.zeros(0, channels, height, width)


def _ddpm_keys(cfg):
    keep = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample",
            "variance_type", "clip_sample_range")
    return {k: v for k, v in cfg.items() if k in keep}
