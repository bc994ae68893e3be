#!/usr/bin/env python
"""Timing of audio-to-audio editing on the bench model (full-size UNet, mel-VAE with encoder, HiFi-GAN, synthetic weights, fp16):

  * one fused latent encode launch (tango_op_latent_encode, Philox draws) at B = 1 and 32 against the torch composition it
    replaces (clamp, exp, randn, scale, clip test and clamp, randn, add_noise on the device), device events over `--reps` calls;
  * B = 1 end to end: Tango.edit_from_embeddings at strength 0.5 with 20-step DPM-Solver++ 2M (mel front-end, VAE encoder, fused
    encode, 10 denoise steps, VAE decoder, vocoder) against a full 20-step generate_from_embeddings, host clock around calls that
    end with the waveform on the host.

usage: python tools/edit_timing.py [--reps 200] [--e2e-reps 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--e2e-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from oracle import stft_oracle as S
    from tango_amd.autoencoder import EDIT_CLIP_RANGE, EDIT_CLIP_TRIGGER, AutoencoderKL
    from tango_amd.engine import UNET_CONFIG_LARGE, VAE_CONFIG
    from tango_amd.models import AudioDiffusion
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler, DPMSolverMultistepScheduler
    from tango_amd.stft import TacotronSTFT
    from tango_amd.tango import Tango, _ddpm_keys

    dev = "cuda:0"
    vae = AutoencoderKL(ddconfig=dict(VAE_CONFIG, resolution=256, in_channels=1, double_z=True, attn_resolutions=[], dropout=0.0),
                        embed_dim=8, scale_factor=VAE_CONFIG["scale_factor"], dtype="fp16", device=dev, with_encoder=True)
    vae.engine.load_synthetic(1234)
    dpm = DPMSolverMultistepScheduler.from_config(DDPMScheduler.from_config(_ddpm_keys(SD21_SCHEDULER_CONFIG)).config)
    start, t_enc = dpm.edit_plan(20, 0.5)
    sa, sb = (float(v) for v in dpm.blend_table(start=start - 1)[0])
    rec = {"reps": args.reps, "encode_us": {}, "e2e_ms": {}}

    def torch_compose(mom, B):
        mean, logvar = torch.chunk(mom.expand(B, -1, -1, -1), 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        z = vae.scale_factor * (mean + std * torch.randn(mean.shape, device=dev))
        if torch.max(torch.abs(z)) > EDIT_CLIP_TRIGGER:                # pipeline.py:209-210 (a host sync, as in the reference)
            z = torch.clip(z, min=-EDIT_CLIP_RANGE, max=EDIT_CLIP_RANGE)
        return sa * z + sb * torch.randn(z.shape, device=dev)

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000.0 / args.reps

    g = torch.Generator().manual_seed(3)
    mom = torch.randn(1, 16, 256, 16, generator=g).to(dev)
    for B in (1, 32):
        for rnd in range(3):                                           # alternate the two, three rounds: the spread shows
            fused = timed(lambda: vae.encode_start_latents(mom, sa, sb, B, seed=5))
            ref = timed(lambda: torch_compose(mom, B))
            rec["encode_us"].setdefault("B%d_fused" % B, []).append(fused)
            rec["encode_us"].setdefault("B%d_torch" % B, []).append(ref)
            print("encode B=%d round %d: fused launch %.1f us, torch composition %.1f us" % (B, rnd, fused, ref), flush=True)

    model = AudioDiffusion(unet_config=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    model.engine.load_synthetic(1234)
    tango = Tango.from_components(model, vae, scheduler=dpm, stft=TacotronSTFT(**S.AUDIOLDM_STFT_CONFIG, device=dev))
    L, d = 64, UNET_CONFIG_LARGE["cross_attention_dim"]
    pe = torch.randn(2, L, d, generator=g).to(dev)
    pm = torch.ones(2, L, dtype=torch.bool)
    pm[:1, 1:] = False
    t = np.arange(5 * 16000) / 16000.0
    audio = (0.3 * np.sin(2 * np.pi * 330 * t) + 0.05 * np.random.default_rng(17).standard_normal(t.shape)).astype(np.float32)

    def edit():
        return tango.edit_from_embeddings(pe, pm, audio, strength=0.5, steps=20, guidance=3, samples=1, seed=1)

    def generate():
        return tango.generate_from_embeddings(pe, pm, steps=20, guidance=3, seed=1)

    for fn in (edit, generate):                                        # plans + graphs
        fn()
    for rnd in range(args.e2e_reps):
        for name, fn in (("edit_strength0.5_20step_dpmpp2m", edit), ("generate_20step_dpmpp2m", generate)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav = fn()
            ms = (time.perf_counter() - t0) * 1000.0
            assert wav.shape == (1, 163872)
            rec["e2e_ms"].setdefault(name, []).append(ms)
            print("B=1 %s round %d: %.1f ms" % (name, rnd, ms), flush=True)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
