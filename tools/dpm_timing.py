#!/usr/bin/env python
"""Multistep DPM-Solver++ against DDPM on the bench model (full-size UNet, synthetic weights, fp16, guidance 3, 64 text tokens):

  * the engine's per-step time (`last_denoise_ms`) of both rules at B = 1 and B = 32: the multistep update is one more elementwise
    kernel in the same captured step, so the two should agree within run-to-run noise;
  * the end-to-end time of one generation at B = 1 (denoise + VAE decode + vocoder, `Tango.generate_from_embeddings`): DPM++ 2M with
    20 and 25 steps against DDPM with 100 steps.

usage: python tools/dpm_timing.py [--reps 3] [--out file.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tango_amd.autoencoder import AutoencoderKL
    from tango_amd.engine import UNET_CONFIG_LARGE, VAE_CONFIG
    from tango_amd.models import AudioDiffusion
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler, DPMSolverMultistepScheduler
    from tango_amd.tango import Tango, _ddpm_keys

    dev = "cuda:0"
    model = AudioDiffusion(unet_config=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    model.engine.load_synthetic(1234)
    vae = AutoencoderKL(ddconfig=dict(VAE_CONFIG, attn_resolutions=[]), embed_dim=8, scale_factor=VAE_CONFIG["scale_factor"],
                        dtype="fp16", device=dev)
    vae.engine.load_synthetic(1234)
    tango = Tango.from_components(model, vae)
    ddpm = DDPMScheduler.from_config(_ddpm_keys(SD21_SCHEDULER_CONFIG))
    dpm = DPMSolverMultistepScheduler.from_config(ddpm.config)          # DPM-Solver++ 2M, the SD-2.1 betas, v-prediction
    L, d = 64, UNET_CONFIG_LARGE["cross_attention_dim"]

    def text(B):
        g = torch.Generator().manual_seed(7)
        pe = torch.randn(2 * B, L, d, generator=g).to(dev)
        pm = torch.ones(2 * B, L, dtype=torch.bool)
        pm[:B, 1:] = False
        return pe, pm

    rec = {"per_step_ms": {}, "generate_b1_s": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        pe, pm = text(B)
        lat = torch.randn(B, 8, 256, 16, generator=torch.Generator().manual_seed(3))
        for name, sch in (("ddpm", ddpm), ("dpmsolver++_2m", dpm)):
            model.inference_from_embeddings(pe, pm, sch, 20, 3.0, latents=lat, seed=1)        # plans + graphs
            torch.cuda.synchronize()
            per = []
            for _ in range(args.reps):
                model.inference_from_embeddings(pe, pm, sch, 20, 3.0, latents=lat, seed=1)
                torch.cuda.synchronize()
                per.append(model.engine.last_denoise_ms()[1])
            rec["per_step_ms"]["B%d_%s" % (B, name)] = per
            print("B=%d %s per-step ms %s" % (B, name, ["%.3f" % v for v in per]), flush=True)
    pe, pm = text(1)
    for name, sch, n in (("ddpm_100", ddpm, 100), ("dpmsolver++_2m_25", dpm, 25), ("dpmsolver++_2m_20", dpm, 20)):
        tango.scheduler = sch
        tango.generate_from_embeddings(pe, pm, steps=n, guidance=3, seed=1)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            tango.generate_from_embeddings(pe, pm, steps=n, guidance=3, seed=1)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rec["generate_b1_s"][name] = ts
        print("generate B=1 %s: %s s" % (name, ["%.4f" % v for v in ts]), flush=True)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
