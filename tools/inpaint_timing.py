#!/usr/bin/env python
"""Per-step time of the masked (inpainting) denoise loop against the unmasked loop on the bench model (full-size UNet, synthetic
weights, fp16, guidance 3, 64 text tokens, 20 steps), DDPM and DPM-Solver++ 2M, from the engine's own `last_denoise_ms`.

The masked loop adds one blend to the update kernel of every step (about 0.15 MB of HBM traffic per sample and step) and one
small kernel before the first step, so its per-step time should equal the unmasked loop's within run-to-run noise.  To compare with
another tree (e.g. the parent commit, which has no masked loop) run this tool once per process and tree, alternating:

  python tools/inpaint_timing.py --mode masked   --out a.json
  python tools/inpaint_timing.py --mode unmasked --tree ../parent --out b.json     # tango_amd imported from ../parent

usage: python tools/inpaint_timing.py [--mode masked|unmasked] [--batches 1,8,32] [--reps 3] [--tree DIR] [--out file.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("masked", "unmasked"), default="masked")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tree", default=ROOT, help="repository tree whose tango_amd is timed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from tango_amd.engine import UNET_CONFIG_LARGE
    from tango_amd.models import AudioDiffusion
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler, DPMSolverMultistepScheduler
    from tango_amd.tango import _ddpm_keys

    dev = "cuda:0"
    model = AudioDiffusion(unet_config=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    model.engine.load_synthetic(1234)
    ddpm = DDPMScheduler.from_config(_ddpm_keys(SD21_SCHEDULER_CONFIG))
    dpm = DPMSolverMultistepScheduler.from_config(ddpm.config)          # DPM-Solver++ 2M, the SD-2.1 betas, v-prediction
    L, d = 64, UNET_CONFIG_LARGE["cross_attention_dim"]
    rec = {"mode": args.mode, "tree": os.path.abspath(args.tree), "steps": args.steps, "per_step_ms": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(7)
        pe = torch.randn(2 * B, L, d, generator=g).to(dev)
        pm = torch.ones(2 * B, L, dtype=torch.bool)
        pm[:B, 1:] = False
        lat = torch.randn(B, 8, 256, 16, generator=g)
        kw = {}
        if args.mode == "masked":
            from tango_amd.inpaint import latent_mask
            kw = dict(known_latents=torch.randn(B, 8, 256, 16, generator=g).to(dev), latent_mask=latent_mask(B).to(dev))
        for name, sch in (("ddpm", ddpm), ("dpmsolver++_2m", dpm)):
            run = model.inpaint_from_embeddings if kw else model.inference_from_embeddings
            run(pe, pm, sch, args.steps, 3.0, latents=lat, seed=1, **kw)              # plans + graphs
            torch.cuda.synchronize()
            per = []
            for _ in range(args.reps):
                run(pe, pm, sch, args.steps, 3.0, latents=lat, seed=1, **kw)
                torch.cuda.synchronize()
                per.append(model.engine.last_denoise_ms()[1])
            rec["per_step_ms"]["B%d_%s" % (B, name)] = per
            print("%s B=%d %s per-step ms %s" % (args.mode, B, name, ["%.3f" % v for v in per]), flush=True)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
