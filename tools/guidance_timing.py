#!/usr/bin/env python
"""What the guided step costs on the bench model (full-size UNet, synthetic weights, fp16, 64 text tokens, DDPM, 10 s latents): the
engine's per-step time (`last_denoise_ms`) at B = 1 and B = 32 of

  * default      scalar guidance 3, no rescale: today's kernels and graph (single-key unconditional half, CFG-shared prefix);
  * table        a [B] guidance row, phi = 0: the guided update kernel, the two statistics launches return at once;
  * rescale      the same row with phi = 0.7: the statistics pass over the step's output (2 B x 4096 x 8 fp32) and the finalise;
  * negative     default guidance with a two-key unconditional half (what a negative prompt gives): the whole-batch plan instead
                 of the CFG-shared prefix -- the cost of a negative prompt is this plan change, not a kernel of its own.

The runs alternate (default, table, rescale, negative) x reps, so a drift of the box shows in every column.
usage: python tools/guidance_timing.py [--reps 3] [--steps 20] [--out file.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tango_amd.engine import UNET_CONFIG_LARGE
    from tango_amd.models import AudioDiffusion
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler
    from tango_amd.tango import _ddpm_keys

    dev = "cuda:0"
    model = AudioDiffusion(unet_config=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    model.engine.load_synthetic(1234)
    ddpm = DDPMScheduler.from_config(_ddpm_keys(SD21_SCHEDULER_CONFIG))
    L, d = 64, UNET_CONFIG_LARGE["cross_attention_dim"]
    rec = {"per_step_ms": {}, "steps": args.steps}
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(7)
        pe = torch.randn(2 * B, L, d, generator=g).to(dev)
        pm = torch.ones(2 * B, L, dtype=torch.bool)
        pm[:B, 1:] = False                       # T5(""): one key
        pm_neg = pm.clone()
        pm_neg[:B, 1] = True                     # a negative prompt: two keys
        lat = torch.randn(B, 8, 256, 16, generator=torch.Generator().manual_seed(3))
        row = np.linspace(2.0, 7.5, B).astype(np.float32) if B > 1 else np.array([3.0], np.float32)
        runs = (("default", pm, 3.0, 0.0), ("table", pm, row, 0.0), ("rescale", pm, row, 0.7), ("negative", pm_neg, 3.0, 0.0))

        def one(mask, guidance, phi):
            model.inference_from_embeddings(pe, mask, ddpm, args.steps, guidance, latents=lat, seed=1, guidance_rescale=phi)
            torch.cuda.synchronize()
            return model.engine.last_denoise_ms()[1]

        for _, mask, guidance, phi in runs:      # plans + graphs
            one(mask, guidance, phi)
        per = {name: [] for name, *_ in runs}
        for _ in range(args.reps):
            for name, mask, guidance, phi in runs:
                per[name].append(one(mask, guidance, phi))
        for name, v in per.items():
            rec["per_step_ms"]["B%d_%s" % (B, name)] = v
            print("B=%d %-8s per-step ms %s" % (B, name, ["%.3f" % x for x in v]), flush=True)
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
