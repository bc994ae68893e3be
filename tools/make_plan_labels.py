#!/usr/bin/env python
"""The ordered op labels (no times) of the engine's plans, per case: what tests/golden/plan_labels.json pins and
tests/test_plan_labels_gpu.py compares.  A label names the op, its shape and the kernel family the planner chose for it
("linear+ln(wide) M=.. N=.. K=..", "conv3x3up(phase) ..", ".. splitK"), so a moved routing threshold shows up as exactly the ops that flipped.
Synthetic weights, default switches.  Regenerate the fixture only when a change of routing or labels is intended:
usage: python tools/make_plan_labels.py [--out tests/golden/plan_labels.json] [--b2 64 ...]   (--b2: extra fp16 UNet batches, L = 64)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# case name -> (engine kind, dtype, profile call arguments)
CASES = {
    "unet_fp16_B2=2_L=64": ("unet", "fp16", dict(batch2=2, text_len=64)),
    "unet_fp16_B2=16_L=64": ("unet", "fp16", dict(batch2=16, text_len=64)),
    "unet_fp16_B2=2_L=64_H=64": ("unet", "fp16", dict(batch2=2, text_len=64, latent_h=64)),
    "unet_fp32_B2=2_L=64": ("unet", "fp32", dict(batch2=2, text_len=64)),
    "vae_fp16_B=1": ("vae", "fp16", dict(batch=1)),
    "vocoder_fp16_B=1_frames=256": ("vocoder", "fp16", dict(batch=1, frames=256)),
}


def collect(cases=None):
    """{case: [label, ...]} on cuda:0; one engine per (kind, dtype), built once"""
    from tango_amd.engine import HIFIGAN_CONFIG, UNET_CONFIG_LARGE, VAE_CONFIG, Engine
    cases = CASES if cases is None else cases
    engines, out = {}, {}
    for name, (kind, dtype, kw) in cases.items():
        key = ("unet" if kind == "unet" else "vv", dtype)
        if key not in engines:
            e = Engine(unet=UNET_CONFIG_LARGE, dtype=dtype) if kind == "unet" else Engine(vae=VAE_CONFIG, hifigan=HIFIGAN_CONFIG, dtype=dtype)
            e.load_synthetic(1234)
            engines[key] = e
        e = engines[key]
        rows = {"unet": e.profile_unet, "vae": e.profile_vae, "vocoder": e.profile_vocoder}[kind](**kw)
        out[name] = [r[0] for r in rows]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "plan_labels.json"))
    ap.add_argument("--b2", type=int, nargs="*", default=[], help="extra fp16 UNet cases at these CFG batches (one-off comparisons)")
    a = ap.parse_args()
    cases = dict(CASES)
    for b2 in a.b2:
        cases["unet_fp16_B2=%d_L=64" % b2] = ("unet", "fp16", dict(batch2=b2, text_len=64))
    labels = collect(cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(labels, f, indent=0)
        f.write("\n")
    print("wrote %s: %s" % (a.out, ", ".join("%s %d ops" % (k, len(v)) for k, v in labels.items())))
