#!/usr/bin/env python
"""Timing of a seamless loop on the bench model (full-size UNet, mel-VAE, HiFi-GAN, synthetic weights, fp16, 64 text tokens, CFG 3):

  * the per-step time of a 10 s loop at B = 1 (H = Hw = 256, s = 128: V = 2 rotated views of the ring, 4 UNet rows of height 256 per step;
    DDIM, --steps steps, graph replay; device events around the replays, Engine.last_denoise_ms) and, in the same process and
    alternating with it, of a plain 10 s call of batch 2 -- the same UNet program of 4 rows, closed by the plain update kernel;
  * the same pair for a 30 s loop (H = 768, Hw = 256, s = 128: V = 6, 12 rows) and a plain 10 s call of batch 6.
    Every call runs --rounds times; the spread of each over the rounds is the yardstick for their difference;
  * the ring VAE decode (V windows decoded, tiles blended on the ring) and the ring vocoder (4 H + 2 Cx frames) of both loops,
    milliseconds per pass (device events, --reps passes after one warm-up pass).

usage: python tools/loop_timing.py [--steps 50] [--rounds 5] [--reps 5] [--out profiles/loop_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 64


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from tango_amd.engine import HIFIGAN_CONFIG, UNET_CONFIG_LARGE, VAE_CONFIG, Engine
    from tango_amd.inpaint import loop_geometry
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler

    dev = "cuda:0"
    rec = {"steps": args.steps, "rounds": args.rounds, "reps": args.reps, "dtype": "fp16", "sampler": "ddim eta 0", "guidance": 3.0,
           "text_len": L, "loops": []}
    g = torch.Generator().manual_seed(7)
    e = Engine(unet=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    e.load_synthetic(1234)
    sch = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    enc1 = torch.randn(2, L, UNET_CONFIG_LARGE["cross_attention_dim"], generator=g)
    mask1 = torch.ones(2, L, dtype=torch.bool)
    mask1[:1, 1:] = False                                     # the unconditional row: T5("") keeps one token
    kw = dict(prediction_type=sch.config.prediction_type, rule=sch.rule, seed=1, use_graph=True)
    geoms = [(d, loop_geometry(d)) for d in (10.0, 30.0)]
    assert [gm for _, gm in geoms] == [(256, 256, 128, 2), (768, 256, 128, 6)]

    for duration, (H, Hw, s, V) in geoms:
        enc, mask = enc1.repeat_interleave(V, 0).to(dev), mask1.repeat_interleave(V, 0)
        ring0 = torch.randn(1, 8, H, 16, generator=g).to(dev)
        plain0 = torch.randn(V, 8, Hw, 16, generator=g).to(dev)

        def ring(n):
            sch.set_timesteps(n)
            lat = ring0.clone()
            e.denoise_ring(lat, enc, mask, sch.timesteps.numpy(), sch.coef_table(), 3.0, window_h=Hw, stride=s, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(lat).all()
            return e.last_denoise_ms()[1]

        def plain(n):
            sch.set_timesteps(n)
            lat = plain0.clone()
            e.denoise(lat, enc, mask, sch.timesteps.numpy(), sch.coef_table(), 3.0, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(lat).all()
            return e.last_denoise_ms()[1]

        ring(2), plain(2)                                     # plan, both graph captures
        rms, pms = [], []
        for _ in range(args.rounds):
            rms.append(ring(args.steps))
            pms.append(plain(args.steps))
        rec["loops"].append({"duration_s": duration, "ring_h": H, "window_h": Hw, "stride": s, "views": V, "unet_rows": 2 * V,
                             "ring_step_ms": rms, "plain_batch%d_step_ms" % V: pms, "ring_median_ms": median(rms),
                             "plain_median_ms": median(pms), "ring_spread_ms": max(rms) - min(rms), "plain_spread_ms": max(pms) - min(pms),
                             "ring_minus_plain_median_ms": median(rms) - median(pms)})
        print("%g s loop, B = 1, V = %d: %s ms per step; plain 10 s batch %d: %s ms per step" %
              (duration, V, ", ".join("%.3f" % x for x in rms), V, ", ".join("%.3f" % x for x in pms)), flush=True)
    del e
    torch.cuda.empty_cache()

    ev = Engine(vae=VAE_CONFIG, hifigan=HIFIGAN_CONFIG, dtype="fp16", device=dev)
    ev.load_synthetic(1234)
    rec["vocoder_ring_context"] = ev.vocoder_ring_context()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
        return out

    for (duration, (H, Hw, s, V)), row in zip(geoms, rec["loops"]):
        z = (torch.randn(1, 8, H, 16, generator=g) * 1.1).to(dev)
        mel = ev.vae_decode_ring(z, Hw, s)
        assert mel.shape == (1, 1, 4 * H, 64) and torch.isfinite(mel).all()
        assert ev.vocode_ring(mel).shape == (1, 640 * H)
        row["vae_ring_ms"] = timed(lambda: ev.vae_decode_ring(z, Hw, s))
        row["vocoder_ring_ms"] = timed(lambda: ev.vocode_ring(mel))
        row["vocoder_plain_ms"] = timed(lambda: ev.vocode(mel))
        row["samples"] = 640 * H
        print("%g s loop: ring VAE decode %s ms; ring vocoder (%d + 2 * %d frames) %s ms; plain vocoder %s ms" %
              (duration, ", ".join("%.2f" % x for x in row["vae_ring_ms"]), 4 * H, rec["vocoder_ring_context"],
               ", ".join("%.2f" % x for x in row["vocoder_ring_ms"]), ", ".join("%.2f" % x for x in row["vocoder_plain_ms"])), flush=True)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
