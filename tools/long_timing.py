#!/usr/bin/env python
"""Timing of a long clip on the bench model (full-size UNet, mel-VAE, HiFi-GAN, synthetic weights, fp16, 64 text tokens, CFG 3):

  * the per-step time of a 30 s clip at B = 1 as windows in time (window 10 s, hop 5 s: V = 5 views, 10 UNet rows of height 256 per
    step; DDIM, --steps steps, graph replay; device events around the replays, Engine.last_denoise_ms);
  * in the same process and alternating with it, the per-step time of a plain 10 s call of batch 5 -- the same UNet program of 10 rows,
    closed by the plain update kernel.  Both run --rounds times; the spread of each over the rounds is the yardstick for their difference;
  * the tiled VAE decode (5 windows decoded, tiles blended) and the vocoder (3072 frames) of that clip, milliseconds per pass
    (device events, --reps passes after one warm-up pass).

usage: python tools/long_timing.py [--steps 50] [--rounds 5] [--reps 5] [--out profiles/long_timing.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--duration", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from tango_amd.engine import HIFIGAN_CONFIG, UNET_CONFIG_LARGE, VAE_CONFIG, Engine
    from tango_amd.inpaint import long_geometry
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler

    dev = "cuda:0"
    H, Hw, s, V = long_geometry(args.duration, 10.0, 5.0)
    rec = {"duration_s": args.duration, "canvas_h": H, "window_h": Hw, "stride": s, "views": V, "steps": args.steps, "rounds": args.rounds,
           "reps": args.reps, "dtype": "fp16", "sampler": "ddim eta 0", "guidance": 3.0, "text_len": L}
    g = torch.Generator().manual_seed(7)
    e = Engine(unet=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    e.load_synthetic(1234)
    sch = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    enc1 = torch.randn(2, L, UNET_CONFIG_LARGE["cross_attention_dim"], generator=g)
    mask1 = torch.ones(2, L, dtype=torch.bool)
    mask1[:1, 1:] = False                                     # the unconditional row: T5("") keeps one token
    enc, mask = enc1.repeat_interleave(V, 0).to(dev), mask1.repeat_interleave(V, 0)
    canvas0 = torch.randn(1, 8, H, 16, generator=g).to(dev)
    plain0 = torch.randn(V, 8, Hw, 16, generator=g).to(dev)
    kw = dict(prediction_type=sch.config.prediction_type, rule=sch.rule, seed=1, use_graph=True)

    def windowed(n):
        sch.set_timesteps(n)
        lat = canvas0.clone()
        e.denoise_windows(lat, enc, mask, sch.timesteps.numpy(), sch.coef_table(), 3.0, window_h=Hw, stride=s, **kw)
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

    windowed(2), plain(2)                                     # plan, both graph captures
    wms, pms = [], []
    for _ in range(args.rounds):
        wms.append(windowed(args.steps))
        pms.append(plain(args.steps))
    rec["windowed_step_ms"], rec["plain_batch%d_step_ms" % V] = wms, pms
    rec["windowed_spread_ms"], rec["plain_spread_ms"] = max(wms) - min(wms), max(pms) - min(pms)
    rec["windowed_minus_plain_median_ms"] = sorted(wms)[len(wms) // 2] - sorted(pms)[len(pms) // 2]
    print("30 s clip, B = 1, V = %d: %s ms per step; plain 10 s batch %d: %s ms per step" %
          (V, ", ".join("%.3f" % x for x in wms), V, ", ".join("%.3f" % x for x in pms)), flush=True)
    del e
    torch.cuda.empty_cache()

    ev = Engine(vae=VAE_CONFIG, hifigan=HIFIGAN_CONFIG, dtype="fp16", device=dev)
    ev.load_synthetic(1234)

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

    z = (torch.randn(1, 8, H, 16, generator=g) * 1.1).to(dev)
    mel = ev.vae_decode_tiled(z, Hw, s)
    assert mel.shape == (1, 1, 4 * H, 64) and torch.isfinite(mel).all()
    rec["vae_tiled_ms"] = timed(lambda: ev.vae_decode_tiled(z, Hw, s))
    rec["vocoder_ms"] = timed(lambda: ev.vocode(mel))
    rec["vocoder_samples"] = ev.vocoder_samples(4 * H)
    print("tiled VAE decode %s ms; vocoder (%d frames) %s ms" % (", ".join("%.2f" % x for x in rec["vae_tiled_ms"]), 4 * H,
                                                                 ", ".join("%.2f" % x for x in rec["vocoder_ms"])), flush=True)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
