#!/usr/bin/env python
"""Timing of timed prompts on the bench model (full-size UNet, synthetic weights, fp16, 64 text tokens, CFG 3, B = 1):

  * the per-step time of a 30 s, three-segment timeline call (H = 768, Hw = 256, s = 128: V = 5 windows, 10 UNet rows of height 256 per
    step; one text row per window gathered from three segment rows, the tapered weights of tango_amd.inpaint.window_taper; DDIM,
    --steps steps, graph replay; device events around the replays, Engine.last_denoise_ms) and, in the same process and alternating
    with it, of generate_long's loop of the same geometry: Engine.denoise_windows with one text for every window and no weights;
  * the same pair for a 10 s, two-segment loop (H = Hw = 256, s = 128: V = 2 views on a ring) against generate_loop's loop,
    Engine.denoise_ring without weights.
    The two arms of a pair run the same UNet program on the same plan; they differ in the update kernel (weighted / unweighted) and in
    the text rows.  Every call runs --rounds times; the spread of each over the rounds is the yardstick for their difference.

usage: python tools/timeline_timing.py [--steps 50] [--rounds 5] [--out profiles/timeline_timing.json]"""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from tango_amd.engine import UNET_CONFIG_LARGE, Engine
    from tango_amd.inpaint import timeline_geometry, window_taper
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler

    dev = "cuda:0"
    rec = {"steps": args.steps, "rounds": args.rounds, "dtype": "fp16", "sampler": "ddim eta 0", "guidance": 3.0, "text_len": L, "batch": 1,
           "calls": []}
    g = torch.Generator().manual_seed(7)
    e = Engine(unet=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    e.load_synthetic(1234)
    sch = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    kw = dict(prediction_type=sch.config.prediction_type, rule=sch.rule, seed=1, use_graph=True)
    cases = [("30 s, three segments", False, 30.0, [("rain", 0), ("thunder rolls in", 12.5), ("birds after the storm", 22)]),
             ("10 s loop, two segments", True, 10.0, [("waves", 0), ("gulls", 5)])]

    for name, loop, duration, segments in cases:
        H, Hw, s, V, wp = timeline_geometry(segments, duration, 10.0, 5.0, loop)
        S = len(segments)
        enc = torch.randn(2 * S, L, UNET_CONFIG_LARGE["cross_attention_dim"], generator=g)
        enc[:S] = enc[0]                                      # the unconditional rows: T5("") for every segment
        mask = torch.ones(2 * S, L, dtype=torch.bool)
        mask[:S, 1:] = False                                  # ... which keeps one token
        rows_t = [half * S + i for half in (0, 1) for i in wp]                  # the timeline call: a row per window from its segment
        rows_u = [half * S for half in (0, 1) for _ in range(V)]                # generate_long / generate_loop: segment 0's text everywhere
        enc_t, mask_t, enc_u, mask_u = enc[rows_t].to(dev), mask[rows_t], enc[rows_u].to(dev), mask[rows_u]
        lat0 = torch.randn(1, 8, H, 16, generator=g).to(dev)
        taper = window_taper(Hw, s)
        run = e.denoise_ring if loop else e.denoise_windows

        def call(n, weighted):
            sch.set_timesteps(n)
            lat = lat0.clone()
            run(lat, enc_t if weighted else enc_u, mask_t if weighted else mask_u, sch.timesteps.numpy(), sch.coef_table(), 3.0, window_h=Hw,
                stride=s, view_weights=taper if weighted else None, **kw)
            torch.cuda.synchronize()
            assert torch.isfinite(lat).all()
            return e.last_denoise_ms()[1]

        call(2, True), call(2, False)                         # the plan, both graph captures
        plans = e.plan_stats()[1]
        tms, ums = [], []
        for _ in range(args.rounds):
            tms.append(call(args.steps, True))
            ums.append(call(args.steps, False))
        assert e.plan_stats()[1] == plans
        rec["calls"].append({"call": name, "loop": loop, "duration_s": duration, "canvas_h": H, "window_h": Hw, "stride": s, "views": V,
                             "window_prompt": wp, "unet_rows": 2 * V, "timeline_step_ms": tms, "unweighted_step_ms": ums,
                             "timeline_median_ms": median(tms), "unweighted_median_ms": median(ums),
                             "timeline_spread_ms": max(tms) - min(tms), "unweighted_spread_ms": max(ums) - min(ums),
                             "timeline_minus_unweighted_median_ms": median(tms) - median(ums)})
        print("%s, B = 1, V = %d: timeline %s ms per step; unweighted, one text: %s ms per step" %
              (name, V, ", ".join("%.3f" % x for x in tms), ", ".join("%.3f" % x for x in ums)), flush=True)
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
