#!/usr/bin/env python
"""Timing of the clip durations on the bench model (full-size UNet, mel-VAE, HiFi-GAN, synthetic weights, fp16, 64 text tokens, CFG):

  * the per-step time of the graph-replayed denoise launch (device events around the replays, Engine.last_denoise_ms) at B = 8 and
    B = 32 prompts for the latent heights 64, 128, 256 and 512 (2.5, 5, 10 and 20 s);
  * the mel-VAE decoder and the vocoder, milliseconds per pass at the same batches and heights (device events, --reps passes);
  * tango_engine_profile_unet's per-op table at every height and at 192 (7.5 s: the one grid height that is no power of two), UNet
    batches 16 and 64, rows with the same label summed; --ops-only takes these tables alone;
  * with --parent-root DIR (a built checkout of the parent commit): the default-height step of that tree, measured twice, in processes of
    their own that alternate with this tree's -- parent, this tree, parent.  The spread between the two parent runs is the yardstick for
    the difference between this tree and the parent at H = 256.

Every tree is measured in a fresh child process (one engine set at a time on the device); the parent is driven through the calls both
trees have (no height argument: the default).

usage: python tools/duration_timing.py [--steps 12] [--reps 3] [--parent-root DIR] [--ops-only] [--out profiles/duration_timing.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEIGHTS = (64, 128, 256, 512)
OPS_HEIGHTS = (64, 128, 192, 256, 512)
BATCHES = (8, 32)
L = 64


def measure(args):
    """one tree (args.package_root), this process: returns the record"""
    sys.path.insert(0, args.package_root)
    import torch
    from tango_amd.engine import HIFIGAN_CONFIG, UNET_CONFIG_LARGE, VAE_CONFIG, Engine
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler

    heights = (256,) if args.only_default else HEIGHTS
    hkw = lambda H: {} if H == 256 else {"latent_h": H}      # noqa: E731  (the default height goes through the default call)
    dev = "cuda:0"
    rec = {"heights": list(heights), "steps": args.steps, "reps": args.reps, "unet_step_ms": {}, "vae_ms": {}, "vocoder_ms": {},
           "unet_ops": {}}
    keys = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
    sch = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in keys})
    g = torch.Generator().manual_seed(7)
    e = Engine(unet=UNET_CONFIG_LARGE, dtype="fp16", device=dev)
    e.load_synthetic(1234)
    for B in () if args.ops_only else BATCHES:
        enc = torch.randn(2 * B, L, UNET_CONFIG_LARGE["cross_attention_dim"], generator=g).to(dev)
        mask = torch.ones(2 * B, L, dtype=torch.bool)
        mask[:B, 1:] = False                                  # the unconditional rows: T5("") keeps one token
        for H in heights:
            lat0 = torch.randn(B, 8, H, 16, generator=g).to(dev)
            runs = []
            for n in (2, args.steps, args.steps):             # plan + graph capture, then two timed calls
                sch.set_timesteps(n)
                lat = lat0.clone()
                e.denoise(lat, enc, mask, sch.timesteps.numpy(), sch.coef_table(), 3.0, seed=1, use_graph=True, **hkw(H))
                torch.cuda.synchronize()
                runs.append(e.last_denoise_ms()[1])
            assert torch.isfinite(lat).all()
            rec["unet_step_ms"]["B%d_H%d" % (B, H)] = runs[1:]
            print("UNet step B=%d H=%d: %.3f / %.3f ms (graph replay, %d steps)" % (B, H, runs[1], runs[2], args.steps), flush=True)
            e.drop_plans()
    if not args.only_default:
        for B2 in (16, 64):
            for H in OPS_HEIGHTS:
                rows = e.profile_unet(B2, L, **hkw(H))
                agg = {}
                for lab, ms, gf in rows:
                    a = agg.setdefault(lab, [0, 0.0, 0.0])
                    a[0] += 1
                    a[1] += ms
                    a[2] += gf
                rec["unet_ops"]["B2_%d_H%d" % (B2, H)] = {"total_ms": sum(r[1] for r in rows),
                                                          "ops": [[k, v[0], round(v[1], 4), round(v[2], 2)] for k, v in agg.items()]}
                print("per-op table B2=%d H=%d: %d ops, %.3f ms eager" % (B2, H, len(rows), sum(r[1] for r in rows)), flush=True)
                e.drop_plans()
    del e
    torch.cuda.empty_cache()
    if args.ops_only:
        return rec

    ev = Engine(vae=VAE_CONFIG, hifigan=HIFIGAN_CONFIG, dtype="fp16", device=dev)
    ev.load_synthetic(1234)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / args.reps

    for B in BATCHES:
        for H in heights:
            z = (torch.randn(B, 8, H, 16, generator=g) * 1.1).to(dev)
            mel = ev.vae_decode(z, **hkw(H))
            rec["vae_ms"]["B%d_H%d" % (B, H)] = timed(lambda: ev.vae_decode(z, **hkw(H)))
            rec["vocoder_ms"]["B%d_H%d" % (B, H)] = timed(lambda: ev.vocode(mel))
            print("B=%d H=%d: VAE decoder %.2f ms, vocoder %.2f ms per pass" % (B, H, rec["vae_ms"]["B%d_H%d" % (B, H)],
                                                                               rec["vocoder_ms"]["B%d_H%d" % (B, H)]), flush=True)
            ev.drop_plans()
    return rec


def child(args, root, only_default):
    """measure the tree at `root` in a fresh process"""
    with tempfile.NamedTemporaryFile(suffix=".json", delete=False) as f:
        tmp = f.name
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package-root", root, "--steps", str(args.steps), "--reps", str(args.reps),
           "--out", tmp] + (["--only-default"] if only_default else []) + (["--ops-only"] if args.ops_only else [])
    subprocess.check_call(cmd, timeout=args.child_timeout)
    with open(tmp) as f:
        rec = json.load(f)
    os.unlink(tmp)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its H = 256 step, measured twice")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ops-only", action="store_true", help="only the per-op tables of this tree (no step, VAE, vocoder or parent timing)")
    ap.add_argument("--child-timeout", type=int, default=600)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package-root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--only-default", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        rec = measure(args)
    else:
        rec = {}
        if args.ops_only:
            args.parent_root = None
        if args.parent_root:
            rec["parent_run1"] = child(args, args.parent_root, True)
        rec["branch"] = child(args, ROOT, False)
        if args.parent_root:
            rec["parent_run2"] = child(args, args.parent_root, True)
            cmp_ = {}
            for B in BATCHES:
                k = "B%d_H256" % B
                p1, p2 = min(rec["parent_run1"]["unet_step_ms"][k]), min(rec["parent_run2"]["unet_step_ms"][k])
                br = min(rec["branch"]["unet_step_ms"][k])
                cmp_[k] = {"parent_run1_ms": p1, "parent_run2_ms": p2, "branch_ms": br, "parent_spread_ms": abs(p1 - p2),
                           "branch_minus_parent_mean_ms": br - 0.5 * (p1 + p2)}
                print("H=256 B=%d step: parent %.3f / %.3f ms, this tree %.3f ms" % (B, p1, p2, br))
            rec["default_height_vs_parent"] = cmp_
    print(json.dumps({k: v for k, v in rec.items() if k != "branch"} if not args.child else {"ok": True}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
