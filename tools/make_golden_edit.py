#!/usr/bin/env python
"""Writes tests/golden/edit_ref.npz: what the fork's schedulers (mustango/diffusers/src/diffusers/schedulers, imported through
oracle.ref_import's path setup) compute for audio-to-audio editing (AudioLDM style_transfer, audioldm/pipeline.py:145-247), as data:

  * `inv_ts/<N>`: DDIMInverseScheduler.set_timesteps(N) on the SD-2.1 config for N in INVERSE_STEPS;
  * `tab/inv|<pred>/coef`, `tab/<rule>|<pred>/{coef,blend}`: the engine's inverse table (LOOP_STEPS rows) and its truncated tables
    `coef_table(start=START)` / `blend_table(start=START)` (tango_amd.scheduler), as computed here, where they reproduce the fork's
    step() bit for bit (the GPU tests drive the kernels with these, so that they do not depend on the torch CPU arithmetic of the
    machine they run on);
  * `inv/<pred>|<cfg>`: the final sample of LOOP_STEPS inverse steps driven by seeded stand-in model outputs (no UNet), over
    prediction type x CFG; `inverse_inputs()` regenerates every input from `seed/inv/<key>`;
  * `trunc/<rule>|<pred>|<cfg>`: the final sample of the truncated loop over `timesteps[START:]` of LOOP_STEPS, from a seeded start,
    with the fork's scheduler after a fresh set_timesteps (the multistep solver therefore restarts at order 1), over TRUNC_RULES x
    prediction type x CFG; `trunc_inputs()` regenerates the inputs from `seed/trunc/<key>`;
  * `an/<kind>/{t,x,n,out}`: the fork's add_noise at the encode timestep `timesteps[START - 1]` for a seeded pair.

While writing, every loop is also replayed with the engine's table rows applied in the fused kernels' expression order
(`table_step`, torch) and must agree bit for bit.  tests/test_edit_host.py and tests/test_edit_gpu.py read the file.
Needs the reference tree: python tools/make_golden_edit.py"""
import importlib.util
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _inpaint_tool():
    spec = importlib.util.spec_from_file_location("make_golden_inpaint", os.path.join(ROOT, "tools", "make_golden_inpaint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


I = _inpaint_tool()          # sd21(), RULES, engine_scheduler(), guided(): the loop conventions of the inpainting fixture

OUT = os.path.join(ROOT, "tests", "golden", "edit_ref.npz")
INVERSE_STEPS = (10, 20, 50)
SHAPE = I.SHAPE                    # (2, 8, 16, 4)
LOOP_STEPS = 10
START = 4
GUIDANCE = I.GUIDANCE
PREDS = ("epsilon", "sample", "v_prediction")
TRUNC_RULES = ("ddpm", "ddim_eta0", "ddim_eta1", "dpmpp_2m", "dpmpp_3m")
INVERSE_GRID = list(itertools.product(PREDS, [True, False]))
TRUNC_GRID = list(itertools.product(TRUNC_RULES, ["epsilon", "v_prediction"], [True, False]))


def inv_key(pred, cfg):
    return "%s|%s" % (pred, "cfg" if cfg else "nocfg")


def trunc_key(rule, pred, cfg):
    return "%s|%s|%s" % (rule, pred, "cfg" if cfg else "nocfg")


def inverse_kwargs(pred):
    """the constructor kwargs of DDIMInverseScheduler on the SD-2.1 config (fork and engine)"""
    kw = I.sd21("ddim", pred)
    kw.pop("set_alpha_to_one")
    return dict(kw, set_alpha_to_zero=True)


def inverse_inputs(seed, n, cfg):
    """clean start x0 and one stand-in model output [B2, ...] per step, from one seeded CPU generator"""
    g = torch.Generator().manual_seed(seed)
    B = SHAPE[0]
    x = torch.randn(*SHAPE, generator=g)
    outs = [torch.randn((2 * B if cfg else B,) + SHAPE[1:], generator=g) for _ in range(n)]
    return x, outs


def noise_seed(seed, i):
    return seed * 1000 + i


def trunc_inputs(seed, n_exec, cfg):
    """start latents, and per EXECUTED step a stand-in model output and the step noise; each step noise comes from a generator of
    its own (noise_seed), the state the fork's step(generator=...) is handed"""
    g = torch.Generator().manual_seed(seed)
    B = SHAPE[0]
    x = torch.randn(*SHAPE, generator=g)
    outs = [torch.randn((2 * B if cfg else B,) + SHAPE[1:], generator=g) for _ in range(n_exec)]
    zn = [torch.randn(*SHAPE, generator=torch.Generator().manual_seed(noise_seed(seed, i))) for i in range(n_exec)]
    return x, outs, zn


def add_noise_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*SHAPE, generator=g), torch.randn(*SHAPE, generator=g)


def table_step(row, rule, pred, v, x, nz=None):
    """one update of the fused one-step kernel (tango_amd/csrc/sched.hip sched_step_kernel) from a table row, in its expression
    order, in torch fp32: rule "ddpm" or "ddim" (the inverse table runs as "ddim")"""
    sa, sb, c0, c1, sig, sap, dirc = (torch.tensor(float(r), dtype=torch.float32) for r in row[:7])
    if pred == "epsilon":
        x0 = (x - sb * v) / sa
    elif pred == "sample":
        x0 = v
    else:
        x0 = sa * x - sb * v
    if rule == "ddpm":
        prev = c0 * x0 + c1 * x
    else:
        if pred == "epsilon":
            e = v
        elif pred == "sample":
            e = (x - sa * x0) / sb
        else:
            e = sa * v + sb * x
        prev = sap * x0 + dirc * e
    if float(sig) > 0:
        prev = prev + sig * nz
    return prev


def run_fork_inverse(cls, pred, cfg, seed, n=LOOP_STEPS):
    sch = cls(**inverse_kwargs(pred))
    sch.set_timesteps(n)
    x, outs = inverse_inputs(seed, n, cfg)
    for i, t in enumerate(sch.timesteps):
        x = sch.step(I.guided(outs[i], cfg), int(t), x).prev_sample
    return x


def run_fork_trunc(forks, rule, pred, cfg, seed, n=LOOP_STEPS, start=START):
    kind, eta, dpm = I.RULES[rule]
    if kind == "ddpm":
        sch = forks["ddpm"](**I.sd21("ddpm", pred))
    elif kind == "ddim":
        sch = forks["ddim"](**I.sd21("ddim", pred))
    else:
        sch = forks["dpm"](**I.sd21("dpm", pred), **dpm)
    sch.set_timesteps(n)
    x, outs, zn = trunc_inputs(seed, n - start, cfg)
    for j, t in enumerate(sch.timesteps[start:]):
        v = I.guided(outs[j], cfg)
        if kind == "ddpm":
            x = sch.step(v, t, x, generator=torch.Generator().manual_seed(noise_seed(seed, j))).prev_sample
        elif kind == "ddim":
            x = sch.step(v, t, x, eta=eta, variance_noise=zn[j] if eta > 0 else None).prev_sample
        else:
            x = sch.step(v, t, x).prev_sample
    return x


def replay_tables(rule, pred, cfg, seed, coef, n=LOOP_STEPS, start=START):
    """the truncated loop from the engine's table (one-step rules: table_step; multistep: the engine scheduler's own step())"""
    kind = I.RULES[rule][0]
    x, outs, zn = trunc_inputs(seed, n - start, cfg)
    if kind == "dpmsolver":
        sch = I.engine_scheduler(rule, pred)
        sch.set_timesteps(n)
        for j, t in enumerate(sch.timesteps[start:]):
            x = sch.step(I.guided(outs[j], cfg), t, x).prev_sample
        return x
    for j in range(n - start):
        x = table_step(coef[j], kind, pred, I.guided(outs[j], cfg), x, zn[j])
    return x


def main():
    from oracle import ref_import as R
    R._setup()
    from diffusers.schedulers.scheduling_ddim import DDIMScheduler
    from diffusers.schedulers.scheduling_ddim_inverse import DDIMInverseScheduler
    from diffusers.schedulers.scheduling_ddpm import DDPMScheduler
    from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    from tango_amd import scheduler as E
    forks = {"ddpm": DDPMScheduler, "ddim": DDIMScheduler, "dpm": DPMSolverMultistepScheduler}
    rec = {}
    for n in INVERSE_STEPS:
        s = DDIMInverseScheduler(**inverse_kwargs("v_prediction"))
        s.set_timesteps(n)
        rec["inv_ts/%d" % n] = s.timesteps.numpy().astype(np.int64)
    for pred in PREDS:
        s = E.DDIMInverseScheduler(**inverse_kwargs(pred))
        s.set_timesteps(LOOP_STEPS)
        rec["tab/inv|%s/coef" % pred] = s.coef_table()
    for rule, pred in itertools.product(TRUNC_RULES, ["epsilon", "v_prediction"]):
        s = I.engine_scheduler(rule, pred)
        s.set_timesteps(LOOP_STEPS)
        rec["tab/%s|%s/coef" % (rule, pred)] = s.coef_table(start=START)
        rec["tab/%s|%s/blend" % (rule, pred)] = s.blend_table(start=START)
    for i, (pred, cfg) in enumerate(INVERSE_GRID):
        seed = 7000 + 89 * i
        x = run_fork_inverse(DDIMInverseScheduler, pred, cfg, seed)
        y, outs = inverse_inputs(seed, LOOP_STEPS, cfg)
        for j in range(LOOP_STEPS):
            y = table_step(rec["tab/inv|%s/coef" % pred][j], "ddim", pred, I.guided(outs[j], cfg), y)
        assert torch.equal(x, y), ("inverse table replay", pred, cfg, (x - y).abs().max())
        rec["inv/" + inv_key(pred, cfg)] = x.numpy()
        rec["seed/inv/" + inv_key(pred, cfg)] = np.int64(seed)
    for i, (rule, pred, cfg) in enumerate(TRUNC_GRID):
        seed = 9000 + 83 * i
        x = run_fork_trunc(forks, rule, pred, cfg, seed)
        y = replay_tables(rule, pred, cfg, seed, rec["tab/%s|%s/coef" % (rule, pred)])
        assert torch.equal(x, y), ("truncated table replay", rule, pred, cfg, (x - y).abs().max())
        rec["trunc/" + trunc_key(rule, pred, cfg)] = x.numpy()
        rec["seed/trunc/" + trunc_key(rule, pred, cfg)] = np.int64(seed)
    for kind in ("ddpm", "ddim", "dpm"):
        s = forks[kind](**I.sd21(kind))
        s.set_timesteps(LOOP_STEPS)
        t = s.timesteps[START - 1:START]
        x, z = add_noise_inputs(400 + len(kind))
        p = "an/%s/" % kind
        rec.update({p + "t": t.numpy().astype(np.int64), p + "x": x.numpy(), p + "n": z.numpy(),
                    p + "out": s.add_noise(x, z, t.expand(SHAPE[0])).numpy()})
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(INVERSE_GRID), "inverse loops,", len(TRUNC_GRID), "truncated loops")


if __name__ == "__main__":
    main()
