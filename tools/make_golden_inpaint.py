#!/usr/bin/env python
"""Writes tests/golden/inpaint_ref.npz: what the fork's schedulers (mustango/diffusers/src/diffusers/schedulers, imported through
oracle.ref_import) compute for masked-latent inpainting (audioldm/latent_diffusion/ddim.py:207-233), as data:

  * `an/<kind>/<N>/{sa,sb,x,n,out}`: add_noise on the SD-2.1 config (tango_amd.scheduler.SD21_SCHEDULER_CONFIG) for kind ddpm /
    ddim / dpm and N in ADD_NOISE_STEPS: its scalars sqrt(abar_t), sqrt(1 - abar_t) at every set timestep (add_noise of ones with
    zero noise, and of zeros with unit noise) and its output for a seeded sample / noise pair with one batch row per timestep;
  * `tab/<rule>|<pred>/{coef,blend}`: the engine's coef_table() / blend_table() (tango_amd.scheduler) of every loop configuration,
    as computed here, where they reproduce the fork's step() / add_noise bit for bit (the GPU test drives the kernel with these, so
    that it does not depend on the torch CPU arithmetic of the machine it runs on);
  * `loop/<key>`: the final sample of a masked step loop driven by seeded stand-in model outputs (no UNet) -- before step 0 and
    after every step but the last, x = add_noise(x0, n_i, t_i) * m + (1 - m) * x, then the fork's step() -- over LOOP_GRID
    (rule x prediction type x CFG x mask kind); `loop_inputs()` regenerates every input from the key's seed.

tests/test_inpaint_host.py compares the engine's add_noise / blend_table() with the first part bit for bit;
tests/test_inpaint_gpu.py replays the loops with the fused masked step (tango_op_sched_masked) and compares bit for bit.
Needs the reference tree: python tools/make_golden_inpaint.py"""
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "inpaint_ref.npz")
ADD_NOISE_STEPS = (10, 20, 50, 100)
SHAPE = (2, 8, 16, 4)              # B, C, H, W of the loops: small, so that the fixture stays a few hundred KB
LOOP_STEPS = 10
GUIDANCE = 3.0
# rule name -> (engine rule, DDIM eta, DPM-Solver kwargs)
RULES = {"ddpm": ("ddpm", None, None), "ddim_eta0": ("ddim", 0.0, None), "ddim_eta1": ("ddim", 1.0, None),
         "dpmpp_2m": ("dpmsolver", None, dict(solver_order=2, algorithm_type="dpmsolver++")),
         "dpmpp_3m": ("dpmsolver", None, dict(solver_order=3, algorithm_type="dpmsolver++")),
         "dpm_2m": ("dpmsolver", None, dict(solver_order=2, algorithm_type="dpmsolver"))}
LOOP_GRID = list(itertools.product(list(RULES), ["epsilon", "v_prediction"], [True, False], ["binary", "soft"]))


def sd21(kind, prediction_type=None):
    """the constructor kwargs of scheduler `kind` (ddpm / ddim / dpm) on the SD-2.1 config, for the fork's and the engine's classes"""
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG as S
    base = dict(num_train_timesteps=S["num_train_timesteps"], beta_start=S["beta_start"], beta_end=S["beta_end"],
                beta_schedule=S["beta_schedule"], prediction_type=prediction_type or S["prediction_type"])
    if kind == "ddpm":
        return dict(base, clip_sample=False, variance_type=S["variance_type"])
    if kind == "ddim":
        return dict(base, clip_sample=False, set_alpha_to_one=S["set_alpha_to_one"], steps_offset=S["steps_offset"])
    return base


def loop_key(rule, pred, cfg, mask):
    return "%s|%s|%s|%s" % (rule, pred, "cfg" if cfg else "nocfg", mask)


def loop_seed(i):
    return 5000 + 97 * i


def add_noise_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 2, 4, 4, generator=g), torch.randn(n, 2, 4, 4, generator=g)


def loop_inputs(seed, n, cfg, mask_kind):
    """x_T, x0, m and per step: model output [B2, ...], step noise, blend noise -- all from one seeded CPU generator"""
    g = torch.Generator().manual_seed(seed)
    B = SHAPE[0]
    x = torch.randn(*SHAPE, generator=g)
    x0 = torch.randn(*SHAPE, generator=g)
    r = torch.rand(B, 1, *SHAPE[2:], generator=g)
    m = (r > 0.5).float() if mask_kind == "binary" else r
    outs, znoise, bnoise = [], [], []
    for _ in range(n):
        outs.append(torch.randn((2 * B if cfg else B,) + SHAPE[1:], generator=g))
        znoise.append(torch.randn(*SHAPE, generator=g))
        bnoise.append(torch.randn(*SHAPE, generator=g))
    return x, x0, m, outs, znoise, bnoise


def guided(mo, cfg):
    if not cfg:
        return mo
    u, c = mo.chunk(2)
    return u + GUIDANCE * (c - u)


def engine_scheduler(rule, pred):
    """the engine's scheduler of a loop rule on the SD-2.1 config"""
    from tango_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    kind, eta, dpm = RULES[rule]
    if kind == "ddpm":
        return DDPMScheduler(**sd21("ddpm", pred))
    if kind == "ddim":
        return DDIMScheduler(**sd21("ddim", pred), eta=eta)
    return DPMSolverMultistepScheduler(**sd21("dpm", pred), **dpm)


def run_fork_loop(forks, rule, pred, cfg, mask_kind, seed, n=LOOP_STEPS):
    """the masked loop with the fork's scheduler of `rule` (forks: dict kind -> class)"""
    kind, eta, dpm = RULES[rule]
    if kind == "ddpm":
        sch = forks["ddpm"](**sd21("ddpm", pred))
    elif kind == "ddim":
        sch = forks["ddim"](**sd21("ddim", pred))
    else:
        sch = forks["dpm"](**sd21("dpm", pred), **dpm)
    sch.set_timesteps(n)
    x, x0, m, outs, znoise, bnoise = loop_inputs(seed, n, cfg, mask_kind)
    ts = sch.timesteps
    x = sch.add_noise(x0, bnoise[0], ts[0:1]) * m + (1.0 - m) * x
    for i, t in enumerate(ts):
        v = guided(outs[i], cfg)
        if kind == "ddpm":
            # the fork draws the step noise with randn_tensor(shape, generator): a CPU generator in the state znoise[i] came from
            gen = torch.Generator().manual_seed(0)
            gen.set_state(_state_before(seed, i, n, cfg, mask_kind))
            assert torch.equal(torch.randn(*SHAPE, generator=torch.Generator().set_state(gen.get_state())), znoise[i])
            x = sch.step(v, t, x, generator=gen).prev_sample
        elif kind == "ddim":
            x = sch.step(v, t, x, eta=eta, variance_noise=znoise[i] if eta > 0 else None).prev_sample
        else:
            x = sch.step(v, t, x).prev_sample
        if i + 1 < n:
            x = sch.add_noise(x0, bnoise[i + 1], ts[i + 1:i + 2]) * m + (1.0 - m) * x
    return x


def _state_before(seed, i, n, cfg, mask_kind):
    """the loop_inputs() generator's state just before znoise[i] is drawn"""
    g = torch.Generator().manual_seed(seed)
    B = SHAPE[0]
    torch.randn(*SHAPE, generator=g)
    torch.randn(*SHAPE, generator=g)
    torch.rand(B, 1, *SHAPE[2:], generator=g)
    for k in range(i + 1):
        torch.randn((2 * B if cfg else B,) + SHAPE[1:], generator=g)
        if k == i:
            return g.get_state()
        torch.randn(*SHAPE, generator=g)
        torch.randn(*SHAPE, generator=g)


def main():
    from oracle import ref_import as R
    R._setup()
    from diffusers.schedulers.scheduling_ddim import DDIMScheduler
    from diffusers.schedulers.scheduling_ddpm import DDPMScheduler
    from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler
    forks = {"ddpm": DDPMScheduler, "ddim": DDIMScheduler, "dpm": DPMSolverMultistepScheduler}
    rec = {}
    for kind, n in itertools.product(("ddpm", "ddim", "dpm"), ADD_NOISE_STEPS):
        s = forks[kind](**sd21(kind))
        s.set_timesteps(n)
        ts = s.timesteps
        sa = s.add_noise(torch.ones(n), torch.zeros(n), ts)
        sb = s.add_noise(torch.zeros(n), torch.ones(n), ts)
        x, z = add_noise_inputs(n, 300 + n)
        out = s.add_noise(x, z, ts)
        p = "an/%s/%d/" % (kind, n)
        rec.update({p + "t": ts.numpy().astype(np.int64), p + "sa": sa.numpy(), p + "sb": sb.numpy(), p + "x": x.numpy(),
                    p + "n": z.numpy(), p + "out": out.numpy()})
    for rule, pred in itertools.product(RULES, ["epsilon", "v_prediction"]):
        s = engine_scheduler(rule, pred)
        s.set_timesteps(LOOP_STEPS)
        rec["tab/%s|%s/coef" % (rule, pred)] = s.coef_table()
        rec["tab/%s|%s/blend" % (rule, pred)] = s.blend_table()
    for i, (rule, pred, cfg, mk) in enumerate(LOOP_GRID):
        seed = loop_seed(i)
        x = run_fork_loop(forks, rule, pred, cfg, mk, seed)
        rec["loop/" + loop_key(rule, pred, cfg, mk)] = x.numpy()
        rec["seed/" + loop_key(rule, pred, cfg, mk)] = np.int64(seed)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(LOOP_GRID), "loops")


if __name__ == "__main__":
    main()
