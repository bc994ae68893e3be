#!/usr/bin/env python
"""Writes tests/golden/dpm_multistep_ref.json: what the fork's DPMSolverMultistepScheduler
(mustango/diffusers/src/diffusers/schedulers/scheduling_dpmsolver_multistep.py, imported through oracle.ref_import) computes, as data:

  * `timesteps`: set_timesteps(n) for the step counts of STEP_COUNTS;
  * `tables`: SHA-256 digests of alpha_t, sigma_t and lambda_t per beta schedule;
  * `loops`: per configuration of the grid (algorithm x solver type x order x prediction type x N x lower_order_final x beta
    schedule), one SHA-256 digest of the fork's per-step prev_sample sequence for the seeded inputs of `loop_inputs()` (any step
    that differs in one bit changes it) and a few sampled values of the final sample.

tests/test_dpm_solver_host.py replays the same loops through tango_amd.scheduler.DPMSolverMultistepScheduler.step and compares.
Needs the reference tree: python tools/make_golden_dpm.py"""
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dpm_multistep_ref.json")
STEP_COUNTS = (1, 2, 3, 5, 10, 20, 25, 50, 100, 999)
BETAS = {"linear": dict(beta_schedule="linear"),
         "scaled_linear": dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012),      # SD-2.1
         "squaredcos_cap_v2": dict(beta_schedule="squaredcos_cap_v2")}
GRID = list(itertools.product(["dpmsolver++", "dpmsolver"], ["midpoint", "heun"], [1, 2, 3], ["epsilon", "sample", "v_prediction"],
                              [10, 20], [True, False], list(BETAS)))
SAMPLE_IDX = (77, 1000)


def config_key(algo, solver, order, pred, n, lof, beta):
    return "%s|%s|%d|%s|%d|%d|%s" % (algo, solver, order, pred, n, int(lof), beta)


def config_kwargs(algo, solver, order, pred, lof, beta):
    return dict(BETAS[beta], algorithm_type=algo, solver_type=solver, solver_order=order, prediction_type=pred, lower_order_final=lof)


def digest(t):
    """SHA-256 of a tensor's dtype, shape and bytes (the pattern of tests/golden/reference_diff.json)"""
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def loop_inputs(n, seed):
    """the initial sample [2, 8, 16, 4] and one model output per step, from one seeded CPU generator"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 8, 16, 4, generator=g)
    return x, [torch.randn(2, 8, 16, 4, generator=g) for _ in range(n)]


def run_loop(sch, n, seed):
    """(digest of the per-step prev_sample sequence, final sample)"""
    sch.set_timesteps(n)
    x, outs = loop_inputs(n, seed)
    h = hashlib.sha256()
    for mo, t in zip(outs, sch.timesteps):
        x = sch.step(mo, t, x).prev_sample
        h.update(digest(x).encode())
    return h.hexdigest(), x


def main():
    from oracle import ref_import as R
    R._setup()
    from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler as Fork
    rec = {"source": "mustango/diffusers/src/diffusers/schedulers/scheduling_dpmsolver_multistep.py", "sample_idx": list(SAMPLE_IDX),
           "timesteps": {}, "tables": {}, "loops": {}}
    for n in STEP_COUNTS:
        s = Fork()
        s.set_timesteps(n)
        rec["timesteps"][str(n)] = s.timesteps.tolist()
    for name, kw in BETAS.items():
        s = Fork(**kw)
        rec["tables"][name] = {k: digest(getattr(s, k)) for k in ("alpha_t", "sigma_t", "lambda_t")}
    for i, (algo, solver, order, pred, n, lof, beta) in enumerate(GRID):
        d, x = run_loop(Fork(**config_kwargs(algo, solver, order, pred, lof, beta)), n, 1000 + i)
        flat = x.flatten()
        # s: input seed, h: digest of the per-step samples, v: final sample at sample_idx
        rec["loops"][config_key(algo, solver, order, pred, n, lof, beta)] = {"s": 1000 + i, "h": d,
                                                                              "v": [float(flat[j]) for j in SAMPLE_IDX]}
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(rec["loops"]), "loops")


if __name__ == "__main__":
    main()
