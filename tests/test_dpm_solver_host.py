"""tango_amd.scheduler.DPMSolverMultistepScheduler on the host: schedule, per-step scalars and the torch step() bit for bit against the
fork's DPMSolverMultistepScheduler (tests/golden/dpm_multistep_ref.json, written by tools/make_golden_dpm.py from
mustango/diffusers/src/diffusers/schedulers/scheduling_dpmsolver_multistep.py), the fork's own known answers, the error surface and the
diffusers interoperability entry points (`from_config`, `from_diffusers`)."""
import hashlib
import itertools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tango_amd.scheduler import (SD21_SCHEDULER_CONFIG, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler,
                                 from_diffusers)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dpm_multistep_ref.json")
BETAS = {"linear": dict(beta_schedule="linear"),
         "scaled_linear": dict(beta_schedule="scaled_linear", beta_start=0.00085, beta_end=0.012),
         "squaredcos_cap_v2": dict(beta_schedule="squaredcos_cap_v2")}
_DDPM_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def digest(t):
    a = t.detach().cpu().contiguous().numpy()
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def loop_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 8, 16, 4, generator=g)
    return x, [torch.randn(2, 8, 16, 4, generator=g) for _ in range(n)]


def run_loop(sch, n, seed):
    sch.set_timesteps(n)
    x, outs = loop_inputs(n, seed)
    h = hashlib.sha256()
    for mo, t in zip(outs, sch.timesteps):
        x = sch.step(mo, t, x).prev_sample
        h.update(digest(x).encode())
    return h.hexdigest(), x


def parse_key(key):
    algo, solver, order, pred, n, lof, beta = key.split("|")
    return dict(BETAS[beta], algorithm_type=algo, solver_type=solver, solver_order=int(order), prediction_type=pred,
                lower_order_final=bool(int(lof))), int(n)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 10, 20, 25, 50, 100, 999])
def test_set_timesteps_matches_fork(gold, n):
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(n)
    assert s.timesteps.dtype == torch.int64
    assert s.timesteps.tolist() == gold["timesteps"][str(n)]


@pytest.mark.parametrize("beta", list(BETAS))
def test_noise_tables_match_fork(gold, beta):
    s = DPMSolverMultistepScheduler(**BETAS[beta])
    for k in ("alpha_t", "sigma_t", "lambda_t"):
        assert digest(getattr(s, k)) == gold["tables"][beta][k], k


def test_step_bitwise_vs_fork_fixture(gold):
    """432 loops: algorithm x solver type x order 1/2/3 x prediction type x N {10, 20} (both sides of the `< 15` lower_order_final
    switch) x lower_order_final on / off x three beta schedules; every step's prev_sample bit for bit"""
    idx = gold["sample_idx"]
    bad = []
    for key, rec in gold["loops"].items():
        kw, n = parse_key(key)
        h, x = run_loop(DPMSolverMultistepScheduler(**kw), n, rec["s"])
        if h != rec["h"] or [float(x.flatten()[j]) for j in idx] != rec["v"]:
            bad.append(key)
    assert len(gold["loops"]) == 432
    assert not bad, "%d of %d loops differ from the fork, e.g. %s" % (len(bad), len(gold["loops"]), bad[:3])


def _table_update(sch, n, seed):
    """the fused kernel's arithmetic, restated in torch from coef_table() rows and a ring of converted outputs"""
    sch.set_timesteps(n)
    tab = torch.from_numpy(sch.coef_table())
    x, outs = loop_inputs(n, seed)
    ring = [None, None, None]
    res = []
    for i, mo in enumerate(outs):
        a, s, kx, c0, c1, c2, ir0, ir1, q, ir01, order, algo = [tab[i, j] for j in range(12)]
        pred = sch.config.prediction_type
        if int(algo) == 0:
            m0 = (x - s * mo) / a if pred == "epsilon" else mo if pred == "sample" else a * x - s * mo
        else:
            m0 = mo if pred == "epsilon" else (x - a * mo) / s if pred == "sample" else a * mo + s * x
        nx = kx * x + c0 * m0
        if int(order) == 2:
            nx = nx + c1 * (ir0 * (m0 - ring[(i + 2) % 3]))
        elif int(order) == 3:
            m1, m2 = ring[(i + 2) % 3], ring[(i + 1) % 3]
            d10, d11 = ir0 * (m0 - m1), ir1 * (m1 - m2)
            nx = (nx + c1 * (d10 + q * (d10 - d11))) + c2 * (ir01 * (d10 - d11))
        ring[i % 3] = m0
        x = nx
        res.append(x)
    return res


@pytest.mark.parametrize("algo,solver,order,pred", list(itertools.product(["dpmsolver++", "dpmsolver"], ["midpoint", "heun"], [1, 2, 3],
                                                                           ["epsilon", "sample", "v_prediction"])))
def test_coef_table_drives_the_step(algo, solver, order, pred):
    """the table row alone (fp32 scalars, ring slot step % 3) reproduces step() bit for bit: what the kernel computes"""
    for n in (10, 20):
        kw = dict(BETAS["scaled_linear"], algorithm_type=algo, solver_type=solver, solver_order=order, prediction_type=pred)
        sch = DPMSolverMultistepScheduler(**kw)
        got = _table_update(sch, n, 5)
        ref = DPMSolverMultistepScheduler(**kw)
        ref.set_timesteps(n)
        x, outs = loop_inputs(n, 5)
        for i, (mo, t) in enumerate(zip(outs, ref.timesteps)):
            x = ref.step(mo, t, x).prev_sample
            assert torch.equal(got[i], x), (n, i)


def test_coef_table_orders():
    s = DPMSolverMultistepScheduler(solver_order=3, lower_order_final=True)
    s.set_timesteps(10)
    t = s.coef_table()
    assert t.shape == (10, 16) and t.dtype == np.float32
    assert t[:, 10].tolist() == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1]       # warm-up, then lower_order_final below 15 steps
    s.set_timesteps(20)
    assert s.coef_table()[:, 10].tolist() == [1, 2] + [3] * 18
    s = DPMSolverMultistepScheduler(solver_order=2, lower_order_final=False, algorithm_type="dpmsolver")
    s.set_timesteps(10)
    t = s.coef_table()
    assert t[:, 10].tolist() == [1] + [2] * 9 and (t[:, 11] == 1).all() and (t[:, 12:] == 0).all()


def _dummy_sample_deter():
    n = 4 * 3 * 8 * 8
    return (torch.arange(n).reshape(3, 8, 8, 4) / n).permute(3, 0, 1, 2)


@pytest.mark.parametrize("pred,expect", [("epsilon", 0.3301), ("v_prediction", 0.2251)])
def test_known_answers(pred, expect):
    """the fork's test_scheduler_dpm_multi.py full_loop answers (10 steps, dummy model sample * t / (t + 1))"""
    s = DPMSolverMultistepScheduler(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", solver_order=2,
                                    prediction_type=pred, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=False)
    s.set_timesteps(10)
    x = _dummy_sample_deter()
    for t in s.timesteps:
        x = s.step(x * t / (t + 1), t, x).prev_sample
    assert abs(torch.mean(torch.abs(x)).item() - expect) < 1e-3


def test_interface_attributes():
    s = DPMSolverMultistepScheduler()
    assert s.order == 1 and s.init_noise_sigma == 1.0 and s.rule == "dpmsolver"
    x = torch.randn(2, 3)
    assert s.scale_model_input(x, 5) is x
    assert s.config.clip_sample is False and s.config.solver_order == 2 and s.config.algorithm_type == "dpmsolver++"
    assert DPMSolverMultistepScheduler(algorithm_type="deis").config.algorithm_type == "dpmsolver++"
    for st in ("logrho", "bh1", "bh2"):
        assert DPMSolverMultistepScheduler(solver_type=st).config.solver_type == "midpoint"


def test_error_surface():
    with pytest.raises(NotImplementedError, match="quantile"):
        DPMSolverMultistepScheduler(thresholding=True)
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(algorithm_type="unipc")
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(solver_type="euler")
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(beta_schedule="sigmoid")
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(1000)                                      # linspace(0, 999, 1001).round() repeats a value
    assert len(set(s.timesteps.tolist())) == 999
    with pytest.raises(ValueError):
        s.coef_table()
    s.set_timesteps(999)
    assert s.coef_table().shape == (999, 16)

    class EulerDiscreteScheduler:
        config = {"num_train_timesteps": 1000}
    with pytest.raises(TypeError, match="DPMSolverMultistepScheduler"):
        from_diffusers(EulerDiscreteScheduler())


def test_from_config_of_the_sd21_ddpm_config():
    """the diffusers idiom on Tango's scheduler: DPMSolverMultistepScheduler.from_config(tango.scheduler.config)"""
    ddpm = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    s = DPMSolverMultistepScheduler.from_config(ddpm.config)
    assert s.config.prediction_type == "v_prediction" and s.config.beta_schedule == "scaled_linear"
    assert torch.equal(s.alphas_cumprod, ddpm.alphas_cumprod)
    s2 = DPMSolverMultistepScheduler.from_config(dict(SD21_SCHEDULER_CONFIG, solver_order=3, _class_name="DDPMScheduler"))
    assert s2.config.solver_order == 3
    s3 = DPMSolverMultistepScheduler.from_config(s2.config)
    s2.set_timesteps(20)
    s3.set_timesteps(20)
    assert np.array_equal(s2.coef_table(), s3.coef_table())


def test_from_diffusers_stand_ins():
    def stand_in(name, **config):
        return type(name, (), {"config": config})()

    kw = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", prediction_type="v_prediction",
              solver_order=2, algorithm_type="dpmsolver++", _class_name="DPMSolverMultistepScheduler", _diffusers_version="0.15.0")
    s = from_diffusers(stand_in("DPMSolverMultistepScheduler", **kw))
    assert isinstance(s, DPMSolverMultistepScheduler)
    ref = DPMSolverMultistepScheduler(**{k: v for k, v in kw.items() if not k.startswith("_")})
    s.set_timesteps(25)
    ref.set_timesteps(25)
    assert np.array_equal(s.coef_table(), ref.coef_table())
    d = from_diffusers(stand_in("DDPMScheduler", **dict(SD21_SCHEDULER_CONFIG, thresholding=False, trained_betas=None)))
    assert isinstance(d, DDPMScheduler) and d.config.prediction_type == "v_prediction"
    i = from_diffusers(stand_in("DDIMScheduler", **SD21_SCHEDULER_CONFIG))
    assert isinstance(i, DDIMScheduler) and i.config.steps_offset == 1
    own = DDPMScheduler()
    assert from_diffusers(own) is own
    ns = from_diffusers(type("DPMSolverMultistepScheduler", (), {"config": SimpleNamespace(**kw)})())
    assert isinstance(ns, DPMSolverMultistepScheduler)


@pytest.mark.reference
@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs the reference tree")
def test_step_bitwise_vs_fork_live():
    """the fixture's loops again, live against the imported fork scheduler (reference tree only)"""
    from oracle import ref_import as R
    if not R.available():
        pytest.skip("reference tree not importable")
    R._setup()
    from diffusers.schedulers.scheduling_dpmsolver_multistep import DPMSolverMultistepScheduler as Fork
    for i, (algo, solver, order, pred, n, beta) in enumerate(itertools.product(["dpmsolver++", "dpmsolver"], ["midpoint", "heun"], [1, 2, 3],
                                                                                ["epsilon", "sample", "v_prediction"], [10, 20],
                                                                                ["scaled_linear", "squaredcos_cap_v2"])):
        kw = dict(BETAS[beta], algorithm_type=algo, solver_type=solver, solver_order=order, prediction_type=pred)
        h1, x1 = run_loop(Fork(**kw), n, 77 + i)
        h2, x2 = run_loop(DPMSolverMultistepScheduler(**kw), n, 77 + i)
        assert h1 == h2 and torch.equal(x1, x2), kw


def test_batch_inference_scheduler_flag():
    from tango_amd.batch_inference import make_scheduler, parse_args
    a = parse_args(["--model", "m"])
    assert a.scheduler == "ddpm" and a.solver_order == 2
    a = parse_args(["--model", "m", "--scheduler", "dpmsolver++", "--solver_order", "3"])
    ddpm = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    s = make_scheduler(a.scheduler, ddpm.config, a.solver_order)
    assert isinstance(s, DPMSolverMultistepScheduler) and s.config.solver_order == 3 and s.config.prediction_type == "v_prediction"
    assert make_scheduler("dpmsolver", ddpm.config).config.algorithm_type == "dpmsolver"
    assert isinstance(make_scheduler("ddpm", ddpm.config), DDPMScheduler)
    assert isinstance(make_scheduler("ddim", ddpm.config), DDIMScheduler)
