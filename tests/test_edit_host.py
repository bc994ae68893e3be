"""Host side of audio-to-audio editing (AudioLDM style_transfer, audioldm/pipeline.py:145-247): DDIMInverseScheduler against the
fork's (tests/golden/edit_ref.npz, written by tools/make_golden_edit.py), the truncated coefficient / blend tables, the multistep
solver's order ramp over a truncated schedule, edit_plan's level convention, and the argument checks of Tango.edit that need no GPU."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tango_amd.scheduler import (SD21_SCHEDULER_CONFIG, DDIMInverseScheduler, DDIMScheduler, DDPMScheduler,
                                 DPMSolverMultistepScheduler, from_diffusers)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_edit", os.path.join(ROOT, "tools", "make_golden_edit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _tool()
_fix = {}


def fixture():
    if not _fix:
        with np.load(os.path.join(ROOT, "tests", "golden", "edit_ref.npz")) as z:
            _fix.update({k: z[k] for k in z.files})
    return _fix


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- DDIMInverseScheduler ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", G.INVERSE_STEPS)
def test_inverse_timesteps_equal_the_forks(n):
    s = DDIMInverseScheduler(**G.inverse_kwargs("v_prediction"))
    s.set_timesteps(n)
    assert s.timesteps.dtype == torch.int64
    assert np.array_equal(s.timesteps.numpy(), fixture()["inv_ts/%d" % n])
    assert np.all(np.diff(s.timesteps.numpy()) > 0)


@pytest.mark.parametrize("pred,cfg", G.INVERSE_GRID)
def test_inverse_step_replays_the_forks_loop_bitwise(pred, cfg):
    f = fixture()
    key = G.inv_key(pred, cfg)
    s = DDIMInverseScheduler(**G.inverse_kwargs(pred))
    s.set_timesteps(G.LOOP_STEPS)
    x, outs = G.inverse_inputs(int(f["seed/inv/" + key]), G.LOOP_STEPS, cfg)
    for i, t in enumerate(s.timesteps):
        x = s.step(G.I.guided(outs[i], cfg), t, x).prev_sample
    assert np.array_equal(bits(x.numpy()), bits(f["inv/" + key])), key


@pytest.mark.parametrize("pred", G.PREDS)
def test_inverse_table_layout_and_values(pred):
    s = DDIMInverseScheduler(**G.inverse_kwargs(pred))
    assert s.rule == "ddim"
    with pytest.raises(ValueError):
        s.coef_table()
    s.set_timesteps(G.LOOP_STEPS)
    tab = s.coef_table()
    assert tab.shape == (G.LOOP_STEPS, 8) and tab.dtype == np.float32
    assert np.array_equal(bits(tab), bits(fixture()["tab/inv|%s/coef" % pred]))
    assert np.array_equal(bits(s.coef_table(count=3)), bits(tab[:3]))
    assert not tab[:, [2, 3, 4, 7]].any()                     # no DDPM coefficients, no sigma: the step is deterministic
    ac = s.alphas_cumprod
    ts = s.timesteps.tolist()
    for i, t in enumerate(ts):
        assert tab[i, 0] == float(ac[t] ** 0.5) and tab[i, 1] == float((1 - ac[t]) ** 0.5)
        if i + 1 < len(ts):                                   # the target of step i is the level of step i + 1
            assert tab[i, 5] == tab[i + 1, 0] and tab[i, 6] == tab[i + 1, 1]
    assert tab[-1, 5] == 0.0 and tab[-1, 6] == 1.0            # set_alpha_to_zero: past the schedule's end abar_next = 0
    for bad in (0, G.LOOP_STEPS + 1):
        with pytest.raises(ValueError):
            s.coef_table(count=bad)


def test_inverse_final_alpha_and_from_diffusers():
    kw = dict(G.inverse_kwargs("epsilon"), set_alpha_to_zero=False)
    s = DDIMInverseScheduler(**kw)
    assert float(s.final_alpha_cumprod) == float(s.alphas_cumprod[-1])
    s.set_timesteps(10)
    assert s.coef_table()[-1, 5] == float(s.alphas_cumprod[-1] ** 0.5)

    class DDIMInverseScheduler_(object):
        config = SimpleNamespace(**G.inverse_kwargs("v_prediction"))
    DDIMInverseScheduler_.__name__ = "DDIMInverseScheduler"
    got = from_diffusers(DDIMInverseScheduler_())
    assert type(got) is DDIMInverseScheduler and got.config.steps_offset == 1 and got.config.prediction_type == "v_prediction"
    # built on a sampler's schedule: same betas, same offset, same prediction type
    d = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    inv = DDIMInverseScheduler.from_scheduler(d)
    assert torch.equal(inv.alphas_cumprod, d.alphas_cumprod) and inv.config.steps_offset == 1
    d.set_timesteps(20)
    inv.set_timesteps(20)
    assert np.array_equal(inv.timesteps.numpy(), d.timesteps.numpy()[::-1])


# ---- truncated tables ---------------------------------------------------------------------------------------------------------------
def _one_step_schedulers():
    keys = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
    return [DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in keys}), DDIMScheduler(**SD21_SCHEDULER_CONFIG),
            DDIMScheduler(**SD21_SCHEDULER_CONFIG, eta=1.0)]


@pytest.mark.parametrize("n,start", [(10, 4), (20, 10), (20, 19), (7, 1)])
def test_one_step_truncated_tables_are_rows_of_the_full_tables(n, start):
    for s in _one_step_schedulers():
        s.set_timesteps(n)
        assert np.array_equal(bits(s.coef_table(start=start)), bits(s.coef_table()[start:]))
        assert np.array_equal(bits(s.blend_table(start=start)), bits(s.blend_table()[start:]))
        assert np.array_equal(bits(s.coef_table(start=0)), bits(s.coef_table()))
        for bad in (-1, n, 1.5):
            with pytest.raises(ValueError):
                s.coef_table(start=bad)
            with pytest.raises(ValueError):
                s.blend_table(start=bad)


@pytest.mark.parametrize("rule,pred", [(r, p) for r in G.TRUNC_RULES for p in ("epsilon", "v_prediction")])
def test_truncated_tables_equal_the_fixtures(rule, pred):
    s = G.I.engine_scheduler(rule, pred)
    s.set_timesteps(G.LOOP_STEPS)
    f = fixture()
    assert np.array_equal(bits(s.coef_table(start=G.START)), bits(f["tab/%s|%s/coef" % (rule, pred)]))
    assert np.array_equal(bits(s.blend_table(start=G.START)), bits(f["tab/%s|%s/blend" % (rule, pred)]))


def _dpm(order, **kw):
    return DPMSolverMultistepScheduler(**G.I.sd21("dpm"), solver_order=order, algorithm_type="dpmsolver++", **kw)


def test_multistep_truncated_table_restarts_the_order_ramp():
    for order, n, start, want in ((2, 10, 4, [1, 2, 2, 2, 2, 1]),              # n < 15: lower_order_final ends at order 1
                                  (3, 10, 4, [1, 2, 3, 3, 2, 1]),
                                  (3, 10, 8, [1, 1]),                          # the ramp meets lower_order_final
                                  (3, 10, 7, [1, 2, 1]),
                                  (2, 20, 10, [1] + [2] * 9),                  # n >= 15: no lower_order_final
                                  (3, 20, 10, [1, 2] + [3] * 8)):
        s = _dpm(order)
        s.set_timesteps(n)
        tab = s.coef_table(start=start)
        assert tab.shape == (n - start, 16)
        assert tab[:, 10].astype(int).tolist() == want, (order, n, start)
        full = s.coef_table()
        # every scalar a row's order does not use is 0, and rows at the full table's order are the full table's rows
        for j, o in enumerate(want):
            if o == int(full[start + j, 10]):
                assert np.array_equal(bits(tab[j]), bits(full[start + j]))
            if o == 1:
                assert not tab[j, 4:10].any()
            # the first columns (alpha_s0, sigma_s0, kx, c0) do not depend on the order
            assert np.array_equal(bits(tab[j, :4]), bits(full[start + j, :4]))
    s = _dpm(2, lower_order_final=False)
    s.set_timesteps(10)
    assert s.coef_table(start=4)[:, 10].astype(int).tolist() == [1, 2, 2, 2, 2, 2]


@pytest.mark.parametrize("rule,pred,cfg", G.TRUNC_GRID)
def test_truncated_loops_replay_the_forks_bitwise(rule, pred, cfg):
    """the multistep solver through its own step() (first called at timesteps[start] after a fresh set_timesteps), the one-step
    rules through their table rows in the fused kernel's expression order"""
    f = fixture()
    key = G.trunc_key(rule, pred, cfg)
    s = G.I.engine_scheduler(rule, pred)
    s.set_timesteps(G.LOOP_STEPS)
    got = G.replay_tables(rule, pred, cfg, int(f["seed/trunc/" + key]), s.coef_table(start=G.START))
    assert np.array_equal(bits(got.numpy()), bits(f["trunc/" + key])), key


def test_multistep_step_follows_the_truncated_table():
    """step() over timesteps[start:] runs the orders the truncated table names (state restarts with set_timesteps)"""
    s = _dpm(3)
    s.set_timesteps(10)
    tab = s.coef_table(start=4)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 8, 4, 4, generator=g)
    for j, t in enumerate(s.timesteps[4:]):
        assert s._step_order(4 + j, s.lower_order_nums) == int(tab[j, 10])
        x = s.step(torch.randn(1, 8, 4, 4, generator=g), t, x).prev_sample
    assert torch.isfinite(x).all()


# ---- add_noise at the encode level, edit_plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
def test_add_noise_at_the_encode_timestep_equals_the_forks(kind):
    f = fixture()
    cls = {"ddpm": DDPMScheduler, "ddim": DDIMScheduler, "dpm": DPMSolverMultistepScheduler}[kind]
    s = cls(**G.I.sd21(kind))
    start, t_enc = s.edit_plan(G.LOOP_STEPS, 0.6)
    assert start == G.START and t_enc == int(f["an/%s/t" % kind][0])
    x, n = torch.from_numpy(f["an/%s/x" % kind]), torch.from_numpy(f["an/%s/n" % kind])
    got = s.add_noise(x, n, torch.full((x.shape[0],), t_enc, dtype=torch.int64))
    assert np.array_equal(bits(got.numpy()), bits(f["an/%s/out" % kind]))
    sa, sb = s.blend_table(start=start - 1)[0]                  # the scalars the fused encode launch is handed
    assert np.array_equal(bits((torch.tensor(sa) * x + torch.tensor(sb) * n).numpy()), bits(f["an/%s/out" % kind]))


def test_edit_plan():
    for s in _one_step_schedulers() + [_dpm(2)]:
        start, t_enc = s.edit_plan(20, 0.5)
        assert (start, t_enc) == (10, int(s.timesteps[9]))
        assert len(s.timesteps) == 20
        assert s.edit_plan(20, 0.99) == (1, int(s.timesteps[0]))       # k = 19
        assert s.edit_plan(20, 0.05) == (19, int(s.timesteps[18]))     # k = 1
        # the encode level lies one entry above the first executed timestep (the reference's convention)
        assert t_enc > int(s.timesteps[start])
        for bad in (0.0, 0.04, 1.0, 1.5):                              # k = 0, 0, N, > N
            with pytest.raises(ValueError):
                s.edit_plan(20, bad)
    # k inverse steps from a clean clip land on the DDIM sampler's encode level
    d = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    start, t_enc = d.edit_plan(20, 0.5)
    inv = DDIMInverseScheduler.from_scheduler(d)
    inv.set_timesteps(20)
    k = 20 - start
    assert int(inv.timesteps[k]) == t_enc
    assert inv.coef_table(count=k)[-1, 5] == d.blend_table(start=start - 1)[0, 0]


@pytest.mark.parametrize("n,strength", [(10, 0.5), (20, 0.5), (100, 0.5), (20, 0.25), (20, 0.95), (7, 0.3)])
def test_inversion_built_on_a_sampler_lands_on_its_encode_timestep(n, strength):
    """mode="invert" must end on the level mode="noise" noises to: k inverse steps of DDIMInverseScheduler.from_scheduler(sampler)
    reach the sampler's encode timestep `timesteps[start - 1]` exactly, for the DDIM sampler (the fork's inverse grid) and for the
    multistep DPM-Solver (linspace-spaced timesteps, clean level 0) alike -- not `timesteps[start]`, one entry lower"""
    for s in (DDIMScheduler(**SD21_SCHEDULER_CONFIG), _dpm(2), _dpm(3)):
        start, t_enc = s.edit_plan(n, strength)
        k = n - start
        desc = [int(t) for t in s.timesteps]
        inv = DDIMInverseScheduler.from_scheduler(s)
        inv.set_timesteps(n)
        ts = inv.timesteps.tolist()
        offset = getattr(s.config, "steps_offset", 0)
        assert ts == [offset] + desc[::-1][1:] and all(b > a for a, b in zip(ts, ts[1:]))
        assert ts[k] == t_enc == desc[start - 1] and ts[k] > desc[start]
        # the last of the k rows steps onto exactly the scalars the noise mode's add_noise uses
        tab = inv.coef_table(count=k)
        assert np.array_equal(bits(tab[-1, 5:7]), bits(s.blend_table(start=start - 1)[0]))
        for i in range(k):                                                # every row steps from its level to the next entry's
            ac = inv.alphas_cumprod
            assert tab[i, 0] == float(ac[ts[i]] ** 0.5) and tab[i, 5] == float(ac[ts[i + 1]] ** 0.5)
        # step() walks the same grid: one step from the table row, bit for bit
        x, outs = G.inverse_inputs(11, 1, False)
        got = inv.step(outs[0], ts[k - 1], x).prev_sample
        want = G.table_step(tab[k - 1], "ddim", s.config.prediction_type, outs[0], x)
        assert np.array_equal(bits(got.numpy()), bits(want.numpy()))
    # a DDIM sampler's inverse grid is the fork's own; the sampler handed in is left as it was
    d = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    d.set_timesteps(5)
    inv, bare = DDIMInverseScheduler.from_scheduler(d), DDIMInverseScheduler(**G.inverse_kwargs("v_prediction"))
    inv.set_timesteps(n)
    bare.set_timesteps(n)
    assert inv.timesteps.tolist() == bare.timesteps.tolist() and len(d.timesteps) == 5
    assert np.array_equal(bits(inv.coef_table()), bits(bare.coef_table()))


def test_dpm_inverse_grid_values():
    """the DPM-Solver case in numbers (N = 20, strength 0.5): encode timestep 549, and ten inverse steps end on 549, not on 500"""
    s = _dpm(2)
    start, t_enc = s.edit_plan(20, 0.5)
    inv = DDIMInverseScheduler.from_scheduler(s)
    inv.set_timesteps(20)
    assert (start, t_enc, int(s.timesteps[start])) == (10, 549, 500)
    assert inv.timesteps.tolist()[:4] == [0, 100, 150, 200] and int(inv.timesteps[10]) == 549 and int(inv.timesteps[-1]) == 999
    assert inv.coef_table()[-1, 5] == 0.0                                 # past 999: final_alpha_cumprod (set_alpha_to_zero)


# ---- Tango.edit argument checks that need no GPU --------------------------------------------------------------------------------------
def _bare_tango(scheduler):
    from tango_amd.tango import Tango
    return Tango.from_components(SimpleNamespace(), SimpleNamespace(), scheduler=scheduler)


def test_tango_edit_argument_checks():
    pe, pm = torch.zeros(2, 4, 8), torch.ones(2, 4, dtype=torch.bool)
    audio = np.zeros(16000, dtype=np.float32)
    ddim = _bare_tango(DDIMScheduler(**SD21_SCHEDULER_CONFIG))
    with pytest.raises(ValueError):
        ddim.edit_from_embeddings(pe, pm, audio, mode="nudge", steps=10, samples=1)
    for strength in (0.0, 1.0, 0.05):
        with pytest.raises(ValueError):
            ddim.edit_from_embeddings(pe, pm, audio, strength=strength, steps=10, samples=1)
        with pytest.raises(ValueError):
            ddim.edit("rain", audio, strength=strength, steps=10)
    with pytest.raises(ValueError):
        ddim.edit_from_embeddings(pe, pm, audio, steps=10, samples=2)              # rows != samples (guidance 3: 1 row)
    with pytest.raises(ValueError):
        ddim.edit_from_embeddings(pe, pm, audio, steps=10, samples=1, mode="invert")   # no source_embeds
    # mode="invert" needs a deterministic sampler
    for sch in (_one_step_schedulers()[0], DDIMScheduler(**SD21_SCHEDULER_CONFIG, eta=1.0)):
        with pytest.raises(ValueError):
            _bare_tango(sch).edit_from_embeddings(pe, pm, audio, steps=10, samples=1, mode="invert", source_embeds=pe[:1])
        with pytest.raises(ValueError):
            _bare_tango(sch).edit("rain", audio, steps=10, mode="invert")
    # no mel front-end / VAE encoder: RuntimeError, before anything touches a device
    for sch in (DDIMScheduler(**SD21_SCHEDULER_CONFIG), _dpm(2)):
        with pytest.raises(RuntimeError):
            _bare_tango(sch).edit_from_embeddings(pe, pm, audio, steps=10, samples=1)
        with pytest.raises(RuntimeError):
            _bare_tango(sch).edit_from_embeddings(pe, pm, audio, steps=10, samples=1, mode="invert", source_embeds=pe[:1])
