"""Masked-latent inpainting, host side (no GPU): the schedulers' add_noise / blend_table() bit for bit against the fork
(tests/golden/inpaint_ref.npz, tools/make_golden_inpaint.py), the latent mask of audioldm/ldm.py:773-777, the waveform preparation
of tools/torch_tools.py:9-54, and the fixture's masked loops replayed on the CPU through the torch step rules."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import tango_oracle as O
from tango_amd.inpaint import SEGMENT, latent_mask, prepare_waveform
from tango_amd.scheduler import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "inpaint_ref.npz")


def golden_tool():
    spec = importlib.util.spec_from_file_location("make_golden_inpaint", os.path.join(ROOT, "tools", "make_golden_inpaint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = golden_tool()
_fix = {}


def fixture():
    if not _fix:
        with np.load(GOLDEN) as z:
            _fix.update({k: z[k] for k in z.files})
    return _fix


ENGINE = {"ddpm": DDPMScheduler, "ddim": DDIMScheduler, "dpm": DPMSolverMultistepScheduler}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- add_noise / blend_table vs the fork ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddpm", "ddim", "dpm"])
@pytest.mark.parametrize("n", G.ADD_NOISE_STEPS)
def test_blend_table_and_add_noise_bitwise(kind, n):
    f = fixture()
    p = "an/%s/%d/" % (kind, n)
    s = ENGINE[kind](**G.sd21(kind))
    s.set_timesteps(n)
    assert np.array_equal(s.timesteps.numpy().astype(np.int64), f[p + "t"])
    tab = s.blend_table()
    assert tab.dtype == np.float32 and tab.shape == (n, 2)
    assert np.array_equal(bits(tab[:, 0]), bits(f[p + "sa"]))
    assert np.array_equal(bits(tab[:, 1]), bits(f[p + "sb"]))
    out = s.add_noise(torch.from_numpy(f[p + "x"]), torch.from_numpy(f[p + "n"]), s.timesteps)
    assert np.array_equal(bits(out.numpy()), bits(f[p + "out"]))


@pytest.mark.parametrize("rule,pred", [(r, p) for r in G.RULES for p in ("epsilon", "v_prediction")])
def test_loop_tables_match_fixture(rule, pred):
    """the tables tests/test_inpaint_gpu.py drives the masked kernel with are what the engine's schedulers compute"""
    f = fixture()
    s = G.engine_scheduler(rule, pred)
    s.set_timesteps(G.LOOP_STEPS)
    assert np.array_equal(bits(s.coef_table()), bits(f["tab/%s|%s/coef" % (rule, pred)]))
    assert np.array_equal(bits(s.blend_table()), bits(f["tab/%s|%s/blend" % (rule, pred)]))


def test_blend_table_needs_set_timesteps():
    with pytest.raises(ValueError):
        DDPMScheduler(**G.sd21("ddpm")).blend_table()


# ---- the fixture's masked loops on the CPU (torch step rules already pinned to the fork bit for bit) --------------------------------
class _Oracle:
    """the scheduler of a fixture rule with a step(guided, t, x, noise) that takes the step noise"""

    def __init__(self, rule, pred):
        kind, eta, dpm = G.RULES[rule]
        self.kind, self.eta = kind, eta
        if kind == "ddpm":
            self.s = O.DDPMOracle(**G.sd21("ddpm", pred))
            self.blend = DDPMScheduler(**G.sd21("ddpm", pred))
        elif kind == "ddim":
            self.s = O.DDIMOracle(**G.sd21("ddim", pred), eta=eta)
            self.blend = DDIMScheduler(**G.sd21("ddim", pred))
        else:
            self.s = DPMSolverMultistepScheduler(**G.sd21("dpm", pred), **dpm)
            self.blend = self.s

    def set_timesteps(self, n):
        self.s.set_timesteps(n)
        self.blend.set_timesteps(n)
        return self.blend.timesteps

    def step(self, v, t, x, z):
        if self.kind == "dpmsolver":
            return self.s.step(v, t, x).prev_sample
        return self.s.step(v, t, x, noise=z)


def cpu_masked_loop(rule, pred, cfg, mk, seed, n=G.LOOP_STEPS):
    o = _Oracle(rule, pred)
    ts = o.set_timesteps(n)
    x, x0, m, outs, zn, bn = G.loop_inputs(seed, n, cfg, mk)
    x = o.blend.add_noise(x0, bn[0], ts[0:1]) * m + (1.0 - m) * x
    for i, t in enumerate(ts):
        x = o.step(G.guided(outs[i], cfg), t, x, zn[i])
        if i + 1 < n:
            x = o.blend.add_noise(x0, bn[i + 1], ts[i + 1:i + 2]) * m + (1.0 - m) * x
    return x


@pytest.mark.parametrize("rule,pred,cfg,mk", G.LOOP_GRID)
def test_fixture_loops_on_cpu(rule, pred, cfg, mk):
    f = fixture()
    key = G.loop_key(rule, pred, cfg, mk)
    got = cpu_masked_loop(rule, pred, cfg, mk, int(f["seed/" + key]))
    assert np.array_equal(bits(got.numpy()), bits(f["loop/" + key])), "max diff %g" % np.abs(got.numpy() - f["loop/" + key]).max()


# ---- latent mask -------------------------------------------------------------------------------------------------------------------
def _mask_by_hand(b, tr, fr, h, w):
    m = np.ones((b, 1, h, w), np.float32)
    r0, r1 = int(h * tr[0]), int(h * tr[1])
    c0, c1 = int(w * fr[0]), int(w * fr[1])
    for r in range(h):
        for c in range(w):
            if r0 <= r < r1 or c0 <= c < c1:
                m[:, 0, r, c] = 0
    return m


@pytest.mark.parametrize("tr,fr", [((0.10, 0.15), (1.0, 1.0)), ((0.25, 0.75), (0.75, 1.0)), ((0.0, 1.0), (0.0, 0.0)),
                                   ((0.5, 0.5), (0.0, 0.5)), ((0.33, 0.67), (0.1, 0.3)), ((0.0, 0.0), (1.0, 1.0))])
def test_latent_mask_matches_ldm_indexing(tr, fr):
    m = latent_mask(3, tr, fr)
    assert m.shape == (3, 1, 256, 16) and m.dtype == torch.float32
    assert np.array_equal(m.numpy(), _mask_by_hand(3, tr, fr, 256, 16))


def test_latent_mask_defaults():
    m = latent_mask(1)
    rows = torch.nonzero((m[0, 0] == 0).all(1)).flatten().tolist()
    assert rows == list(range(25, 38))                       # int(25.6) .. int(38.4) - 1
    assert bool((m[0, 0, :25] == 1).all()) and bool((m[0, 0, 38:] == 1).all())   # (1.0, 1.0): no frequency column zeroed
    m2 = latent_mask(2, (0.10, 0.15), (0.5, 1.0), h=40, w=10)
    assert m2.shape == (2, 1, 40, 10)
    assert bool((m2[:, :, :, 5:] == 0).all()) and bool((m2[:, :, 4:6] == 0).all()) and float(m2[0, 0, 0, 0]) == 1.0


# ---- waveform preparation ------------------------------------------------------------------------------------------------------------
def _prepare_by_hand(a):
    a = np.asarray(a, np.float32)
    a = a - np.float32(a.mean(dtype=np.float64))
    a = a / (np.abs(a).max() + np.float32(1e-8))
    a = a * np.float32(0.5)
    a = a[:SEGMENT] if len(a) >= SEGMENT else np.concatenate([a, np.zeros(SEGMENT - len(a), np.float32)])
    return np.float32(0.5) * (a / np.abs(a).max())


def test_prepare_waveform_short_clip():
    a = np.array([1.0, -3.0, 2.0, 0.0], np.float32)             # mean 0 -> / 3 -> * 0.5 -> pad -> / 0.5 -> * 0.5
    w = prepare_waveform(a)
    assert w.shape == (SEGMENT,) and w.dtype == torch.float32
    exp = np.zeros(SEGMENT, np.float32)
    exp[:4] = np.array([1 / 3, -1, 2 / 3, 0], np.float32) * 0.5
    np.testing.assert_allclose(w.numpy(), exp, rtol=0, atol=1e-7)
    assert float(w.abs().max()) == 0.5


def test_prepare_waveform_long_clip_is_cropped():
    g = np.random.default_rng(3)
    a = g.standard_normal(SEGMENT + 5000).astype(np.float32)
    w = prepare_waveform(torch.from_numpy(a))
    assert w.shape == (SEGMENT,)
    np.testing.assert_allclose(w.numpy(), _prepare_by_hand(a), rtol=0, atol=1e-6)


def test_prepare_waveform_removes_dc_offset():
    t = np.arange(16000, dtype=np.float64) / 16000
    a = (3.0 + 0.25 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)
    w = prepare_waveform(a)
    np.testing.assert_allclose(w.numpy(), _prepare_by_hand(a), rtol=0, atol=1e-6)
    assert abs(float(w[:16000].mean())) < 1e-3               # the 3.0 offset is gone
    assert float(w.abs().max()) == 0.5 and bool((w[16000:] == 0).all())


def test_prepare_waveform_rejects_batches():
    with pytest.raises(ValueError):
        prepare_waveform(np.zeros((2, 100), np.float32))
