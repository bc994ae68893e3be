"""Clips longer than 20 s (MultiDiffusion windows in time): everything that needs no GPU -- the geometry helper, the engine's argument
checks through tango_debug_denoise_windows_check, the Python refusals that fire before any engine call, the C ABI, and the torch
restatement of the windowed update that tests/test_long_gpu.py compares the kernel with.  The restatement is built from the per-view
step arithmetic the existing bit-exact tests pin (the oracle's DDPM / DDIM step(), tests/test_guidance_gpu.py Case.torch_step) and is
checked here against that step (one view) and against the fork's panorama loop written out (value += step(view); count += 1;
value / count, pipeline_stable_diffusion_panorama.py:614-652)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import tango_oracle as O
from tango_amd import _lib
from tango_amd.inpaint import duration_geometry, long_geometry
from tango_amd.models import AudioDiffusion
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
from tango_amd.tango import Tango

_DDPM_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
SD21 = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
N_OP = 4            # steps of the op-level schedules


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
class Sampler:
    """one rule ("ddpm", "ddim0": DDIM eta = 0, "ddim1": DDIM eta = 1), prediction type and clip setting: the engine's coefficient
    table and the oracle step on the same host, paired as the existing bit-exact tests pair them"""

    def __init__(self, rule, pred=None, clip=None, steps=N_OP):
        self.rule, self.pred, self.clip = rule, pred, clip
        over = {k: v for k, v in (("prediction_type", pred), ("clip_sample", clip)) if v is not None}     # None: the SD 2.1 config's own
        if rule == "ddpm":
            self.sch = DDPMScheduler.from_config(dict({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS}, **over))
            self.ora = O.DDPMOracle(**dict(O.SD21_SCHEDULER, **over))
        else:
            eta = 1.0 if rule == "ddim1" else 0.0
            self.sch = DDIMScheduler(**dict(SD21_SCHEDULER_CONFIG, **over), eta=eta)
            self.ora = O.DDIMOracle(**dict(SD21_SCHEDULER_CONFIG, **over), eta=eta)
        self.sch.set_timesteps(steps)
        self.ora.set_timesteps(steps)
        self.coef = np.ascontiguousarray(self.sch.coef_table(), dtype=np.float32)
        self.engine_rule = self.sch.rule

    def step(self, out, i, x, noise):
        """the oracle's step at loop index i: what tango_op_sched_step is pinned to bit for bit"""
        return self.ora.step(out, int(self.sch.timesteps[i]), x, noise=noise)

    def sigma(self, i):
        return float(self.coef[i, 4])


def cover(h, Hw, s, V):
    return [v for v in range(V) if v * s <= h < v * s + Hw]


def window_update(smp, i, x, outs, nz, Hw, s, guidance=None):
    """the windowed update at loop index i.  x [B, C, H, W] the canvas; outs [B2 * V, C, Hw, W] the model outputs in the window
    batch's order (row half * B * V + b * V + v; two halves when `guidance` is given); nz [B, C, H, W] one draw per canvas element.
    Per view, ascending: d_v = the step's result before its noise term (the oracle step with zero noise: prev + sigma * 0 is prev);
    acc = 0 + d_.. + d_..; r = acc / count (an fp32 division); r + sigma * nz when sigma > 0."""
    B, Cc, H, W = x.shape
    V = (H - Hw) // s + 1
    assert (H - Hw) % s == 0
    if guidance is not None:
        u, c = outs.chunk(2)
        outs = u + guidance * (c - u)                          # models.py:246
    o = outs.view(B, V, Cc, Hw, W)
    acc = torch.zeros_like(x)
    cnt = torch.zeros(H, dtype=torch.float32)
    for v in range(V):
        rows = slice(v * s, v * s + Hw)
        xv = x[:, :, rows]
        d = smp.step(o[:, v], i, xv, torch.zeros_like(xv))
        acc[:, :, rows] = acc[:, :, rows] + d
        cnt[rows] += 1
    r = acc / cnt.view(1, 1, H, 1)
    sig = smp.sigma(i)
    if sig > 0:
        r = r + torch.tensor(sig, dtype=torch.float32) * nz
    return r


def window_inputs(B, H, Hw, s, W=16, cfg=True, seed=0, steps=2):
    """a canvas, `steps` model outputs of the window batch and `steps` canvas noises"""
    g = torch.Generator().manual_seed(seed)
    V = (H - Hw) // s + 1
    x = torch.randn(B, 8, H, W, generator=g)
    outs = [torch.randn((2 if cfg else 1) * B * V, 8, Hw, W, generator=g) for _ in range(steps)]
    nz = torch.randn(steps, B, 8, H, W, generator=g)
    return x, outs, nz


CASES = [("ddpm", "epsilon", False), ("ddpm", "v_prediction", False), ("ddpm", "sample", True), ("ddim0", "epsilon", False),
         ("ddim0", "v_prediction", False), ("ddim1", "sample", False), ("ddim1", "v_prediction", True)]


@pytest.mark.parametrize("rule,pred,clip", CASES)
def test_one_view_is_the_plain_step_bit_for_bit(rule, pred, clip):
    """V = 1: (0 + d) / 1 is exact, and sigma * nz is the step's own noise term"""
    smp = Sampler(rule, pred, clip)
    x, outs, nz = window_inputs(2, 16, 16, 16, seed=3)
    for i in (0, N_OP - 1):                                   # a noisy step and the last one (DDPM: sigma = 0)
        u, c = outs[0].chunk(2)
        ref = smp.step(u + 3.0 * (c - u), i, x, nz[0])
        got = window_update(smp, i, x, outs[0], nz[0], 16, 16, guidance=3.0)
        assert torch.equal(got, ref), (rule, pred, i, (got - ref).abs().max().item())


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("H,Hw,s", [(31, 16, 3), (48, 16, 16), (120, 64, 8)])
def test_sigma_zero_is_the_panorama_loop(H, Hw, s, pred):
    """DDIM eta = 0 against the fork's loop (pipeline_stable_diffusion_panorama.py:614-652), written out over DDIMOracle.step per
    view.  Both add the same n = |cover(h)| <= V per-view results in view order and divide once, so they differ by at most the
    roundings of those operations: n - 1 additions of partial sums bounded by n max|d| and one division, each half an ulp -- at
    most n / 2 ulp of n max|d| before the division, i.e. (n / 2 + 1 / 2) ulp of max|d| after it.  The bound asserted is
    (V + 1) / 2 * 2^-23 * max|d| over the views (ulp(max|d|) <= 2^-23 max|d|); equal evaluation order makes the difference 0."""
    smp = Sampler("ddim0", pred)
    B, V = 2, (H - Hw) // s + 1
    x, outs, nz = window_inputs(B, H, Hw, s, cfg=False, seed=11)
    i = 1
    t = int(smp.sch.timesteps[i])
    value, count = torch.zeros_like(x), torch.zeros_like(x)
    o = outs[0].view(B, V, 8, Hw, 16)
    dmax = 0.0
    for v in range(V):                                        # get_views: h_start = v * stride
        h0, h1 = v * s, v * s + Hw
        d = smp.ora.step(o[:, v], t, x[:, :, h0:h1])
        value[:, :, h0:h1] += d
        count[:, :, h0:h1] += 1
        dmax = max(dmax, d.abs().max().item())
    assert (count > 0).all(), "the geometries of this test cover their canvas exactly"
    ref = torch.where(count > 0, value / count, value)
    got = window_update(smp, i, x, outs[0], nz[0], Hw, s)
    bound = (V + 1) / 2 * 2.0 ** -23 * dmax
    err = (got - ref).abs().max().item()
    print("H=%d Hw=%d s=%d %s: max |restatement - panorama| = %.3e (bound %.3e)" % (H, Hw, s, pred, err, bound))
    assert err <= bound
    counts = sorted({len(cover(h, Hw, s, V)) for h in range(H)})
    assert counts == {(31, 16, 3): [1, 2, 3, 4, 5, 6], (48, 16, 16): [1], (120, 64, 8): list(range(1, 9))}[(H, Hw, s)]


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def test_long_geometry():
    assert long_geometry(30) == (768, 256, 128, 5)
    assert long_geometry(15) == (384, 256, 128, 2)
    assert long_geometry(5, window=2.5, hop=1.25) == (128, 64, 32, 3)
    assert long_geometry(40, window=20, hop=20) == (1024, 512, 512, 2)                 # no overlap
    assert long_geometry(12.5, window=10, hop=0.3125) == (320, 256, 8, 9)              # the smallest stride
    assert long_geometry(165) == (4224, 256, 128, 32)                                  # the most windows
    H, Hw, s, V = long_geometry(22.5, 10, 2.5)
    assert Hw == duration_geometry(10)[0] and H == Hw + (V - 1) * s
    with pytest.raises(ValueError, match="30 and 35"):
        long_geometry(31)
    with pytest.raises(ValueError, match="15 and 20"):
        long_geometry(12)
    with pytest.raises(ValueError, match="does not exceed the window"):
        long_geometry(10)
    with pytest.raises(ValueError, match="does not exceed the window"):
        long_geometry(5)
    with pytest.raises(ValueError, match="multiple of 8"):
        long_geometry(30, hop=4.9)
    with pytest.raises(ValueError, match="multiple of 8"):
        long_geometry(30, hop=0)
    with pytest.raises(ValueError, match="exceeds the window"):
        long_geometry(30, window=2.5, hop=5)
    with pytest.raises(ValueError, match="at most 32"):
        long_geometry(170)
    with pytest.raises(ValueError, match="grid"):
        long_geometry(30, window=11)                           # the window is a duration of generate()'s grid
    for bad in (float("nan"), float("inf"), "long"):
        with pytest.raises(ValueError):
            long_geometry(bad)


# ---- the engine's refusals, without a GPU ---------------------------------------------------------------------------------------------
def _wcheck(lib, H=128, Hw=64, s=32, steps=2, batch=1, **fields):
    a = _lib.DenoiseArgs()
    a.num_steps, a.batch, a.guidance_scale, a.latent_h = steps, batch, 3.0, H
    for k, v in fields.items():
        setattr(a, k, v)
    w = _lib.WindowArgs(window_h=Hw, stride=s)
    return lib.tango_debug_denoise_windows_check(C.byref(a), C.byref(w)).decode()


def test_window_refusals(lib):
    assert _wcheck(lib) == "" and _wcheck(lib, rule=1) == "" and _wcheck(lib, H=64) == "", "V = 1 is a good call"
    assert _wcheck(lib, H=112, Hw=64, s=24) == "" and _wcheck(lib, H=64 + 31 * 8, s=8) == ""
    assert "multistep rule is not supported with windows" in _wcheck(lib, rule=2, coef_width=16)
    assert "multistep rule is not supported with windows" in _wcheck(lib, rule=2)
    dummy = np.zeros(8, dtype=np.float32)
    p = dummy.ctypes.data
    assert "known_latents (masked-latent inpainting) is not supported with windows" in _wcheck(lib, known_latents=p, latent_mask=p, blend_coef=p)
    assert "cover the canvas exactly" in _wcheck(lib, H=100)
    assert "cover the canvas exactly" in _wcheck(lib, H=129)
    assert "stride must be in [1, window_h]" in _wcheck(lib, s=0)
    assert "stride must be in [1, window_h]" in _wcheck(lib, s=65)
    assert "window_h must be positive" in _wcheck(lib, Hw=0)
    assert "at least window_h" in _wcheck(lib, H=32)
    assert "at most 32 windows" in _wcheck(lib, H=64 + 32 * 8, s=8)
    assert "not a UNet height" in _wcheck(lib, H=64, Hw=60, s=4)
    assert "states its canvas height" in _wcheck(lib, H=0)
    # tango_engine_denoise's own checks still speak
    assert "num_steps must be positive" in _wcheck(lib, steps=0)
    assert "unknown rule" in _wcheck(lib, rule=7)
    assert "8-float coefficient rows" in _wcheck(lib, coef_width=16)
    assert lib.tango_debug_denoise_windows_check(None, None).decode() == "denoise_windows: null args"


def _bare_model():
    m = AudioDiffusion.__new__(AudioDiffusion)
    m.device = torch.device("cpu")
    return m


def test_python_refusals_before_any_engine_call():
    m = _bare_model()
    pe, pm = torch.zeros(2, 4, 8), torch.ones(2, 4, dtype=torch.bool)
    ddpm = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    dpm = DPMSolverMultistepScheduler(**SD21, solver_order=2, algorithm_type="dpmsolver++")
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported with windows"):
        m.inference_long_from_embeddings(pe, pm, dpm, 4, 3.0, duration=30)
    with pytest.raises(ValueError, match="guidance table is not supported with windows"):
        m.inference_long_from_embeddings(pe, pm, ddpm, 4, [3.0], duration=30)
    with pytest.raises(ValueError, match="30 and 35"):
        m.inference_long_from_embeddings(pe, pm, ddpm, 4, 3.0, duration=33)
    with pytest.raises(ValueError, match="30 and 35"):
        m.inference_long(["rain"], ddpm, 4, 3.0, duration=33)
    t = Tango.__new__(Tango)
    t.scheduler = dpm
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported with windows"):
        t.generate_long("rain", 30)
    t.scheduler = ddpm
    with pytest.raises(ValueError, match="does not exceed the window"):
        t.generate_long("rain", 10)
    with pytest.raises(ValueError, match="guidance table is not supported"):
        t.generate_long("rain", 30, guidance=[3.0])


def test_prepare_latents_takes_a_long_height_only_by_keyword():
    m = _bare_model()
    sch = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    torch.manual_seed(5)
    a = m.prepare_latents(2, sch, 8, torch.float32, "cpu", long_h=768)
    assert a.shape == (2, 8, 768, 16)
    with pytest.raises(ValueError):
        m.prepare_latents(2, sch, 8, torch.float32, "cpu", latent_h=768)       # the default path keeps the duration grid
    with pytest.raises(ValueError):
        m.prepare_latents(2, sch, 8, torch.float32, "cpu", long_h=0)
    torch.manual_seed(5)
    b = m.prepare_latents(2, sch, 8, torch.float32, "cpu", latent_h=256)
    torch.manual_seed(5)
    assert torch.equal(b, m.prepare_latents(2, sch, 8, torch.float32, "cpu")) and b.shape == (2, 8, 256, 16)


def test_abi(lib):
    assert _lib.DenoiseArgs._fields_[-1][0] == "latent_h" and len(_lib.DenoiseArgs._fields_) == 30, "tango_denoise_args_t stays frozen"
    assert [f[0] for f in _lib.WindowArgs._fields_] == ["window_h", "stride"] and C.sizeof(_lib.WindowArgs) == 8
    names = ("tango_engine_denoise_windows", "tango_debug_denoise_windows_check", "tango_engine_vae_decode_tiled_h", "tango_op_sched_windows",
             "tango_op_mel_tile_blend")
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tango_engine.h")).read()
    for s in names:
        assert hasattr(lib, s) and s in _lib.SYMBOLS and s in header
    assert "tango_window_args_t" in header
    from tango_amd.engine import Engine
    import inspect
    for fn, kws in ((Engine.denoise_windows, ("window_h", "stride")), (Engine.vae_decode_tiled, ("window_h", "stride")),
                    (Tango.generate_long, ("duration", "window", "hop", "negative_prompt", "seed")),
                    (AudioDiffusion.inference_long, ("duration", "window", "hop")),
                    (AudioDiffusion.inference_long_from_embeddings, ("duration", "window", "hop"))):
        assert all(k in inspect.signature(fn).parameters for k in kws), fn
