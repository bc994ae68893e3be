"""Timed prompts (a prompt per window, tapered MultiDiffusion weights): everything that needs no GPU -- the taper, the torch restatement of
the weighted update that tests/test_timeline_gpu.py compares the kernels with, the assignment of windows to segments, the engine's
argument checks through tango_debug_denoise_*_weighted_check, the Python refusals that fire before any engine call, and the C ABI.  The
restatement stands on tests/test_long_host.py's Sampler and tests/test_loop_host.py's ring walk: with all weights 1 it must be their
unweighted updates, bit for bit."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import test_long_host as LH
import test_loop_host as LP
from tango_amd import _lib
from tango_amd.inpaint import timeline_geometry, window_taper
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler, DPMSolverMultistepScheduler
from tango_amd.tango import Tango

LINEAR = [(31, 16, 3), (48, 16, 16), (120, 64, 8)]


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def weighted_window_update(smp, i, x, outs, nz, Hw, s, w, guidance=None, ring=False):
    """the weighted update at loop index i, linear or on a ring.  x [B, C, H, W] the canvas; outs [B2 * V, C, Hw, W] the model outputs in
    the window batch's order; nz [B, C, H, W]; w [Hw] fp32, one weight per local window row.  Per view d_v = the step's result before
    its noise term; per canvas row, over the covering views in the unweighted update's order (ascending; the ring's order),
    acc = 0 + w d + ..., wsum = 0 + w + ...; r = acc / wsum (an fp32 division); r + sigma * nz when sigma > 0.  The product w d is a
    tensor of its own: no multiply-add is fused."""
    B, Cc, H, W = x.shape
    w = torch.as_tensor(np.asarray(w), dtype=torch.float32)
    assert w.shape == (Hw,)
    V = H // s if ring else (H - Hw) // s + 1
    if guidance is not None:
        u, c = outs.chunk(2)
        outs = u + guidance * (c - u)                          # models.py:246
    o = outs.view(B, V, Cc, Hw, W)
    acc = torch.zeros_like(x)
    wsum = torch.zeros(H, dtype=torch.float32)
    if ring:
        assert H % s == 0 and 1 <= s <= Hw <= H
        d = []
        for v in range(V):
            xv = x[:, :, LP.ring_rows(v, H, Hw, s)]
            d.append(smp.step(o[:, v], i, xv, torch.zeros_like(xv)))

        def add(k, v, rows, y):
            t = w[y].view(1, 1, -1, 1) * d[v][:, :, y]
            acc[:, :, rows] = acc[:, :, rows] + t
            wsum[rows] = wsum[rows] + w[y]

        LP._ring_accumulate(H, Hw, s, add)
    else:
        assert (H - Hw) % s == 0
        for v in range(V):
            rows = slice(v * s, v * s + Hw)
            xv = x[:, :, rows]
            t = w.view(1, 1, Hw, 1) * smp.step(o[:, v], i, xv, torch.zeros_like(xv))
            acc[:, :, rows] = acc[:, :, rows] + t
            wsum[rows] = wsum[rows] + w
    r = acc / wsum.view(1, 1, H, 1)
    sig = smp.sigma(i)
    if sig > 0:
        r = r + torch.tensor(sig, dtype=torch.float32) * nz
    return r


def random_weights(Hw, seed=0):
    """a positive table with no structure: values in [0.05, 2)"""
    g = torch.Generator().manual_seed(1000 + seed)
    return (0.05 + 1.95 * torch.rand(Hw, generator=g)).numpy().astype(np.float32)


# ---- the taper ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hw,s", [(64, 40), (64, 64), (16, 3)])
def test_window_taper(Hw, s):
    w = window_taper(Hw, s)
    assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.shape == (Hw,)
    assert (w > 0).all() and (w <= 1).all() and np.isfinite(w).all()
    assert np.array_equal(w, w[::-1]), "symmetric"
    E = Hw - s
    if E == 0:
        assert np.array_equal(w, np.ones(Hw, dtype=np.float32))
        return
    y = np.arange(Hw, dtype=np.float64)
    exact = np.minimum(1.0, (y + 0.5) / E) * np.minimum(1.0, (Hw - y - 0.5) / E)
    assert np.abs(w - exact).max() <= 2.0 ** -22, "two divisions and a product in fp32: below 2 ulp of 1"
    assert w[0] == np.float32(0.5) / np.float32(E)
    # the same profile as the ring tile blend's (tests/test_loop_host.py), bit for bit
    assert np.array_equal(w, LP.ring_blend_weights(Hw, s).numpy())


def test_window_taper_values_and_refusals():
    w = window_taper(64, 40)                                   # E = 24: a ramp of 24 rows at either end, 16 rows of 1 between
    assert np.array_equal(w[24:40], np.ones(16, dtype=np.float32)) and w[23] == np.float32(23.5) / np.float32(24) and w[0] == np.float32(0.5) / np.float32(24)
    w = window_taper(16, 3)                                    # E = 13 > Hw / 2: both ramps bite in the middle rows
    assert w[7] == (np.float32(7.5) / np.float32(13)) * (np.float32(8.5) / np.float32(13)) and w.max() < 1
    assert w[2] == np.float32(2.5) / np.float32(13), "the falling ramp is still at 1 at row 2: (16 - 2 - 0.5) / 13 > 1"
    h = window_taper(64, 32)                                   # half overlap: two overlapping weights sum to 1
    assert np.array_equal(h[:32] + h[32:], np.ones(32, dtype=np.float32))
    for bad in ((16, 0), (16, 17), (0, 0), (16.5, 3)):
        with pytest.raises(ValueError):
            window_taper(*bad)


# ---- the weighted update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,pred,clip", LH.CASES)
@pytest.mark.parametrize("H,Hw,s", LINEAR)
def test_all_ones_is_the_unweighted_update_linear(H, Hw, s, rule, pred, clip):
    smp = LH.Sampler(rule, pred, clip)
    x, outs, nz = LH.window_inputs(2, H, Hw, s, seed=5)
    ones = np.ones(Hw, dtype=np.float32)
    for i in (0, LH.N_OP - 1):
        ref = LH.window_update(smp, i, x, outs[0], nz[0], Hw, s, guidance=3.0)
        got = weighted_window_update(smp, i, x, outs[0], nz[0], Hw, s, ones, guidance=3.0)
        assert torch.equal(got, ref), (rule, pred, i)


@pytest.mark.parametrize("rule,pred,clip", LH.CASES)
@pytest.mark.parametrize("H,Hw,s", LP.GEOMS)
def test_all_ones_is_the_unweighted_update_ring(H, Hw, s, rule, pred, clip):
    smp = LH.Sampler(rule, pred, clip)
    x, outs, nz = LP.ring_inputs(2, H, Hw, s, seed=6)
    ones = np.ones(Hw, dtype=np.float32)
    for i in (0, LH.N_OP - 1):
        ref = LP.ring_update(smp, i, x, outs[0], nz[0], Hw, s, guidance=3.0)
        got = weighted_window_update(smp, i, x, outs[0], nz[0], Hw, s, ones, guidance=3.0, ring=True)
        assert torch.equal(got, ref), (rule, pred, i)


@pytest.mark.parametrize("ring,H,Hw,s", [(False, 31, 16, 3), (False, 120, 64, 8), (True, 96, 64, 24), (True, 64, 64, 16)])
def test_the_weighted_update_is_a_convex_combination_and_differs_from_the_mean(ring, H, Hw, s):
    """sigma = 0: every canvas element lies between the smallest and the largest per-view result (to rounding), and the taper changes
    the result wherever two views overlap"""
    smp = LH.Sampler("ddim0", "v_prediction")
    x, outs, nz = (LP.ring_inputs if ring else LH.window_inputs)(2, H, Hw, s, cfg=False, seed=9)
    w = window_taper(Hw, s)
    got = weighted_window_update(smp, 1, x, outs[0], nz[0], Hw, s, w, ring=ring)
    ref = (LP.ring_update if ring else LH.window_update)(smp, 1, x, outs[0], nz[0], Hw, s)
    assert not torch.equal(got, ref)
    V = H // s if ring else (H - Hw) // s + 1
    lo, hi = torch.full_like(x, float("inf")), torch.full_like(x, float("-inf"))
    o = outs[0].view(2, V, 8, Hw, 16)
    for v in range(V):
        rows = LP.ring_rows(v, H, Hw, s) if ring else torch.arange(v * s, v * s + Hw)
        xv = x[:, :, rows]
        d = smp.step(o[:, v], 1, xv, torch.zeros_like(xv))
        lo[:, :, rows] = torch.minimum(lo[:, :, rows], d)
        hi[:, :, rows] = torch.maximum(hi[:, :, rows], d)
    tol = 8 * 2.0 ** -23 * max(lo.abs().max().item(), hi.abs().max().item())
    assert (got >= lo - tol).all() and (got <= hi + tol).all()


@pytest.mark.parametrize("H,Hw,s", LP.GEOMS[:3])
def test_the_weighted_ring_update_commutes_with_a_rotation_by_one_stride(H, Hw, s):
    smp = LH.Sampler("ddpm", "v_prediction")
    x, outs, nz = LP.ring_inputs(2, H, Hw, s, seed=17)
    V, w = H // s, window_taper(Hw, s)
    ref = weighted_window_update(smp, 1, x, outs[0], nz[0], Hw, s, w, guidance=3.0, ring=True)
    got = weighted_window_update(smp, 1, x.roll(s, 2), LP.roll_views(outs[0], 4, V), nz[0].roll(s, 2), Hw, s, w, guidance=3.0, ring=True)
    assert torch.equal(got, ref.roll(s, 2))


# ---- windows to segments ------------------------------------------------------------------------------------------------------------------
def test_timeline_geometry_assignments():
    seg = [("rain", 0), ("thunder rolls in", 12.5), ("birds after the storm", 22)]
    # 30 s / 10 / 5: H 768, Hw 256, s 128, V 5; centres at rows 128, 256, 384, 512, 640; the segments start at rows 0, 320, round(563.2) = 563
    assert timeline_geometry(seg, 30, 10, 5) == (768, 256, 128, 5, [0, 0, 1, 1, 2])
    assert timeline_geometry(seg, 30) == (768, 256, 128, 5, [0, 0, 1, 1, 2])
    assert timeline_geometry([("rain", 0)], 30, 10, 5) == (768, 256, 128, 5, [0] * 5)
    # a centre row belongs to the segment that starts on it: 15 s is row 384
    assert timeline_geometry([("a", 0), ("b", 15)], 30, 10, 5)[4] == [0, 0, 1, 1, 1]
    assert timeline_geometry([("a", 0), ("b", 15.04)], 30, 10, 5)[4] == [0, 0, 0, 1, 1]      # round(385.02) = 385: one row past the centre
    # a 20 s loop: H 512, V 4, centres at rows 128, 256, 384 and 512 mod 512 = 0: the last window's centre wraps into the first segment
    assert timeline_geometry([("a", 0), ("b", 10)], 20, 10, 5, loop=True) == (512, 256, 128, 4, [0, 1, 1, 0])
    assert timeline_geometry([("a", 0), ("b", 2), ("c", 12)], 20, 10, 5, loop=True)[4] == [1, 1, 2, 0]   # rows 0, 51, 307
    # a linear clip of the same length has no wrapped centre: 20 s / 10 / 5 has centres 128, 256, 384
    assert timeline_geometry([("a", 0), ("b", 10)], 20, 10, 5) == (512, 256, 128, 3, [0, 1, 1])


def test_timeline_geometry_refusals():
    with pytest.raises(ValueError, match=r"ascend: segment 1 starts at 20 s, segment 2 at 12\.5 s"):
        timeline_geometry([("a", 0), ("b", 20), ("c", 12.5)], 30)
    with pytest.raises(ValueError, match="ascend"):
        timeline_geometry([("a", 0), ("b", 10), ("c", 10)], 30)
    with pytest.raises(ValueError, match=r"first segment must start at 0 s, got 2\.5 s"):
        timeline_geometry([("a", 2.5), ("b", 10)], 30)
    with pytest.raises(ValueError, match="segment 1 starts at 30 s, at or beyond the duration of 30 s"):
        timeline_geometry([("a", 0), ("b", 30)], 30)
    with pytest.raises(ValueError, match="segment 1 starts at 41 s, at or beyond the duration of 30 s"):
        timeline_geometry([("a", 0), ("b", 41)], 30)
    # rows 0, 282, 358: segment 1 lies between the centres at rows 256 (10 s) and 384 (15 s); the nearest to its start is 10 s
    with pytest.raises(ValueError, match=r"segment 1 \(rows 282 to 358, .*holds no window centre.*every 5 s from 5 s.*nearest is at 10 s \(row 256\)"):
        timeline_geometry([("a", 0), ("b", 11), ("c", 14)], 30)
    # the first segment ends before the first centre (row 128, 5 s)
    with pytest.raises(ValueError, match=r"segment 0 \(rows 0 to 102, .*holds no window centre.*nearest is at 5 s \(row 128\)"):
        timeline_geometry([("a", 0), ("b", 4)], 30)
    # on a linear clip the last 5 s hold no centre (the last is at 25 s); on a ring of 30 s (V = 6) the centre of window 5 is at row 0
    with pytest.raises(ValueError, match=r"segment 1 \(rows 691 to 768, .*holds no window centre.*nearest is at 25 s \(row 640\)"):
        timeline_geometry([("a", 0), ("b", 27)], 30)
    # the geometry's own refusals come through
    with pytest.raises(ValueError, match="30 and 35"):
        timeline_geometry([("a", 0)], 33)
    with pytest.raises(ValueError, match="overlapping windows"):
        timeline_geometry([("a", 0)], 20, 10, 10, loop=True)
    for bad in ([], [("a", "soon")], [("a",)], "rain"):
        with pytest.raises(ValueError):
            timeline_geometry(bad, 30)


# ---- the engine's refusals, without a GPU -------------------------------------------------------------------------------------------------
def _check(lib, ring, weights="taper", H=128, Hw=64, s=32, steps=2, batch=1, **fields):
    a = _lib.DenoiseArgs()
    a.num_steps, a.batch, a.guidance_scale, a.latent_h = steps, batch, 3.0, H
    for k, v in fields.items():
        setattr(a, k, v)
    w = _lib.WindowArgs(window_h=Hw, stride=s)
    if isinstance(weights, str):
        weights = window_taper(Hw, s) if Hw > 0 and 1 <= s <= Hw else np.ones(max(Hw, 1), dtype=np.float32)
    fn = lib.tango_debug_denoise_ring_weighted_check if ring else lib.tango_debug_denoise_windows_weighted_check
    return fn(C.byref(a), C.byref(w), C.c_void_p(weights.ctypes.data) if weights is not None else None).decode()


@pytest.mark.parametrize("ring", [False, True])
def test_weighted_refusals(lib, ring):
    pre = "denoise_ring_weighted: " if ring else "denoise_windows_weighted: "
    how = "on a ring" if ring else "with windows"
    assert _check(lib, ring) == "" and _check(lib, ring, rule=1) == ""
    assert _check(lib, ring, weights=random_weights(64)) == "", "the engine takes any positive table"
    assert _check(lib, ring, H=64, Hw=64, s=64) == "", "one view"
    assert _check(lib, ring, weights=None).startswith(pre + "view_weights must not be NULL")
    for bad, what in ((0.0, "zero"), (-1.0, "negative"), (float("nan"), "NaN"), (float("inf"), "inf")):
        for at in (0, 37, 63):
            t = window_taper(64, 32)
            t[at] = bad
            assert _check(lib, ring, weights=t).startswith(pre + "view_weights entries must be finite and > 0 at "), (what, at)
    # whatever the unweighted call refuses, with its message under the new prefix
    p = np.zeros(8, dtype=np.float32).ctypes.data
    known = dict(known_latents=p, latent_mask=p, blend_coef=p)
    ms = ("the multistep rule is not supported on a ring: use DDPM or DDIM" if ring else
          "the multistep rule is not supported with windows (a per-view history has no reference behaviour): use DDPM or DDIM")
    assert _check(lib, ring, rule=2, coef_width=16).startswith(pre + ms + " at ")
    assert _check(lib, ring, rule=2).startswith(pre + ms + " at ")
    assert _check(lib, ring, **known).startswith(pre + "known_latents (masked-latent inpainting) is not supported " + how + " at ")
    assert _check(lib, ring, steps=0).startswith(pre + "num_steps must be positive at ")
    assert _check(lib, ring, rule=7).startswith(pre + "unknown rule at ")
    assert _check(lib, ring, H=0).startswith(pre + ("a ring call" if ring else "a windowed call") + " states its canvas height (latent_h > 0) at ")
    assert _check(lib, ring, s=0).startswith(pre + "stride must be in [1, window_h] at ")
    assert _check(lib, ring, H=60, Hw=60, s=4).startswith(pre + "window_h is not a UNet height at ")
    assert (pre + ("the ring's height must be a multiple of stride" if ring else "the windows must cover the canvas exactly")) in _check(lib, ring, H=100)
    # the unweighted refusals win over the table's
    assert "multistep rule" in _check(lib, ring, rule=2, weights=None) and "known_latents" in _check(lib, ring, weights=None, **known)
    fn = lib.tango_debug_denoise_ring_weighted_check if ring else lib.tango_debug_denoise_windows_weighted_check
    assert fn(None, None, None).decode() == pre + "null args"
    # the unweighted checks keep their own prefix
    assert LP._rcheck(lib, rule=2).startswith("denoise_ring: ") and LH._wcheck(lib, rule=2).startswith("denoise_windows: ")


def test_python_refusals_before_any_engine_call():
    m = LH._bare_model()
    pe, pm = torch.zeros(4, 4, 8), torch.ones(4, 4, dtype=torch.bool)
    ddpm = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in LH._DDPM_KEYS})
    dpm = DPMSolverMultistepScheduler(**LH.SD21, solver_order=2, algorithm_type="dpmsolver++")
    wp = [0, 0, 1, 1, 1]
    seg = [("rain", 0), ("thunder", 15)]
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported with windows"):
        m.inference_timeline_from_embeddings(pe, pm, wp, dpm, 4, 3.0, duration=30)
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported on a ring"):
        m.inference_timeline_from_embeddings(pe, pm, [0, 1, 1, 0], dpm, 4, 3.0, duration=20, loop=True)
    with pytest.raises(ValueError, match="guidance table is not supported with windows"):
        m.inference_timeline_from_embeddings(pe, pm, wp, ddpm, 4, [3.0], duration=30)
    with pytest.raises(ValueError, match="guidance table is not supported on a ring"):
        m.inference_timeline_from_embeddings(pe, pm, [0, 1, 1, 0], ddpm, 4, [3.0], duration=20, loop=True)
    with pytest.raises(ValueError, match="30 and 35"):
        m.inference_timeline_from_embeddings(pe, pm, wp, ddpm, 4, 3.0, duration=33)
    with pytest.raises(ValueError, match="window_prompt must hold 5 segment indices below 2"):
        m.inference_timeline_from_embeddings(pe, pm, [0, 1], ddpm, 4, 3.0, duration=30)
    with pytest.raises(ValueError, match="window_prompt must hold 5 segment indices below 2"):
        m.inference_timeline_from_embeddings(pe, pm, [0, 0, 1, 1, 2], ddpm, 4, 3.0, duration=30)
    with pytest.raises(ValueError, match="30 and 35"):
        m.inference_timeline(seg, ddpm, 4, 3.0, duration=33)
    with pytest.raises(ValueError, match="holds no window centre"):
        m.inference_timeline([("rain", 0), ("thunder", 4)], ddpm, 4, 3.0, duration=30)
    t = Tango.__new__(Tango)
    t.scheduler = dpm
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported with windows"):
        t.generate_timeline(seg, 30)
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported on a ring"):
        t.generate_timeline(seg, 30, loop=True)
    t.scheduler = ddpm
    with pytest.raises(ValueError, match="guidance table is not supported with windows"):
        t.generate_timeline(seg, 30, guidance=[3.0])
    with pytest.raises(ValueError, match="guidance table is not supported on a ring"):
        t.generate_timeline(seg, 30, guidance=[3.0], loop=True)
    with pytest.raises(ValueError, match="does not exceed the window"):
        t.generate_timeline([("rain", 0)], 10)
    with pytest.raises(ValueError, match="ascend"):
        t.generate_timeline([("rain", 0), ("a", 20), ("b", 10)], 30)
    with pytest.raises(ValueError, match="at or beyond the duration"):
        t.generate_timeline([("rain", 0), ("a", 30)], 30, loop=True)


def test_abi(lib):
    names = ("tango_engine_denoise_windows_weighted", "tango_engine_denoise_ring_weighted", "tango_debug_denoise_windows_weighted_check",
             "tango_debug_denoise_ring_weighted_check", "tango_op_sched_windows_weighted", "tango_op_sched_ring_weighted")
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tango_engine.h")).read()
    for s in names:
        assert hasattr(lib, s) and s in _lib.SYMBOLS and s in header
    assert _lib.DenoiseArgs._fields_[-1][0] == "latent_h" and len(_lib.DenoiseArgs._fields_) == 30, "tango_denoise_args_t stays frozen"
    assert [f[0] for f in _lib.WindowArgs._fields_] == ["window_h", "stride"] and C.sizeof(_lib.WindowArgs) == 8
    from tango_amd.engine import Engine
    from tango_amd.models import AudioDiffusion
    for fn, kws in ((Engine.denoise_windows, ("view_weights",)), (Engine.denoise_ring, ("kw",)),
                    (Tango.generate_timeline, ("segments", "duration", "steps", "guidance", "samples", "window", "hop", "loop", "taper",
                                               "negative_prompt", "seed")),
                    (AudioDiffusion.inference_timeline, ("segments", "duration", "window", "hop", "loop", "taper", "negative_prompt")),
                    (AudioDiffusion.inference_timeline_from_embeddings, ("prompt_embeds", "boolean_prompt_mask", "window_prompt", "taper"))):
        assert all(k in inspect.signature(fn).parameters for k in kws), fn
    sig = inspect.signature(Tango.generate_timeline).parameters
    assert (sig["window"].default, sig["hop"].default, sig["loop"].default, sig["taper"].default) == (10, 5, False, True)
    assert inspect.signature(Engine.denoise_windows).parameters["view_weights"].default is None
