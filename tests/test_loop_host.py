"""Seamless loops (MultiDiffusion windows on a ring in time): everything that needs no GPU -- the geometry helper, the ring cover's closed
form against its brute-force definition, the torch restatements of the ring update and of the ring tile blend that
tests/test_loop_gpu.py compares the kernels with, the engine's argument checks through tango_debug_denoise_ring_check, the Python
refusals that fire before any engine call, and the C ABI.  The restatements stand on tests/test_long_host.py's Sampler: the per-view
step arithmetic that the existing bit-exact tests pin."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import test_long_host as LH
from tango_amd import _lib
from tango_amd.inpaint import loop_geometry
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler, DPMSolverMultistepScheduler
from tango_amd.tango import Tango

#: (H, Hw, s): counts 2 / 3 mixed (s does not divide Hw); H == Hw, 4 rotated views of the whole ring; 2 everywhere; one view, no wrap
GEOMS = [(96, 64, 24), (64, 64, 16), (128, 64, 32), (64, 64, 64)]
COUNTS = {(96, 64, 24): [2, 3], (64, 64, 16): [4], (128, 64, 32): [2], (64, 64, 64): [1]}


# ---- the restatements -------------------------------------------------------------------------------------------------------------------
def ring_cover(h, H, Hw, s):
    """the closed form of common.h: [(v_k, y_k)] for k = 0 .. n - 1, v_k = (h / s - k) mod V, y_k = h % s + k s, n = ceil((Hw - h % s) / s)"""
    V, q, r = H // s, h // s, h % s
    n = -(-(Hw - r) // s)
    return [((q - k) % V, r + k * s) for k in range(n)]


def ring_rows(v, H, Hw, s):
    """the canvas rows of view v, in the view's own order"""
    return (v * s + torch.arange(Hw)) % H


def _ring_accumulate(H, Hw, s, add):
    """walks the cover in accumulation order, k descending: add(k, v, canvas rows, local rows) for every view v and its block
    y in [k s, min((k + 1) s, Hw)), which lands on canvas rows ((v + k) mod V) s + (y - k s).  For one k the blocks of different views
    are disjoint, so per canvas row the order is k = n - 1, ..., 0: the view that starts farthest below the row first."""
    V = H // s
    for k in reversed(range(-(-Hw // s))):
        for v in range(V):
            y = torch.arange(k * s, min((k + 1) * s, Hw))
            add(k, v, ((v + k) % V) * s + (y - k * s), y)


def ring_update(smp, i, x, outs, nz, Hw, s, guidance=None):
    """the ring update at loop index i.  x [B, C, H, W] the ring; outs [B2 * V, C, Hw, W] the model outputs in the window batch's order
    (row half * B * V + b * V + v); nz [B, C, H, W] one draw per canvas element.  Per view d_v = the step's result before its noise term
    on the view's rows (v s + y) mod H; per canvas row acc = 0 + d_.. + d_.. in the cover order; r = acc / n; r + sigma * nz when sigma > 0."""
    B, Cc, H, W = x.shape
    V = H // s
    assert H % s == 0 and 1 <= s <= Hw <= H
    if guidance is not None:
        u, c = outs.chunk(2)
        outs = u + guidance * (c - u)                          # models.py:246
    o = outs.view(B, V, Cc, Hw, W)
    d = []
    for v in range(V):
        xv = x[:, :, ring_rows(v, H, Hw, s)]
        d.append(smp.step(o[:, v], i, xv, torch.zeros_like(xv)))
    acc = torch.zeros_like(x)
    cnt = torch.zeros(H, dtype=torch.float32)

    def add(k, v, rows, y):
        acc[:, :, rows] = acc[:, :, rows] + d[v][:, :, y]
        cnt[rows] += 1

    _ring_accumulate(H, Hw, s, add)
    r = acc / cnt.view(1, 1, H, 1)
    sig = smp.sigma(i)
    if sig > 0:
        r = r + torch.tensor(sig, dtype=torch.float32) * nz
    return r


def ring_inputs(B, H, Hw, s, W=16, cfg=True, seed=0, steps=2):
    """a ring, `steps` model outputs of the window batch and `steps` canvas noises"""
    g = torch.Generator().manual_seed(seed)
    V = H // s
    x = torch.randn(B, 8, H, W, generator=g)
    outs = [torch.randn((2 if cfg else 1) * B * V, 8, Hw, W, generator=g) for _ in range(steps)]
    nz = torch.randn(steps, B, 8, H, W, generator=g)
    return x, outs, nz


def ring_blend_weights(Hw4, s4):
    """the weight of a tile at its local rows, fp32 in the kernel's evaluation order: both ramps on every tile"""
    E = Hw4 - s4
    one = torch.ones(Hw4)
    if E <= 0:
        return one
    y, e = torch.arange(Hw4, dtype=torch.float32), torch.full((Hw4,), float(E))            # tensor / tensor: a true division
    return torch.minimum(one, (y + 0.5) / e) * torch.minimum(one, ((Hw4 - y) - 0.5) / e)


def torch_ring_blend(tiles, B, V, Hw4, s4):
    """tango_op_mel_ring_blend in the kernel's evaluation order: per ring row the covering tiles in the cover order,
    num = 0 + w tile + ..., den = 0 + w + ..., num / den.  tiles [B * V, 1, Hw4, F] -> [B, 1, V s4, F]"""
    F, H4 = tiles.shape[-1], V * s4
    t4 = tiles.view(B, V, Hw4, F)
    w = ring_blend_weights(Hw4, s4)
    num, den = torch.zeros(B, H4, F), torch.zeros(H4, 1)

    def add(k, t, rows, y):
        num[:, rows] = num[:, rows] + w[y].view(1, -1, 1) * t4[:, t, y]
        den[rows] = den[rows] + w[y].view(-1, 1)

    _ring_accumulate(H4, Hw4, s4, add)
    return (num / den).view(B, 1, H4, F)


# ---- the cover ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hw,s", GEOMS + [(40, 16, 8), (21, 7, 3), (16, 16, 1)])
def test_ring_cover_closed_form_is_the_brute_force_definition(H, Hw, s):
    V = H // s
    counts = set()
    for h in range(H):
        brute = {(v, y) for v in range(V) for y in range(Hw) if (v * s + y) % H == h}
        closed = ring_cover(h, H, Hw, s)
        assert len(closed) == len(set(closed)) and set(closed) == brute, (h, closed, sorted(brute))
        assert [y for _, y in closed] == sorted(y for _, y in closed), "k ascending is local row ascending: k descending starts farthest below h"
        counts.add(len(closed))
    if (H, Hw, s) in COUNTS:
        assert sorted(counts) == COUNTS[(H, Hw, s)]
    # the accumulation walk of the restatements visits every row's cover in descending k
    seen = {h: [] for h in range(H)}
    _ring_accumulate(H, Hw, s, lambda k, v, rows, y: [seen[int(h)].append((v, int(yy))) for h, yy in zip(rows, y)])
    for h in range(H):
        assert seen[h] == ring_cover(h, H, Hw, s)[::-1], h


def test_rows_no_view_wraps_over_are_accumulated_in_ascending_view_order():
    """for a row whose covering views all start at or below it on the segment, the order is sched_window_kernel's ascending v"""
    H, Hw, s = 96, 64, 24
    for h in range(H):
        order = [v for v, _ in ring_cover(h, H, Hw, s)[::-1]]
        if all(v * s <= h for v in order):
            assert order == sorted(order) == LH.cover(h, Hw, s, H // s), h
    assert [v for v, _ in ring_cover(0, H, Hw, s)[::-1]] == [2, 3, 0], "the wrap point: views 2 and 3 wrap over row 0, then view 0 starts there"


# ---- the update ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,pred,clip", LH.CASES)
def test_one_view_is_the_plain_step_bit_for_bit(rule, pred, clip):
    """H == Hw == s: one view that does not wrap; (0 + d) / 1 is exact"""
    smp = LH.Sampler(rule, pred, clip)
    x, outs, nz = ring_inputs(2, 16, 16, 16, seed=3)
    for i in (0, LH.N_OP - 1):
        u, c = outs[0].chunk(2)
        ref = smp.step(u + 3.0 * (c - u), i, x, nz[0])
        got = ring_update(smp, i, x, outs[0], nz[0], 16, 16, guidance=3.0)
        assert torch.equal(got, ref), (rule, pred, i)


def roll_views(outs, B2, V, shift=1):
    """the window batch after a rotation of the ring by `shift` strides: view v holds what view v - shift held"""
    return outs.view(B2, V, *outs.shape[1:]).roll(shift, 1).reshape(outs.shape).contiguous()


@pytest.mark.parametrize("H,Hw,s", GEOMS[:3])
def test_the_update_commutes_with_a_rotation_by_one_stride(H, Hw, s):
    smp = LH.Sampler("ddpm", "v_prediction")
    x, outs, nz = ring_inputs(2, H, Hw, s, seed=17)
    V = H // s
    ref = ring_update(smp, 1, x, outs[0], nz[0], Hw, s, guidance=3.0)
    got = ring_update(smp, 1, x.roll(s, 2), roll_views(outs[0], 4, V), nz[0].roll(s, 2), Hw, s, guidance=3.0)
    assert torch.equal(got, ref.roll(s, 2)) and not torch.equal(ref, x)


# ---- the blend ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hw4,s4,V", [(64, 32, 2), (64, 16, 4), (64, 24, 4), (64, 64, 1)])
def test_ring_blend_restatement(Hw4, s4, V):
    """tiles sliced from one ring mel give it back (a weighted mean of equal values), and the blend commutes with a rotation by one stride"""
    B, F, H4 = 2, 8, V * s4
    g = torch.Generator().manual_seed(Hw4 + s4)
    mel = torch.randn(B, 1, H4, F, generator=g) * 3.0 - 4.0
    sl = torch.stack([mel[:, :, ring_rows(t, H4, Hw4, s4)] for t in range(V)], 1).reshape(B * V, 1, Hw4, F)
    out = torch_ring_blend(sl.contiguous(), B, V, Hw4, s4)
    assert (out - mel).abs().max().item() <= 16 * 2.0 ** -23 * mel.abs().max().item()
    tiles = torch.randn(B * V, 1, Hw4, F, generator=g)
    a = torch_ring_blend(tiles, B, V, Hw4, s4)
    b = torch_ring_blend(roll_views(tiles, B, V), B, V, Hw4, s4)
    assert torch.equal(b, a.roll(s4, 2))
    if s4 == Hw4:
        assert torch.equal(out, mel)


def test_ring_blend_half_overlap_weights_sum_to_one():
    """s4 == Hw4 / 2: at every ring row the two weights are (y + 0.5) / E and 1 - (y + 0.5) / E, in fp32 too"""
    Hw4, s4 = 64, 32
    w = ring_blend_weights(Hw4, s4)
    assert torch.equal(w[:s4] + w[s4:], torch.ones(s4))
    w64 = ring_blend_weights(64, 24)                          # E = 40 > Hw4 / 2: both ramps bite in the middle rows
    assert w64[30] < 1 and torch.equal(w64, w64.flip(0))


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
def test_loop_geometry():
    assert loop_geometry(2.5) == (64, 64, 32, 2)
    assert loop_geometry(5) == (128, 128, 64, 2)
    assert loop_geometry(10) == (256, 256, 128, 2)
    assert loop_geometry(20) == (512, 256, 128, 4)                                     # past 10 s the window is 10 s
    assert loop_geometry(30) == (768, 256, 128, 6)
    assert loop_geometry(30, window=10) == (768, 256, 128, 6)
    assert loop_geometry(32.5, window=10, hop=2.5) == (832, 256, 64, 13)
    assert loop_geometry(10, window=10, hop=0.3125) == (256, 256, 8, 32)               # the smallest stride, the most windows
    assert loop_geometry(160) == (4096, 256, 128, 32)
    assert loop_geometry(10, window=5) == (256, 128, 64, 4)
    assert loop_geometry(10, hop=2.5) == (256, 256, 64, 4)
    with pytest.raises(ValueError, match="30 and 35"):
        loop_geometry(31)                                      # H % s != 0
    with pytest.raises(ValueError, match="10 and 15"):
        loop_geometry(12.5)
    with pytest.raises(ValueError, match="30 and 35"):
        loop_geometry(30.01)                                   # a fractional row
    with pytest.raises(ValueError, match="10 and 15"):
        loop_geometry(10.02, window=10)                        # below the first neighbour pair: the pair at the window
    with pytest.raises(ValueError, match="shorter than the window"):
        loop_geometry(5, window=10)
    with pytest.raises(ValueError, match="shorter than the window"):
        loop_geometry(7)                                       # off the grid: the window defaults to 10 s
    with pytest.raises(ValueError, match="overlapping windows"):
        loop_geometry(20, window=10, hop=10)
    with pytest.raises(ValueError, match="overlapping windows"):
        loop_geometry(20, window=5, hop=10)
    with pytest.raises(ValueError, match="multiple of 8"):
        loop_geometry(30, hop=4.9)
    with pytest.raises(ValueError, match="multiple of 8"):
        loop_geometry(30, hop=0)
    with pytest.raises(ValueError, match="at most 32"):
        loop_geometry(165)
    with pytest.raises(ValueError, match="at most 32"):
        loop_geometry(10.3125, window=10, hop=0.3125)
    with pytest.raises(ValueError, match="grid"):
        loop_geometry(30, window=11)
    for bad in (float("nan"), float("inf"), "loop"):
        with pytest.raises(ValueError):
            loop_geometry(bad)


# ---- the engine's refusals, without a GPU -------------------------------------------------------------------------------------------------
def _rcheck(lib, H=128, Hw=64, s=32, steps=2, batch=1, **fields):
    a = _lib.DenoiseArgs()
    a.num_steps, a.batch, a.guidance_scale, a.latent_h = steps, batch, 3.0, H
    for k, v in fields.items():
        setattr(a, k, v)
    w = _lib.WindowArgs(window_h=Hw, stride=s)
    return lib.tango_debug_denoise_ring_check(C.byref(a), C.byref(w)).decode()


def test_ring_refusals_and_their_order(lib):
    for H, Hw, s in GEOMS:
        assert _rcheck(lib, H=H, Hw=Hw, s=s) == "" and _rcheck(lib, H=H, Hw=Hw, s=s, rule=1) == ""
    assert _rcheck(lib, H=256, Hw=64, s=8) == "", "32 views"
    p = np.zeros(8, dtype=np.float32).ctypes.data
    known = dict(known_latents=p, latent_mask=p, blend_coef=p)
    # one message each, every one under the caller's prefix
    msgs = [
        ("the multistep rule is not supported on a ring: use DDPM or DDIM", dict(rule=2, coef_width=16)),
        ("num_steps must be positive", dict(steps=0)),
        ("known_latents (masked-latent inpainting) is not supported on a ring", known),
        ("a ring call states its canvas height (latent_h > 0)", dict(H=0)),
        ("the ring must be at least window_h rows long", dict(H=32)),
        ("the ring's height must be a multiple of stride", dict(H=100)),
        ("stride must be in [1, window_h]", dict(s=0)),
        ("at most 32 windows per ring", dict(H=264, s=8)),
        ("window_h is not a UNet height", dict(H=60, Hw=60, s=4)),
    ]
    for m, f in msgs:
        assert _rcheck(lib, **f).startswith("denoise_ring: " + m + " at "), (m, _rcheck(lib, **f))      # (then the source line)
    assert "stride must be in [1, window_h]" in _rcheck(lib, H=130, s=65) and "stride must be in" in _rcheck(lib, s=-3)
    assert "window_h must be positive" in _rcheck(lib, Hw=0)
    # the order: each refusal wins over every later one
    assert "multistep rule" in _rcheck(lib, rule=2, steps=0, H=0, **known)                      # 1 before 2, 3, 5
    assert "multistep rule" in _rcheck(lib, rule=2)                                             # ... whatever its table looks like
    assert "num_steps must be positive" in _rcheck(lib, steps=0, H=0, **known)                  # 2 before 3, 5
    assert "unknown rule" in _rcheck(lib, rule=7, H=100) and "8-float coefficient rows" in _rcheck(lib, coef_width=16, H=0)
    assert "known_latents" in _rcheck(lib, H=0, **known) and "known_latents" in _rcheck(lib, H=100, **known)   # 3 before 5, 6
    assert "states its canvas height" in _rcheck(lib, H=0, s=0) and "states its canvas height" in _rcheck(lib, H=-5, Hw=60)   # 5 before 6
    assert "at least window_h" in _rcheck(lib, H=40, s=24)                                      # H < Hw before H % s
    assert "multiple of stride" in _rcheck(lib, H=100, s=65)                                    # H % s before the range of s
    assert "multiple of stride" in _rcheck(lib, H=257, s=8)                                     # ... and before V > 32
    assert "stride must be in" in _rcheck(lib, H=130, Hw=60, s=65)                              # the range of s before the UNet height
    assert "at most 32 windows" in _rcheck(lib, H=264, Hw=60, s=8)                              # V > 32 before the UNet height
    assert lib.tango_debug_denoise_ring_check(None, None).decode() == "denoise_ring: null args"
    a, w = _lib.DenoiseArgs(), _lib.WindowArgs()
    assert lib.tango_debug_denoise_ring_check(C.byref(a), None).decode() == "denoise_ring: null args"
    assert lib.tango_debug_denoise_ring_check(None, C.byref(w)).decode() == "denoise_ring: null args"
    # the linear call keeps its own messages
    assert "with windows" in LH._wcheck(lib, rule=2) and "cover the canvas exactly" in LH._wcheck(lib, H=100)


def test_python_refusals_before_any_engine_call():
    m = LH._bare_model()
    pe, pm = torch.zeros(2, 4, 8), torch.ones(2, 4, dtype=torch.bool)
    ddpm = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in LH._DDPM_KEYS})
    dpm = DPMSolverMultistepScheduler(**LH.SD21, solver_order=2, algorithm_type="dpmsolver++")
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported on a ring"):
        m.inference_loop_from_embeddings(pe, pm, dpm, 4, 3.0, duration=10)
    with pytest.raises(ValueError, match="guidance table is not supported on a ring"):
        m.inference_loop_from_embeddings(pe, pm, ddpm, 4, [3.0], duration=10)
    with pytest.raises(ValueError, match="30 and 35"):
        m.inference_loop_from_embeddings(pe, pm, ddpm, 4, 3.0, duration=33)
    with pytest.raises(ValueError, match="30 and 35"):
        m.inference_loop(["rain"], ddpm, 4, 3.0, duration=33)
    with pytest.raises(ValueError, match="overlapping windows"):
        m.inference_loop(["rain"], ddpm, 4, 3.0, duration=10, hop=10)
    t = Tango.__new__(Tango)
    t.scheduler = dpm
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported on a ring"):
        t.generate_loop("rain", 10)
    t.scheduler = ddpm
    with pytest.raises(ValueError, match="shorter than the window"):
        t.generate_loop("rain", 5, window=10)
    with pytest.raises(ValueError, match="guidance table is not supported on a ring"):
        t.generate_loop("rain", 10, guidance=[3.0])
    with pytest.raises(ValueError, match="at most 32"):
        t.generate_loop("rain", 165)


def test_abi(lib):
    assert _lib.DenoiseArgs._fields_[-1][0] == "latent_h" and len(_lib.DenoiseArgs._fields_) == 30, "tango_denoise_args_t stays frozen"
    assert [f[0] for f in _lib.WindowArgs._fields_] == ["window_h", "stride"] and C.sizeof(_lib.WindowArgs) == 8
    names = ("tango_engine_denoise_ring", "tango_debug_denoise_ring_check", "tango_engine_vae_decode_ring_h", "tango_engine_vocode_ring",
             "tango_engine_vocoder_ring_context", "tango_op_sched_ring", "tango_op_mel_ring_blend", "tango_op_mel_ring_pad")
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "tango_engine.h")).read()
    for s in names:
        assert hasattr(lib, s) and s in _lib.SYMBOLS and s in header
    from tango_amd.engine import Engine
    from tango_amd.models import AudioDiffusion
    for fn, kws in ((Engine.denoise_ring, ("window_h", "stride")), (Engine.vae_decode_ring, ("window_h", "stride")), (Engine.vocode_ring, ("mel",)),
                    (Tango.generate_loop, ("duration", "steps", "guidance", "samples", "window", "hop", "negative_prompt", "seed")),
                    (AudioDiffusion.inference_loop, ("duration", "window", "hop")),
                    (AudioDiffusion.inference_loop_from_embeddings, ("duration", "window", "hop"))):
        assert all(k in inspect.signature(fn).parameters for k in kws), fn
    assert lib.tango_engine_vocoder_ring_context(None) == -1
