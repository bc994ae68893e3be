"""Seamless loops on the GPU (MultiDiffusion windows on a ring in time): the ring update through tango_op_sched_ring, bit for bit against
the torch restatement of tests/test_loop_host.py and under a rotation of the ring; Engine.denoise_ring against Engine.denoise (one view),
against a loop composed from the oracle's UNet and scheduler steps per rolled view, under a rotation, and between plain and windowed
calls of the same plan; the ring tile blend and the ring VAE decode; the vocoder on a ring; Tango.generate_loop against the
hand-composed chain."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_duration_gpu as TD  # noqa: E402  (LOOP_TOL, the VAE engines and state dict, the synthetic Tango stack with a tokenizer)
import test_inpaint_gpu as TI  # noqa: E402  (shared tiny-UNet engines and their state dict)
import test_long_gpu as LG  # noqa: E402  (the plain and windowed runners, _ulp, the Philox hook)
import test_long_host as LH  # noqa: E402  (Sampler, CASES)
import test_loop_host as RH  # noqa: E402  (the restatements of the ring update and of the ring blend)
from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.inpaint import loop_geometry  # noqa: E402

vp, hp = LG.vp, LG.hp
_cache = {}


# ---- 1. the op, bit for bit ---------------------------------------------------------------------------------------------------------------
def _op(lib, smp, lat, out, noise, i, H, Hw, s, seed=0, offset=0, cfg=1):
    B, Cc, W = lat.shape[0], lat.shape[1], lat.shape[3]
    rc = lib.tango_op_sched_ring(vp(lat), vp(out), vp(noise), hp(smp.coef[i]), B, Cc, H, W, Hw, s, cfg, 3.0, LG.PRED[smp.sch.config.prediction_type],
                                 LG.RULE[smp.engine_rule], 1 if smp.sch.config.clip_sample else 0, 1.0, seed, offset, i, None)
    assert rc == 0, lib.tango_last_error().decode()


@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("H,Hw,s", RH.GEOMS)
@pytest.mark.parametrize("rule,pred,clip", LH.CASES)
def test_op_ring_bitwise(lib, rule, pred, clip, H, Hw, s, cfg):
    """B = 2, C = 8, W = 16, two consecutive steps with injected canvas noise: torch.equal to the restatement"""
    smp = LH.Sampler(rule, pred, clip)
    x, outs, nz = RH.ring_inputs(2, H, Hw, s, cfg=cfg, seed=200 + H + s)
    lat = x.clone().cuda()
    ref = x
    for i in (0, 1):
        _op(lib, smp, lat, outs[i].cuda(), nz[i].contiguous().cuda(), i, H, Hw, s, cfg=1 if cfg else 0)
        ref = RH.ring_update(smp, i, ref, outs[i], nz[i], Hw, s, guidance=3.0 if cfg else None)
        assert torch.equal(lat.cpu(), ref), (rule, pred, i, (lat.cpu() - ref).abs().max().item())
    assert not torch.equal(ref, x)


@pytest.mark.parametrize("H,Hw,s", RH.GEOMS)
def test_op_ring_philox_draws_one_value_per_canvas_element(lib, H, Hw, s):
    """noise NULL: the draws are tango_op_philox_normal's on the CANVAS shape, whichever views cover the element"""
    smp = LH.Sampler("ddpm", "v_prediction")
    x, outs, _ = RH.ring_inputs(2, H, Hw, s, seed=7)
    lat = x.clone().cuda()
    _op(lib, smp, lat, outs[0].cuda(), None, 1, H, Hw, s, seed=1234567, offset=5)
    nz = LG._philox(lib, 2, H * 16, 1, 1234567, 5).view(2, 8, H, 16)
    assert smp.sigma(1) > 0
    assert torch.equal(lat.cpu(), RH.ring_update(smp, 1, x, outs[0], nz, Hw, s, guidance=3.0))


# ---- 2. rotation, at the hook -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hw,s", [(96, 64, 24), (64, 64, 16)])
def test_op_ring_commutes_with_a_rotation_by_one_stride(lib, H, Hw, s):
    """the canvas, the noise and the views' eps rows rolled by one stride give the rolled result, bit for bit: the wrap point is no special row"""
    V = H // s
    for rule, pred in (("ddpm", "v_prediction"), ("ddim1", "sample"), ("ddim0", "epsilon")):
        smp = LH.Sampler(rule, pred)
        x, outs, nz = RH.ring_inputs(2, H, Hw, s, seed=31)
        a = x.clone().cuda()
        _op(lib, smp, a, outs[0].cuda(), nz[0].contiguous().cuda(), 1, H, Hw, s)
        b = x.roll(s, 2).contiguous().cuda()
        _op(lib, smp, b, RH.roll_views(outs[0], 4, V).cuda(), nz[0].roll(s, 2).contiguous().cuda(), 1, H, Hw, s)
        assert torch.equal(b.cpu(), a.cpu().roll(s, 2)), (rule, pred)
        assert not torch.equal(a.cpu(), x)


# ---- tiny-UNet loops ----------------------------------------------------------------------------------------------------------------------
def _run_ring(e, rule, N, inputs, Hw, s, use_graph=True, noise=True, seed=0, offset=0, weights=None):
    enc, mask, lat0, noises = inputs
    V = lat0.shape[2] // s
    sch = LG._sched(rule)
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    e.denoise_ring(lat, enc.repeat_interleave(V, 0).cuda(), mask.repeat_interleave(V, 0).cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0,
                   window_h=Hw, stride=s, prediction_type=sch.config.prediction_type, rule=sch.rule,
                   noise=noises[:N].cuda() if noise else None, seed=seed, sample_offset=offset, use_graph=use_graph, view_weights=weights)
    torch.cuda.synchronize()
    return lat.cpu()


# ---- 3. one view is Engine.denoise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule,noise", [("ddpm", False), ("ddpm", True), ("ddim1", True)])
def test_one_view_is_the_plain_call_bit_for_bit(rule, noise, dtype):
    """H == Hw == s: V = 1, no wrap"""
    N, H = 4, 64
    inputs = LG._canvas_inputs(H)
    enc, mask, lat0, noises = inputs
    e = TI.unet_engine(dtype)
    ref = LG._run_plain(e, rule, N, enc, mask, lat0, noises if noise else None, H, seed=77)
    for use_graph in (True, False):
        got = _run_ring(e, rule, N, inputs, 64, 64, use_graph=use_graph, noise=noise, seed=77)
        assert torch.equal(got, ref), (rule, noise, dtype, use_graph)


# ---- 4. the loop against the oracle -------------------------------------------------------------------------------------------------------
H4, HW4, S4, N4 = 96, 64, 24, 10           # V = 4, counts 2 / 3; views 2 and 3 wrap


def _loop_oracle(rule):
    """the loop composed from the oracle: per step, O.unet_forward on the rolled views of the ring (both CFG halves as one batch, every
    view under its sample's text) and the restated ring update"""
    if ("loop", rule) not in _cache:
        enc, mask, lat0, noises = LG._canvas_inputs(H4)
        B, V = lat0.shape[0], H4 // S4
        smp = LH.Sampler(rule, steps=N4)
        encw, maskw = enc.repeat_interleave(V, 0), mask.repeat_interleave(V, 0)
        x = lat0.clone()
        with torch.no_grad():
            for i, t in enumerate(smp.sch.timesteps):
                views = torch.stack([torch.roll(x, -v * S4, 2)[:, :, :HW4] for v in range(V)], 1).reshape(B * V, 8, HW4, 16)
                out = O.unet_forward(TI.unet_sd(), O.UNET_CONFIG_TINY, torch.cat([views, views]), int(t), encw, maskw, prefix="unet.")
                x = RH.ring_update(smp, i, x, out, noises[i], HW4, S4, guidance=3.0)
        _cache[("loop", rule)] = x
    return _cache[("loop", rule)]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule", ["ddim0", "ddpm"])
def test_ring_loop_graph_eager_and_oracle(rule, dtype):
    """bounds: tests/test_duration_gpu.py LOOP_TOL, the plain tiny loop's -- the average is a convex combination of per-view results"""
    inputs = LG._canvas_inputs(H4)
    ref = _loop_oracle(rule)
    e = TI.unet_engine(dtype)
    g = _run_ring(e, rule, N4, inputs, HW4, S4, use_graph=True)
    x = _run_ring(e, rule, N4, inputs, HW4, S4, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    err = (g - ref).abs().max().item()
    print("ring loop H=%d Hw=%d s=%d %s N=%d %s max abs err %.3e (|ref| max %.2f)" % (H4, HW4, S4, rule, N4, dtype, err, ref.abs().max()))
    assert err <= TD.LOOP_TOL[dtype]


# ---- 5. rotation, whole loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_ring_loop_commutes_with_a_rotation(dtype):
    """Every window of a sample runs under the same prompt row, so rolling lat0 and the noises by one stride hands every UNet row the
    input of its predecessor: the result is the rolled result -- no row of the loop is special, the wrap point included.  The update
    commutes bit for bit (test 2); the UNet sees the same rows in another order of the batch, which is batch-invariant only to
    rounding (tests/test_long_gpu.py test_philox_rows_do_not_depend_on_the_batch_split), so the bound is LOOP_TOL and the
    measured figure is printed."""
    enc, mask, lat0, noises = LG._canvas_inputs(H4)
    e = TI.unet_engine(dtype)
    a = _run_ring(e, "ddpm", N4, (enc, mask, lat0, noises), HW4, S4)
    b = _run_ring(e, "ddpm", N4, (enc, mask, lat0.roll(S4, 2).contiguous(), noises.roll(S4, 3).contiguous()), HW4, S4)
    d = (b - a.roll(S4, 2)).abs().max().item()
    print("ring loop rolled by one stride, %s: max abs diff to the rolled result %.3e, bit-equal: %s" % (dtype, d, torch.equal(b, a.roll(S4, 2))))
    assert d <= TD.LOOP_TOL[dtype]
    assert not torch.equal(a, lat0)


# ---- 6. state isolation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
@pytest.mark.parametrize("first", ["windows", "ring"])
def test_plain_windowed_ring_plain_on_one_plan(lib, first, weighted):
    """a plain call of batch B * V at H = 64, a windowed call and a ring call of V = 4 views share one plan; each gives the bits it gives
    alone (on a fresh engine).  The windowed and the ring call replay the SAME captured steps (UNetPlan::wgraphs[weighted]: the kernel
    reads linear-or-ring from the call's block), so whichever of the two captures them must serve the other: `first` runs first on the
    shared engine.  weighted: the same pair with a non-constant positive table of view weights (wgraphs[1])."""
    N, V = 3, 4
    ring_in = LG._canvas_inputs(H4)                            # (96, 64, 24): V = 4
    enc, mask, _, _ = ring_in
    win_in = LG._canvas_inputs(64 + 3 * 24)                    # (136, 64, 24) linear: V = 4
    g = torch.Generator().manual_seed(8)
    plain = (enc.repeat_interleave(V, 0), mask.repeat_interleave(V, 0), torch.randn(2 * V, 8, 64, 16, generator=g), torch.randn(N, 2 * V, 8, 64, 16, generator=g))
    win_in = (enc, mask) + tuple(win_in[2:])                   # the same text rows: the same single-key prefix, the same plan key
    wts = np.linspace(0.5, 1.5, 64, dtype=np.float32) if weighted else None

    def fresh():
        e = Engine(unet=O.UNET_CONFIG_TINY, dtype="fp32")
        e.load_synthetic(1234)
        return e

    def run_w(e):
        return LG._run_windows(e, "ddpm", N, win_in, 64, 24, weights=wts)

    def run_r(e):
        return _run_ring(e, "ddpm", N, ring_in, 64, 24, weights=wts)

    alone = (LG._run_plain(fresh(), "ddpm", N, *plain, 64), run_w(fresh()), run_r(fresh()))
    e = fresh()
    a = LG._run_plain(e, "ddpm", N, *plain, 64)
    plans = e.plan_stats()[1]
    if first == "windows":
        w = run_w(e)
        r = run_r(e)
    else:
        r = run_r(e)
        w = run_w(e)
    b = LG._run_plain(e, "ddpm", N, *plain, 64)
    assert e.plan_stats()[1] == plans, "the windowed and the ring call run the plain call's plan"
    assert torch.equal(a, alone[0]) and torch.equal(w, alone[1]) and torch.equal(r, alone[2]) and torch.equal(b, alone[0])
    assert torch.equal(r, run_r(e)) and torch.equal(w, run_w(e))
    with TI.tuning(lib, TANGO_GRAPH_STEPS=2):                 # k steps per graph: a 2-step replay plus a remainder
        assert torch.equal(r, run_r(e)) and torch.equal(w, run_w(e))
    e.drop_plans()                                            # the plan goes with graphs in its windowed slots
    assert e.plan_stats() == (0, 0)
    assert torch.equal(r, run_r(e))


# ---- 7. the ring tile blend ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hw4,s4,V", [(64, 32, 2), (64, 16, 4), (64, 24, 4)])
def test_mel_ring_blend(lib, Hw4, s4, V):
    """the criterion of tests/test_long_gpu.py test_mel_tile_blend: torch.equal to the restatement in the kernel's evaluation order, and
    tiles sliced from one ring mel give it back within 16 ulp (n <= 4 covering tiles: n products, 2 (n - 1) additions, one division)"""
    B, F, H4r = 2, 64, V * s4
    g = torch.Generator().manual_seed(Hw4 + s4)
    tiles = torch.randn(B * V, 1, Hw4, F, generator=g) * 3.0 - 4.0
    out = torch.empty(B, 1, H4r, F, device="cuda")
    assert lib.tango_op_mel_ring_blend(vp(tiles.cuda()), vp(out), B, V, Hw4, F, s4, None) == 0, lib.tango_last_error().decode()
    assert torch.equal(out.cpu(), RH.torch_ring_blend(tiles, B, V, Hw4, s4))
    mel = torch.randn(B, 1, H4r, F, generator=g) * 3.0 - 4.0
    sl = torch.stack([mel[:, :, RH.ring_rows(t, H4r, Hw4, s4)] for t in range(V)], 1).reshape(B * V, 1, Hw4, F).contiguous()
    assert lib.tango_op_mel_ring_blend(vp(sl.cuda()), vp(out), B, V, Hw4, F, s4, None) == 0
    d = (out.cpu().double() - mel.double()).abs() / LG._ulp(mel)
    print("ring blend (%d, %d) V=%d: tiles of one ring mel give it back within %.1f ulp" % (Hw4, s4, V, d.max().item()))
    assert d.max().item() <= 16
    if 2 * s4 == Hw4:
        w = RH.ring_blend_weights(Hw4, s4)
        assert torch.equal(w[:s4] + w[s4:], torch.ones(s4)), "the two weights at every row sum to 1"
    assert lib.tango_op_mel_ring_blend(vp(sl.cuda()), vp(out), B, V, Hw4, F, Hw4 + 1, None) != 0
    assert lib.tango_op_mel_ring_blend(vp(sl.cuda()), vp(out), B, 1, Hw4, F, s4, None) != 0 and "at least window_h" in lib.tango_last_error().decode()


# ---- 8. the ring decode -------------------------------------------------------------------------------------------------------------------
def _ring_decode_ref():
    if "ringdec" not in _cache:
        H, Hw, s, V = 96, 64, 24, 4
        z = torch.randn(1, 8, H, 16, generator=torch.Generator().manual_seed(4200)) * 1.1
        tiles = torch.cat([z[:, :, RH.ring_rows(v, H, Hw, s)] for v in range(V)])
        with torch.no_grad():
            dec = O.vae_decode_first_stage(TD._vae_sd(), O.VAE_CONFIG, tiles)
        _cache["ringdec"] = (z, dec.contiguous(), RH.torch_ring_blend(dec.contiguous(), 1, V, 4 * Hw, 4 * s))
    return _cache["ringdec"]


@pytest.mark.parametrize("dtype,mel_tol", [("fp32", 1e-5), ("fp16", 1.0e-2)])       # tests/test_long_gpu.py test_vae_decode_tiled
def test_vae_decode_ring(dtype, mel_tol):
    z, _, ref = _ring_decode_ref()
    e = TD._vae_engine(dtype)
    mel = e.vae_decode_ring(z.cuda(), 64, 24).cpu()
    err = TD.relerr(mel, ref)
    print("ring decode H=96 Hw=64 s=24 %s: mel rel err %.3e" % (dtype, err))
    assert mel.shape == (1, 1, 384, 64) == ref.shape and err <= mel_tol
    # the engine's own tiles (vae_decode of the rolled views) through the restated blend: the same comparison without the oracle's decoder
    tiles = torch.cat([e.vae_decode(z[:, :, RH.ring_rows(v, 96, 64, 24)].contiguous().cuda(), latent_h=64).cpu() for v in range(4)])
    err2 = TD.relerr(mel, RH.torch_ring_blend(tiles.contiguous(), 1, 4, 256, 96))
    print("ring decode against vae_decode's tiles blended by the restatement, %s: rel err %.3e" % (dtype, err2))
    assert err2 <= mel_tol
    one = e.vae_decode_ring(z[:, :, :64].contiguous().cuda(), 64, 64).cpu()
    assert torch.equal(one, e.vae_decode(z[:, :, :64].contiguous().cuda(), latent_h=64).cpu()), "one tile is the plain decode"
    with pytest.raises(ValueError, match="multiple of stride"):
        e.vae_decode_ring(torch.zeros(1, 8, 100, 16), 64, 24)
    with pytest.raises(ValueError, match="shorter than its windows"):
        e.vae_decode_ring(torch.zeros(1, 8, 48, 16), 64, 24)


# ---- 9. the vocoder on a ring -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_vocode_ring(lib, dtype):
    """T = 128 frames, B = 2.  The length is exactly 160 T; the output is the centre slice of vocode(circularly padded mel), bit for
    bit; and vocoding the mel twice round the ring reproduces the single loop twice -- fp32 within 1 LSB at every sample (the CPU
    residual of the fp32 oracle is 8.6e-6 of full scale, 0.28 LSB before truncation), fp16 with an SNR of at least the 45 dB floor
    that tests/test_duration_gpu.py test_vae_decoder_encoder_and_vocoder uses for this vocoder."""
    T, B = 128, 2
    e = TD._vae_engine(dtype)
    cx = e.vocoder_ring_context()
    assert cx == 24, "the receptive field of O.HIFIGAN_CONFIG reaches 23.16 frames: 24 after rounding up to a multiple of 4"
    mel = (torch.randn(B, 1, T, 64, generator=torch.Generator().manual_seed(77)) * 2.0 - 4.0).cuda()
    w1 = e.vocode_ring(mel)
    assert w1.shape == (B, 160 * T) and w1.dtype == torch.int16
    idx = (torch.arange(T + 2 * cx) - cx) % T
    padded = mel[:, :, idx.cuda()].contiguous()
    got = torch.empty_like(padded)
    assert lib.tango_op_mel_ring_pad(vp(mel), vp(got), B, T, 64, cx, None) == 0, lib.tango_last_error().decode()
    assert torch.equal(got, padded)
    full = e.vocode(padded)
    assert full.shape == (B, 160 * (T + 2 * cx) + 32)
    assert torch.equal(w1, full[:, 160 * cx + 16:160 * cx + 16 + 160 * T])
    w2 = e.vocode_ring(torch.cat([mel, mel], 2).contiguous())
    assert w2.shape == (B, 320 * T)
    ref = torch.cat([w1, w1], 1).cpu().numpy().astype(np.int32)
    d = np.abs(w2.cpu().numpy().astype(np.int32) - ref)
    snr = 10 * np.log10((ref.astype(np.float64) ** 2).mean() / ((d.astype(np.float64) ** 2).mean() + 1e-9))
    print("vocode_ring %s: twice round the ring against the loop twice: int16 |diff| max %d, SNR %.1f dB" % (dtype, d.max(), snr))
    assert np.abs(ref).max() > 0
    if dtype == "fp32":
        assert d.max() <= 1
    else:
        assert snr >= 45.0
    # a ring shorter than the context is walked more than once
    short = mel[:, :, :8].contiguous()
    assert e.vocode_ring(short).shape == (B, 160 * 8)
    with pytest.raises(ValueError, match="vocode_ring: mel must be"):
        e.vocode_ring(torch.zeros(1, 1, 8, 32))


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------------
def test_generate_loop_equals_the_hand_composed_chain():
    t = TD._tango_text()
    H, Hw, s, V = loop_geometry(5, 2.5, 1.25)
    assert (H, Hw, s, V) == (128, 64, 32, 4)
    torch.manual_seed(21)
    w = t.generate_loop("rain on a tin roof", 5, steps=4, guidance=3, window=2.5, hop=1.25, seed=9)
    assert w.dtype == np.int16 and w.shape == (1, 640 * H) and np.abs(w.astype(np.float32)).max() > 0
    torch.manual_seed(21)
    m = t.model
    lat = m.inference_loop(["rain on a tin roof"], t.scheduler, 4, 3, 1, 5, 2.5, 1.25, seed=9)
    assert lat.shape == (1, 8, 128, 16)
    mel = t.vae.engine.vae_decode_ring(lat, Hw, s)
    assert mel.shape == (1, 1, 4 * H, 64)
    assert np.array_equal(w, t.vae.engine.vocode_ring(mel).cpu().numpy())
    # inference_loop itself is the engine call on one embedding row per window
    torch.manual_seed(21)
    pe, pm, host = m._encode_text_classifier_free(["rain on a tin roof"], 1)
    lat2 = m.prepare_latents(1, t.scheduler, 8, torch.float32, m.device, long_h=H)
    pe, pm, host = m._pad_text(pe.float(), pm, host)
    t.scheduler.set_timesteps(4, device=m.device)
    c = t.scheduler.config
    m.engine.denoise_ring(lat2, pe.repeat_interleave(V, 0), pm.repeat_interleave(V, 0), t.scheduler.timesteps.cpu().numpy(), t.scheduler.coef_table(),
                          3, window_h=Hw, stride=s, prediction_type=c.prediction_type, rule=t.scheduler.rule, clip_sample=c.clip_sample,
                          clip_sample_range=getattr(c, "clip_sample_range", 1.0), seed=9, prompt_mask_host=host.repeat_interleave(V, 0))
    assert torch.equal(lat2, lat)
    # the default geometry: one window of the clip's own length every half window
    one = t.generate_loop("rain", 2.5, steps=2, seed=4)
    assert one.shape == (1, 640 * 64)
    # two samples are rows of one call, or one chunk each when a call may hold only 2 * V = 8 UNet rows
    for rows in (t.LONG_MAX_ROWS, 8):
        t.LONG_MAX_ROWS = rows
        try:
            two = t.generate_loop("rain", 5, steps=2, samples=2, window=2.5, hop=1.25, seed=4)
        finally:
            del t.LONG_MAX_ROWS
        assert two.shape == (2, 640 * H) and not np.array_equal(two[0], two[1])
