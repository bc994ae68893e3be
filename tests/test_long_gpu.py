"""Clips longer than 20 s on the GPU (MultiDiffusion windows in time): the windowed update kernel through tango_op_sched_windows, bit for
bit against the torch restatement of tests/test_long_host.py; Engine.denoise_windows against Engine.denoise (one view), against a loop
composed from the oracle's UNet and scheduler steps per view, across plain calls of the same plan, and across a batch split; the mel
tile blend and the tiled VAE decode; Tango.generate_long against the hand-composed chain; the refusals of the Python and C layers."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_duration_gpu as TD  # noqa: E402  (LOOP_TOL, the VAE engines and state dict, the synthetic Tango stack with a tokenizer)
import test_inpaint_gpu as TI  # noqa: E402  (shared tiny-UNet engines and their state dict)
import test_long_host as LH  # noqa: E402  (the restatement of the windowed update)
from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd import _lib  # noqa: E402
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.inpaint import long_geometry, vocoder_samples  # noqa: E402

PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}
RULE = {"ddpm": 0, "ddim": 1}
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. the op, bit for bit ---------------------------------------------------------------------------------------------------------------
GEOMS = [(31, 16, 3), (48, 16, 16), (120, 64, 8)]      # (H, Hw, s): odd stride that does not divide Hw (counts 1..6); no overlap; V = 8, count 8


def _op(lib, smp, lat, out, noise, i, H, Hw, s, seed=0, offset=0, cfg=1):
    B, Cc, W = lat.shape[0], lat.shape[1], lat.shape[3]
    rc = lib.tango_op_sched_windows(vp(lat), vp(out), vp(noise), hp(smp.coef[i]), B, Cc, H, W, Hw, s, cfg, 3.0, PRED[smp.sch.config.prediction_type],
                                    RULE[smp.engine_rule], 1 if smp.sch.config.clip_sample else 0, 1.0, seed, offset, i, None)
    assert rc == 0, lib.tango_last_error().decode()


@pytest.mark.parametrize("H,Hw,s", GEOMS)
@pytest.mark.parametrize("rule,pred,clip", LH.CASES)
def test_op_windows_bitwise(lib, rule, pred, clip, H, Hw, s):
    """B = 2, CFG on, two consecutive steps with injected canvas noise: torch.equal to the restatement"""
    smp = LH.Sampler(rule, pred, clip)
    x, outs, nz = LH.window_inputs(2, H, Hw, s, seed=100 + H)
    lat = x.clone().cuda()
    ref = x
    for i in (0, 1):
        _op(lib, smp, lat, outs[i].cuda(), nz[i].contiguous().cuda(), i, H, Hw, s)
        ref = LH.window_update(smp, i, ref, outs[i], nz[i], Hw, s, guidance=3.0)
        assert torch.equal(lat.cpu(), ref), (rule, pred, i, (lat.cpu() - ref).abs().max().item())
    assert not torch.equal(ref, x)


def _philox(lib, B, HW, step, seed, offset):
    out = torch.empty(B, 8, HW, device="cuda")
    assert lib.tango_op_philox_normal(vp(out), B, 8, HW, step, seed, offset, None) == 0
    return out.cpu()


def test_op_windows_philox_draws_one_value_per_canvas_element(lib):
    """noise NULL: the draws are tango_op_philox_normal's on the CANVAS shape (counter (h * W + w, c / 4, sample, step))"""
    H, Hw, s = GEOMS[0]
    smp = LH.Sampler("ddpm", "v_prediction")
    x, outs, _ = LH.window_inputs(2, H, Hw, s, seed=7)
    lat = x.clone().cuda()
    _op(lib, smp, lat, outs[0].cuda(), None, 1, H, Hw, s, seed=1234567, offset=5)
    nz = _philox(lib, 2, H * 16, 1, 1234567, 5).view(2, 8, H, 16)
    assert torch.equal(lat.cpu(), LH.window_update(smp, 1, x, outs[0], nz, Hw, s, guidance=3.0))


# ---- tiny-UNet loops ----------------------------------------------------------------------------------------------------------------------
def _sched(rule):
    return LH.Sampler(rule, steps=1).sch if rule in ("ddim0", "ddim1") else TI._sched("ddpm")


def _canvas_inputs(H, B=2, L=9, N=10):
    """a CFG batch of B prompts (one-token unconditional rows, one ragged conditional row), a canvas and canvas-shaped step noise"""
    if ("in", H, B) not in _cache:
        g = torch.Generator().manual_seed(5100 + H + B)
        enc = torch.randn(2 * B, L, O.UNET_CONFIG_TINY["cross_attention_dim"], generator=g)
        mask = torch.ones(2 * B, L, dtype=torch.bool)
        mask[:B, 1:] = False
        mask[2 * B - 1, L // 2:] = False
        lat0 = torch.randn(B, 8, H, 16, generator=g)
        noises = torch.randn(N, B, 8, H, 16, generator=g)
        _cache[("in", H, B)] = (enc, mask, lat0, noises)
    return _cache[("in", H, B)]


def _run_windows(e, rule, N, inputs, Hw, s, use_graph=True, noise=True, seed=0, offset=0, weights=None):
    enc, mask, lat0, noises = inputs
    V = (lat0.shape[2] - Hw) // s + 1
    sch = _sched(rule)
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    e.denoise_windows(lat, enc.repeat_interleave(V, 0).cuda(), mask.repeat_interleave(V, 0).cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0,
                      window_h=Hw, stride=s, prediction_type=sch.config.prediction_type, rule=sch.rule,
                      noise=noises[:N].cuda() if noise else None, seed=seed, sample_offset=offset, use_graph=use_graph, view_weights=weights)
    torch.cuda.synchronize()
    return lat.cpu()


def _run_plain(e, rule, N, enc, mask, lat0, noises, H, use_graph=True, seed=0):
    sch = _sched(rule)
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type=sch.config.prediction_type, rule=sch.rule,
              noise=noises[:N].cuda() if noises is not None else None, seed=seed, use_graph=use_graph, latent_h=H)
    torch.cuda.synchronize()
    return lat.cpu()


# ---- 2. one view is Engine.denoise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule,noise", [("ddpm", False), ("ddpm", True), ("ddim1", True)])
def test_one_window_is_the_plain_call_bit_for_bit(rule, noise, dtype):
    N, H = 4, 64
    inputs = _canvas_inputs(H)
    enc, mask, lat0, noises = inputs
    e = TI.unet_engine(dtype)
    ref = _run_plain(e, rule, N, enc, mask, lat0, noises if noise else None, H, seed=77)
    for use_graph in (True, False):
        got = _run_windows(e, rule, N, inputs, 64, 64, use_graph=use_graph, noise=noise, seed=77)
        assert torch.equal(got, ref), (rule, noise, dtype, use_graph)
    assert torch.equal(_run_windows(e, rule, N, inputs, 64, 17, noise=noise, seed=77), ref), "with H == Hw any stride is one view"


# ---- 3. the loop against the oracle -------------------------------------------------------------------------------------------------------
H3, HW3, S3, N3 = 112, 64, 24, 10          # V = 3, counts 1 / 2 / 3 / 2 / 1


def _loop_oracle(rule):
    """the loop composed from the oracle: per step, O.unet_forward on every view of the canvas (the views of both CFG halves as one
    batch, every view under its sample's text), the scheduler oracle per view and the averaging of the restatement"""
    if ("loop", rule) not in _cache:
        enc, mask, lat0, noises = _canvas_inputs(H3)
        B, V = lat0.shape[0], (H3 - HW3) // S3 + 1
        smp = LH.Sampler(rule, steps=N3)
        encw, maskw = enc.repeat_interleave(V, 0), mask.repeat_interleave(V, 0)
        x = lat0.clone()
        with torch.no_grad():
            for i, t in enumerate(smp.sch.timesteps):
                views = torch.stack([x[:, :, v * S3:v * S3 + HW3] for v in range(V)], 1).reshape(B * V, 8, HW3, 16)
                out = O.unet_forward(TI.unet_sd(), O.UNET_CONFIG_TINY, torch.cat([views, views]), int(t), encw, maskw, prefix="unet.")
                x = LH.window_update(smp, i, x, out, noises[i], HW3, S3, guidance=3.0)
        _cache[("loop", rule)] = x
    return _cache[("loop", rule)]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule", ["ddim0", "ddpm"])
def test_window_loop_graph_eager_and_oracle(rule, dtype):
    """bounds: tests/test_duration_gpu.py LOOP_TOL, the plain tiny loop's -- the average is a convex combination of per-view results"""
    inputs = _canvas_inputs(H3)
    ref = _loop_oracle(rule)
    e = TI.unet_engine(dtype)
    g = _run_windows(e, rule, N3, inputs, HW3, S3, use_graph=True)
    x = _run_windows(e, rule, N3, inputs, HW3, S3, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    err = (g - ref).abs().max().item()
    print("window loop H=%d Hw=%d s=%d %s N=%d %s max abs err %.3e (|ref| max %.2f)" % (H3, HW3, S3, rule, N3, dtype, err, ref.abs().max()))
    assert err <= TD.LOOP_TOL[dtype]


# ---- 4. state isolation -----------------------------------------------------------------------------------------------------------------------
def test_plain_windowed_plain_on_one_plan(lib):
    """a plain call of batch B * V at H = 64 has the windowed call's plan key: both use one plan, each replays its own graph"""
    N = 3
    inputs = _canvas_inputs(H3)
    enc, mask, lat0, noises = inputs
    V = (H3 - HW3) // S3 + 1
    g = torch.Generator().manual_seed(8)
    plain = (enc.repeat_interleave(V, 0), mask.repeat_interleave(V, 0), torch.randn(2 * V, 8, 64, 16, generator=g), torch.randn(N, 2 * V, 8, 64, 16, generator=g))
    e = Engine(unet=O.UNET_CONFIG_TINY, dtype="fp32")
    e.load_synthetic(1234)
    a = _run_plain(e, "ddpm", N, *plain, 64)
    plans = e.plan_stats()[1]
    w = _run_windows(e, "ddpm", N, inputs, HW3, S3)
    assert e.plan_stats()[1] == plans, "the windowed call runs the plain call's plan"
    b = _run_plain(e, "ddpm", N, *plain, 64)
    assert torch.equal(a, b)
    assert torch.equal(w, _run_windows(e, "ddpm", N, inputs, HW3, S3)), "and the windowed graph replays the same bits after a plain call"
    fresh = Engine(unet=O.UNET_CONFIG_TINY, dtype="fp32")
    fresh.load_synthetic(1234)
    assert torch.equal(w, _run_windows(fresh, "ddpm", N, inputs, HW3, S3))
    with TI.tuning(lib, TANGO_GRAPH_STEPS=2):                 # k steps per graph: a 2-step replay plus a remainder
        assert torch.equal(w, _run_windows(e, "ddpm", N, inputs, HW3, S3))
    e.drop_plans()                                            # the plan goes with graphs in its windowed slot
    assert e.plan_stats() == (0, 0)
    assert torch.equal(w, _run_windows(e, "ddpm", N, inputs, HW3, S3))


# ---- 5. batch split ---------------------------------------------------------------------------------------------------------------------------
def test_philox_rows_do_not_depend_on_the_batch_split(lib):
    """Rows of a B = 2 Philox call equal two B = 1 calls with sample_offset 0 and 1, bit for bit, through the update itself (op level,
    three consecutive steps: the draws are keyed by the global sample index and the canvas position).  Through the UNet the loop is
    batch-invariant only to rounding, like the plain loop (tests/test_inpaint_gpu.py test_blend_noise_batch_split_invariance,
    test_parity_full_gpu.py): the GEMMs of a 12-row and of a 6-row batch tile differently.  Each run is within LOOP_TOL of the same
    oracle loop (test 3), so two runs are within twice that of each other; the measured figure is printed."""
    H, Hw, s = GEOMS[0]
    smp = LH.Sampler("ddpm", "v_prediction")
    V = (H - Hw) // s + 1
    x, outs, _ = LH.window_inputs(2, H, Hw, s, seed=19, steps=3)

    def run(lo, hi):
        lat = x[lo:hi].clone().cuda()
        for i in range(3):
            o = outs[i].view(2, 2, V, 8, Hw, 16)[:, lo:hi].reshape(-1, 8, Hw, 16).contiguous()
            _op(lib, smp, lat, o.cuda(), None, i, H, Hw, s, seed=4242, offset=lo)
        return lat.cpu()

    both = run(0, 2)
    assert torch.equal(both, torch.cat([run(0, 1), run(1, 2)])) and not torch.equal(both[0], both[1])
    N = 3
    enc, mask, lat0, noises = _canvas_inputs(H3)
    e = TI.unet_engine("fp32")
    full = _run_windows(e, "ddpm", N, (enc, mask, lat0, noises), HW3, S3, noise=False, seed=99)
    for b in (0, 1):
        one = (enc[[b, 2 + b]], mask[[b, 2 + b]], lat0[b:b + 1], None)
        d = (_run_windows(e, "ddpm", N, one, HW3, S3, noise=False, seed=99, offset=b)[0] - full[b]).abs().max().item()
        print("window loop, sample %d alone against its row of the B = 2 call: max abs diff %.3e" % (b, d))
        assert d <= 2 * TD.LOOP_TOL["fp32"]
    assert not torch.equal(full[0], full[1])


# ---- 6. the mel tile blend ----------------------------------------------------------------------------------------------------------------------
def torch_tile_blend(tiles, B, V, Hw4, s4):
    """the weight formula of tango_op_mel_tile_blend in the kernel's evaluation order, all fp32: per output row the covering tiles in
    ascending order, num = 0 + w_t tile_t + ..., den = 0 + w_t + ..., num / den"""
    F = tiles.shape[-1]
    Hout, E = (V - 1) * s4 + Hw4, Hw4 - s4
    t4 = tiles.view(B, V, Hw4, F)
    num, den = torch.zeros(B, Hout, F), torch.zeros(Hout, 1)
    y, one, e = torch.arange(Hw4, dtype=torch.float32), torch.ones(Hw4), torch.full((Hw4,), float(max(E, 1)))   # tensor / tensor: a true division
    for t in range(V):
        w = one
        if E > 0 and t > 0:
            w = torch.minimum(one, (y + 0.5) / e)
        if E > 0 and t < V - 1:
            w = w * torch.minimum(one, ((Hw4 - y) - 0.5) / e)
        rows = slice(t * s4, t * s4 + Hw4)
        num[:, rows] = num[:, rows] + w.view(1, Hw4, 1) * t4[:, t]
        den[rows] = den[rows] + w.view(Hw4, 1)
    return (num / den).view(B, 1, Hout, F)


def _ulp(x):
    """the spacing of fp32 at |x| (2^-149 at 0)"""
    _, e = torch.frexp(x.abs().double())
    return torch.maximum(torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 24), torch.full_like(x, 2.0 ** -149, dtype=torch.float64))


@pytest.mark.parametrize("Hw4,s4,V", [(64, 40, 3), (64, 64, 3), (64, 12, 8)])
def test_mel_tile_blend(lib, Hw4, s4, V):
    """Same evaluation order as the kernel (fp32 multiply, add and IEEE division, no contraction): torch.equal holds.  Tiles sliced from one
    mel must give it back: out = (sum w_t m) / (sum w_t) takes n products, n - 1 + n - 1 additions that matter pairwise (numerator and
    denominator err alike) and one division -- at most n + 2 roundings of half an ulp on a value of the mel's size with n <= 8 covering
    tiles, within 16 ulp of the value."""
    B, F = 2, 64
    Hout = (V - 1) * s4 + Hw4
    g = torch.Generator().manual_seed(Hw4 + s4)
    tiles = torch.randn(B * V, 1, Hw4, F, generator=g) * 3.0 - 4.0
    out = torch.empty(B, 1, Hout, F, device="cuda")
    assert lib.tango_op_mel_tile_blend(vp(tiles.cuda()), vp(out), B, V, Hw4, F, s4, None) == 0, lib.tango_last_error().decode()
    assert torch.equal(out.cpu(), torch_tile_blend(tiles, B, V, Hw4, s4))
    mel = torch.randn(B, 1, Hout, F, generator=g) * 3.0 - 4.0
    sl = torch.stack([mel[:, :, t * s4:t * s4 + Hw4] for t in range(V)], 1).reshape(B * V, 1, Hw4, F).contiguous()
    assert lib.tango_op_mel_tile_blend(vp(sl.cuda()), vp(out), B, V, Hw4, F, s4, None) == 0
    d = (out.cpu().double() - mel.double()).abs() / _ulp(mel)
    print("blend (%d, %d) V=%d: tiles of one mel give it back within %.1f ulp" % (Hw4, s4, V, d.max().item()))
    assert d.max().item() <= 16
    if s4 == Hw4:
        assert torch.equal(out.cpu(), mel)


def test_mel_tile_blend_half_overlap_weights_sum_to_one():
    """s >= Hw / 2: two overlapping weights are the fork's blend_v ramp at half-pixel centres, (y + 0.5) / E and 1 - (y + 0.5) / E"""
    Hw4, s4 = 64, 40
    E = Hw4 - s4
    y = torch.arange(E, dtype=torch.float64)
    up, down = (y + 0.5) / E, (Hw4 - (y + s4) - 0.5) / E      # tile t + 1 at local row y, tile t at local row y + s4
    assert torch.equal(up + down, torch.ones(E, dtype=torch.float64))


# ---- 7. the tiled decode ------------------------------------------------------------------------------------------------------------------------
def _tiled_ref():
    if "tiled" not in _cache:
        H, Hw, s, V = 144, 64, 40, 3
        z = torch.randn(1, 8, H, 16, generator=torch.Generator().manual_seed(4100)) * 1.1
        tiles = torch.cat([z[:, :, v * s:v * s + Hw] for v in range(V)])
        with torch.no_grad():
            dec = O.vae_decode_first_stage(TD._vae_sd(), O.VAE_CONFIG, tiles)
        _cache["tiled"] = (z, torch_tile_blend(dec.contiguous(), 1, V, 4 * Hw, 4 * s))
    return _cache["tiled"]


@pytest.mark.parametrize("dtype,mel_tol", [("fp32", 1e-5), ("fp16", 1.0e-2)])       # tests/test_duration_gpu.py test_vae_decoder_encoder_and_vocoder
def test_vae_decode_tiled(dtype, mel_tol):
    z, ref = _tiled_ref()
    e = TD._vae_engine(dtype)
    mel = e.vae_decode_tiled(z.cuda(), 64, 40).cpu()
    err = TD.relerr(mel, ref)
    print("tiled decode H=144 Hw=64 s=40 %s: mel rel err %.3e" % (dtype, err))
    assert mel.shape == (1, 1, 576, 64) == ref.shape and err <= mel_tol
    one = e.vae_decode_tiled(z[:, :, :64].contiguous().cuda(), 64, 64).cpu()
    assert torch.equal(one, e.vae_decode(z[:, :, :64].contiguous().cuda(), latent_h=64).cpu()), "one tile is the plain decode"


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_generate_long_equals_the_hand_composed_chain():
    t = TD._tango_text()
    H, Hw, s, V = long_geometry(5, 2.5, 1.25)
    assert (H, Hw, s, V) == (128, 64, 32, 3)
    torch.manual_seed(21)
    w = t.generate_long("rain on a tin roof", 5, steps=4, guidance=3, window=2.5, hop=1.25, seed=9)
    assert w.dtype == np.int16 and w.shape == (1, vocoder_samples(4 * H)) and np.abs(w.astype(np.float32)).max() > 0
    torch.manual_seed(21)
    m = t.model
    pe, pm, host = m._encode_text_classifier_free(["rain on a tin roof"], 1)
    lat = m.prepare_latents(1, t.scheduler, 8, torch.float32, m.device, long_h=H)
    assert lat.shape == (1, 8, 128, 16)
    pe, pm, host = m._pad_text(pe.float(), pm, host)
    t.scheduler.set_timesteps(4, device=m.device)
    c = t.scheduler.config
    m.engine.denoise_windows(lat, pe.repeat_interleave(V, 0), pm.repeat_interleave(V, 0), t.scheduler.timesteps.cpu().numpy(), t.scheduler.coef_table(),
                             3, window_h=Hw, stride=s, prediction_type=c.prediction_type, rule=t.scheduler.rule, clip_sample=c.clip_sample,
                             clip_sample_range=getattr(c, "clip_sample_range", 1.0), seed=9, prompt_mask_host=host.repeat_interleave(V, 0))
    mel = t.vae.engine.vae_decode_tiled(lat, Hw, s)
    assert mel.shape == (1, 1, 4 * H, 64)
    assert np.array_equal(w, t.vae.engine.vocode(mel).cpu().numpy())
    # two samples are rows of one call, or one chunk each when a call may hold only 2 * V = 6 UNet rows
    for rows in (t.LONG_MAX_ROWS, 6):
        t.LONG_MAX_ROWS = rows
        try:
            two = t.generate_long("rain", 5, steps=2, samples=2, window=2.5, hop=1.25, seed=4)
        finally:
            del t.LONG_MAX_ROWS
        assert two.shape == (2, vocoder_samples(4 * H)) and not np.array_equal(two[0], two[1])


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_python_and_c_layers(lib):
    e = TI.unet_engine("fp32")
    enc, mask, lat0, noises = _canvas_inputs(H3)
    sch = TI._sched("ddpm")
    sch.set_timesteps(2)
    V = 3

    def call(lat=lat0, Hw=HW3, s=S3, rows=V, **kw):
        e.denoise_windows(lat.clone().cuda(), enc.repeat_interleave(rows, 0).cuda(), mask.repeat_interleave(rows, 0).cuda(), sch.timesteps.numpy(),
                          sch.coef_table(), 3.0, window_h=Hw, stride=s, **kw)

    call()
    dpm = TI._sched("dpmpp_2m")
    dpm.set_timesteps(2)
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported with windows"):
        call(rule="dpmsolver")
    with pytest.raises(ValueError, match="known_latents .* not supported with windows"):
        call(known_latents=lat0.cuda())
    with pytest.raises(ValueError, match="guidance table or rescale is not supported with windows"):
        call(guidance_table=np.full((2, 2), 3.0, np.float32))
    with pytest.raises(ValueError, match="guidance table or rescale is not supported with windows"):
        call(guidance_rescale=0.5)
    with pytest.raises(ValueError, match="not covered exactly"):
        call(s=25)
    with pytest.raises(ValueError, match="stride"):
        call(s=0)
    with pytest.raises(ValueError, match="stride"):
        call(s=65)
    with pytest.raises(ValueError, match="at most 32"):
        call(lat=torch.zeros(2, 8, 64 + 32 * 8, 16), s=8, rows=33)
    with pytest.raises(ValueError, match="latent height"):
        call(lat=torch.zeros(2, 8, 96, 16), Hw=32, s=32)
    with pytest.raises(ValueError, match="one row per window"):
        call(rows=2)
    with pytest.raises(ValueError, match="noise must be"):
        call(noise=noises[:2, :, :, :64])
    ve = TD._vae_engine("fp32")
    with pytest.raises(ValueError, match="not covered exactly"):
        ve.vae_decode_tiled(torch.zeros(1, 8, 100, 16), 64, 32)
    with pytest.raises(ValueError, match="latents must be"):
        ve.vae_decode_tiled(torch.zeros(1, 4, 128, 16), 64, 32)

    # the C layer: every refusal fires before a pointer is read
    def c_call(H=H3, Hw=HW3, s=S3, **fields):
        a = _lib.DenoiseArgs()
        a.num_steps, a.batch, a.guidance_scale, a.latent_h = 2, 2, 3.0, H
        for k, v in fields.items():
            setattr(a, k, v)
        w = _lib.WindowArgs(window_h=Hw, stride=s)
        rc = lib.tango_engine_denoise_windows(e._h, C.byref(a), C.byref(w), None)
        assert rc != 0
        return lib.tango_last_error().decode()

    p = np.zeros(8, np.float32).ctypes.data
    assert "denoise_windows: the multistep rule is not supported with windows" in c_call(rule=2, coef_width=16)
    assert "denoise_windows: known_latents" in c_call(known_latents=p, latent_mask=p, blend_coef=p)
    assert "cover the canvas exactly" in c_call(H=100)
    assert "stride must be in [1, window_h]" in c_call(s=0)
    assert "at most 32 windows" in c_call(H=64 + 32 * 8, s=8)
    assert "not a UNet height" in c_call(H=60, Hw=60, s=4)
    assert "multiple of 64" in c_call(H=96, Hw=32, s=32), "a multiple of 8 that this UNet's four levels cannot halve"
    assert lib.tango_engine_denoise_windows(e._h, None, None, None) != 0
    x = torch.zeros(2, 8, 31, 16, device="cuda")
    o = torch.zeros(2 * 2 * 6, 8, 16, 16, device="cuda")
    row = np.zeros(16, np.float32)
    assert lib.tango_op_sched_windows(vp(x), vp(o), None, hp(row), 2, 8, 31, 16, 16, 3, 1, 3.0, 2, 2, 0, 1.0, 0, 0, 0, None) != 0
    assert "op_sched_windows: the multistep rule is not supported with windows" in lib.tango_last_error().decode()
    assert lib.tango_op_sched_windows(vp(x), vp(o), None, hp(row), 2, 8, 31, 16, 16, 4, 1, 3.0, 2, 0, 0, 1.0, 0, 0, 0, None) != 0
    assert "cover the canvas exactly" in lib.tango_last_error().decode()
    assert lib.tango_engine_vae_decode_tiled_h(TD._vae_engine("fp32")._h, vp(x), vp(o), 1, 100, 64, 32, None) != 0
    assert "vae_decode_tiled: the windows must cover the canvas exactly" in lib.tango_last_error().decode()
    assert lib.tango_op_mel_tile_blend(vp(x), vp(o), 1, 2, 64, 64, 65, None) != 0
