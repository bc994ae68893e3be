"""Timed prompts on the GPU (a prompt per window, tapered MultiDiffusion weights): the weighted update through
tango_op_sched_windows_weighted / tango_op_sched_ring_weighted, bit for bit against the torch restatement of tests/test_timeline_host.py,
against the unweighted hooks (all-ones weights) and under a rotation of the ring; the routing of one text row per window through
Engine.denoise_windows, without a tolerance, against a plain batch of the same rows; the weighted loop against a loop composed from the
oracle's UNet and scheduler steps; weighted and unweighted calls on one plan; Tango.generate_timeline against the hand-composed chain;
the refusals of the Python and C layers."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_duration_gpu as TD  # noqa: E402  (LOOP_TOL, the synthetic Tango stack with a tokenizer)
import test_inpaint_gpu as TI  # noqa: E402  (shared tiny-UNet engines and their state dict)
import test_long_gpu as LG  # noqa: E402  (the plain runner, the canvas inputs, the schedulers)
import test_long_host as LH  # noqa: E402  (Sampler, CASES, window_update)
import test_loop_gpu as RG  # noqa: E402  (the ring geometry of the oracle loop)
import test_loop_host as LP  # noqa: E402  (the ring restatement and its geometries)
import test_timeline_host as TH  # noqa: E402  (the weighted restatement)
from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd import _lib  # noqa: E402
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.inpaint import long_geometry, loop_geometry, timeline_geometry, vocoder_samples, window_taper  # noqa: E402

vp, hp = LG.vp, LG.hp
_cache = {}


# ---- 1. the op, bit for bit ---------------------------------------------------------------------------------------------------------------
def _op(lib, ring, smp, lat, out, noise, i, H, Hw, s, w, seed=0, offset=0, cfg=1):
    """w None: the unweighted hook"""
    B, Cc, W = lat.shape[0], lat.shape[1], lat.shape[3]
    tail = (B, Cc, H, W, Hw, s, cfg, 3.0, LG.PRED[smp.sch.config.prediction_type], LG.RULE[smp.engine_rule],
            1 if smp.sch.config.clip_sample else 0, 1.0, seed, offset, i, None)
    if w is None:
        fn = lib.tango_op_sched_ring if ring else lib.tango_op_sched_windows
        rc = fn(vp(lat), vp(out), vp(noise), hp(smp.coef[i]), *tail)
    else:
        w = np.ascontiguousarray(w, dtype=np.float32)
        fn = lib.tango_op_sched_ring_weighted if ring else lib.tango_op_sched_windows_weighted
        rc = fn(vp(lat), vp(out), vp(noise), hp(smp.coef[i]), hp(w), *tail)
    assert rc == 0, lib.tango_last_error().decode()


GEOMS = [(False,) + g for g in TH.LINEAR] + [(True,) + g for g in LP.GEOMS]


def _inputs(ring, H, Hw, s, seed):
    return (LP.ring_inputs if ring else LH.window_inputs)(2, H, Hw, s, seed=seed)


@pytest.mark.parametrize("table", ["taper", "random"])
@pytest.mark.parametrize("ring,H,Hw,s", GEOMS)
@pytest.mark.parametrize("rule,pred,clip", LH.CASES)
def test_op_weighted_bitwise(lib, rule, pred, clip, ring, H, Hw, s, table):
    """B = 2, CFG on, two consecutive steps with injected canvas noise: torch.equal to the restatement"""
    smp = LH.Sampler(rule, pred, clip)
    x, outs, nz = _inputs(ring, H, Hw, s, 300 + H + s)
    w = window_taper(Hw, s) if table == "taper" else TH.random_weights(Hw, H)
    lat = x.clone().cuda()
    ref = x
    for i in (0, 1):
        _op(lib, ring, smp, lat, outs[i].cuda(), nz[i].contiguous().cuda(), i, H, Hw, s, w)
        ref = TH.weighted_window_update(smp, i, ref, outs[i], nz[i], Hw, s, w, guidance=3.0, ring=ring)
        assert torch.equal(lat.cpu(), ref), (rule, pred, i, (lat.cpu() - ref).abs().max().item())
    assert not torch.equal(ref, x)


# ---- 2. all-ones weights are the unweighted op --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,H,Hw,s", GEOMS)
def test_op_all_ones_is_the_unweighted_op(lib, ring, H, Hw, s):
    ones = np.ones(Hw, dtype=np.float32)
    for rule, pred, clip in LH.CASES:
        smp = LH.Sampler(rule, pred, clip)
        x, outs, nz = _inputs(ring, H, Hw, s, 41)
        a, b = x.clone().cuda(), x.clone().cuda()
        for i in (0, 1):
            _op(lib, ring, smp, a, outs[i].cuda(), nz[i].contiguous().cuda(), i, H, Hw, s, None)
            _op(lib, ring, smp, b, outs[i].cuda(), nz[i].contiguous().cuda(), i, H, Hw, s, ones)
            assert torch.equal(a, b), (rule, pred, i)
        assert not torch.equal(a.cpu(), x)
    # ... and the Philox draws are the unweighted op's: one per canvas element
    smp = LH.Sampler("ddpm", "v_prediction")
    a, b = x.clone().cuda(), x.clone().cuda()
    _op(lib, ring, smp, a, outs[0].cuda(), None, 1, H, Hw, s, None, seed=1234567, offset=5)
    _op(lib, ring, smp, b, outs[0].cuda(), None, 1, H, Hw, s, ones, seed=1234567, offset=5)
    assert torch.equal(a, b) and smp.sigma(1) > 0


# ---- 3. rotation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hw,s", [(96, 64, 24), (64, 64, 16)])
def test_op_weighted_ring_commutes_with_a_rotation_by_one_stride(lib, H, Hw, s):
    V, w = H // s, window_taper(Hw, s)
    for rule, pred in (("ddpm", "v_prediction"), ("ddim1", "sample"), ("ddim0", "epsilon")):
        smp = LH.Sampler(rule, pred)
        x, outs, nz = LP.ring_inputs(2, H, Hw, s, seed=31)
        a = x.clone().cuda()
        _op(lib, True, smp, a, outs[0].cuda(), nz[0].contiguous().cuda(), 1, H, Hw, s, w)
        b = x.roll(s, 2).contiguous().cuda()
        _op(lib, True, smp, b, LP.roll_views(outs[0], 4, V).cuda(), nz[0].roll(s, 2).contiguous().cuda(), 1, H, Hw, s, w)
        assert torch.equal(b.cpu(), a.cpu().roll(s, 2)), (rule, pred)
        assert not torch.equal(a.cpu(), x)


# ---- 4. prompt routing, without a tolerance -------------------------------------------------------------------------------------------------
def _routing_inputs(L=9, N=4):
    """B = 1 on a canvas of two disjoint windows: the rows [uncond; uncond; A; B] of the window batch, A and B with different ragged masks"""
    if "route" not in _cache:
        g = torch.Generator().manual_seed(7300)
        enc = torch.randn(4, L, O.UNET_CONFIG_TINY["cross_attention_dim"], generator=g)
        enc[1] = enc[0]                                       # one sample: both windows' unconditional rows are its own
        mask = torch.ones(4, L, dtype=torch.bool)
        mask[:2, 1:] = False
        mask[2, 6:] = False
        mask[3, 3:] = False
        _cache["route"] = (enc, mask, torch.randn(1, 8, 128, 16, generator=g), torch.randn(N, 1, 8, 128, 16, generator=g))
    return _cache["route"]


def _halves(t, dim):
    """a canvas tensor's rows [0, 64) and [64, 128) as the two samples of a batch"""
    return torch.cat(t.split(64, dim), dim - 2).contiguous()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule", ["ddim0", "ddpm"])
def test_each_window_runs_under_its_own_text(rule, dtype):
    N = 4
    enc, mask, lat0, noises = _routing_inputs(N=N)
    e = TI.unet_engine(dtype)
    w = window_taper(64, 64)
    assert np.array_equal(w, np.ones(64, dtype=np.float32)), "E = 0: the taper is all ones, (1 d) / 1 is exact"
    # the same rows in the same order, the same plan key: sample 0 is the top half under A, sample 1 the bottom half under B
    ref = LG._run_plain(e, rule, N, enc, mask, _halves(lat0, 2), _halves(noises, 3), 64)

    def run(enc, mask, use_graph, weights):
        sch = LG._sched(rule)
        sch.set_timesteps(N)
        lat = lat0.clone().cuda()
        e.denoise_windows(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, window_h=64, stride=64,
                          prediction_type=sch.config.prediction_type, rule=sch.rule, noise=noises[:N].cuda(), use_graph=use_graph,
                          view_weights=weights)
        torch.cuda.synchronize()
        return lat.cpu()

    for use_graph in (True, False):
        got = run(enc, mask, use_graph, w)
        assert torch.equal(got[0, :, :64], ref[0]) and torch.equal(got[0, :, 64:], ref[1]), (rule, dtype, use_graph)
        assert torch.equal(got, run(enc, mask, use_graph, None)), "and the unweighted call routes the rows alike"
    both_a = run(enc[[0, 1, 2, 2]], mask[[0, 1, 2, 2]], True, w)
    assert torch.equal(both_a[0, :, :64], ref[0]), "window 0 still runs under A"
    assert not torch.equal(both_a[0, :, 64:], ref[1]), "window 1 under A differs from window 1 under B"


# ---- 5. the weighted loop against the oracle --------------------------------------------------------------------------------------------------
LOOPS = {"linear": (False, LG.H3, LG.HW3, LG.S3, LG.N3), "ring": (True, RG.H4, RG.HW4, RG.S4, RG.N4)}


def _window_rows(B, V):
    """per-window text for a CFG batch of B = 2 prompts: the first V - 1 windows of a sample under its own rows (text A), the last one
    under the other sample's (text B) -- the window batch's order, row half * B * V + b * V + v"""
    return [half * B + (b if v < V - 1 else 1 - b) for half in (0, 1) for b in range(B) for v in range(V)]


def _loop_oracle(kind):
    """tests/test_long_gpu.py _loop_oracle / tests/test_loop_gpu.py _loop_oracle with a text per window and the weighted restatement"""
    if ("loop", kind) not in _cache:
        ring, H, Hw, s, N = LOOPS[kind]
        enc, mask, lat0, noises = LG._canvas_inputs(H)
        B, V = lat0.shape[0], H // s if ring else (H - Hw) // s + 1
        rows = _window_rows(B, V)
        smp = LH.Sampler("ddpm", steps=N)
        w = window_taper(Hw, s)
        x = lat0.clone()
        with torch.no_grad():
            for i, t in enumerate(smp.sch.timesteps):
                views = torch.stack([x[:, :, LP.ring_rows(v, H, Hw, s) if ring else slice(v * s, v * s + Hw)] for v in range(V)], 1)
                views = views.reshape(B * V, 8, Hw, 16)
                out = O.unet_forward(TI.unet_sd(), O.UNET_CONFIG_TINY, torch.cat([views, views]), int(t), enc[rows], mask[rows], prefix="unet.")
                x = TH.weighted_window_update(smp, i, x, out, noises[i], Hw, s, w, guidance=3.0, ring=ring)
        _cache[("loop", kind)] = x
    return _cache[("loop", kind)]


def _run_timeline(e, kind, N, use_graph=True, weights="taper", rows=None):
    ring, H, Hw, s, _ = LOOPS[kind]
    enc, mask, lat0, noises = LG._canvas_inputs(H)
    V = H // s if ring else (H - Hw) // s + 1
    rows = _window_rows(lat0.shape[0], V) if rows is None else rows
    sch = LG._sched("ddpm")
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    (e.denoise_ring if ring else e.denoise_windows)(
        lat, enc[rows].cuda(), mask[rows].cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, window_h=Hw, stride=s,
        prediction_type=sch.config.prediction_type, rule=sch.rule, noise=noises[:N].cuda(), use_graph=use_graph,
        view_weights=window_taper(Hw, s) if isinstance(weights, str) else weights)
    torch.cuda.synchronize()
    return lat.cpu()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["linear", "ring"])
def test_weighted_loop_graph_eager_and_oracle(kind, dtype):
    """bounds: tests/test_duration_gpu.py LOOP_TOL, the plain tiny loop's -- the weighted mean is still a convex combination of
    per-view results"""
    N = LOOPS[kind][4]
    ref = _loop_oracle(kind)
    e = TI.unet_engine(dtype)
    g = _run_timeline(e, kind, N, use_graph=True)
    x = _run_timeline(e, kind, N, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    err = (g - ref).abs().max().item()
    print("weighted %s loop (H, Hw, s) = %s N=%d %s: max abs err %.3e (|ref| max %.2f)" % (kind, LOOPS[kind][1:4], N, dtype, err, ref.abs().max()))
    assert err <= TD.LOOP_TOL[dtype]
    assert not torch.equal(g, _run_timeline(e, kind, N, weights=None)), "the taper changes the result"


# ---- 6. state isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "ring"])
def test_unweighted_weighted_unweighted_on_one_plan(lib, kind):
    N = 3

    def fresh():
        e = Engine(unet=O.UNET_CONFIG_TINY, dtype="fp32")
        e.load_synthetic(1234)
        return e

    alone = (_run_timeline(fresh(), kind, N, weights=None), _run_timeline(fresh(), kind, N))
    assert not torch.equal(alone[0], alone[1])
    e = fresh()
    a = _run_timeline(e, kind, N, weights=None)
    plans = e.plan_stats()[1]
    w = _run_timeline(e, kind, N)
    b = _run_timeline(e, kind, N, weights=None)
    w2 = _run_timeline(e, kind, N, weights=TH.random_weights(64, 3))      # another table replays the weighted graph with its own weights
    assert e.plan_stats()[1] == plans, "the weighted call runs the unweighted call's plan"
    assert torch.equal(a, alone[0]) and torch.equal(b, alone[0]) and torch.equal(w, alone[1])
    assert not torch.equal(w2, w) and torch.equal(w, _run_timeline(e, kind, N))
    with TI.tuning(lib, TANGO_GRAPH_STEPS=2):                 # k steps per graph: a 2-step replay plus a remainder
        assert torch.equal(w, _run_timeline(e, kind, N)) and torch.equal(a, _run_timeline(e, kind, N, weights=None))
    e.drop_plans()                                            # the plan goes with graphs in its weighted slots
    assert e.plan_stats() == (0, 0)
    assert torch.equal(w, _run_timeline(e, kind, N)) and torch.equal(a, _run_timeline(e, kind, N, weights=None))


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------------
SEG = [("rain on a tin roof", 0), ("thunder", 2.5)]


@pytest.mark.parametrize("loop", [False, True])
def test_generate_timeline_equals_the_hand_composed_chain(loop):
    t = TD._tango_text()
    m, eng = t.model, t.vae.engine
    H, Hw, s, V, wp = timeline_geometry(SEG, 5, 2.5, 1.25, loop)
    assert (H, Hw, s, V, wp) == ((128, 64, 32, 4, [0, 1, 1, 0]) if loop else (128, 64, 32, 3, [0, 1, 1]))
    n = 640 * H if loop else vocoder_samples(4 * H)

    def finish(lat):
        if loop:
            return eng.vocode_ring(eng.vae_decode_ring(lat, Hw, s)).cpu().numpy()
        return eng.vocode(eng.vae_decode_tiled(lat, Hw, s)).cpu().numpy()

    torch.manual_seed(21)
    w = t.generate_timeline(SEG, 5, steps=4, guidance=3, window=2.5, hop=1.25, loop=loop, seed=9)
    assert w.dtype == np.int16 and w.shape == (1, n) and np.abs(w.astype(np.float32)).max() > 0
    torch.manual_seed(21)
    lat = m.inference_timeline(SEG, t.scheduler, 4, 3, 1, 5, 2.5, 1.25, loop, True, seed=9)
    assert lat.shape == (1, 8, H, 16)
    assert np.array_equal(w, finish(lat))
    # inference_timeline itself is the engine call on the rows gathered per window, with the taper
    torch.manual_seed(21)
    pe, pm, host = m._encode_text_classifier_free([p for p, _ in SEG], 1)
    assert pm.sum(1).tolist() == [1, 1, 6, 2], "two unconditional rows of one key, two ragged conditional rows"
    lat2 = m.prepare_latents(1, t.scheduler, 8, torch.float32, m.device, long_h=H)
    pe, pm, host = m._pad_text(pe.float(), pm, host)
    rows = [half * 2 + i for half in (0, 1) for i in wp]
    t.scheduler.set_timesteps(4, device=m.device)
    c = t.scheduler.config
    (m.engine.denoise_ring if loop else m.engine.denoise_windows)(
        lat2, pe[rows], pm[rows], t.scheduler.timesteps.cpu().numpy(), t.scheduler.coef_table(), 3, window_h=Hw, stride=s,
        prediction_type=c.prediction_type, rule=t.scheduler.rule, clip_sample=c.clip_sample,
        clip_sample_range=getattr(c, "clip_sample_range", 1.0), seed=9, prompt_mask_host=host[rows], view_weights=window_taper(Hw, s))
    assert torch.equal(lat2, lat)
    # the prompts and the taper matter
    torch.manual_seed(21)
    assert not np.array_equal(w, t.generate_timeline(SEG, 5, steps=4, guidance=3, window=2.5, hop=1.25, loop=loop, taper=False, seed=9))
    torch.manual_seed(21)
    assert not np.array_equal(w, t.generate_timeline([(SEG[0][0], 0), ("birds", 2.5)], 5, steps=4, guidance=3, window=2.5, hop=1.25, loop=loop, seed=9))
    # one segment without the taper is generate_long / generate_loop
    torch.manual_seed(33)
    one = t.generate_timeline([("rain on a tin roof", 0)], 5, steps=4, guidance=3, window=2.5, hop=1.25, loop=loop, taper=False,
                              negative_prompt="wind", seed=5)
    torch.manual_seed(33)
    old = (t.generate_loop if loop else t.generate_long)("rain on a tin roof", 5, steps=4, guidance=3, window=2.5, hop=1.25,
                                                         negative_prompt="wind", seed=5)
    assert np.array_equal(one, old)
    # two samples are rows of one call, or one chunk each when a call may hold only 2 * V UNet rows
    for rows in (t.LONG_MAX_ROWS, 2 * V):
        t.LONG_MAX_ROWS = rows
        try:
            two = t.generate_timeline(SEG, 5, steps=2, samples=2, window=2.5, hop=1.25, loop=loop, negative_prompt=["wind", "hum"], seed=4)
        finally:
            del t.LONG_MAX_ROWS
        assert two.shape == (2, n) and not np.array_equal(two[0], two[1])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring", [False, True])
def test_refusals_of_the_python_and_c_layers(lib, ring):
    e = TI.unet_engine("fp32")
    H, Hw, s, V = (RG.H4, RG.HW4, RG.S4, 4) if ring else (LG.H3, LG.HW3, LG.S3, 3)
    enc, mask, lat0, noises = LG._canvas_inputs(H)
    sch = TI._sched("ddpm")
    sch.set_timesteps(2)
    how = "on a ring" if ring else "with windows"
    pre = "denoise_ring_weighted: " if ring else "denoise_windows_weighted: "

    def call(weights, **kw):
        (e.denoise_ring if ring else e.denoise_windows)(lat0.clone().cuda(), enc.repeat_interleave(V, 0).cuda(), mask.repeat_interleave(V, 0).cuda(),
                                                        sch.timesteps.numpy(), sch.coef_table(), 3.0, window_h=Hw, stride=s, view_weights=weights, **kw)

    good = window_taper(Hw, s)
    call(good)
    call(torch.from_numpy(good))
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        t = good.copy()
        t[Hw // 2] = bad
        with pytest.raises(ValueError, match="view_weights entries must be finite and > 0"):
            call(t)
    for n in (Hw - 1, Hw + 1, s):
        with pytest.raises(ValueError, match=r"view_weights must be \[window_h = %d\], got \(%d,\)" % (Hw, n)):
            call(np.ones(n, dtype=np.float32))
    with pytest.raises(ValueError, match="view_weights must be"):
        call(np.ones((1, Hw), dtype=np.float32))
    with pytest.raises(ValueError, match="multistep DPM-Solver rule is not supported " + how):
        call(good, rule="dpmsolver")
    with pytest.raises(ValueError, match="known_latents .* not supported " + how):
        call(good, known_latents=lat0.cuda())
    with pytest.raises(ValueError, match="guidance table or rescale is not supported " + how):
        call(good, guidance_rescale=0.5)

    # the C layer: every refusal fires before a device pointer is read
    run = lib.tango_engine_denoise_ring_weighted if ring else lib.tango_engine_denoise_windows_weighted

    def c_call(weights, H=H, Hw=Hw, s=s, **fields):
        a = _lib.DenoiseArgs()
        a.num_steps, a.batch, a.guidance_scale, a.latent_h = 2, 2, 3.0, H
        for k, v in fields.items():
            setattr(a, k, v)
        w = _lib.WindowArgs(window_h=Hw, stride=s)
        rc = run(e._h, C.byref(a), C.byref(w), hp(weights) if weights is not None else None, None)
        assert rc != 0
        return lib.tango_last_error().decode()

    p = np.zeros(8, np.float32).ctypes.data
    assert c_call(good, rule=2, coef_width=16).startswith(pre + "the multistep rule is not supported " + how)
    assert c_call(good, rule=2).startswith(pre + "the multistep rule is not supported " + how)
    assert c_call(good, known_latents=p, latent_mask=p, blend_coef=p).startswith(pre + "known_latents")
    assert c_call(None).startswith(pre + "view_weights must not be NULL")
    z = good.copy()
    z[0] = 0.0
    assert c_call(z).startswith(pre + "view_weights entries must be finite and > 0")
    z[0] = float("nan")
    assert c_call(z).startswith(pre + "view_weights entries must be finite and > 0")
    assert "stride must be in [1, window_h]" in c_call(good, s=0)
    assert run(e._h, None, None, None, None) != 0 and lib.tango_last_error().decode().startswith(pre + "null args")
    # the hooks
    x = torch.zeros(2, 8, 64, 16, device="cuda")
    o = torch.zeros(2 * 2 * 4, 8, 16, 16, device="cuda")
    row = np.zeros(16, np.float32)
    hook = lib.tango_op_sched_ring_weighted if ring else lib.tango_op_sched_windows_weighted
    name = "op_sched_ring_weighted: " if ring else "op_sched_windows_weighted: "
    w16 = np.ones(16, dtype=np.float32)
    assert hook(vp(x), vp(o), None, hp(row), hp(w16), 2, 8, 64, 16, 16, 16, 1, 3.0, 2, 2, 0, 1.0, 0, 0, 0, None) != 0
    assert lib.tango_last_error().decode().startswith(name + "the multistep rule is not supported " + how)
    assert hook(vp(x), vp(o), None, hp(row), None, 2, 8, 64, 16, 16, 16, 1, 3.0, 2, 0, 0, 1.0, 0, 0, 0, None) != 0
    assert lib.tango_last_error().decode().startswith(name + "view_weights must not be NULL")
    w16[5] = -1.0
    assert hook(vp(x), vp(o), None, hp(row), hp(w16), 2, 8, 64, 16, 16, 16, 1, 3.0, 2, 0, 0, 1.0, 0, 0, 0, None) != 0
    assert lib.tango_last_error().decode().startswith(name + "view_weights entries must be finite and > 0")
