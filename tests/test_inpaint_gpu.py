"""Masked-latent audio inpainting on the engine (audioldm/pipeline.py:249-301 -> ldm.py:724-818 -> latent_diffusion/ddim.py:207-233):
the fused masked step bit for bit against the fork's loops (tests/golden/inpaint_ref.npz), a zero mask against the unmasked loop,
the tiny-UNet loop against the fp32 oracle (graph / eager / k-step), one production-size chain against the oracle, the blend noise's
Philox stream, state isolation, argument checks and the public entry points (AudioDiffusion / MusicAudioDiffusion / Tango)."""
import contextlib
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd import weights as W  # noqa: E402
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.inpaint import latent_mask, prepare_waveform  # noqa: E402
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}
RULE = {"ddpm": 0, "ddim": 1, "dpmsolver": 2}
_DDPM_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
_cache = {}


def golden_tool():
    spec = importlib.util.spec_from_file_location("make_golden_inpaint", os.path.join(ROOT, "tools", "make_golden_inpaint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = golden_tool()


def fixture():
    if "fix" not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", "inpaint_ref.npz")) as z:
            _cache["fix"] = {k: z[k] for k in z.files}
    return _cache["fix"]


def unet_engine(dtype):
    if dtype not in _cache:
        e = Engine(unet=O.UNET_CONFIG_TINY, dtype=dtype)
        e.load_synthetic(1234)
        _cache[dtype] = e
    return _cache[dtype]


def unet_sd():
    if "sd" not in _cache:
        _cache["sd"] = W.synth_state_dict(W.unet_param_shapes(O.UNET_CONFIG_TINY, "unet."), 1234)
    return _cache["sd"]


@contextlib.contextmanager
def tuning(lib, **env):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    lib.tango_tuning_reload()
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib.tango_tuning_reload()


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- 1. op level: the fused masked step replays the fork's loops bit for bit --------------------------------------------------------
@pytest.mark.parametrize("rule,pred,cfg,mk", G.LOOP_GRID)
def test_op_masked_loop_bitwise(lib, rule, pred, cfg, mk):
    """the tables are the fixture's: the engine's coef_table() / blend_table() as computed where the fixture was made (pinned there
    by tests/test_inpaint_host.py).  Computed on another host they can differ in the last bit: torch's CPU arithmetic of the
    schedule (linspace, cumprod) is not the same on every x86 vector unit -- nothing this kernel check is about."""
    f = fixture()
    key = G.loop_key(rule, pred, cfg, mk)
    n = G.LOOP_STEPS
    sch = G.engine_scheduler(rule, pred)
    coef = np.ascontiguousarray(f["tab/%s|%s/coef" % (rule, pred)], dtype=np.float32)
    bc = np.ascontiguousarray(f["tab/%s|%s/blend" % (rule, pred)], dtype=np.float32)
    x, x0, m, outs, zn, bn = G.loop_inputs(int(f["seed/" + key]), n, cfg, mk)
    B, Cc, H, Wd = G.SHAPE
    HW = H * Wd
    lat = x.clone().cuda()
    x0d, md = x0.cuda(), m.cuda()
    bnd = torch.stack(bn).cuda()
    ms = sch.rule == "dpmsolver"
    znd = None if ms else torch.stack(zn).cuda()
    ring = torch.zeros(3, B, Cc, HW, device="cuda")
    for i in range(n):
        mod = outs[i].contiguous().cuda()          # [uncond; cond] when cfg: the op combines them
        rc = lib.tango_op_sched_masked(vp(lat), vp(mod), vp(znd), vp(ring), coef.ctypes.data_as(C.c_void_p), coef.shape[1], i, n,
                                       vp(x0d), vp(md), bc.ctypes.data_as(C.c_void_p), vp(bnd), 0, 0, B, Cc, HW, 1 if cfg else 0,
                                       G.GUIDANCE, PRED[pred], RULE[sch.rule], None)
        assert rc == 0, lib.tango_last_error().decode()
    got = lat.cpu().numpy()
    ref = f["loop/" + key]
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), "%s: max diff %g" % (key, np.abs(got - ref).max())


# ---- tiny-UNet loops ------------------------------------------------------------------------------------------------------------------
def _inputs(B=2, L=9, seed=31, N=10):
    cfg = O.UNET_CONFIG_TINY
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(2 * B, L, cfg["cross_attention_dim"], generator=g)
    mask = torch.ones(2 * B, L, dtype=torch.bool)
    mask[0, 1:] = False
    mask[2, L // 2:] = False
    lat0 = torch.randn(B, 8, 256, 16, generator=g)
    known = torch.randn(B, 8, 256, 16, generator=g) * 0.8
    noises = torch.randn(N, B, 8, 256, 16, generator=g)
    bnoise = torch.randn(N, B, 8, 256, 16, generator=g)
    # row 0: the AudioLDM default time mask (pipeline.py:259-262); row 1: a mel-frequency band (super-resolution style)
    lm = torch.cat([latent_mask(1), latent_mask(1, (0.0, 0.0), (0.5, 0.75))])
    return enc, mask, lat0, known, lm, noises, bnoise


def _sched(rule):
    if rule == "ddpm":
        return DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    if rule == "ddim_eta1":
        return DDIMScheduler(**SD21_SCHEDULER_CONFIG, eta=1.0)
    return DPMSolverMultistepScheduler(**G.sd21("dpm"), solver_order=2, algorithm_type="dpmsolver++")


def _oracle_sched(rule):
    if rule == "ddpm":
        return O.DDPMOracle(**O.SD21_SCHEDULER)
    if rule == "ddim_eta1":
        return O.DDIMOracle(**SD21_SCHEDULER_CONFIG, eta=1.0)
    return _DPMAdapter(_sched(rule))


class _DPMAdapter:
    """O.denoise_loop calls step(out, t, latents, noise=...) and takes the latents back"""

    def __init__(self, sch):
        self.s = sch

    def __getattr__(self, k):
        return getattr(self.s, k)

    def step(self, out, t, lat, noise=None):
        return self.s.step(out, t, lat).prev_sample


def masked_oracle(sd, cfg, rule, enc, mask, lat0, known, lm, noises, bnoise, N, prefix="unet.", music=None):
    """O.denoise_loop with the blend of ddim.py:210-217: before step 0 on the initial latents, after step i (in place, t_{i+1}) in
    the callback, none after the last step"""
    bl = _sched(rule)                         # add_noise (pinned to the fork bit for bit by tests/test_inpaint_host.py)
    bl.set_timesteps(N)
    ts = bl.timesteps
    x = bl.add_noise(known, bnoise[0], ts[0:1]) * lm + (1.0 - lm) * lat0

    def cb(i, t, lat):
        if i + 1 < N:
            lat.copy_(bl.add_noise(known, bnoise[i + 1], ts[i + 1:i + 2]) * lm + (1.0 - lm) * lat)

    with torch.no_grad():
        return O.denoise_loop(sd, cfg, _oracle_sched(rule), enc, mask, x, N, 3.0,
                              noises=None if rule == "dpmpp_2m" else list(noises), prefix=prefix, callback=cb, music=music)


def _oracle(rule, N, inputs):
    key = ("oracle", rule, N)
    if key not in _cache:
        enc, mask, lat0, known, lm, noises, bnoise = inputs
        _cache[key] = masked_oracle(unet_sd(), O.UNET_CONFIG_TINY, rule, enc, mask, lat0, known, lm, noises, bnoise, N)
    return _cache[key]


def _engine_run(e, rule, N, inputs, use_graph=True, masked=True, seed=0, blend=True, known=None, lm=None):
    enc, mask, lat0, kn, m, noises, bnoise = inputs
    sch = _sched(rule)
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    kw = {}
    if masked:
        kw = dict(known_latents=(kn if known is None else known).cuda(), latent_mask=(m if lm is None else lm).cuda(),
                  blend_coef=sch.blend_table(), blend_noise=bnoise[:N].cuda() if blend else None)
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type=sch.config.prediction_type,
              rule=sch.rule, noise=noises[:N].cuda() if (rule != "dpmpp_2m" and noises is not None) else None, seed=seed,
              use_graph=use_graph, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


RULES3 = ["ddpm", "ddim_eta1", "dpmpp_2m"]


# ---- 2. a zero mask is the unmasked loop, bit for bit (device-Philox step noise) ------------------------------------------------------
@pytest.mark.parametrize("rule", RULES3)
def test_zero_mask_equals_unmasked(lib, rule):
    e = unet_engine("fp32")
    enc, mask, lat0, known, lm, _, _ = _inputs(N=6)
    inputs = (enc, mask, lat0, known, torch.zeros_like(lm), None, None)
    for mode in ("graph", "eager", "k3"):
        with tuning(lib, TANGO_GRAPH_STEPS=3) if mode == "k3" else contextlib.nullcontext():
            g = mode != "eager"
            plain = _engine_run(e, rule, 6, inputs, use_graph=g, masked=False, seed=77)
            zero = _engine_run(e, rule, 6, inputs, use_graph=g, masked=True, seed=77, blend=False)
        assert torch.equal(plain, zero), "%s %s: max diff %g" % (rule, mode, (plain - zero).abs().max())


# ---- 3. loop vs the oracle; graph / eager / k-step agree bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("N", [10, 20])
@pytest.mark.parametrize("rule", RULES3)
def test_masked_loop_vs_oracle(lib, rule, N, dtype):
    inputs = _inputs(N=20)
    ref = _oracle(rule, N, inputs)
    e = unet_engine(dtype)
    g = _engine_run(e, rule, N, inputs, use_graph=True)
    x = _engine_run(e, rule, N, inputs, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    with tuning(lib, TANGO_GRAPH_STEPS=3):
        k = _engine_run(e, rule, N, inputs, use_graph=True)
    assert torch.equal(g, k), "the k-step graph must equal the one-step graph"
    err = (g - ref).abs().max().item()
    print("masked %s N=%d %s max abs err %.3e (|ref| max %.2f)" % (rule, N, dtype, err, ref.abs().max()))
    assert err <= (1e-2 if dtype == "fp32" else 1e-1)


# ---- 5. the blend noise's Philox stream --------------------------------------------------------------------------------------------
def _philox(lib, B, step, seed, offset, blend):
    out = torch.empty(B, 8, 4096, device="cuda")
    fn = lib.tango_op_philox_normal_blend if blend else lib.tango_op_philox_normal
    assert fn(vp(out), B, 8, 4096, step, seed, offset, None) == 0, lib.tango_last_error().decode()
    return out


def test_injected_blend_noise_equals_philox(lib):
    e = unet_engine("fp32")
    enc, mask, lat0, known, lm, noises, _ = _inputs(N=6)
    seed = 2024
    draws = torch.stack([_philox(lib, 2, i, seed, 0, True).view(2, 8, 256, 16) for i in range(6)]).cpu()
    for rule in ("ddpm", "dpmpp_2m"):
        inj = _engine_run(e, rule, 6, (enc, mask, lat0, known, lm, noises, draws), seed=seed, blend=True)
        phx = _engine_run(e, rule, 6, (enc, mask, lat0, known, lm, noises, draws), seed=seed, blend=False)
        assert torch.equal(inj, phx), "%s: max diff %g" % (rule, (inj - phx).abs().max())


def test_blend_noise_batch_split_invariance(lib):
    """the blend draws of samples [0, 2) at offset 0 == those of two one-sample calls at offsets 0 and 1; and so is the fused masked
    step that consumes them (op level, no UNet: the full loop is batch-invariant only to rounding, test_parity_full_gpu.py)"""
    for step in (0, 5):
        full = _philox(lib, 2, step, 99, 0, True)
        assert torch.equal(full, torch.cat([_philox(lib, 1, step, 99, 0, True), _philox(lib, 1, step, 99, 1, True)]))
    sch = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    N = 4
    sch.set_timesteps(N)
    coef, bc = sch.coef_table(), sch.blend_table()
    g = torch.Generator().manual_seed(8)
    x, x0 = torch.randn(2, 8, 4096, generator=g), torch.randn(2, 8, 4096, generator=g)
    m = (torch.rand(2, 4096, generator=g) > 0.3).float()
    outs = [torch.randn(4, 8, 4096, generator=g) for _ in range(N)]

    def run(lo, hi):
        lat, kn, md = x[lo:hi].clone().cuda(), x0[lo:hi].contiguous().cuda(), m[lo:hi].contiguous().cuda()
        B = hi - lo
        for i in range(N):
            mo = torch.cat([outs[i][lo:hi], outs[i][2 + lo:2 + hi]]).cuda()
            rc = lib.tango_op_sched_masked(vp(lat), vp(mo), None, None, coef.ctypes.data_as(C.c_void_p), 8, i, N, vp(kn), vp(md),
                                           bc.ctypes.data_as(C.c_void_p), None, 4242, lo, B, 8, 4096, 1, 3.0, 2, 0, None)
            assert rc == 0, lib.tango_last_error().decode()
        return lat.cpu()

    assert torch.equal(run(0, 2), torch.cat([run(0, 1), run(1, 2)]))


@pytest.mark.parametrize("seed", [1, 77, 31337])
def test_blend_draws_independent_of_step_draws(lib, seed):
    for step in (0, 3, 19):
        a = _philox(lib, 2, step, seed, 0, True).flatten().double()       # 65 536 values
        s = _philox(lib, 2, step, seed, 0, False).flatten().double()
        corr = torch.corrcoef(torch.stack([a, s]))[0, 1].item()
        mean, std = a.mean().item(), a.std().item()
        print("seed %d step %d: corr %.4f mean %.4f std %.4f" % (seed, step, corr, mean, std))
        assert abs(corr) < 0.02 and abs(mean) < 0.02 and abs(std - 1) < 0.02


# ---- 6. state isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["ddpm", "dpmpp_2m"])
def test_state_isolation_unmasked_masked_unmasked(lib, rule):
    e = unet_engine("fp32")
    inputs = _inputs(N=5)
    a = _engine_run(e, rule, 5, inputs, masked=False, seed=5)
    mk = _engine_run(e, rule, 5, inputs, masked=True, seed=5)
    b = _engine_run(e, rule, 5, inputs, masked=False, seed=5)
    assert torch.equal(a, b)
    assert not torch.equal(a, mk)


def test_every_step_graph_slot_of_one_plan_and_its_teardown(lib):
    """One UNet plan holds a captured step graph per (masked, multistep) pair -- the two bits that fix the update kernel.  All four on
    one engine, the k-step slot of plain DDPM re-captured when k changes (N = 5: a 2-step replay plus a remainder, and the multistep
    table reaches order 3), then the plan is dropped with graphs in every slot and each combination computes the same bits again."""
    e = Engine(unet=O.UNET_CONFIG_TINY, dtype="fp32")
    e.load_synthetic(1234)
    inputs = _inputs(N=5)
    combos = [(rule, masked) for rule in ("ddpm", "dpmpp_2m") for masked in (False, True)]
    first = {c: _engine_run(e, c[0], 5, inputs, masked=c[1], seed=5) for c in combos}
    for k in (2, 3):
        with tuning(lib, TANGO_GRAPH_STEPS=k):
            assert torch.equal(_engine_run(e, "ddpm", 5, inputs, masked=False, seed=5), first[("ddpm", False)]), k
    e.drop_plans()
    assert e.plan_stats() == (0, 0)
    for c in combos:
        assert torch.equal(_engine_run(e, c[0], 5, inputs, masked=c[1], seed=5), first[c]), c


# ---- 7. argument errors ------------------------------------------------------------------------------------------------------------
def test_masked_argument_errors(lib):
    e = unet_engine("fp32")
    enc, mask, lat0, known, lm, _, bnoise = _inputs(N=4)
    sch = _sched("ddpm")
    sch.set_timesteps(4)
    lat = lat0.clone().cuda()

    def call(**kw):
        e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, **kw)

    bc = sch.blend_table()
    for kw in (dict(known_latents=known.cuda(), blend_coef=bc), dict(latent_mask=lm.cuda(), blend_coef=bc),
               dict(known_latents=known[:1].cuda(), latent_mask=lm.cuda(), blend_coef=bc),
               dict(known_latents=known.cuda(), latent_mask=lm.expand(2, 8, 256, 16).contiguous().cuda(), blend_coef=bc),
               dict(known_latents=known.cuda(), latent_mask=lm.cuda(), blend_coef=bc[:3]),
               dict(known_latents=known.cuda(), latent_mask=lm.cuda(), blend_coef=bc[:, :1]),
               dict(known_latents=known.cuda(), latent_mask=lm.cuda()),
               dict(known_latents=known.cuda(), latent_mask=lm.cuda(), blend_coef=bc, blend_noise=bnoise[:3].cuda()),
               dict(known_latents=known.cuda(), latent_mask=lm * 2.0, blend_coef=bc),
               dict(blend_coef=bc)):
        with pytest.raises(ValueError):
            call(**kw)


# ---- 8. public entry points ------------------------------------------------------------------------------------------------------------
def _tango():
    if "tango" not in _cache:
        from oracle import stft_oracle as S
        from tango_amd.autoencoder import AutoencoderKL
        from tango_amd.models import AudioDiffusion
        from tango_amd.stft import TacotronSTFT
        from tango_amd.tango import Tango
        model = AudioDiffusion(unet_config=O.UNET_CONFIG_TINY, dtype="fp16")
        model.engine.load_synthetic(1234)
        vae = AutoencoderKL(ddconfig=dict(O.VAE_CONFIG, resolution=256, in_channels=1, double_z=True, attn_resolutions=[], dropout=0.0),
                            embed_dim=8, scale_factor=O.VAE_CONFIG["scale_factor"], dtype="fp16", with_encoder=True)
        vae.engine.load_synthetic(1234)
        _cache["tango"] = Tango.from_components(model, vae, stft=TacotronSTFT(**S.AUDIOLDM_STFT_CONFIG))
    return _cache["tango"]


def _clip():
    t = np.arange(3 * 16000) / 16000.0
    g = np.random.default_rng(17)
    return (0.3 * np.sin(2 * np.pi * 330 * t) + 0.05 * g.standard_normal(t.shape) + 0.1).astype(np.float32)


def test_tango_inpaint_end_to_end_matches_hand_composed_chain(lib):
    from tango_amd.stft import wav_to_fbank
    t = _tango()
    enc, mask, *_ = _inputs(B=2, N=1)
    audio = _clip()
    torch.manual_seed(11)
    w1 = t.inpaint_from_embeddings(enc.cuda(), mask.cuda(), audio, steps=5, guidance=3, samples=2, seed=7)
    assert w1.dtype == np.int16 and w1.shape == (2, 163872)
    torch.manual_seed(11)
    wav = prepare_waveform(audio)[None].cuda()
    fbank, _, _ = wav_to_fbank(wav, 1024, fn_STFT=t.stft)
    z = t.vae.get_first_stage_encoding(t.vae.encode_first_stage(fbank.unsqueeze(1)))
    lat = t.model.inpaint_from_embeddings(enc.cuda(), mask.cuda(), t.scheduler, 5, 3, known_latents=z.repeat_interleave(2, 0),
                                          latent_mask=latent_mask(2), seed=7)
    w2 = t.vae.decode_to_waveform(t.vae.decode_first_stage(lat))
    assert np.array_equal(w1, w2)
    assert np.abs(w1.astype(np.float32)).max() > 0


def test_tango_inpaint_needs_encoder(lib):
    from tango_amd.tango import Tango
    t = _tango()
    bare = Tango.from_components(t.model, t.vae)             # no stft
    enc, mask, *_ = _inputs(B=2, N=1)
    with pytest.raises(RuntimeError):
        bare.inpaint_from_embeddings(enc.cuda(), mask.cuda(), _clip(), steps=2, samples=2)


def test_music_masked_dpm_vs_oracle(lib):
    from oracle.make_golden import music_inputs
    from tango_amd.models import MusicAudioDiffusion
    cfg = O.UNET_CONFIG_MUSIC_TINY
    m = MusicAudioDiffusion(unet_config=cfg, dtype="fp32")
    sd = W.synth_state_dict(W.unet_param_shapes(cfg), 1234)
    m.load_state_dict({"unet." + k: v for k, v in sd.items()})
    B, N = 2, 5
    _, enc, beat, chord, em, bm, cm = music_inputs(cfg, 2 * B, 11)
    g = torch.Generator().manual_seed(12)
    lat0 = torch.randn(B, 8, 256, 16, generator=g)
    known = torch.randn(B, 8, 256, 16, generator=g)
    bnoise = torch.randn(N, B, 8, 256, 16, generator=g)
    lm = torch.cat([latent_mask(1), latent_mask(1, (0.0, 0.0), (0.5, 0.75))])
    sch = _sched("dpmpp_2m")
    got = m.inpaint_from_embeddings(enc, em, sch, N, 3.0, known_latents=known, latent_mask=lm, latents=lat0, blend_noise=bnoise,
                                    encoded_beats=beat, beat_mask=bm, encoded_chords=chord, chord_mask=cm).cpu()
    ref = masked_oracle(sd, cfg, "dpmpp_2m", enc, em, lat0, known, lm, None, bnoise, N, prefix="",
                        music=dict(beat_features=beat, chord_features=chord, beat_attention_mask=bm, chord_attention_mask=cm))
    err = (got - ref).abs().max().item()
    print("Music masked DPM++ 5 steps max abs err %.3e" % err)
    assert err <= 1e-2


# ---- 4. production size: B = 1, 20 DDPM steps, fp16, against the oracle (DESIGN.md section 4 floors) ----------------------------------
FP16_LATENT_MAX_ABS, FP16_MEL_PSNR_DB, FP16_WAVE_SNR_DB = 5e-2, 65.0, 40.0


def _full_inputs(N=20, seed=606):
    L = 64
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(2, L, 1024, generator=g)            # [uncond; cond]
    mask = torch.ones(2, L, dtype=torch.bool)
    mask[0, 1:] = False                                   # T5(""): one valid token (models.py:282-289)
    lat0 = torch.randn(1, 8, 256, 16, generator=g)
    known = torch.randn(1, 8, 256, 16, generator=g)
    noises = torch.randn(N, 1, 8, 256, 16, generator=g)
    bnoise = torch.randn(N, 1, 8, 256, 16, generator=g)
    return enc, mask, lat0, known, latent_mask(1), noises, bnoise


def _full_oracle_job(N):
    """the fp32 CPU oracle of the production-size case, in a worker process (16 threads)"""
    torch.set_num_threads(16)
    enc, mask, lat0, known, lm, noises, bnoise = _full_inputs(N)
    sd = W.synth_state_dict(W.unet_param_shapes(O.UNET_CONFIG_LARGE, "unet."), 1234)
    shapes = W.vae_decoder_param_shapes(O.VAE_CONFIG)
    shapes.update(W.hifigan_param_shapes(O.HIFIGAN_CONFIG))
    vsd = W.synth_state_dict(shapes, 1234)
    rlat = masked_oracle(sd, O.UNET_CONFIG_LARGE, "ddpm", enc, mask, lat0, known, lm, noises, bnoise, N)
    with torch.no_grad():
        rmel = O.vae_decode_first_stage(vsd, O.VAE_CONFIG, rlat)
        rwav = O.decode_to_waveform(vsd, O.HIFIGAN_CONFIG, rmel)
    return rlat.numpy(), rmel.numpy(), np.asarray(rwav)


def _psnr(x, ref):
    mse = ((x.double() - ref.double()) ** 2).mean().item()
    peak = (ref.max() - ref.min()).item()
    return 10 * np.log10(peak * peak / (mse + 1e-30))


def _snr(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return 10 * np.log10((ref ** 2).mean() / (((x - ref) ** 2).mean() + 1e-30))


def test_full_size_masked_ddpm_chain_fp16_vs_oracle(lib):
    import concurrent.futures as cf
    import multiprocessing as mp
    N = 20
    with cf.ProcessPoolExecutor(max_workers=1, mp_context=mp.get_context("spawn")) as pool:
        job = pool.submit(_full_oracle_job, N)
        enc, mask, lat0, known, lm, noises, bnoise = _full_inputs(N)
        e = Engine(unet=O.UNET_CONFIG_LARGE, dtype="fp16")
        e.load_synthetic(1234)
        sch = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
        sch.set_timesteps(N)
        lat = lat0.clone().cuda()
        e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, noise=noises.cuda(),
                  known_latents=known.cuda(), latent_mask=lm.cuda(), blend_coef=sch.blend_table(), blend_noise=bnoise.cuda())
        torch.cuda.synchronize()
        del e
        ev = Engine(vae=O.VAE_CONFIG, hifigan=O.HIFIGAN_CONFIG, dtype="fp16")
        ev.load_synthetic(1234)
        mel = ev.vae_decode(lat)
        wav = ev.vocode(mel).cpu().numpy()
        del ev
        rlat, rmel, rwav = job.result()
    rlat, rmel = torch.from_numpy(rlat), torch.from_numpy(rmel)
    lat, mel = lat.cpu(), mel.cpu()
    err = (lat - rlat).abs().max().item()
    psnr, snr = _psnr(mel[0], rmel[0]), _snr(wav[0], rwav[0])
    print("masked chain B=1, %d DDPM steps, fp16 vs fp32 oracle: latents max abs err %.3e (|ref| max %.2f), mel PSNR %.1f dB, "
          "waveform SNR %.1f dB" % (N, err, rlat.abs().max(), psnr, snr))
    assert wav.dtype == np.int16 and wav.shape == rwav.shape == (1, 163872)
    assert err <= FP16_LATENT_MAX_ABS
    assert psnr >= FP16_MEL_PSNR_DB and snr >= FP16_WAVE_SNR_DB
