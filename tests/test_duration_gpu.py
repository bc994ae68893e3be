"""Clip durations other than 10 s on the engine: latent heights 64 (2.5 s: the smallest images, a level-3 image is 8 x 2 pixels), 192 (7.5 s:
the one height of the grid that is no power of two -- 48 pixels per level-3 image, 3072 rows per sample at level 0) and 512 (20 s: the
longest rows, 8192 keys in a level-0 self-attention) through every layer -- the UNet forward and the fused loops on the tiny UNet, the
full-width UNet (config 3's widths) with the product's dispatch AND with the big-tile kernels forced onto these small problems, the mel-VAE
decoder / encoder, HiFi-GAN and the mel front-end, plan isolation across heights, and the public `duration=` surface.  The reference for every
number is the fp32 CPU oracle (plain torch, any height); bounds are the ones the same quantity's test uses at the default height 256:
tests/test_engine_gpu.py UTOL (tiny forward), test_inpaint_gpu.py / test_edit_gpu.py (tiny loops), test_parity_batch_gpu.py (full-width forward
and loop, VAE + vocoder), test_engine_gpu.py test_vae_encoder (encoder), test_stft_gpu.py (front-end)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_edit_gpu as TE  # noqa: E402  (the truncated-loop oracle adapter and the fp32 tiny model)
import test_inpaint_gpu as TI  # noqa: E402  (shared engines, schedulers, oracle adapters and the synthetic Tango stack)
from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd import weights as W  # noqa: E402
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.inpaint import duration_geometry, latent_mask, prepare_waveform, vocoder_samples  # noqa: E402
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler  # noqa: E402

_cache = {}
UTOL = {"fp32": 1e-3, "fp16": 3e-2}                     # tests/test_engine_gpu.py
LOOP_TOL = {"fp32": 1e-2, "fp16": 1e-1}                 # tests/test_inpaint_gpu.py, tests/test_edit_gpu.py
FULL_FWD_TOL = {"fp32": 1e-5, "fp16": 4.5e-3, "bf16": 3.4e-2}    # tests/test_parity_batch_gpu.py:97
FULL_LOOP_TOL = {"fp16": 1.8e-2}                        # the same line: the CFG loop's latents, max abs


def relerr(a, b):
    return ((a - b).abs().max() / (b.abs().max() + 1e-9)).item()


# ---- 1. tiny-UNet forward ------------------------------------------------------------------------------------------------------------------
def _fwd_case(H):
    if ("fwd", H) not in _cache:
        cfg = O.UNET_CONFIG_TINY
        g = torch.Generator().manual_seed(7000 + H)
        x = torch.randn(3, 8, H, 16, generator=g)
        enc = torch.randn(3, 13, cfg["cross_attention_dim"], generator=g)
        mask = torch.ones(3, 13, dtype=torch.bool)
        mask[0, 1:] = False
        mask[2, 6:] = False
        with torch.no_grad():
            ref = O.unet_forward(TI.unet_sd(), cfg, x, 801, enc, mask, prefix="unet.")
        _cache[("fwd", H)] = (x, enc, mask, ref)
    return _cache[("fwd", H)]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("H", [64, 192, 512])
def test_tiny_unet_forward(H, dtype):
    x, enc, mask, ref = _fwd_case(H)
    e = TI.unet_engine(dtype)
    out = e.unet_forward(x.cuda(), 801, enc.cuda(), mask.cuda(), latent_h=H).cpu()
    err = relerr(out, ref)
    print("tiny UNet forward H=%d %s rel err %.3e" % (H, dtype, err))
    assert out.shape == (3, 8, H, 16) and err <= UTOL[dtype]


def test_tiny_music_unet_forward_h64():
    from oracle.make_golden import music_inputs
    cfg = O.UNET_CONFIG_MUSIC_TINY
    sd = W.synth_state_dict(W.unet_param_shapes(cfg, "unet."), 1234)
    _, enc, beat, chord, em, bm, cm = music_inputs(cfg, 4, 77)
    x = torch.randn(4, 8, 64, 16, generator=torch.Generator().manual_seed(78))
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, 333, enc, em, prefix="unet.", beat_features=beat, chord_features=chord, beat_attention_mask=bm,
                             chord_attention_mask=cm)
    e = Engine(unet=cfg, dtype="fp32")
    e.load_synthetic(1234)
    out = e.unet_forward(x.cuda(), 333, enc.cuda(), em.cuda(), beat_features=beat.cuda(), chord_features=chord.cuda(),
                         beat_attention_mask=bm.cuda(), chord_attention_mask=cm.cuda(), latent_h=64).cpu()
    err = relerr(out, ref)
    print("tiny Music UNet forward H=64 fp32 rel err %.3e" % err)
    assert err <= UTOL["fp32"]


def test_music_model_draws_latents_of_the_duration():
    """MusicAudioDiffusion.inference_from_embeddings(duration=) sizes the latents it draws, like the plain model's"""
    from oracle.make_golden import music_inputs
    from tango_amd.models import MusicAudioDiffusion
    cfg = O.UNET_CONFIG_MUSIC_TINY
    m = MusicAudioDiffusion(unet_config=cfg, dtype="fp32")
    m.engine.load_synthetic(1234)
    _, enc, beat, chord, em, bm, cm = music_inputs(cfg, 2, 11)
    kw = dict(encoded_beats=beat, beat_mask=bm, encoded_chords=chord, chord_mask=cm)
    torch.manual_seed(3)
    a = m.inference_from_embeddings(enc, em, TI._sched("dpmpp_2m"), 2, 3.0, duration=2.5, **kw)
    torch.manual_seed(3)
    lat = m.prepare_latents(1, TI._sched("dpmpp_2m"), 8, torch.float32, m.device, latent_h=64)
    b = m.inference_from_embeddings(enc, em, TI._sched("dpmpp_2m"), 2, 3.0, latents=lat, **kw)
    assert a.shape == (1, 8, 64, 16) and torch.equal(a, b)
    with pytest.raises(ValueError):
        m.inference_from_embeddings(enc, em, TI._sched("dpmpp_2m"), 2, 3.0, duration=3, **kw)


# ---- 2. tiny-UNet loops ---------------------------------------------------------------------------------------------------------------------
def _loop_inputs(H, B=2, L=9, N=10):
    if ("in", H, B) not in _cache:
        cfg = O.UNET_CONFIG_TINY
        g = torch.Generator().manual_seed(900 + H + B)
        enc = torch.randn(2 * B, L, cfg["cross_attention_dim"], generator=g)
        mask = torch.ones(2 * B, L, dtype=torch.bool)
        mask[:B, 1:] = False                                  # the unconditional rows: T5("") keeps one token
        mask[2 * B - 1, L // 2:] = False
        lat0 = torch.randn(B, 8, H, 16, generator=g)
        known = torch.randn(B, 8, H, 16, generator=g) * 0.8
        noises = torch.randn(N, B, 8, H, 16, generator=g)
        bnoise = torch.randn(N, B, 8, H, 16, generator=g)
        lm = torch.cat([latent_mask(1, h=H)] + [latent_mask(1, (0.0, 0.0), (0.5, 0.75), h=H)] * (B - 1))
        _cache[("in", H, B)] = (enc, mask, lat0, known, lm, noises, bnoise)
    return _cache[("in", H, B)]


def _run(e, rule, N, inputs, H, use_graph=True, noise=True, seed=0):
    enc, mask, lat0, _, _, noises, _ = inputs
    sch = TI._sched(rule)
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type=sch.config.prediction_type,
              rule=sch.rule, noise=noises[:N].cuda() if (rule != "dpmpp_2m" and noise) else None, seed=seed, use_graph=use_graph,
              latent_h=H)
    torch.cuda.synchronize()
    return lat.cpu()


def _loop_oracle(rule, H, N):
    if ("loop", rule, H) not in _cache:
        enc, mask, lat0, _, _, noises, _ = _loop_inputs(H)
        with torch.no_grad():
            _cache[("loop", rule, H)] = O.denoise_loop(TI.unet_sd(), O.UNET_CONFIG_TINY, TI._oracle_sched(rule), enc, mask, lat0.clone(), N,
                                                       3.0, noises=None if rule == "dpmpp_2m" else list(noises), prefix="unet.")
    return _cache[("loop", rule, H)]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule", TI.RULES3)
@pytest.mark.parametrize("H", [64, 192])
def test_tiny_loops_graph_eager_and_oracle(H, rule, dtype):
    N = 10
    inputs = _loop_inputs(H)
    ref = _loop_oracle(rule, H, N)
    e = TI.unet_engine(dtype)
    g = _run(e, rule, N, inputs, H, use_graph=True)
    x = _run(e, rule, N, inputs, H, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    err = (g - ref).abs().max().item()
    print("tiny loop H=%d %s N=%d %s max abs err %.3e (|ref| max %.2f)" % (H, rule, N, dtype, err, ref.abs().max()))
    assert err <= LOOP_TOL[dtype]


def test_masked_loop_h64_vs_oracle():
    N, H = 10, 64
    enc, mask, lat0, known, lm, noises, bnoise = _loop_inputs(H)
    assert lm.shape == (2, 1, 64, 16)
    ref = TI.masked_oracle(TI.unet_sd(), O.UNET_CONFIG_TINY, "dpmpp_2m", enc, mask, lat0, known, lm, None, bnoise, N)
    m = TE._model("fp32")
    got = m.inpaint_from_embeddings(enc.cuda(), mask.cuda(), TI._sched("dpmpp_2m"), N, 3.0, known_latents=known, latent_mask=lm,
                                    latents=lat0, blend_noise=bnoise).cpu()
    err = (got - ref).abs().max().item()
    print("masked DPM++ loop H=64 fp32 max abs err %.3e" % err)
    assert got.shape == (2, 8, 64, 16) and err <= LOOP_TOL["fp32"]
    assert not torch.equal(got, _run(m.engine, "dpmpp_2m", N, _loop_inputs(H), H))      # the mask did something


def test_truncated_loop_h64_vs_oracle():
    N, H = 10, 64
    enc, mask, lat0, _, _, noises, _ = _loop_inputs(H)
    with torch.no_grad():
        ref = O.denoise_loop(TI.unet_sd(), O.UNET_CONFIG_TINY, TE._Truncated(TI._oracle_sched("ddpm"), N // 2), enc, mask, lat0.clone(), N,
                             3.0, noises=list(noises), prefix="unet.")
    m = TE._model("fp32")
    got = m.edit_from_embeddings(enc.cuda(), mask.cuda(), TI._sched("ddpm"), N, 3.0, start_latents=lat0, strength=0.5,
                                 noise=noises[:N - N // 2], seed=3).cpu()
    err = (got - ref).abs().max().item()
    print("truncated DDPM loop H=64 fp32 max abs err %.3e" % err)
    assert got.shape == (2, 8, 64, 16) and err <= LOOP_TOL["fp32"]


# ---- 3. full width (config 3: 320 / 640 / 1280 / 1280 channels, 64 text tokens), synthetic weights ------------------------------------------
L_FULL, T_FULL = 64, 500
# the product's own dispatch at these sizes, and the big-tile kernels forced onto them: the 256 x 320 / 256 x 160 GEMMs and halo convs, the
# four-phase upsamplers, ff_fused, qkv_stat and the GroupNorm-statistics proj_in -- the families a large batch runs, on 2.5 s / 7.5 s images
BIG = dict(TANGO_FORCE_DMA_GEMM=1, TANGO_FF_MIN_ROWS=0, TANGO_QKV_MIN_ROWS=0)


def _full_sd():
    if "full_sd" not in _cache:
        _cache["full_sd"] = W.synth_state_dict(W.unet_param_shapes(O.UNET_CONFIG_LARGE, "unet."), 1234)
    return _cache["full_sd"]


def _full_engine(dtype, **kw):
    key = ("full", dtype, tuple(sorted(kw.items())))
    if key not in _cache:
        for k in [k for k in _cache if isinstance(k, tuple) and k[0] == "full"]:
            del _cache[k]                                     # one full-width engine at a time (1.7 GB of packed weights each)
        e = Engine(unet=O.UNET_CONFIG_LARGE, dtype=dtype, **kw)
        e.load_synthetic(1234)
        _cache[key] = e
    return _cache[key]


def _full_inputs(H, B):
    """B prompts as a CFG batch [uncond; cond]: one-token unconditional rows, one ragged conditional row"""
    if ("fin", H, B) not in _cache:
        g = torch.Generator().manual_seed(6400 + H + B)
        enc = torch.randn(2 * B, L_FULL, 1024, generator=g)
        mask = torch.ones(2 * B, L_FULL, dtype=torch.bool)
        mask[:B, 1:] = False
        mask[2 * B - 1, 40:] = False
        x2 = torch.randn(2 * B, 8, H, 16, generator=g)
        lat0 = torch.randn(B, 8, H, 16, generator=g)
        noises = torch.randn(2, B, 8, H, 16, generator=g)
        _cache[("fin", H, B)] = (enc, mask, x2, lat0, noises)
    return _cache[("fin", H, B)]


def _full_fwd_ref(H):
    if ("fref", H) not in _cache:
        enc, mask, x2, _, _ = _full_inputs(H, 1)
        with torch.no_grad():
            _cache[("fref", H)] = O.unet_forward(_full_sd(), O.UNET_CONFIG_LARGE, x2, T_FULL, enc, mask, prefix="unet.")
    return _cache[("fref", H)]


@contextlib.contextmanager
def _dispatch(lib, e, big):
    """routing decisions are taken when a plan is built: plans of the other arm must not be reused"""
    e.drop_plans()
    with TI.tuning(lib, **BIG) if big else contextlib.nullcontext():
        yield
    e.drop_plans()


@pytest.mark.parametrize("big", [False, True], ids=["product", "big-tiles"])
@pytest.mark.parametrize("H", [64, 192])
def test_full_width_forward_fp16(lib, H, big):
    enc, mask, x2, _, _ = _full_inputs(H, 1)
    ref = _full_fwd_ref(H)
    e = _full_engine("fp16")
    with _dispatch(lib, e, big):
        out = e.unet_forward(x2.cuda(), T_FULL, enc.cuda(), mask.cuda(), latent_h=H).cpu()
    err = relerr(out, ref)
    print("full-width forward H=%d fp16 (%s dispatch) rel err %.3e" % (H, "big-tile" if big else "product", err))
    assert torch.isfinite(out).all() and err <= FULL_FWD_TOL["fp16"]


@pytest.mark.parametrize("big", [False, True], ids=["product", "big-tiles"])
def test_full_width_cfg_loop_h64_single_key_and_cfg_shared(lib, big):
    """two CFG DDPM steps at H = 64, B = 2 through the CFG-shared plan (the default for a [single-key; text] batch) and through the plain
    single-key plan (TANGO_NO_CFG_SHARED=1); both against the oracle loop, graph replay against eager launches bit for bit"""
    H, B, N = 64, 2, 2
    enc, mask, _, lat0, noises = _full_inputs(H, B)
    if ("lref", H) not in _cache:
        with torch.no_grad():
            _cache[("lref", H)] = O.denoise_loop(_full_sd(), O.UNET_CONFIG_LARGE, O.DDPMOracle(**O.SD21_SCHEDULER), enc, mask, lat0.clone(), N,
                                                 3.0, noises=list(noises), prefix="unet.")
    ref = _cache[("lref", H)]
    sch = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in TI._DDPM_KEYS})
    sch.set_timesteps(N)
    e = _full_engine("fp16")

    def run(use_graph=True):
        lat = lat0.clone().cuda()
        e.denoise(lat, enc.cuda(), mask, sch.timesteps.numpy(), sch.coef_table(), 3.0, noise=noises.cuda(), use_graph=use_graph, latent_h=H)
        torch.cuda.synchronize()
        return lat.cpu(), e.last_step_gflop()

    with _dispatch(lib, e, big):
        shared, gf_shared = run()
        eager, _ = run(use_graph=False)
        with TI.tuning(lib, TANGO_NO_CFG_SHARED=1):
            plain, gf_plain = run()
    assert torch.equal(shared, eager), "hipGraph replay and eager launches must agree bit for bit"
    assert gf_shared < gf_plain, "the CFG-shared plan executes less work than the single-key plan"
    for what, got in (("CFG-shared", shared), ("single-key", plain)):
        err = (got - ref).abs().max().item()
        print("full-width 2-step CFG loop H=64 B=2 fp16, %s plan (%s dispatch): latents max abs err %.3e" % (what, "big-tile" if big else "product", err))
        assert err <= FULL_LOOP_TOL["fp16"], (what, err)


def test_full_width_forward_bf16_fp8_attention_h64(lib):
    enc, mask, x2, _, _ = _full_inputs(64, 1)
    ref = _full_fwd_ref(64)
    e = _full_engine("bf16", attn_fp8=True)
    out = e.unet_forward(x2.cuda(), T_FULL, enc.cuda(), mask.cuda(), latent_h=64).cpu()
    err = relerr(out, ref)
    print("full-width forward H=64 bf16 + fp8 P.V rel err %.3e" % err)
    assert torch.isfinite(out).all() and err <= FULL_FWD_TOL["bf16"]
    _cache.pop(("full", "bf16", (("attn_fp8", True),)), None)


# ---- 4. mel-VAE decoder / encoder, HiFi-GAN, mel front-end ---------------------------------------------------------------------------------------
def _vae_sd():
    if "vae_sd" not in _cache:
        shapes = W.vae_decoder_param_shapes(O.VAE_CONFIG)
        shapes.update(W.vae_encoder_param_shapes(O.VAE_CONFIG))
        shapes.update(W.hifigan_param_shapes(O.HIFIGAN_CONFIG))
        _cache["vae_sd"] = W.synth_state_dict(shapes, 1234)
    return _cache["vae_sd"]


def _vae_engine(dtype):
    if ("vae", dtype) not in _cache:
        e = Engine(vae=O.VAE_CONFIG, hifigan=O.HIFIGAN_CONFIG, dtype=dtype, vae_encoder=True)
        e.load_synthetic(1234)
        _cache[("vae", dtype)] = e
    return _cache[("vae", dtype)]


def _vae_ref(H):
    if ("vref", H) not in _cache:
        g = torch.Generator().manual_seed(3300 + H)
        z = torch.randn(2, 8, H, 16, generator=g) * 1.1
        mel_in = torch.randn(2, 1, 4 * H, 64, generator=g) * 2.0 - 4.0
        with torch.no_grad():
            mel = O.vae_decode_first_stage(_vae_sd(), O.VAE_CONFIG, z)
            wav = O.decode_to_waveform(_vae_sd(), O.HIFIGAN_CONFIG, mel)
            mom = O.vae_encode_moments(_vae_sd(), O.VAE_CONFIG, mel_in)
        _cache[("vref", H)] = (z, mel_in, mel, wav, mom)
    return _cache[("vref", H)]


# bounds of test_vae_and_vocoder_at_benchmarked_batch (decoder + vocoder end to end) and of test_vae_encoder (moments)
@pytest.mark.parametrize("dtype,mel_tol,lsb_frac,snr_floor,enc_tol", [("fp32", 1e-5, 0.999, 80.0, 1e-3), ("fp16", 1.0e-2, 0.0, 45.0, 3e-2)])
@pytest.mark.parametrize("H", [64, 192])
def test_vae_decoder_encoder_and_vocoder(lib, H, dtype, mel_tol, lsb_frac, snr_floor, enc_tol):
    z, mel_in, mel_ref, wav_ref, mom_ref = _vae_ref(H)
    frames = 4 * H
    samples = vocoder_samples(frames)
    assert (H, frames, samples) == duration_geometry(H / 64 * 2.5)
    e = _vae_engine(dtype)
    mel = e.vae_decode(z.cuda(), latent_h=H)
    wav = e.vocode(mel)
    mom = e.vae_encode(mel_in.cuda(), latent_h=H)
    torch.cuda.synchronize()
    mel, wav, mom = mel.cpu(), wav.cpu().numpy(), mom.cpu()
    assert mel.shape == (2, 1, frames, 64) == mel_ref.shape and wav.shape == (2, samples) == wav_ref.shape and wav.dtype == np.int16
    assert samples == e.vocoder_samples(frames) == vocoder_samples(frames)
    assert mom.shape == (2, 16, H, 16)
    merr = relerr(mel, mel_ref)
    d = np.abs(wav.astype(np.int32) - wav_ref.astype(np.int32))
    frac1 = float((d <= 1).mean())
    snr = 10 * np.log10((wav_ref.astype(np.float64) ** 2).mean() / ((d.astype(np.float64) ** 2).mean() + 1e-9))
    eerr = relerr(mom, mom_ref)
    print("H=%d %s: mel rel err %.3e, int16 |diff| max %d, <=1 LSB on %.5f, wave SNR %.1f dB, encoder moments rel err %.3e"
          % (H, dtype, merr, d.max(), frac1, snr, eerr))
    assert merr <= mel_tol and frac1 >= lsb_frac and snr >= snr_floor and eerr <= enc_tol
    # encode -> tango_op_latent_encode -> decode: the shapes of an edit's round trip at this height
    from tango_amd.autoencoder import AutoencoderKL
    vae = AutoencoderKL.__new__(AutoencoderKL)
    vae.engine, vae._device, vae.scale_factor, vae.embed_dim, vae.vae_cfg = e, torch.device("cuda:0"), O.VAE_CONFIG["scale_factor"], 8, O.VAE_CONFIG
    xt, z0 = vae.encode_start_latents(mom.cuda()[:1], 0.8, 0.6, 2, seed=5, want_clean=True)
    assert xt.shape == z0.shape == (2, 8, H, 16)
    assert vae.decode_first_stage(z0).shape == (2, 1, frames, 64)


def test_vae_fp32_at_20_s():
    """H = 512, one sample, fp32: the mid-block attention's softmax rows are 8192 fp32 columns, twice what the 10 s rows hold per thread
    (norm.hip softmax_rows_kernel's long form); decoder and encoder against the oracle at the bounds of the shorter clips"""
    H = 512
    g = torch.Generator().manual_seed(3300 + H)
    z = torch.randn(1, 8, H, 16, generator=g) * 1.1
    mel_in = torch.randn(1, 1, 4 * H, 64, generator=g) * 2.0 - 4.0
    with torch.no_grad():
        mel_ref = O.vae_decode_first_stage(_vae_sd(), O.VAE_CONFIG, z)
        mom_ref = O.vae_encode_moments(_vae_sd(), O.VAE_CONFIG, mel_in)
    e = _vae_engine("fp32")
    mel = e.vae_decode(z.cuda(), latent_h=H).cpu()
    mom = e.vae_encode(mel_in.cuda(), latent_h=H).cpu()
    merr, eerr = relerr(mel, mel_ref), relerr(mom, mom_ref)
    print("H=512 fp32: mel rel err %.3e, encoder moments rel err %.3e" % (merr, eerr))
    assert mel.shape == (1, 1, 2048, 64) and mom.shape == (1, 16, 512, 16)
    assert merr <= 1e-5 and eerr <= 1e-3
    h16 = _vae_engine("fp16").vae_decode(z.cuda(), latent_h=H).cpu()
    assert relerr(h16, mel_ref) <= 1.0e-2


@pytest.mark.parametrize("H", [64, 192])
def test_mel_front_end_at_the_matching_sample_count(H):
    from oracle import stft_oracle as S
    from oracle.make_golden import stft_wave
    from tango_amd.stft import wav_to_fbank
    stft = TI._tango().stft
    frames = 4 * H
    y = stft_wave(B=2, N=frames * 160, seed=H)
    mel, logmag, _ = stft.mel_spectrogram(y.cuda())
    assert mel.shape == (2, 64, frames + 1)
    m0, l0, _ = S.mel_spectrogram(y, stft.mel_basis, stft.stft_fn.forward_basis)
    g, r = mel.cpu().double().exp(), m0.double().exp()
    peak = r.amax(dim=(1, 2), keepdim=True)
    lin = ((g - r).abs() / peak).max().item()
    logerr = (mel.cpu().double() - m0.double()).abs()[r >= 1e-4 * peak].max().item()
    print("mel front-end, %d frames: linear err %.3e of the peak, log err above the floor %.3e" % (frames, lin, logerr))
    assert lin <= 2e-6 and logerr <= 5e-3                       # tests/test_stft_gpu.py _compare
    fbank, _, _ = wav_to_fbank(y.cuda(), frames, fn_STFT=stft)
    assert fbank.shape == (2, frames, 64) and torch.equal(fbank, mel.transpose(1, 2)[:, :frames])


# ---- 5. plan isolation -------------------------------------------------------------------------------------------------------------------------
def _fresh(dtype="fp32"):
    e = Engine(unet=O.UNET_CONFIG_TINY, dtype=dtype)
    e.load_synthetic(1234)
    return e


def test_heights_keep_plans_of_their_own():
    N = 3
    e = _fresh()
    i64, i256 = _loop_inputs(64), _loop_inputs(256)
    a = _run(e, "ddpm", N, i64, 64)
    assert e.plan_stats()[1] == 1
    b = _run(e, "ddpm", N, i256, 256)
    assert e.plan_stats()[1] == 2
    c = _run(e, "ddpm", N, i64, 64)
    assert e.plan_stats()[1] == 2, "the second H = 64 call reuses the first one's plan"
    assert torch.equal(a, c)
    alone = _run(_fresh(), "ddpm", N, i256, 256)
    assert torch.equal(b, alone), "an engine that has run another height computes the same bits at H = 256"
    enc, mask, lat0, *_ = i256
    sch = TI._sched("ddpm")
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, noise=i256[5][:N].cuda())   # latent_h omitted: the default
    assert torch.equal(lat.cpu(), b) and e.plan_stats()[1] == 2


def test_multistep_ring_grows_with_the_height_not_only_the_batch():
    """B = 2 at H = 64, then B = 1 at H = 512: fewer samples, four times the history elements"""
    N = 4
    e = _fresh()
    assert e.ring_elems() == 0
    _run(e, "dpmpp_2m", N, _loop_inputs(64), 64)
    assert e.ring_elems() == 3 * 2 * 8 * 64 * 16
    _run(e, "ddpm", N, _loop_inputs(192), 192)
    assert e.ring_elems() == 3 * 2 * 8 * 64 * 16, "only the multistep rule keeps a history"
    big = _loop_inputs(512, B=1, N=N)
    got = _run(e, "dpmpp_2m", N, big, 512)
    assert e.ring_elems() == 3 * 1 * 8 * 512 * 16, "the ring holds the call's 3 x B x C x H x W floats, whatever the batch was before"
    ref = _run(_fresh(), "dpmpp_2m", N, big, 512)
    assert torch.equal(got, ref)
    assert torch.equal(_run(e, "dpmpp_2m", N, _loop_inputs(64), 64), _run(_fresh(), "dpmpp_2m", N, _loop_inputs(64), 64))
    assert e.ring_elems() == 3 * 1 * 8 * 512 * 16                # a smaller call keeps the larger ring


# ---- 6. the public surface, on the synthetic Tango stack -----------------------------------------------------------------------------------------
class _Tok:
    """a whitespace tokenizer with the T5 convention (ids, then '</s>' = 1, then padding 0): "" is one token"""
    model_max_length = 16

    def __call__(self, prompts, max_length=None, padding=True, truncation=True, return_tensors="pt"):
        rows = [[2 + sum(map(ord, w)) % 90 for w in p.split()][:self.model_max_length - 1] + [1] for p in prompts]
        n = max_length if padding == "max_length" else max(len(r) for r in rows)
        ids, am = torch.zeros(len(rows), n, dtype=torch.long), torch.zeros(len(rows), n, dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r[:n])
            am[i, :len(r)] = 1
        return type("Batch", (), dict(input_ids=ids, attention_mask=am))()


class _Enc:
    def __init__(self, d):
        self.table = torch.randn(100, d, generator=torch.Generator().manual_seed(99)).cuda()

    def __call__(self, input_ids=None, attention_mask=None):
        return (self.table[input_ids],)


def _tango_text():
    if "tango" not in _cache:
        from tango_amd.models import AudioDiffusion
        from tango_amd.tango import Tango
        base = TI._tango()
        model = AudioDiffusion(unet_config=O.UNET_CONFIG_TINY, dtype="fp16", tokenizer=_Tok(), text_encoder=_Enc(O.UNET_CONFIG_TINY["cross_attention_dim"]))
        model.engine.load_synthetic(1234)
        _cache["tango"] = Tango.from_components(model, base.vae, stft=base.stft)
    return _cache["tango"]


def test_generate_duration_equals_the_hand_composed_chain():
    t = _tango_text()
    H, frames, samples = duration_geometry(2.5)
    torch.manual_seed(21)
    w = t.generate("rain on a tin roof", steps=3, guidance=3, duration=2.5)
    assert w.dtype == np.int16 and w.shape == (samples,) == (t.vae.engine.vocoder_samples(256),)
    torch.manual_seed(21)
    pe, pm, host = t.model._encode_text_classifier_free(["rain on a tin roof"], 1)
    lat = t.model.prepare_latents(1, t.scheduler, 8, torch.float32, t.model.device, latent_h=H)
    assert lat.shape == (1, 8, 64, 16)
    lat = t.model.inference_from_embeddings(pe.float(), pm, t.scheduler, 3, 3, latents=lat, mask_host=host)
    mel = t.vae.decode_first_stage(lat)
    assert mel.shape == (1, 1, frames, 64)
    assert np.array_equal(w, t.vae.decode_to_waveform(mel)[0])
    assert np.abs(w.astype(np.float32)).max() > 0


def test_default_call_is_the_10_s_call():
    t = _tango_text()
    torch.manual_seed(4)
    a = t.generate("a dog barks", steps=2)
    torch.manual_seed(4)
    b = t.generate("a dog barks", steps=2, duration=10)
    assert a.shape == (163872,) and np.array_equal(a, b)


def test_generate_for_batch_duration_lengths():
    t = _tango_text()
    n = duration_geometry(5)[2]
    outs = t.generate_for_batch(["a dog barks", "rain", "wind in the trees"], steps=2, guidance=3, samples=1, batch_size=2, duration=5)
    assert len(outs) == 3 and all(o.shape == (n,) and o.dtype == np.int16 for o in outs)
    groups = t.generate_for_batch(["rain"], steps=2, samples=2, duration=5)
    assert len(groups) == 1 and len(groups[0]) == 2 and groups[0][0].shape == (n,)
    enc, mask, *_ = _loop_inputs(64)
    w = t.generate_from_embeddings(enc.cuda(), mask.cuda(), steps=2, guidance=3, duration=5)
    assert w.shape == (2, n)


def test_inpaint_and_edit_fit_a_3_s_clip_into_5_s():
    t = _tango_text()
    audio = TI._clip()                                           # 3 s at 16 kHz
    n = duration_geometry(5)[2]
    assert t.encode_audio(audio, None).shape == (1, 8, 128, 16) and t.encode_moments(audio, None).shape == (1, 16, 128, 16)
    assert t.encode_audio(audio).shape == (1, 8, 256, 16)       # the default stays 10 s
    w = t.inpaint("rain", audio, steps=3, guidance=3, samples=2, duration=None)
    assert w.dtype == np.int16 and w.shape == (2, n)
    v = t.edit("rain", audio, strength=0.5, steps=4, guidance=3, samples=1, seed=7, duration=None)
    assert v.shape == (1, n)
    assert np.array_equal(v, t.edit("rain", audio, strength=0.5, steps=4, guidance=3, samples=1, seed=7, duration=5))
    # the hand-composed chain of the fitted inpaint, bit for bit
    enc, mask, *_ = _loop_inputs(64)
    torch.manual_seed(11)
    w1 = t.inpaint_from_embeddings(enc.cuda(), mask.cuda(), audio, steps=3, guidance=3, samples=2, seed=7, duration=None)
    torch.manual_seed(11)
    from tango_amd.stft import wav_to_fbank
    fbank, _, _ = wav_to_fbank(prepare_waveform(audio, duration=None)[None].cuda(), 512, fn_STFT=t.stft)
    z = t.vae.get_first_stage_encoding(t.vae.encode_first_stage(fbank.unsqueeze(1)))
    lat = t.model.inpaint_from_embeddings(enc.cuda(), mask.cuda(), t.scheduler, 3, 3, known_latents=z.repeat_interleave(2, 0),
                                          latent_mask=latent_mask(2, h=128), seed=7)
    assert np.array_equal(w1, t.vae.decode_to_waveform(t.vae.decode_first_stage(lat)))


def test_off_grid_durations_and_heights_raise():
    t = _tango_text()
    with pytest.raises(ValueError, match="2.5 and 5"):
        t.generate("rain", steps=2, duration=3)
    with pytest.raises(ValueError):
        t.generate_for_batch(["rain"], steps=2, duration=22.5)
    with pytest.raises(ValueError):
        t.inpaint("rain", TI._clip(), steps=2, duration=3)
    enc, mask, *_ = _loop_inputs(64)
    bad = torch.randn(2, 8, 100, 16)
    with pytest.raises(ValueError, match="64 and 128"):
        t.model.inference_from_embeddings(enc.cuda(), mask.cuda(), t.scheduler, 2, 3, latents=bad)
    with pytest.raises(ValueError):
        t.vae.decode_first_stage(bad.cuda())
    e = t.model.engine
    with pytest.raises(ValueError):
        e.unet_forward(bad.cuda(), 5, enc.cuda(), mask.cuda(), latent_h=100)
    with pytest.raises(ValueError):
        e.unet_forward(torch.randn(4, 8, 128, 16).cuda(), 5, enc.cuda(), mask.cuda(), latent_h=64)     # the tensor is not the stated height
    # the C ABI refuses what the UNet's levels cannot halve (the Python grid is stricter)
    import ctypes as C
    x = torch.randn(4, 8, 96, 16).cuda()
    out = torch.empty_like(x)
    rc = e.lib.tango_engine_unet_forward_h(e._h, C.c_void_p(x.data_ptr()), 5, C.c_void_p(enc.cuda().data_ptr()), None,
                                           C.c_void_p(out.data_ptr()), 4, enc.shape[1], 96, None)
    assert rc != 0 and b"multiple of 64" in e.lib.tango_last_error()
