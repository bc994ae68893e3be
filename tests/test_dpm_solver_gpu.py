"""Multistep DPM-Solver / DPM-Solver++ on the engine (rule 2, sched_multistep_kernel): the fused step bit for bit against the torch
`step()` of tango_amd.scheduler.DPMSolverMultistepScheduler (itself pinned bit for bit to the fork's scheduler by
tests/test_dpm_solver_host.py), the tiny-UNet loop against the fp32 oracle, graph replay, state isolation from the DDPM rule and
the public entry points."""
import contextlib
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd import weights as W  # noqa: E402
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDPMScheduler, DPMSolverMultistepScheduler, from_diffusers  # noqa: E402

SD21 = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
_DDPM_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}
_cache = {}


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


# ---- op level: the fused step == torch step(), bitwise, step after step ------------------------------------------------------------
_GRID = list(itertools.product(["dpmsolver++", "dpmsolver"], ["midpoint", "heun"], [1, 2, 3], ["epsilon", "sample", "v_prediction"]))


@pytest.mark.parametrize("algo,solver,order,pred", _GRID)
@pytest.mark.parametrize("N,cfg_on", [(10, True), (20, False)])
def test_op_multistep_bitwise(lib, algo, solver, order, pred, N, cfg_on):
    B, Cc, HW = 3, 8, 4096
    sch = DPMSolverMultistepScheduler(**SD21, solver_order=order, prediction_type=pred, algorithm_type=algo, solver_type=solver)
    sch.set_timesteps(N)
    coef = sch.coef_table()
    g = torch.Generator().manual_seed(7 + order)
    lat = torch.randn(B, Cc, 256, 16, generator=g)
    lat_d = lat.clone().cuda()
    ring = torch.zeros(3, B, Cc, HW, device="cuda")
    B2 = 2 * B if cfg_on else B
    for i, t in enumerate(sch.timesteps):
        mo = torch.randn(B2, Cc, 256, 16, generator=g)
        guided = mo.chunk(2)[0] + 3.0 * (mo.chunk(2)[1] - mo.chunk(2)[0]) if cfg_on else mo
        lat = sch.step(guided, t, lat).prev_sample
        mo_d = mo.cuda()
        rc = lib.tango_op_sched_multistep(C.c_void_p(lat_d.data_ptr()), C.c_void_p(mo_d.data_ptr()), C.c_void_p(ring.data_ptr()),
                                          coef.ctypes.data_as(C.c_void_p), i, B, Cc, HW, 1 if cfg_on else 0, 3.0, PRED[pred],
                                          0 if algo == "dpmsolver++" else 1, None)
        assert rc == 0, lib.tango_last_error().decode()
        got = lat_d.cpu()
        assert torch.equal(got, lat), "step %d (t=%d, order %d): max diff %g" % (i, int(t), int(coef[i, 10]), (got - lat).abs().max())


# ---- loop vs oracle ---------------------------------------------------------------------------------------------------------------
def _inputs(B=2, L=9, seed=31):
    cfg = O.UNET_CONFIG_TINY
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(2 * B, L, cfg["cross_attention_dim"], generator=g)
    mask = torch.ones(2 * B, L, dtype=torch.bool)
    mask[0, 1:] = False
    mask[2, L // 2:] = False
    lat0 = torch.randn(B, 8, 256, 16, generator=g)
    return enc, mask, lat0


class _OracleAdapter:
    """O.denoise_loop calls step(out, t, latents, noise=...) and takes the latents back"""

    def __init__(self, sch):
        self.s = sch

    def __getattr__(self, k):
        return getattr(self.s, k)

    def step(self, out, t, lat, noise=None):
        return self.s.step(out, t, lat).prev_sample


def _oracle(kw, N, enc, mask, lat0):
    key = (tuple(sorted(kw.items())), N)
    if key not in _cache:
        sch = DPMSolverMultistepScheduler(**kw)
        _cache[key] = O.denoise_loop(unet_sd(), O.UNET_CONFIG_TINY, _OracleAdapter(sch), enc, mask, lat0.clone(), N, 3.0, prefix="unet.")
    return _cache[key]


def _engine_run(e, sch, N, enc, mask, lat0, use_graph=True):
    sch.set_timesteps(N)
    lat = lat0.clone().cuda()
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type=sch.config.prediction_type,
              rule=sch.rule, use_graph=use_graph)
    torch.cuda.synchronize()
    return lat.cpu()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("N", [10, 20])
def test_dpmpp_2m_loop_vs_oracle(lib, dtype, N):
    kw = dict(SD21, solver_order=2, prediction_type="v_prediction", algorithm_type="dpmsolver++")
    enc, mask, lat0 = _inputs()
    ref = _oracle(kw, N, enc, mask, lat0)
    e = unet_engine(dtype)
    g = _engine_run(e, DPMSolverMultistepScheduler(**kw), N, enc, mask, lat0, use_graph=True)
    x = _engine_run(e, DPMSolverMultistepScheduler(**kw), N, enc, mask, lat0, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    with tuning(lib, TANGO_GRAPH_STEPS=3):     # k-step replays (+ the one-step graph for the remainder)
        k = _engine_run(e, DPMSolverMultistepScheduler(**kw), N, enc, mask, lat0, use_graph=True)
    assert torch.equal(g, k), "the k-step graph must equal the one-step graph"
    err = (g - ref).abs().max().item()
    print("DPM++ 2M N=%d %s max abs err %.3e (|ref| max %.2f)" % (N, dtype, err, ref.abs().max()))
    assert err <= (1e-2 if dtype == "fp32" else 1e-1)


@pytest.mark.parametrize("algo,order", [("dpmsolver++", 3), ("dpmsolver", 2), ("dpmsolver", 3)])
def test_multistep_variants_loop_vs_oracle(lib, algo, order):
    kw = dict(SD21, solver_order=order, prediction_type="v_prediction", algorithm_type=algo)
    enc, mask, lat0 = _inputs()
    ref = _oracle(kw, 10, enc, mask, lat0)
    got = _engine_run(unet_engine("fp32"), DPMSolverMultistepScheduler(**kw), 10, enc, mask, lat0)
    err = (got - ref).abs().max().item()
    print("%s order %d max abs err %.3e" % (algo, order, err))
    assert err <= 1e-2


def test_state_isolation_ddpm_dpm_ddpm(lib):
    """the multistep rule's graphs, table width and history ring leave a DDPM call on the same engine and plan unchanged"""
    e = unet_engine("fp32")
    enc, mask, lat0 = _inputs()
    ddpm = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    dpm = DPMSolverMultistepScheduler.from_config(ddpm.config)

    def run_ddpm():
        ddpm.set_timesteps(5)
        lat = lat0.clone().cuda()
        e.denoise(lat, enc.cuda(), mask.cuda(), ddpm.timesteps.numpy(), ddpm.coef_table(), 3.0, prediction_type="v_prediction",
                  rule="ddpm", seed=99)
        torch.cuda.synchronize()
        return lat.cpu()

    a = run_ddpm()
    d1 = _engine_run(e, dpm, 6, enc, mask, lat0)
    b = run_ddpm()
    d2 = _engine_run(e, dpm, 6, enc, mask, lat0)
    assert torch.equal(a, b)
    assert torch.equal(d1, d2)
    assert not torch.equal(a, d1)


def test_multistep_argument_errors(lib):
    e = unet_engine("fp32")
    enc, mask, lat0 = _inputs()
    sch = DPMSolverMultistepScheduler(**SD21, prediction_type="v_prediction")
    sch.set_timesteps(4)
    lat = lat0.clone().cuda()
    with pytest.raises(ValueError):
        e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type="v_prediction",
                  rule="dpmsolver", noise=torch.zeros(4, *lat0.shape, device="cuda"))
    with pytest.raises(ValueError):
        e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type="v_prediction",
                  rule="dpmsolver", clip_sample=True)
    with pytest.raises(ValueError):     # an [N, 8] table with the multistep rule
        e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table()[:, :8], 3.0, rule="dpmsolver")


# ---- public surface ---------------------------------------------------------------------------------------------------------------
class DPMSolverMultistepSchedulerStandIn:
    """a diffusers-style scheduler object: only its class name and `config` mapping matter to from_diffusers"""
    order = 1

    def __init__(self, **config):
        self.config = dict(config)


DPMSolverMultistepSchedulerStandIn.__name__ = "DPMSolverMultistepScheduler"


def _audio_diffusion():
    if "ad" not in _cache:
        from tango_amd.models import AudioDiffusion
        ad = AudioDiffusion(unet_config=O.UNET_CONFIG_TINY, dtype="fp32")
        ad.engine.load_synthetic(1234)
        _cache["ad"] = ad
    return _cache["ad"]


def test_inference_from_embeddings_from_diffusers(lib):
    """a diffusers-style scheduler object goes through from_diffusers() and runs exactly the native class's loop"""
    ad = _audio_diffusion()
    enc, mask, lat0 = _inputs()
    kw = dict(SD21, prediction_type="v_prediction", solver_order=2, algorithm_type="dpmsolver++", _class_name="x", thresholding=False)
    outs = []
    for sch in (DPMSolverMultistepSchedulerStandIn(**kw), DPMSolverMultistepScheduler.from_config(kw)):
        outs.append(ad.inference_from_embeddings(enc.cuda(), mask.cuda(), sch, 8, 3.0, latents=lat0.clone()).cpu())
    assert torch.equal(outs[0], outs[1])
    ref = _oracle(dict(SD21, prediction_type="v_prediction", solver_order=2, algorithm_type="dpmsolver++"), 8, enc, mask, lat0)
    assert (outs[0] - ref).abs().max().item() <= 1e-2
    assert isinstance(from_diffusers(DPMSolverMultistepSchedulerStandIn(**kw)), DPMSolverMultistepScheduler)


def test_tango_swapped_scheduler_generates(lib):
    """the diffusers idiom `tango.scheduler = DPMSolverMultistepScheduler.from_config(tango.scheduler.config)` on the SD-2.1 DDPM
    config, then the generate path (text-encoder outputs given: there is no T5 checkpoint here): tiny UNet + full VAE / vocoder"""
    from tango_amd.autoencoder import AutoencoderKL
    from tango_amd.models import AudioDiffusion
    from tango_amd.tango import Tango
    model = AudioDiffusion(unet_config=O.UNET_CONFIG_TINY, dtype="fp16")
    model.engine.load_synthetic(1234)
    vae = AutoencoderKL(ddconfig=dict(O.VAE_CONFIG, resolution=256, in_channels=1, double_z=True, attn_resolutions=[], dropout=0.0),
                        embed_dim=8, scale_factor=O.VAE_CONFIG["scale_factor"], dtype="fp16")
    vae.engine.load_synthetic(1234)
    t = Tango.from_components(model, vae)
    t.scheduler = DPMSolverMultistepScheduler.from_config(t.scheduler.config)
    assert t.scheduler.config.prediction_type == "v_prediction" and t.scheduler.config.beta_schedule == "scaled_linear"
    enc, mask, _ = _inputs()
    w1 = t.generate_from_embeddings(enc.cuda(), mask.cuda(), steps=5, guidance=3, seed=7, latents=torch.randn(2, 8, 256, 16))
    assert w1.dtype == np.int16 and w1.shape == (2, 163872)
    assert np.abs(w1.astype(np.float32)).max() > 0


def test_music_inference_dpm(lib):
    """MusicAudioDiffusion.inference_from_embeddings with a 5-step DPM-Solver++ loop vs the oracle"""
    from oracle.make_golden import music_inputs
    from tango_amd.models import MusicAudioDiffusion
    cfg = O.UNET_CONFIG_MUSIC_TINY
    m = MusicAudioDiffusion(unet_config=cfg, dtype="fp32")
    sd = W.synth_state_dict(W.unet_param_shapes(cfg), 1234)
    m.load_state_dict({"unet." + k: v for k, v in sd.items()})
    B, N = 2, 5
    _, enc, beat, chord, em, bm, cm = music_inputs(cfg, 2 * B, 11)
    lat0 = torch.randn(B, 8, 256, 16, generator=torch.Generator().manual_seed(12))
    kw = dict(SD21, prediction_type="v_prediction", solver_order=2, algorithm_type="dpmsolver++")
    got = m.inference_from_embeddings(enc, em, DPMSolverMultistepScheduler(**kw), N, 3.0, latents=lat0, encoded_beats=beat,
                                      beat_mask=bm, encoded_chords=chord, chord_mask=cm).cpu()
    with torch.no_grad():
        ref = O.denoise_loop(sd, cfg, _OracleAdapter(DPMSolverMultistepScheduler(**kw)), enc, em, lat0.clone(), N, 3.0,
                             music=dict(beat_features=beat, chord_features=chord, beat_attention_mask=bm, chord_attention_mask=cm))
    err = (got - ref).abs().max().item()
    print("Music DPM++ 5 steps max abs err %.3e" % err)
    assert err <= 1e-2
