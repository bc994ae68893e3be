"""Generate tests/golden/* from the REAL reference modules (runs only in the build container, where
/root/reference exists).  TEST INFRASTRUCTURE.  Usage:  python oracle/make_golden.py

Every fixture is produced by importing the reference's own code (oracle/ref_import.py):
  scheduler_sd21.json  fork DDPMScheduler / DDIMScheduler tables for the SD-2.1 config
  kat_blocks.npz       the fork's block/layer known-answer tests re-run here
                       (mustango/diffusers/tests/test_unet_2d_blocks.py:23-30,50-61,168-179,200-210,226-241;
                        tests/test_layers_utils.py:225-239,395-418): default-init state_dicts + the
                        hard-coded expected slices, asserted green before saving
  unet_ref.npz         fork UNet2DConditionModel (tiny + full Tango config) loaded with the seeded synthetic
                       weights of tango_amd.weights: output slices + checksums (masked cross-attention path,
                       which no fork KAT covers)
  loop_ref.npz         models.py:224-249 loop (fork UNet + fork DDPMScheduler, global-RNG draws), 3 steps
  vae_voc_ref.npz      reference AutoencoderKL.decode_first_stage / decode_to_waveform outputs
  vae_enc_ref.npz      reference AutoencoderKL.encode_first_stage / get_first_stage_encoding outputs
  music_unet_ref.npz   Mustango UNet2DConditionModelMusic.forward (unet_2d_condition_music.py:536-757) output slices, tiny widths
  stft_ref.npz         reference TacotronSTFT.mel_spectrogram (audioldm/audio/stft.py:164-186) outputs on a seeded test signal
                       (librosa stubbed by oracle/stft_oracle.py's restatements: pins everything downstream of the filterbank)
  reference_diff.json / reference_diff.npz
                       what tests/test_reference_diff.py and the stft "live" test compare against: the reference's state-dict
                       inventories, SHA-256 digests of the tensors they check bit for bit (fork DDPMScheduler.step, the STFT
                       bases) and, for the outputs they check to a tolerance (tiny UNet with a ragged mask, tiny Music UNet, STFT),
                       a fixed sample of elements (see sample_fixture) with the full tensor's checksum and max |x|
Inputs are re-derived from seeds by the tests; only small slices / checksums / tiny state_dicts are stored.
"""
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import as R  # noqa: E402
from oracle import tango_oracle as O  # noqa: E402
from tango_amd import weights as W  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)


def checksum(t):
    a = t.detach().double()
    return [float(a.sum()), float(a.abs().sum()), float((a * a).sum())]


def sched_golden():
    D, I = R.ddpm_cls(), R.ddim_cls()
    cfg = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
               prediction_type="v_prediction", clip_sample=False, variance_type="fixed_small")
    out = {"config": cfg, "timesteps": {}, "coef": {}}
    for n in (200, 100, 10, 1000, 7):
        s = D(**cfg)
        s.set_timesteps(n)
        out["timesteps"][str(n)] = s.timesteps.tolist()
        rows = {}
        for t in sorted(set([s.timesteps[0].item(), s.timesteps[len(s.timesteps) // 2].item(), s.timesteps[-2].item(), 0])):
            prev_t = t - 1000 // n
            a_t = s.alphas_cumprod[t]
            a_prev = s.alphas_cumprod[prev_t] if prev_t >= 0 else s.one
            b_t, b_prev = 1 - a_t, 1 - a_prev
            cur_a = a_t / a_prev
            cur_b = 1 - cur_a
            rows[str(t)] = [float(a_t ** 0.5), float(b_t ** 0.5), float((a_prev ** 0.5 * cur_b) / b_t),
                            float(cur_a ** 0.5 * b_prev / b_t), float(s._get_variance(t) ** 0.5) if t > 0 else 0.0]
        out["coef"][str(n)] = rows
    s = D(**cfg)
    out["betas"] = [float(s.betas[0]), float(s.betas[999])]
    out["alphas_cumprod"] = {str(i): float(s.alphas_cumprod[i]) for i in (0, 5, 495, 990, 995, 999)}
    dd = I(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", clip_sample=True, steps_offset=1)
    dd.set_timesteps(5)
    out["ddim_offset1_5"] = dd.timesteps.tolist()
    json.dump(out, open(os.path.join(OUT, "scheduler_sd21.json"), "w"), indent=0)
    print("scheduler_sd21.json")


def kat_golden():
    B = R.unet_blocks()
    R._setup()
    from diffusers.models.resnet import ResnetBlock2D
    from diffusers.models.transformer_2d import Transformer2DModel
    store = {}

    def save_sd(prefix, m):
        for k, v in m.state_dict().items():
            store[prefix + "/" + k] = v.numpy().copy()

    def block(name, cls, btype, expected, cross=False, extra=None):
        # harness: tests/test_unet_blocks_common.py:41-105 (seed 0 -> inputs, then module construction)
        torch.manual_seed(0)
        hs = torch.randn(4, 32, 32, 32)
        temb = torch.randn(4, 128)
        kw = dict(in_channels=32, out_channels=32, temb_channels=128)
        if btype == "up":
            kw["prev_output_channel"] = 32
        if btype == "mid":
            kw.pop("out_channels")
        if cross:
            kw["cross_attention_dim"] = 32
        if extra:
            kw.update(extra)
        inputs = dict(hidden_states=hs, temb=temb)
        if btype == "up":
            torch.manual_seed(1)
            inputs["res_hidden_states_tuple"] = (torch.randn(4, 32, 32, 32),)
        # NB: the fork's cross-attention block KATs pass NO encoder_hidden_states (dummy_input is not
        # overridden, tests/test_unet_2d_blocks.py:50-61,168-179,226-241): attn2 attends to the hidden states
        enc = None
        m = cls(**kw).eval()
        out = m(**inputs)
        if isinstance(out, tuple):
            out = out[0]
        sl = out[0, -1, -3:, -3:].flatten()
        exp = torch.tensor(expected)
        assert torch.allclose(sl, exp, atol=5e-3), (name, sl, exp)
        save_sd(name, m)
        store[name + "/expected_slice"] = np.asarray(expected, np.float32)
        store[name + "/out_slice"] = sl.numpy()
        store[name + "/out_checksum"] = np.asarray(checksum(out))
        if enc is not None:
            store[name + "/enc"] = enc.numpy()
        print("KAT green:", name)

    block("DownBlock2D", B.DownBlock2D, "down", [-0.0232, -0.9869, 0.8054, -0.0637, -0.1688, -1.4264, 0.4470, -1.3394, 0.0904])
    block("CrossAttnDownBlock2D", B.CrossAttnDownBlock2D, "down",
          [0.2440, -0.6953, -0.2140, -0.3874, 0.1966, 1.2077, 0.0441, -0.7718, 0.2800], cross=True)
    block("UNetMidBlock2DCrossAttn", B.UNetMidBlock2DCrossAttn, "mid",
          [0.1879, 2.2653, 0.5987, 1.1568, -0.8454, -1.6109, -0.8919, 0.8306, 1.6758], cross=True)
    block("UpBlock2D", B.UpBlock2D, "up", [-0.2041, -0.4165, -0.3022, 0.0041, -0.6628, -0.7053, 0.1928, -0.0325, 0.0523])
    block("CrossAttnUpBlock2D", B.CrossAttnUpBlock2D, "up",
          [-0.2796, -0.4364, -0.1067, -0.2693, 0.1894, 0.3869, -0.3470, 0.4584, 0.5091], cross=True)

    # tests/test_layers_utils.py:225-239
    torch.manual_seed(0)
    sample = torch.randn(1, 32, 64, 64)
    temb = torch.randn(1, 128)
    rb = ResnetBlock2D(in_channels=32, temb_channels=128).eval()
    out = rb(sample, temb)
    exp = [-1.9010, -0.2974, -0.8245, -1.3533, 0.8742, -0.9645, -2.0584, 1.3387, -0.4746]
    assert torch.allclose(out[0, -1, -3:, -3:].flatten(), torch.tensor(exp), atol=1e-3)
    save_sd("ResnetBlock2D", rb)
    store["ResnetBlock2D/expected_slice"] = np.asarray(exp, np.float32)
    store["ResnetBlock2D/out_checksum"] = np.asarray(checksum(out))
    print("KAT green: ResnetBlock2D")
    # tests/test_layers_utils.py:395-418
    torch.manual_seed(0)
    sample = torch.randn(1, 64, 64, 64)
    st = Transformer2DModel(in_channels=64, num_attention_heads=2, attention_head_dim=32, dropout=0.0, cross_attention_dim=64).eval()
    context = torch.randn(1, 4, 64)
    out = st(sample, context).sample
    exp = [-0.2555, -0.8877, -2.4739, -2.2251, 1.2714, 0.0807, -0.4161, -1.6408, -0.0471]
    assert torch.allclose(out[0, -1, -3:, -3:].flatten(), torch.tensor(exp), atol=1e-3)
    save_sd("Transformer2DModel", st)
    store["Transformer2DModel/expected_slice"] = np.asarray(exp, np.float32)
    store["Transformer2DModel/context"] = context.numpy()
    store["Transformer2DModel/out_checksum"] = np.asarray(checksum(out))
    print("KAT green: Transformer2DModel")
    np.savez_compressed(os.path.join(OUT, "kat_blocks.npz"), **store)


def unet_inputs(cfg, B2, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B2, 8, 256, 16, generator=g)
    enc = torch.randn(B2, L, cfg["cross_attention_dim"], generator=g)
    mask = torch.ones(B2, L, dtype=torch.bool)
    mask[0, 1:] = False
    if B2 > 2:
        mask[2, L // 2:] = False
    return x, enc, mask


def ref_unet(cfgo):
    cfg = dict(R.unet_config())
    cfg.update({k: cfgo[k] for k in ("block_out_channels", "attention_head_dim", "cross_attention_dim")})
    unet = R.unet_cls()(**cfg).eval()
    unet.load_state_dict(W.synth_state_dict(W.unet_param_shapes(cfgo), 1234))
    return unet


def unet_golden():
    store = {}
    for name, cfgo, B2, L, t in (("tiny", O.UNET_CONFIG_TINY, 4, 13, 801), ("large", O.UNET_CONFIG_LARGE, 2, 64, 995)):
        unet = ref_unet(cfgo)
        x, enc, mask = unet_inputs(cfgo, B2, L, 100 + B2)
        out = unet(x, torch.tensor(t), encoder_hidden_states=enc, encoder_attention_mask=mask).sample
        store[name + "/slice"] = out[:, :, ::37, ::5].numpy().copy()
        store[name + "/checksum"] = np.asarray(checksum(out))
        store[name + "/meta"] = np.asarray([B2, L, t, 100 + B2])
        print("unet", name, checksum(out))
        if name == "tiny":
            # models.py:224-249 with the fork scheduler and the global torch RNG, 3 steps, guidance 3
            sch = R.ddpm_cls()(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                               prediction_type="v_prediction", clip_sample=False, variance_type="fixed_small")
            torch.manual_seed(77)
            sch.set_timesteps(3)
            B = 2
            _, enc2, mask2 = unet_inputs(cfgo, 2 * B, 9, 31)
            lat = torch.randn(B, 8, 256, 16) * sch.init_noise_sigma
            for tt in sch.timesteps:
                inp = sch.scale_model_input(torch.cat([lat] * 2), tt)
                npred = unet(inp, tt, encoder_hidden_states=enc2, encoder_attention_mask=mask2).sample
                u, c = npred.chunk(2)
                npred = u + 3.0 * (c - u)
                lat = sch.step(npred, tt, lat).prev_sample
            np.savez_compressed(os.path.join(OUT, "loop_ref.npz"), slice=lat[:, :, ::37, ::5].numpy().copy(),
                                checksum=np.asarray(checksum(lat)), meta=np.asarray([B, 9, 3, 77, 31]))
            print("loop", checksum(lat))
        del unet
    np.savez_compressed(os.path.join(OUT, "unet_ref.npz"), **store)


def vae_golden():
    vae = R.autoencoder_cls()(**R.vae_config()).eval()
    shapes = W.vae_decoder_param_shapes(O.VAE_CONFIG)
    shapes.update(W.hifigan_param_shapes(O.HIFIGAN_CONFIG))
    vae.load_state_dict(W.synth_state_dict(shapes, 1234), strict=False)
    g = torch.Generator().manual_seed(41)
    z = torch.randn(2, 8, 256, 16, generator=g)
    mel = vae.decode_first_stage(z)
    wav = vae.decode_to_waveform(mel)
    assert wav.dtype == np.int16 and wav.shape == (2, 163872)
    np.savez_compressed(os.path.join(OUT, "vae_voc_ref.npz"), mel_slice=mel[:, 0, ::41, ::3].numpy().copy(),
                        mel_checksum=np.asarray(checksum(mel)), wav_head=wav[:, :4096].copy(), wav_tail=wav[:, -4096:].copy(),
                        wav_crc=np.asarray([zlib.crc32(wav.tobytes())], dtype=np.int64),
                        wav_abs_sum=np.asarray([np.abs(wav.astype(np.int64)).sum()]))
    print("vae/voc", checksum(mel), zlib.crc32(wav.tobytes()))


def vae_enc_golden():
    """reference AutoencoderKL.encode / get_first_stage_encoding (autoencoder.py:52-58,126-135) on a synthetic mel"""
    vae = R.autoencoder_cls()(**R.vae_config()).eval()
    shapes = W.vae_encoder_param_shapes(O.VAE_CONFIG)
    vae.load_state_dict(W.synth_state_dict(shapes, 4321), strict=False)
    g = torch.Generator().manual_seed(43)
    mel = torch.randn(2, 1, 1024, 64, generator=g) * 2.0 - 4.0          # log-mel-like range
    with torch.no_grad():
        post = vae.encode_first_stage(mel)
        torch.manual_seed(5)
        z = vae.get_first_stage_encoding(post)                           # draws randn(mean.shape) from the global generator
    mom = post.parameters
    assert mom.shape == (2, 16, 256, 16) and z.shape == (2, 8, 256, 16)
    np.savez_compressed(os.path.join(OUT, "vae_enc_ref.npz"), mom_slice=mom[:, :, ::17, ::3].numpy().copy(),
                        mom_checksum=np.asarray(checksum(mom)), z_slice=z[:, :, ::17, ::3].numpy().copy(),
                        z_checksum=np.asarray(checksum(z)))
    print("vae enc", checksum(mom), checksum(z))


def music_inputs(cfg, B2, seed, L=9, Lb=50, Lc=20):
    """seeded Music-UNet inputs (re-derived by the tests): ragged text mask, uncond rows with ALL beat / chord tokens masked
    (what the empty uncond beat / chord lists tokenise to, mustango/models.py:664-676,713-727), ragged cond rows"""
    g = torch.Generator().manual_seed(seed)
    d = cfg["cross_attention_dim"]
    x = torch.randn(B2, 8, 256, 16, generator=g)
    enc, beat, chord = torch.randn(B2, L, d, generator=g), torch.randn(B2, Lb, d, generator=g), torch.randn(B2, Lc, d, generator=g)
    em, bm, cm = torch.ones(B2, L, dtype=torch.bool), torch.ones(B2, Lb, dtype=torch.bool), torch.ones(B2, Lc, dtype=torch.bool)
    h = B2 // 2
    em[:h, 1:] = False
    bm[:h] = False
    cm[:h] = False
    bm[h:, 17:] = False
    cm[h:, 5:] = False
    return x, enc, beat, chord, em, bm, cm


def music_golden():
    """Mustango's UNet2DConditionModelMusic (unet_2d_condition_music.py:536-757) with the seeded synthetic weights, tiny widths"""
    cfgo = O.UNET_CONFIG_MUSIC_TINY
    cfg = json.load(open(os.path.join(R.REF, "mustango", "configs", "music_diffusion_model_config.json")))
    cfg = {k: v for k, v in cfg.items() if not k.startswith("_")}
    cfg.update({k: cfgo[k] for k in ("block_out_channels", "attention_head_dim", "cross_attention_dim")})
    unet = R.unet_music_cls()(**cfg).eval()
    unet.load_state_dict(W.synth_state_dict(W.unet_param_shapes(cfgo), 1234))
    x, enc, beat, chord, em, bm, cm = music_inputs(cfgo, 4, 3)
    out = unet(x, torch.tensor(801), encoder_hidden_states=enc, beat_features=beat, chord_features=chord, encoder_attention_mask=em,
               beat_attention_mask=bm, chord_attention_mask=cm).sample
    np.savez_compressed(os.path.join(OUT, "music_unet_ref.npz"), out_slice=out[:, :, ::9, ::3].numpy().copy(),
                        out_checksum=np.asarray(checksum(out)), n_tensors=np.asarray(len(unet.state_dict())))
    print("music unet", checksum(out))


def stft_wave(B=2, N=20000, seed=1):
    """deterministic test signal for the mel front-end: two partials + noise, a quiet stretch and a full-scale click (re-derived by the tests)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(N, dtype=torch.float64) / 16000.0
    y = 0.4 * torch.sin(2 * np.pi * 440 * t) + 0.2 * torch.sin(2 * np.pi * 3000 * t + 1) + 0.05 * torch.randn(N, generator=g, dtype=torch.float64)
    y[N // 2:N // 2 + 2000] *= 1e-4          # near-silence: exercises the 1e-5 clamp
    y[777] = 1.0
    y = y.clamp(-1, 1).float()
    return torch.stack([torch.roll(y, 777 * b) * (0.5 ** b) for b in range(B)])


def stft_golden():
    """reference TacotronSTFT (audioldm/audio/stft.py:136-186, librosa stubbed: oracle/ref_import.py tacotron_stft_cls) on stft_wave()"""
    from oracle import stft_oracle as S
    ref = R.tacotron_stft_cls()(**S.AUDIOLDM_STFT_CONFIG).eval()
    y = stft_wave()
    mel, logmag, energy = ref.mel_spectrogram(y)
    np.savez_compressed(os.path.join(OUT, "stft_ref.npz"), mel=mel.numpy(), logmag_slice=logmag[:, ::9, ::5].numpy().copy(),
                        logmag_checksum=np.asarray(checksum(logmag)), energy=energy.numpy(),
                        mel_basis_checksum=np.asarray(checksum(ref.mel_basis)), basis_checksum=np.asarray(checksum(ref.stft_fn.forward_basis)))
    print("stft", mel.shape, checksum(mel), checksum(logmag))


def digest(t):
    """SHA-256 of a tensor's dtype, shape and bytes: a bitwise comparison against a stored value"""
    import hashlib
    a = t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(("%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


SUM_BLOCK = 16


def block_sums(x):
    """float64 sums of consecutive SUM_BLOCK-element blocks of x.flatten() (the last block may be shorter)"""
    a = x.detach().flatten().double().numpy()
    return np.add.reduceat(a, np.arange(0, a.size, SUM_BLOCK))


def sample_fixture(store, name, ref, ours, n, top=1024, seed=0):
    """`n` elements of the reference output `ref` for a tolerance check, stored exactly: the `top` elements where the oracle's
    output `ours` (at fixture time) is farthest from `ref`, and a seeded uniform sample of the rest; with `ref`'s shape, checksum,
    max |ref| and its SUM_BLOCK-element block sums (float32).  (A full fp32 output of these sizes would be megabytes.)"""
    r = ref.detach().flatten()
    worst = torch.topk((r.double() - ours.detach().flatten().double()).abs(), top).indices.numpy()
    rest = np.setdiff1d(np.arange(r.numel()), worst)
    idx = np.sort(np.concatenate([worst, np.random.default_rng(seed).choice(rest, n - top, replace=False)])).astype(np.int32)
    store[name + "/idx"], store[name + "/val"] = idx, r[torch.from_numpy(idx).long()].numpy()
    store[name + "/shape"], store[name + "/checksum"] = np.asarray(ref.shape), np.asarray(checksum(ref))
    store[name + "/absmax"] = np.asarray(float(r.abs().max()))
    store[name + "/block_sums"] = block_sums(ref).astype(np.float32)


def sample_err(z, name, got, tol):
    """max |got - ref| over a sample_fixture() sample, after checking `got`'s shape, and that its checksum and block sums agree
    with the full reference within what max |got - ref| <= tol over ALL elements implies (sum, sum |x| within N tol; sum x^2
    within tol (2 sum |ref| + N tol); a block's sum within its length x tol, plus the float32 rounding of the stored sum): a
    non-finite element, or one off by more than ~SUM_BLOCK x tol, fails wherever it is"""
    assert tuple(got.shape) == tuple(int(v) for v in z[name + "/shape"]), (tuple(got.shape), z[name + "/shape"])
    n, c, ref_cs = got.numel(), checksum(got), z[name + "/checksum"]
    bound = [n * tol, n * tol, tol * (2 * ref_cs[1] + n * tol)]
    for i in range(3):
        assert abs(c[i] - ref_cs[i]) <= bound[i] * (1 + 1e-9), (name, i, c[i], ref_cs[i], bound[i])
    rs = z[name + "/block_sums"].astype(np.float64)
    lens = np.diff(np.append(np.arange(0, n, SUM_BLOCK), n))
    excess = np.abs(block_sums(got) - rs) - (lens * tol * (1 + 1e-9) + np.abs(rs) * 2.0 ** -23)
    assert not (excess > 0).any() and np.isfinite(excess).all(), (name, "block", int(np.argmax(excess)), float(np.max(excess)))
    idx = torch.from_numpy(z[name + "/idx"].astype(np.int64))
    return (got.detach().flatten()[idx].double() - torch.from_numpy(z[name + "/val"]).double()).abs().max().item()


def reference_diff_golden():
    """the reference side of tests/test_reference_diff.py and test_stft_oracle.py's live test, on the same seeded inputs"""
    from oracle import stft_oracle as S
    js, arr = {}, {}
    with torch.device("meta"):
        unet = R.unet_cls()(**R.unet_config())
    js["unet_large_inventory"] = {k: list(v.shape) for k, v in unet.state_dict().items()}
    vae = R.autoencoder_cls()(**R.vae_config())
    js["vae_inventory"] = {k: list(v.shape) for k, v in vae.state_dict().items()}
    del unet, vae
    # tiny UNet, ragged mask (test_unet_tiny_matches_fork_with_ragged_mask)
    cfgo = O.UNET_CONFIG_TINY
    cfg = dict(R.unet_config())
    cfg.update({k: cfgo[k] for k in ("block_out_channels", "attention_head_dim", "cross_attention_dim")})
    unet = R.unet_cls()(**cfg).eval()
    unet.load_state_dict(W.synth_state_dict(W.unet_param_shapes(cfgo), 7))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 8, 256, 16, generator=g)
    enc = torch.randn(3, 11, cfgo["cross_attention_dim"], generator=g)
    mask = torch.ones(3, 11, dtype=torch.bool)
    mask[0, 1:] = False
    mask[2, 4:] = False
    sample_fixture(arr, "unet_tiny_ragged", unet(x, torch.tensor(123), encoder_hidden_states=enc, encoder_attention_mask=mask).sample,
                   O.unet_forward(W.synth_state_dict(W.unet_param_shapes(cfgo), 7), cfgo, x, 123, enc, mask), 8192)
    # fork DDPMScheduler.step, bitwise (test_scheduler_step_matches_fork_bitwise)
    sch = R.ddpm_cls()(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                       prediction_type="v_prediction", clip_sample=False, variance_type="fixed_small")
    sch.set_timesteps(200)
    g = torch.Generator().manual_seed(0)
    x, v = torch.randn(2, 8, 256, 16, generator=g), torch.randn(2, 8, 256, 16, generator=g)
    js["ddpm_step_sha256"] = {str(t): digest(sch.step(v, t, x, generator=torch.Generator().manual_seed(9)).prev_sample)
                              for t in (995, 500, 5, 0)}
    # Mustango's Music UNet: inventory at the real config, forward at tiny widths (test_music_unet_inventory_and_forward_match_mustango)
    mcfg = json.load(open(os.path.join(R.REF, "mustango", "configs", "music_diffusion_model_config.json")))
    mcfg = {k: v for k, v in mcfg.items() if not k.startswith("_")}
    with torch.device("meta"):
        big = R.unet_music_cls()(**dict(mcfg, **{k: O.UNET_CONFIG_MUSIC[k] for k in ("block_out_channels", "attention_head_dim",
                                                                                         "cross_attention_dim")}))
    js["music_unet_inventory"] = {k: list(v.shape) for k, v in big.state_dict().items()}
    del big
    cfgo = O.UNET_CONFIG_MUSIC_TINY
    torch.manual_seed(0)
    unet = R.unet_music_cls()(**dict(mcfg, **{k: cfgo[k] for k in ("block_out_channels", "attention_head_dim", "cross_attention_dim")})).eval()
    unet.load_state_dict(W.synth_state_dict(W.unet_param_shapes(cfgo), 1234))
    x, enc, beat, chord, em, bm, cm = music_inputs(cfgo, 4, 3)
    want = unet(x, torch.tensor(801), encoder_hidden_states=enc, beat_features=beat, chord_features=chord,
                encoder_attention_mask=em, beat_attention_mask=bm, chord_attention_mask=cm).sample
    got = O.unet_forward(W.synth_state_dict(W.unet_param_shapes(cfgo), 1234), cfgo, x, 801, enc, em, "", beat_features=beat,
                         chord_features=chord, beat_attention_mask=bm, chord_attention_mask=cm)
    sample_fixture(arr, "music_unet_tiny", want, got, 8192)
    # TacotronSTFT on an odd-length 3-clip batch (test_mel_spectrogram_matches_imported_reference_live)
    ref = R.tacotron_stft_cls()(**S.AUDIOLDM_STFT_CONFIG).eval()
    y = stft_wave(B=3, N=16000 * 2 + 123, seed=5)
    m0, l0, e0 = ref.mel_spectrogram(y)
    m1, l1, _ = S.mel_spectrogram(y, ref.mel_basis, ref.stft_fn.forward_basis)
    sample_fixture(arr, "stft_odd_mel", m0, m1, 6144)
    sample_fixture(arr, "stft_odd_logmag", l0, l1, 12288)
    arr["stft_odd_energy"] = e0.numpy()
    js["stft_mel_basis_sha256"], js["stft_forward_basis_sha256"] = digest(ref.mel_basis), digest(ref.stft_fn.forward_basis)
    json.dump(js, open(os.path.join(OUT, "reference_diff.json"), "w"), separators=(",", ":"), sort_keys=True)
    np.savez_compressed(os.path.join(OUT, "reference_diff.npz"), **arr)
    print("reference_diff", {k: v.shape for k, v in arr.items() if not k.endswith(("/checksum", "/absmax"))})


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    assert R.available(), "needs /root/reference"
    if len(sys.argv) > 1 and sys.argv[1] in ("stft", "music", "reference_diff"):      # regenerate only one later fixture
        {"stft": stft_golden, "music": music_golden, "reference_diff": reference_diff_golden}[sys.argv[1]]()
        sys.exit(0)
    sched_golden()
    kat_golden()
    unet_golden()
    vae_golden()
    vae_enc_golden()
    stft_golden()
    music_golden()
    reference_diff_golden()
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))
