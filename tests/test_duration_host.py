"""Clip durations on the host: the duration grid helper (tango_amd.inpaint.duration_geometry: 2.5 .. 20 s in steps of 2.5 s -> latent
height, mel frames, samples), the clip-derived duration of prepare_waveform, and the kernel family every conv / linear problem of the UNet
(config 3's widths: 320 / 640 / 1280 / 1280 channels) lands on at the latent heights 64, 128, 192 and 512 for UNet batches 2, 16 and 64 --
asked of the dispatcher itself through tango_debug_conv2d_route / tango_debug_linear_route, no GPU needed.  The table is DESIGN.md's route
table kept honest: a pin that differs from the family the same problem takes at the default height 256 says so in its comment.  Most
differences are the row count's (a 2.5 s batch of 64 has the rows of a 10 s batch of 16); the ones that are the image geometry's are the
height-192 levels 2 and 3 (192 and 48 pixels per image divide no 256-row tile: the halo convs refuse, the tile kernels take them) and
the 8 x 2 / 16 x 2 images of level 3 at heights 64 / 128 (16 / 8 images per tile need more halo rows than the LDS holds)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tango_amd import _lib
from tango_amd.inpaint import (HOP, SEGMENT, check_latent_h, clip_duration, duration_geometry, latent_mask, prepare_waveform,
                               vocoder_samples)

SWITCHES = [k for k in os.environ if k.startswith("TANGO_")]


# ---- the duration grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,h", [(10, 256), (2.5, 64), (5, 128), (7.5, 192), (12.5, 320), (15.0, 384), (17.5, 448), (20, 512)])
def test_duration_geometry_on_the_grid(d, h):
    H, frames, samples = duration_geometry(d)
    assert (H, frames) == (h, 4 * h)
    assert H == int(d * 25.6)                                   # duration_to_latent_t_size, audioldm/pipeline.py:94-95
    assert frames == int(d * 102.4)                             # pipeline.py:113-126
    assert samples == 160 * frames + 32 == vocoder_samples(frames)
    assert check_latent_h(H) == H


def test_default_duration_is_the_engines_fixed_size():
    assert duration_geometry(10) == (256, 1024, 163872)
    assert duration_geometry(10.0)[1] * HOP == SEGMENT


@pytest.mark.parametrize("d,lo,hi", [(3.0, "2.5", "5"), (0, "2.5", "5"), (22.5, "17.5", "20"), (-2.5, "2.5", "5"), (9.99, "7.5", "10"),
                                     (20.0001, "17.5", "20")])
def test_off_grid_durations_name_both_neighbours(d, lo, hi):
    with pytest.raises(ValueError) as e:
        duration_geometry(d)
    msg = str(e.value)
    assert ("%s and %s" % (lo, hi)) in msg, msg


@pytest.mark.parametrize("bad", [None, "long", float("nan"), float("inf")])
def test_non_numbers_are_refused(bad):
    with pytest.raises(ValueError):
        duration_geometry(bad)


@pytest.mark.parametrize("h", [0, 100, 32, 576, 257, -64])
def test_latent_heights_off_the_grid_are_refused(h):
    with pytest.raises(ValueError) as e:
        check_latent_h(h)
    assert "neighbouring heights" in str(e.value)


def test_clip_duration_is_the_smallest_grid_value_that_holds_the_clip():
    sr = 16000
    assert clip_duration(3 * sr) == 5.0                          # 48000 samples > 256 frames x 160
    assert clip_duration(int(2.5 * 1.024 * sr)) == 2.5           # 40960 samples fill 256 frames exactly: no extra block (round_up_duration adds one)
    assert clip_duration(40961) == 5.0
    assert clip_duration(1) == 2.5
    assert clip_duration(25 * sr) == 20.0
    for k in range(1, 9):
        assert clip_duration(k * 40960) == 2.5 * k


def test_prepare_waveform_pads_to_the_clip_duration_and_cuts_at_20_s():
    g = np.random.default_rng(5)
    a = g.standard_normal(3 * 16000).astype(np.float32)
    w = prepare_waveform(a, duration=None)
    assert w.shape == (duration_geometry(5)[1] * HOP,) == (81920,)
    assert bool((w[48000:] == 0).all()) and float(w.abs().max()) == 0.5
    # the first 3 s are the default call's: padding further changes nothing in front
    assert torch.equal(w[:48000], prepare_waveform(a)[:48000])
    long = g.standard_normal(25 * 16000).astype(np.float32)
    c = prepare_waveform(long, duration=None)
    assert c.shape == (duration_geometry(20)[1] * HOP,) == (327680,)
    assert torch.equal(c, prepare_waveform(long, duration=20))
    assert prepare_waveform(a).shape == (SEGMENT,) and torch.equal(prepare_waveform(a), prepare_waveform(a, duration=10))
    assert prepare_waveform(a, duration=2.5).shape == (40960,)   # an explicit shorter duration cuts
    with pytest.raises(ValueError):
        prepare_waveform(a, duration=3)
    with pytest.raises(ValueError, match="not both"):
        prepare_waveform(a, 1000, duration=5)                    # a segment length of one's own and a duration contradict each other
    assert prepare_waveform(a, 1000).shape == (1000,)


def test_latent_mask_follows_the_height():
    m = latent_mask(2, (0.10, 0.15), (0.5, 0.75), h=64)
    assert m.shape == (2, 1, 64, 16)
    assert float(m[0, 0, 6:9].sum()) == 0 and float(m[0, 0, :6, :8].min()) == 1 and float(m[0, 0, :, 8:12].sum()) == 0


def test_the_c_abi_carries_the_height():
    names = [f[0] for f in _lib.DenoiseArgs._fields_]
    assert names[-1] == "latent_h" and names[-2] == "blend_noise"        # appended: every earlier field keeps its offset
    assert _lib.DenoiseArgs().latent_h == 0                               # 0 = the configured height
    lib = _lib.load()
    for s in ("tango_engine_unet_forward_h", "tango_engine_unet_forward_music_h", "tango_engine_vae_decode_h", "tango_engine_vae_encode_h",
              "tango_engine_profile_unet_h", "tango_engine_profile_vae_h"):
        assert hasattr(lib, s) and s in _lib.SYMBOLS


# ---- routes ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def routes():
    lib = _lib.load()
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    lib.tango_tuning_reload()

    def ask(kind, args, dtype=1):
        if kind == "conv":
            return lib.tango_debug_conv2d_route(dtype, *args, C.byref(C.c_int(0))).decode()
        return lib.tango_debug_linear_route(dtype, *args).decode()
    yield ask
    os.environ.update(saved)
    lib.tango_tuning_reload()


# (latent height, UNet batch) -> [(what, "conv" | "lin", arguments of the route query, family)]
#   conv: (B, Cin, H, W, Cout, stride, upsample, pad, residual, e_act, out_f32) with H x W the SOURCE image
#   lin:  (M, N, K, geglu, ln_fold, residual, vt); the query's v^T epilogue assumes a sequence that is a multiple of 256, so the q | k | v^T
#         shape is listed only where H * W of the level is one (elsewhere the 256-row GEMMs refuse the epilogue: vt_S % 256; never at level 3,
#         whose self-attention projection is therefore not in the table -- its cross-attention to_q, proj, GEGLU and ff2 are)
ROUTES = {
    (64, 2): [
        ('L0 res conv2 320->320 +res', 'conv', (2, 320, 64, 16, 320, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L0 up res conv1 960->320', 'conv', (2, 960, 64, 16, 320, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L0 downsample 320 s2', 'conv', (2, 320, 64, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (2, 640, 32, 8, 640, 1, 1, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L1 res conv2 640->640 +res', 'conv', (2, 640, 32, 8, 640, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L1 up res conv1 1920->640', 'conv', (2, 1920, 32, 8, 640, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L1 downsample 640 s2', 'conv', (2, 640, 32, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (2, 1280, 16, 4, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L2 res conv2 1280->1280 +res', 'conv', (2, 1280, 16, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L2 up res conv1 2560->1280', 'conv', (2, 2560, 16, 4, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 downsample 1280 s2', 'conv', (2, 1280, 16, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (2, 1280, 8, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),
        ('L3 res conv2 1280->1280 +res', 'conv', (2, 1280, 8, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (2, 2560, 8, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('conv_out 320->8 f32', 'conv', (2, 320, 64, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),
        ('L0 proj / to_out 320 +res', 'lin', (2048, 320, 320, 0, 0, 1, 0), 'tile'),
        ('L0 q|k|v^T ln', 'lin', (2048, 960, 320, 0, 1, 0, 1), 'layernorm+tile'),   # H = 256: duo
        ('L0 GEGLU ln', 'lin', (2048, 2560, 320, 1, 1, 0, 0), 'layernorm+duo'),   # H = 256: stream
        ('L0 ff2 1280->320 +res', 'lin', (2048, 320, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: tile
        ('L1 proj / to_out 640 +res', 'lin', (512, 640, 640, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: tile
        ('L1 q|k|v^T ln', 'lin', (512, 1920, 640, 0, 1, 0, 1), 'layernorm+tile'),
        ('L1 GEGLU ln', 'lin', (512, 5120, 640, 1, 1, 0, 0), 'layernorm+tile'),   # H = 256: layernorm+duo
        ('L1 ff2 2560->640 +res', 'lin', (512, 640, 2560, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 proj / to_out 1280 +res', 'lin', (128, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 GEGLU ln', 'lin', (128, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),   # H = 256: layernorm+duo
        ('L2 ff2 5120->1280 +res', 'lin', (128, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (32, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (32, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (32, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (32, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (64, 16): [
        ('L0 res conv2 320->320 +res', 'conv', (16, 320, 64, 16, 320, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_wide
        ('L0 up res conv1 960->320', 'conv', (16, 960, 64, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_wide
        ('L0 downsample 320 s2', 'conv', (16, 320, 64, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (16, 640, 32, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide+phase
        ('L1 res conv2 640->640 +res', 'conv', (16, 640, 32, 8, 640, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_halo
        ('L1 up res conv1 1920->640', 'conv', (16, 1920, 32, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_halo
        ('L1 downsample 640 s2', 'conv', (16, 640, 32, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (16, 1280, 16, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_wide+phase
        ('L2 res conv2 1280->1280 +res', 'conv', (16, 1280, 16, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L2 up res conv1 2560->1280', 'conv', (16, 2560, 16, 4, 1280, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L2 downsample 1280 s2', 'conv', (16, 1280, 16, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (16, 1280, 8, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L3 res conv2 1280->1280 +res', 'conv', (16, 1280, 8, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (16, 2560, 8, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (16, 320, 64, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),   # H = 256: conv_halo
        ('L0 proj / to_out 320 +res', 'lin', (16384, 320, 320, 0, 0, 1, 0), 'duo'),
        ('L0 q|k|v^T ln', 'lin', (16384, 960, 320, 0, 1, 0, 1), 'duo'),   # H = 256: stream
        ('L0 GEGLU ln', 'lin', (16384, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (16384, 320, 1280, 0, 0, 1, 0), 'duo'),   # H = 256: wide
        ('L1 proj / to_out 640 +res', 'lin', (4096, 640, 640, 0, 0, 1, 0), 'tile'),   # H = 256: duo
        ('L1 q|k|v^T ln', 'lin', (4096, 1920, 640, 0, 1, 0, 1), 'duo'),
        ('L1 GEGLU ln', 'lin', (4096, 5120, 640, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: wide+xstats+pers
        ('L1 ff2 2560->640 +res', 'lin', (4096, 640, 2560, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: duo
        ('L2 proj / to_out 1280 +res', 'lin', (1024, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: duo
        ('L2 GEGLU ln', 'lin', (1024, 10240, 1280, 1, 1, 0, 0), 'layernorm+duo'),   # H = 256: wide+xstats+pers
        ('L2 ff2 5120->1280 +res', 'lin', (1024, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (256, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (256, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (256, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),   # H = 256: layernorm+duo
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (256, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (64, 64): [
        ('L0 res conv2 320->320 +res', 'conv', (64, 320, 64, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L0 up res conv1 960->320', 'conv', (64, 960, 64, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L0 downsample 320 s2', 'conv', (64, 320, 64, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: dma
        ('L0 upsampler 640 (from L1)', 'conv', (64, 640, 32, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (64, 640, 32, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_halo'),   # H = 256: conv_wide
        ('L1 up res conv1 1920->640', 'conv', (64, 1920, 32, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide
        ('L1 downsample 640 s2', 'conv', (64, 640, 32, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: tile
        ('L1 upsampler 1280 (from L2)', 'conv', (64, 1280, 16, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L2 res conv2 1280->1280 +res', 'conv', (64, 1280, 16, 4, 1280, 1, 0, 1, 1, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_wide
        ('L2 up res conv1 2560->1280', 'conv', (64, 2560, 16, 4, 1280, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_wide
        ('L2 downsample 1280 s2', 'conv', (64, 1280, 16, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (64, 1280, 8, 2, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_wide+phase
        ('L3 res conv2 1280->1280 +res', 'conv', (64, 1280, 8, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L3 up res conv1 2560->1280', 'conv', (64, 2560, 8, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (64, 320, 64, 16, 8, 1, 0, 1, 0, 0, 1), 'conv_halo'),
        ('L0 proj / to_out 320 +res', 'lin', (65536, 320, 320, 0, 0, 1, 0), 'duo'),   # H = 256: wide+pers
        ('L0 q|k|v^T ln', 'lin', (65536, 960, 320, 0, 1, 0, 1), 'stream'),   # H = 256: wide+pers
        ('L0 GEGLU ln', 'lin', (65536, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (65536, 320, 1280, 0, 0, 1, 0), 'wide'),   # H = 256: wide+pers
        ('L1 proj / to_out 640 +res', 'lin', (16384, 640, 640, 0, 0, 1, 0), 'duo'),   # H = 256: wide+pers
        ('L1 q|k|v^T ln', 'lin', (16384, 1920, 640, 0, 1, 0, 1), 'duo'),   # H = 256: wide+pers
        ('L1 GEGLU ln', 'lin', (16384, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (16384, 640, 2560, 0, 0, 1, 0), 'duo'),   # H = 256: wide+pers
        ('L2 proj / to_out 1280 +res', 'lin', (4096, 1280, 1280, 0, 0, 1, 0), 'duo'),   # H = 256: wide
        ('L2 GEGLU ln', 'lin', (4096, 10240, 1280, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L2 ff2 5120->1280 +res', 'lin', (4096, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: wide
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (1024, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: duo
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (1024, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),   # H = 256: duo
        ('L3 (mid) GEGLU ln', 'lin', (1024, 10240, 1280, 1, 1, 0, 0), 'layernorm+duo'),   # H = 256: wide+xstats+pers
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (1024, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (128, 2): [
        ('L0 res conv2 320->320 +res', 'conv', (2, 320, 128, 16, 320, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L0 up res conv1 960->320', 'conv', (2, 960, 128, 16, 320, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L0 downsample 320 s2', 'conv', (2, 320, 128, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (2, 640, 64, 8, 640, 1, 1, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L1 res conv2 640->640 +res', 'conv', (2, 640, 64, 8, 640, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L1 up res conv1 1920->640', 'conv', (2, 1920, 64, 8, 640, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L1 downsample 640 s2', 'conv', (2, 640, 64, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (2, 1280, 32, 4, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L2 res conv2 1280->1280 +res', 'conv', (2, 1280, 32, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L2 up res conv1 2560->1280', 'conv', (2, 2560, 32, 4, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 downsample 1280 s2', 'conv', (2, 1280, 32, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (2, 1280, 16, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),
        ('L3 res conv2 1280->1280 +res', 'conv', (2, 1280, 16, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (2, 2560, 16, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('conv_out 320->8 f32', 'conv', (2, 320, 128, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),
        ('L0 proj / to_out 320 +res', 'lin', (4096, 320, 320, 0, 0, 1, 0), 'tile'),
        ('L0 q|k|v^T ln', 'lin', (4096, 960, 320, 0, 1, 0, 1), 'stream'),   # H = 256: duo
        ('L0 GEGLU ln', 'lin', (4096, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (4096, 320, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: tile
        ('L1 proj / to_out 640 +res', 'lin', (1024, 640, 640, 0, 0, 1, 0), 'tile'),
        ('L1 q|k|v^T ln', 'lin', (1024, 1920, 640, 0, 1, 0, 1), 'layernorm+tile'),
        ('L1 GEGLU ln', 'lin', (1024, 5120, 640, 1, 1, 0, 0), 'layernorm+duo'),
        ('L1 ff2 2560->640 +res', 'lin', (1024, 640, 2560, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 proj / to_out 1280 +res', 'lin', (256, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 GEGLU ln', 'lin', (256, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),   # H = 256: layernorm+duo
        ('L2 ff2 5120->1280 +res', 'lin', (256, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (64, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (64, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (64, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (64, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (128, 16): [
        ('L0 res conv2 320->320 +res', 'conv', (16, 320, 128, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_halo'),   # H = 256: conv_wide
        ('L0 up res conv1 960->320', 'conv', (16, 960, 128, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide
        ('L0 downsample 320 s2', 'conv', (16, 320, 128, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (16, 640, 64, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (16, 640, 64, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_halo
        ('L1 up res conv1 1920->640', 'conv', (16, 1920, 64, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_halo
        ('L1 downsample 640 s2', 'conv', (16, 640, 64, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (16, 1280, 32, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide+phase
        ('L2 res conv2 1280->1280 +res', 'conv', (16, 1280, 32, 4, 1280, 1, 0, 1, 1, 0, 0), 'conv_wide+splitk'),
        ('L2 up res conv1 2560->1280', 'conv', (16, 2560, 32, 4, 1280, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L2 downsample 1280 s2', 'conv', (16, 1280, 32, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (16, 1280, 16, 2, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L3 res conv2 1280->1280 +res', 'conv', (16, 1280, 16, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (16, 2560, 16, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (16, 320, 128, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),   # H = 256: conv_halo
        ('L0 proj / to_out 320 +res', 'lin', (32768, 320, 320, 0, 0, 1, 0), 'duo'),
        ('L0 q|k|v^T ln', 'lin', (32768, 960, 320, 0, 1, 0, 1), 'duo'),   # H = 256: stream
        ('L0 GEGLU ln', 'lin', (32768, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (32768, 320, 1280, 0, 0, 1, 0), 'duo'),   # H = 256: wide
        ('L1 proj / to_out 640 +res', 'lin', (8192, 640, 640, 0, 0, 1, 0), 'duo'),
        ('L1 q|k|v^T ln', 'lin', (8192, 1920, 640, 0, 1, 0, 1), 'duo'),
        ('L1 GEGLU ln', 'lin', (8192, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (8192, 640, 2560, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: duo
        ('L2 proj / to_out 1280 +res', 'lin', (2048, 1280, 1280, 0, 0, 1, 0), 'tile'),   # H = 256: duo
        ('L2 GEGLU ln', 'lin', (2048, 10240, 1280, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: wide+xstats+pers
        ('L2 ff2 5120->1280 +res', 'lin', (2048, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (512, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (512, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (512, 10240, 1280, 1, 1, 0, 0), 'layernorm+duo'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (512, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (128, 64): [
        ('L0 res conv2 320->320 +res', 'conv', (64, 320, 128, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L0 up res conv1 960->320', 'conv', (64, 960, 128, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L0 downsample 320 s2', 'conv', (64, 320, 128, 16, 320, 2, 0, 1, 0, 0, 0), 'tile'),   # H = 256: dma
        ('L0 upsampler 640 (from L1)', 'conv', (64, 640, 64, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (64, 640, 64, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L1 up res conv1 1920->640', 'conv', (64, 1920, 64, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L1 downsample 640 s2', 'conv', (64, 640, 64, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: tile
        ('L1 upsampler 1280 (from L2)', 'conv', (64, 1280, 32, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L2 res conv2 1280->1280 +res', 'conv', (64, 1280, 32, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile'),   # H = 256: conv_wide
        ('L2 up res conv1 2560->1280', 'conv', (64, 2560, 32, 4, 1280, 1, 0, 1, 0, 0, 0), 'tile'),   # H = 256: conv_wide
        ('L2 downsample 1280 s2', 'conv', (64, 1280, 32, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (64, 1280, 16, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile'),   # H = 256: conv_wide+phase
        ('L3 res conv2 1280->1280 +res', 'conv', (64, 1280, 16, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L3 up res conv1 2560->1280', 'conv', (64, 2560, 16, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (64, 320, 128, 16, 8, 1, 0, 1, 0, 0, 1), 'conv_halo'),
        ('L0 proj / to_out 320 +res', 'lin', (131072, 320, 320, 0, 0, 1, 0), 'wide+pers'),
        ('L0 q|k|v^T ln', 'lin', (131072, 960, 320, 0, 1, 0, 1), 'wide+pers'),
        ('L0 GEGLU ln', 'lin', (131072, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (131072, 320, 1280, 0, 0, 1, 0), 'wide+pers'),
        ('L1 proj / to_out 640 +res', 'lin', (32768, 640, 640, 0, 0, 1, 0), 'duo'),   # H = 256: wide+pers
        ('L1 q|k|v^T ln', 'lin', (32768, 1920, 640, 0, 1, 0, 1), 'wide+pers'),
        ('L1 GEGLU ln', 'lin', (32768, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (32768, 640, 2560, 0, 0, 1, 0), 'wide'),   # H = 256: wide+pers
        ('L2 proj / to_out 1280 +res', 'lin', (8192, 1280, 1280, 0, 0, 1, 0), 'duo'),   # H = 256: wide
        ('L2 GEGLU ln', 'lin', (8192, 10240, 1280, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L2 ff2 5120->1280 +res', 'lin', (8192, 1280, 5120, 0, 0, 1, 0), 'dma'),   # H = 256: wide
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (2048, 1280, 1280, 0, 0, 1, 0), 'tile'),   # H = 256: duo
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (2048, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile'),   # H = 256: duo
        ('L3 (mid) GEGLU ln', 'lin', (2048, 10240, 1280, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: wide+xstats+pers
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (2048, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (192, 2): [
        ('L0 res conv2 320->320 +res', 'conv', (2, 320, 192, 16, 320, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L0 up res conv1 960->320', 'conv', (2, 960, 192, 16, 320, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L0 downsample 320 s2', 'conv', (2, 320, 192, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (2, 640, 96, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L1 res conv2 640->640 +res', 'conv', (2, 640, 96, 8, 640, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L1 up res conv1 1920->640', 'conv', (2, 1920, 96, 8, 640, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L1 downsample 640 s2', 'conv', (2, 640, 96, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (2, 1280, 48, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L2 res conv2 1280->1280 +res', 'conv', (2, 1280, 48, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L2 up res conv1 2560->1280', 'conv', (2, 2560, 48, 4, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 downsample 1280 s2', 'conv', (2, 1280, 48, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (2, 1280, 24, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),
        ('L3 res conv2 1280->1280 +res', 'conv', (2, 1280, 24, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (2, 2560, 24, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('conv_out 320->8 f32', 'conv', (2, 320, 192, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),
        ('L0 proj / to_out 320 +res', 'lin', (6144, 320, 320, 0, 0, 1, 0), 'tile'),
        ('L0 q|k|v^T ln', 'lin', (6144, 960, 320, 0, 1, 0, 1), 'duo'),
        ('L0 GEGLU ln', 'lin', (6144, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (6144, 320, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: tile
        ('L1 proj / to_out 640 +res', 'lin', (1536, 640, 640, 0, 0, 1, 0), 'tile'),
        ('L1 q|k|v^T ln', 'lin', (1536, 1920, 640, 0, 1, 0, 1), 'layernorm+tile'),
        ('L1 GEGLU ln', 'lin', (1536, 5120, 640, 1, 1, 0, 0), 'layernorm+duo'),
        ('L1 ff2 2560->640 +res', 'lin', (1536, 640, 2560, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 proj / to_out 1280 +res', 'lin', (384, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 GEGLU ln', 'lin', (384, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),   # H = 256: layernorm+duo
        ('L2 ff2 5120->1280 +res', 'lin', (384, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (96, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (96, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (96, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (96, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (192, 16): [
        ('L0 res conv2 320->320 +res', 'conv', (16, 320, 192, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_halo'),   # H = 256: conv_wide
        ('L0 up res conv1 960->320', 'conv', (16, 960, 192, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide
        ('L0 downsample 320 s2', 'conv', (16, 320, 192, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (16, 640, 96, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (16, 640, 96, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_halo
        ('L1 up res conv1 1920->640', 'conv', (16, 1920, 96, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: conv_halo
        ('L1 downsample 640 s2', 'conv', (16, 640, 96, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (16, 1280, 48, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide+phase
        ('L2 res conv2 1280->1280 +res', 'conv', (16, 1280, 48, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L2 up res conv1 2560->1280', 'conv', (16, 2560, 48, 4, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L2 downsample 1280 s2', 'conv', (16, 1280, 48, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (16, 1280, 24, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L3 res conv2 1280->1280 +res', 'conv', (16, 1280, 24, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (16, 2560, 24, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (16, 320, 192, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),   # H = 256: conv_halo
        ('L0 proj / to_out 320 +res', 'lin', (49152, 320, 320, 0, 0, 1, 0), 'duo'),
        ('L0 q|k|v^T ln', 'lin', (49152, 960, 320, 0, 1, 0, 1), 'stream'),
        ('L0 GEGLU ln', 'lin', (49152, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (49152, 320, 1280, 0, 0, 1, 0), 'wide'),
        ('L1 proj / to_out 640 +res', 'lin', (12288, 640, 640, 0, 0, 1, 0), 'duo'),
        ('L1 q|k|v^T ln', 'lin', (12288, 1920, 640, 0, 1, 0, 1), 'duo'),
        ('L1 GEGLU ln', 'lin', (12288, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (12288, 640, 2560, 0, 0, 1, 0), 'tile'),   # H = 256: duo
        ('L2 proj / to_out 1280 +res', 'lin', (3072, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: duo
        ('L2 GEGLU ln', 'lin', (3072, 10240, 1280, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: wide+xstats+pers
        ('L2 ff2 5120->1280 +res', 'lin', (3072, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (768, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (768, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (768, 10240, 1280, 1, 1, 0, 0), 'layernorm+duo'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (768, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (192, 64): [
        ('L0 res conv2 320->320 +res', 'conv', (64, 320, 192, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L0 up res conv1 960->320', 'conv', (64, 960, 192, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L0 downsample 320 s2', 'conv', (64, 320, 192, 16, 320, 2, 0, 1, 0, 0, 0), 'tile'),   # H = 256: dma
        ('L0 upsampler 640 (from L1)', 'conv', (64, 640, 96, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (64, 640, 96, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L1 up res conv1 1920->640', 'conv', (64, 1920, 96, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L1 downsample 640 s2', 'conv', (64, 640, 96, 8, 640, 2, 0, 1, 0, 0, 0), 'tile'),
        ('L1 upsampler 1280 (from L2)', 'conv', (64, 1280, 48, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide'),   # H = 256: conv_wide+phase
        ('L2 res conv2 1280->1280 +res', 'conv', (64, 1280, 48, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile'),   # H = 256: conv_wide
        ('L2 up res conv1 2560->1280', 'conv', (64, 2560, 48, 4, 1280, 1, 0, 1, 0, 0, 0), 'tile'),   # H = 256: conv_wide
        ('L2 downsample 1280 s2', 'conv', (64, 1280, 48, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (64, 1280, 24, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile'),   # H = 256: conv_wide+phase
        ('L3 res conv2 1280->1280 +res', 'conv', (64, 1280, 24, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('L3 up res conv1 2560->1280', 'conv', (64, 2560, 24, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (64, 320, 192, 16, 8, 1, 0, 1, 0, 0, 1), 'conv_halo'),
        ('L0 proj / to_out 320 +res', 'lin', (196608, 320, 320, 0, 0, 1, 0), 'wide+pers'),
        ('L0 q|k|v^T ln', 'lin', (196608, 960, 320, 0, 1, 0, 1), 'wide+pers'),
        ('L0 GEGLU ln', 'lin', (196608, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (196608, 320, 1280, 0, 0, 1, 0), 'wide+pers'),
        ('L1 proj / to_out 640 +res', 'lin', (49152, 640, 640, 0, 0, 1, 0), 'duo'),   # H = 256: wide+pers
        ('L1 q|k|v^T ln', 'lin', (49152, 1920, 640, 0, 1, 0, 1), 'wide+pers'),
        ('L1 GEGLU ln', 'lin', (49152, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (49152, 640, 2560, 0, 0, 1, 0), 'wide'),   # H = 256: wide+pers
        ('L2 proj / to_out 1280 +res', 'lin', (12288, 1280, 1280, 0, 0, 1, 0), 'wide'),
        ('L2 GEGLU ln', 'lin', (12288, 10240, 1280, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L2 ff2 5120->1280 +res', 'lin', (12288, 1280, 5120, 0, 0, 1, 0), 'wide'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (3072, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),   # H = 256: duo
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (3072, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),   # H = 256: duo
        ('L3 (mid) GEGLU ln', 'lin', (3072, 10240, 1280, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: wide+xstats+pers
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (3072, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (512, 2): [
        ('L0 res conv2 320->320 +res', 'conv', (2, 320, 512, 16, 320, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L0 up res conv1 960->320', 'conv', (2, 960, 512, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L0 downsample 320 s2', 'conv', (2, 320, 512, 16, 320, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L0 upsampler 640 (from L1)', 'conv', (2, 640, 256, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide+splitk
        ('L1 res conv2 640->640 +res', 'conv', (2, 640, 256, 8, 640, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L1 up res conv1 1920->640', 'conv', (2, 1920, 256, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L1 downsample 640 s2', 'conv', (2, 640, 256, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (2, 1280, 128, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('L2 res conv2 1280->1280 +res', 'conv', (2, 1280, 128, 4, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L2 up res conv1 2560->1280', 'conv', (2, 2560, 128, 4, 1280, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),   # H = 256: tile+splitk
        ('L2 downsample 1280 s2', 'conv', (2, 1280, 128, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (2, 1280, 64, 2, 1280, 1, 1, 1, 0, 0, 0), 'tile+splitk'),
        ('L3 res conv2 1280->1280 +res', 'conv', (2, 1280, 64, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile+splitk'),
        ('L3 up res conv1 2560->1280', 'conv', (2, 2560, 64, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('conv_out 320->8 f32', 'conv', (2, 320, 512, 16, 8, 1, 0, 1, 0, 0, 1), 'tile+splitk'),
        ('L0 proj / to_out 320 +res', 'lin', (16384, 320, 320, 0, 0, 1, 0), 'duo'),   # H = 256: tile
        ('L0 q|k|v^T ln', 'lin', (16384, 960, 320, 0, 1, 0, 1), 'duo'),
        ('L0 GEGLU ln', 'lin', (16384, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (16384, 320, 1280, 0, 0, 1, 0), 'duo'),   # H = 256: tile
        ('L1 proj / to_out 640 +res', 'lin', (4096, 640, 640, 0, 0, 1, 0), 'tile'),
        ('L1 q|k|v^T ln', 'lin', (4096, 1920, 640, 0, 1, 0, 1), 'duo'),   # H = 256: layernorm+tile
        ('L1 GEGLU ln', 'lin', (4096, 5120, 640, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: layernorm+duo
        ('L1 ff2 2560->640 +res', 'lin', (4096, 640, 2560, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 proj / to_out 1280 +res', 'lin', (1024, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L2 q|k|v^T ln', 'lin', (1024, 3840, 1280, 0, 1, 0, 1), 'layernorm+tile'),
        ('L2 GEGLU ln', 'lin', (1024, 10240, 1280, 1, 1, 0, 0), 'layernorm+duo'),
        ('L2 ff2 5120->1280 +res', 'lin', (1024, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (256, 1280, 1280, 0, 0, 1, 0), 'tile+splitk'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (256, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile+splitk'),
        ('L3 (mid) GEGLU ln', 'lin', (256, 10240, 1280, 1, 1, 0, 0), 'layernorm+tile'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (256, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (512, 16): [
        ('L0 res conv2 320->320 +res', 'conv', (16, 320, 512, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L0 up res conv1 960->320', 'conv', (16, 960, 512, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L0 downsample 320 s2', 'conv', (16, 320, 512, 16, 320, 2, 0, 1, 0, 0, 0), 'tile'),   # H = 256: tile+splitk
        ('L0 upsampler 640 (from L1)', 'conv', (16, 640, 256, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (16, 640, 256, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_wide'),   # H = 256: conv_halo
        ('L1 up res conv1 1920->640', 'conv', (16, 1920, 256, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide'),   # H = 256: conv_halo
        ('L1 downsample 640 s2', 'conv', (16, 640, 256, 8, 640, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L1 upsampler 1280 (from L2)', 'conv', (16, 1280, 128, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L2 res conv2 1280->1280 +res', 'conv', (16, 1280, 128, 4, 1280, 1, 0, 1, 1, 0, 0), 'conv_halo'),   # H = 256: conv_wide+splitk
        ('L2 up res conv1 2560->1280', 'conv', (16, 2560, 128, 4, 1280, 1, 0, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide+splitk
        ('L2 downsample 1280 s2', 'conv', (16, 1280, 128, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile+splitk'),
        ('L2 upsampler 1280 (from L3)', 'conv', (16, 1280, 64, 2, 1280, 1, 1, 1, 0, 0, 0), 'conv_halo'),   # H = 256: conv_wide+splitk
        ('L3 res conv2 1280->1280 +res', 'conv', (16, 1280, 64, 2, 1280, 1, 0, 1, 1, 0, 0), 'conv_wide+splitk'),   # H = 256: tile+splitk
        ('L3 up res conv1 2560->1280', 'conv', (16, 2560, 64, 2, 1280, 1, 0, 1, 0, 0, 0), 'conv_wide+splitk'),
        ('conv_out 320->8 f32', 'conv', (16, 320, 512, 16, 8, 1, 0, 1, 0, 0, 1), 'conv_halo'),
        ('L0 proj / to_out 320 +res', 'lin', (131072, 320, 320, 0, 0, 1, 0), 'wide+pers'),   # H = 256: duo
        ('L0 q|k|v^T ln', 'lin', (131072, 960, 320, 0, 1, 0, 1), 'wide+pers'),   # H = 256: stream
        ('L0 GEGLU ln', 'lin', (131072, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (131072, 320, 1280, 0, 0, 1, 0), 'wide+pers'),   # H = 256: wide
        ('L1 proj / to_out 640 +res', 'lin', (32768, 640, 640, 0, 0, 1, 0), 'duo'),
        ('L1 q|k|v^T ln', 'lin', (32768, 1920, 640, 0, 1, 0, 1), 'wide+pers'),   # H = 256: duo
        ('L1 GEGLU ln', 'lin', (32768, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (32768, 640, 2560, 0, 0, 1, 0), 'wide'),   # H = 256: duo
        ('L2 proj / to_out 1280 +res', 'lin', (8192, 1280, 1280, 0, 0, 1, 0), 'duo'),
        ('L2 q|k|v^T ln', 'lin', (8192, 3840, 1280, 0, 1, 0, 1), 'wide'),
        ('L2 GEGLU ln', 'lin', (8192, 10240, 1280, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L2 ff2 5120->1280 +res', 'lin', (8192, 1280, 5120, 0, 0, 1, 0), 'dma'),   # H = 256: tile+splitk
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (2048, 1280, 1280, 0, 0, 1, 0), 'tile'),   # H = 256: tile+splitk
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (2048, 1280, 1280, 0, 1, 0, 0), 'layernorm+tile'),   # H = 256: layernorm+tile+splitk
        ('L3 (mid) GEGLU ln', 'lin', (2048, 10240, 1280, 1, 1, 0, 0), 'wide+xstats'),   # H = 256: layernorm+duo
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (2048, 1280, 5120, 0, 0, 1, 0), 'tile+splitk'),
    ],
    (512, 64): [
        ('L0 res conv2 320->320 +res', 'conv', (64, 320, 512, 16, 320, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L0 up res conv1 960->320', 'conv', (64, 960, 512, 16, 320, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L0 downsample 320 s2', 'conv', (64, 320, 512, 16, 320, 2, 0, 1, 0, 0, 0), 'dma'),
        ('L0 upsampler 640 (from L1)', 'conv', (64, 640, 256, 8, 640, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L1 res conv2 640->640 +res', 'conv', (64, 640, 256, 8, 640, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L1 up res conv1 1920->640', 'conv', (64, 1920, 256, 8, 640, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L1 downsample 640 s2', 'conv', (64, 640, 256, 8, 640, 2, 0, 1, 0, 0, 0), 'dma'),   # H = 256: tile
        ('L1 upsampler 1280 (from L2)', 'conv', (64, 1280, 128, 4, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L2 res conv2 1280->1280 +res', 'conv', (64, 1280, 128, 4, 1280, 1, 0, 1, 1, 0, 0), 'conv_wide'),
        ('L2 up res conv1 2560->1280', 'conv', (64, 2560, 128, 4, 1280, 1, 0, 1, 0, 0, 0), 'conv_wide'),
        ('L2 downsample 1280 s2', 'conv', (64, 1280, 128, 4, 1280, 2, 0, 1, 0, 0, 0), 'tile'),   # H = 256: tile+splitk
        ('L2 upsampler 1280 (from L3)', 'conv', (64, 1280, 64, 2, 1280, 1, 1, 1, 0, 0, 0), 'conv_wide+phase'),
        ('L3 res conv2 1280->1280 +res', 'conv', (64, 1280, 64, 2, 1280, 1, 0, 1, 1, 0, 0), 'tile'),   # H = 256: conv_wide+splitk
        ('L3 up res conv1 2560->1280', 'conv', (64, 2560, 64, 2, 1280, 1, 0, 1, 0, 0, 0), 'tile'),   # H = 256: conv_wide+splitk
        ('conv_out 320->8 f32', 'conv', (64, 320, 512, 16, 8, 1, 0, 1, 0, 0, 1), 'conv_halo'),
        ('L0 proj / to_out 320 +res', 'lin', (524288, 320, 320, 0, 0, 1, 0), 'wide+pers'),
        ('L0 q|k|v^T ln', 'lin', (524288, 960, 320, 0, 1, 0, 1), 'wide+pers'),
        ('L0 GEGLU ln', 'lin', (524288, 2560, 320, 1, 1, 0, 0), 'stream'),
        ('L0 ff2 1280->320 +res', 'lin', (524288, 320, 1280, 0, 0, 1, 0), 'wide+pers'),
        ('L1 proj / to_out 640 +res', 'lin', (131072, 640, 640, 0, 0, 1, 0), 'wide+pers'),
        ('L1 q|k|v^T ln', 'lin', (131072, 1920, 640, 0, 1, 0, 1), 'wide+pers'),
        ('L1 GEGLU ln', 'lin', (131072, 5120, 640, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L1 ff2 2560->640 +res', 'lin', (131072, 640, 2560, 0, 0, 1, 0), 'wide+pers'),
        ('L2 proj / to_out 1280 +res', 'lin', (32768, 1280, 1280, 0, 0, 1, 0), 'wide+pers'),   # H = 256: wide
        ('L2 q|k|v^T ln', 'lin', (32768, 3840, 1280, 0, 1, 0, 1), 'wide+pers'),
        ('L2 GEGLU ln', 'lin', (32768, 10240, 1280, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L2 ff2 5120->1280 +res', 'lin', (32768, 1280, 5120, 0, 0, 1, 0), 'wide+pers'),   # H = 256: wide
        ('L3 (mid) proj / to_out 1280 +res', 'lin', (8192, 1280, 1280, 0, 0, 1, 0), 'duo'),
        ('L3 (mid) to_q ln (cross-attention)', 'lin', (8192, 1280, 1280, 0, 1, 0, 0), 'duo'),
        ('L3 (mid) GEGLU ln', 'lin', (8192, 10240, 1280, 1, 1, 0, 0), 'wide+xstats+pers'),
        ('L3 (mid) ff2 5120->1280 +res', 'lin', (8192, 1280, 5120, 0, 0, 1, 0), 'dma'),   # H = 256: tile+splitk
    ],
}


@pytest.mark.parametrize("key", sorted(ROUTES))
def test_route_at_height(routes, key):
    for what, kind, args, want in ROUTES[key]:
        got = routes(kind, args)
        assert got == want, (key, what, args, got, want)
        assert routes(kind, args, dtype=2) == want, (key, what, "bf16")


def test_route_table_covers_every_level():
    for (H, B2), rows in ROUTES.items():
        convs = [a for _, k, a, _ in rows if k == "conv"]
        assert {(a[2], a[3]) for a in convs} >= {(H >> l, 16 >> l) for l in range(4)}, (H, B2)
        assert all(a[0] == B2 for a in convs)
        lins = [a for _, k, a, _ in rows if k == "lin"]
        assert {a[0] for a in lins} == {B2 * (H >> l) * (16 >> l) for l in range(4)}      # level 3: the mid-block transformer
