"""Nearest x2 upsampling + 3x3 / pad 1 conv == four 2x2-tap phase convolutions over the source image with summed weights
(tango_amd/weights.py upsample_phase_weights: the rule the engine's upsampler convs are packed by).  CPU only, fp64."""
import pytest
import torch
import torch.nn.functional as F

from tango_amd.weights import UPS_PHASE_TAPS, upsample_phase_conv, upsample_phase_weights

SHAPES = [  # B, Cin, Cout, H, W
    (2, 3, 5, 1, 1), (1, 4, 2, 1, 7), (2, 2, 3, 6, 1), (1, 3, 4, 5, 3), (2, 5, 2, 7, 9),
    (2, 4, 6, 32, 2), (1, 4, 6, 64, 4), (1, 3, 5, 128, 8),      # the three UNet upsampler geometries
]


@pytest.mark.parametrize("B,Cin,Cout,H,W", SHAPES)
def test_phase_convs_equal_upsampled_conv(B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(1000 * H + W)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)
    out = upsample_phase_conv(x, upsample_phase_weights(w), b)
    assert out.shape == ref.shape
    assert (out - ref).abs().max().item() <= 1e-12


def test_every_original_tap_lands_in_exactly_one_phase_tap():
    for p in (0, 1):
        taps = UPS_PHASE_TAPS[(p, 0)] + UPS_PHASE_TAPS[(p, 1)]
        assert sorted(taps) == [0, 1, 2]
    w = torch.arange(9, dtype=torch.float64).reshape(1, 1, 3, 3) + 1.0
    wp = upsample_phase_weights(w)
    assert wp.shape == (4, 1, 2, 2, 1)
    for ph in range(4):
        assert wp[ph].sum().item() == w.sum().item()       # each phase sees all nine weights once


def test_fp32_sum_order_is_fixed():
    """ascending (ky, kx): the device pack kernel adds in the same order, so 16-bit roundings agree bit for bit"""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(8, 16, 3, 3, generator=g)
    wp = upsample_phase_weights(w)
    manual = ((w[:, :, 1, 1] + w[:, :, 1, 2]) + w[:, :, 2, 1]) + w[:, :, 2, 2]      # phase (0, 0), tap (1, 1)
    assert torch.equal(wp[0, :, 1, 1, :], manual)
    assert wp.dtype == torch.float32
