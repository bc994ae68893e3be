"""The UNet upsampler convs (nearest x2 + 3x3 / pad 1) as four 2x2-tap phase convolutions on the source grid (conv_wide.hip PH),
through the C ABI: `tango_op_conv2d_ups(..., phases = 1 | 0)` runs the phase form or the nine-tap gather form on the same inputs,
`tango_op_pack_ups_phase` returns the device-packed phase weights.

The weights are NOT pre-rounded here: both forms round the fp32 checkpoint values themselves (the phase form after summing the folded
taps, the nine-tap form before), and the reference is the fp64 torch conv of the unrounded weights.  Activations are rounded to the
engine dtype first (that rounding belongs to the producer of x, not to this op).  Tolerance: `close()` / `TOL` of tests/test_ops_gpu.py."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from tango_amd.weights import upsample_phase_weights  # noqa: E402

DT = {"fp16": 1, "bf16": 2}
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp16": 4e-3, "bf16": 3e-2}          # tests/test_ops_gpu.py TOL: max abs error over the reference's max abs
# B (UNet batch), C (Cin = Cout), source H, W: the three upsamplers of the UNet at UNet batch 64, and level 1's at B = 8 prompts (UNet batch 16)
SHAPES = [(64, 1280, 32, 2), (64, 1280, 64, 4), (64, 640, 128, 8), (16, 1280, 64, 4)]
_KEEP = []


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def check(lib, rc):
    assert rc == 0, lib.tango_last_error().decode()


@pytest.fixture(autouse=True)
def _clear_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def _problem(B, Cc, H, W, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, Cc, H, W, device="cuda", generator=g).to(TDT[dtype]).float()
    w = torch.randn(Cc, Cc, 3, 3, device="cuda", generator=g) / (9 * Cc) ** 0.5
    b = torch.randn(Cc, device="cuda", generator=g)
    return x, w, b


def _run(lib, dtype, x, w, b, b2, phases):
    B, Cc, H, W = x.shape
    out = torch.empty(B, w.shape[0], 2 * H, 2 * W, device="cuda")
    _KEEP.extend([x, w, b, b2, out])
    check(lib, lib.tango_op_conv2d_ups(DT[dtype], ptr(x), ptr(w), ptr(b), ptr(b2), ptr(out), B, Cc, H, W, w.shape[0], phases, None))
    return out


def _ref64(x, w, b):
    """fp64 reference of conv2d(interpolate(x, 2, "nearest"), w, b, padding=1) on the GPU: the nine taps as nine fp64 matrix products
    over shifted views of the padded UPSAMPLED image (no use of the phase identity), in batch slices (level 0: 64 x 640 x 256 x 16)"""
    O = w.shape[0]
    w64 = w.double()
    outs = []
    for i in range(0, x.shape[0], 8):
        up = F.pad(F.interpolate(x[i:i + 8].double(), scale_factor=2, mode="nearest"), (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
        n, Hp, Wp, _ = up.shape
        acc = b.double().view(1, 1, 1, O).expand(n, Hp - 2, Wp - 2, O).clone()
        for ky in range(3):
            for kx in range(3):
                acc += up[:, ky:ky + Hp - 2, kx:kx + Wp - 2, :] @ w64[:, :, ky, kx].t()
        outs.append(acc.permute(0, 3, 1, 2))
    return torch.cat(outs)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("Cc", [640, 1280])
def test_device_phase_weights_equal_the_helpers_bit_for_bit(lib, dtype, Cc):
    g = torch.Generator().manual_seed(Cc)
    w = torch.randn(Cc, Cc, 3, 3, generator=g) / (9 * Cc) ** 0.5
    want = upsample_phase_weights(w).to(TDT[dtype]).reshape(4, Cc, 4, Cc)         # fp32 sums, ONE rounding
    wd = w.cuda()
    got = torch.empty(4, Cc, 4, Cc, dtype=TDT[dtype], device="cuda")
    check(lib, lib.tango_op_pack_ups_phase(DT[dtype], ptr(wd), ptr(got), Cc, Cc, None))
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,Cc,H,W", SHAPES)
def test_phase_conv_against_fp64_and_the_nine_tap_form(lib, dtype, B, Cc, H, W):
    """(b) phase conv vs the fp64 conv of the UNROUNDED weights within TOL; (c) its rms error is not above the nine-tap form's by more
    than 10 % (the bound says "not worse": |round(a + b) - (a + b)| <= 2^-11 |a + b| <= the separate roundings' bound; the margin is the
    scatter of one random draw); (d) two runs are bitwise equal."""
    x, w, b = _problem(B, Cc, H, W, dtype, 100 * H + W + B)
    ref = _ref64(x, w, b)
    scale = ref.abs().max().item() + 1e-6
    out_p = _run(lib, dtype, x, w, b, None, 1)
    out_p2 = _run(lib, dtype, x, w, b, None, 1)
    out_9 = _run(lib, dtype, x, w, b, None, 0)
    torch.cuda.synchronize()
    err_p = (out_p.double() - ref).abs().max().item() / scale
    err_9 = (out_9.double() - ref).abs().max().item() / scale
    rms_p = (out_p.double() - ref).pow(2).mean().sqrt().item()
    rms_9 = (out_9.double() - ref).pow(2).mean().sqrt().item()
    print("ups conv B2=%d C=%d %dx%d %s: max rel err phase %.3e / nine-tap %.3e (tol %.1e); rms err phase %.4e / nine-tap %.4e, ratio %.4f (output rms %.3f)"
          % (B, Cc, H, W, dtype, err_p, err_9, TOL[dtype], rms_p, rms_9, rms_p / rms_9, ref.pow(2).mean().sqrt().item()))
    assert torch.isfinite(out_p).all()
    assert err_p <= TOL[dtype], "phase conv: rel err %.3e > %.1e" % (err_p, TOL[dtype])
    assert rms_p <= 1.10 * rms_9, "phase form rms error %.4e vs nine-tap %.4e" % (rms_p, rms_9)
    assert torch.equal(out_p, out_p2), "the phase form must be run-to-run bit-stable"
    assert not torch.equal(out_p, out_9), "the switch changed nothing: did the phase form run?"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_bias_and_per_step_bias_once_per_output_pixel_in_every_phase(lib, dtype):
    """(e) zero activations: every output pixel of every phase is exactly round(bias + bias2); and with data, adding bias2 moves every
    pixel by bias2 (within one output rounding)"""
    B, Cc, H, W = 16, 1280, 64, 4
    x, w, b = _problem(B, Cc, H, W, dtype, 7)
    g = torch.Generator(device="cuda").manual_seed(8)
    b2 = torch.randn(Cc, device="cuda", generator=g)
    out0 = _run(lib, dtype, torch.zeros_like(x), w, b, b2, 1)
    want = (b + b2).to(TDT[dtype]).float().view(1, Cc, 1, 1).expand_as(out0)
    assert torch.equal(out0, want)
    out_a = _run(lib, dtype, x, w, b, None, 1)
    out_b = _run(lib, dtype, x, w, b, b2, 1)
    d = (out_b - out_a - b2.view(1, Cc, 1, 1)).abs()
    ulp = 2.0 ** (-10 if dtype == "fp16" else -7)
    bound = ulp * (out_a.abs() + out_b.abs()) + 1e-6          # one rounding of each output (half an ulp each, taken whole)
    assert (d <= bound).all(), "bias2 not applied exactly once somewhere: max excess %.3e" % (d - bound).max().item()
    for py in (0, 1):
        for px in (0, 1):
            assert (out_b[:, :, py::2, px::2] - out_a[:, :, py::2, px::2]).abs().max().item() > 0.5     # each phase got it
    # as the engine passes it: row `step` of a table through the device step counter (the other rows are O(1) away from b2)
    table = torch.stack([b2 + 3.0, b2 - 2.0, b2]).contiguous()
    out_t = torch.empty_like(out_b)
    plan = C.create_string_buffer(64)
    _KEEP.extend([table, out_t])
    check(lib, lib.tango_op_conv2d_ups_temb(DT[dtype], ptr(x), ptr(w), ptr(b), ptr(table), 3, 2, ptr(out_t), B, Cc, H, W, Cc, 1, plan, 64, None))
    assert plan.value.decode() == "conv_wide+phase"
    assert torch.equal(out_t, out_b), "row 2 of the table through the step counter is not the single row b2"


def test_full_size_unet_forward_switch_on_against_off(lib):
    """(f) the full-size fp16 UNet forward at the benchmarked batch (the inputs of tests/test_parity_batch_gpu.py, B = 32) with
    TANGO_UPS_PHASES=1 against =0.  The switch changes three of 66 convs by one weight rounding; the relative error between the two
    outputs must stay below the fp16-engine-vs-oracle error of the same forward, which tests/test_parity_batch_gpu.py measured at
    1.2e-3 ... 1.7e-3 on the parent (its comment above test_unet_and_loop_at_benchmarked_batch): the bound is the lower end."""
    from tango_amd.engine import UNET_CONFIG_LARGE, Engine
    ORACLE_ERR = 1.2e-3
    BMAX, L = 32, 64
    g = torch.Generator().manual_seed(3232)
    cond = torch.randn(BMAX, L, 1024, generator=g)
    unc = torch.randn(BMAX, L, 1024, generator=g)
    mask_c = torch.ones(BMAX, L, dtype=torch.bool)
    mask_c[1::3, 40:] = False
    mask_u = torch.zeros(BMAX, L, dtype=torch.bool)
    mask_u[:, 0] = True
    torch.randn(BMAX, 8, 256, 16, generator=g)
    torch.randn(3, BMAX, 8, 256, 16, generator=g)
    x2 = torch.randn(2 * BMAX, 8, 256, 16, generator=g)
    enc, mask = torch.cat([unc, cond]).cuda(), torch.cat([mask_u, mask_c]).cuda()
    e = Engine(unet=UNET_CONFIG_LARGE, dtype="fp16")
    e.load_synthetic(1234)
    outs = {}
    saved = os.environ.get("TANGO_UPS_PHASES")
    try:
        for sw in ("0", "1"):
            os.environ["TANGO_UPS_PHASES"] = sw
            lib.tango_tuning_reload()
            e.drop_plans()
            outs[sw] = e.unet_forward(x2.cuda(), 500, enc, mask).cpu()
    finally:
        if saved is None:
            os.environ.pop("TANGO_UPS_PHASES", None)
        else:
            os.environ["TANGO_UPS_PHASES"] = saved
        lib.tango_tuning_reload()
        e.drop_plans()
    del e
    rel = ((outs["1"] - outs["0"]).abs().max() / outs["0"].abs().max()).item()
    print("full-size fp16 UNet forward, UNet batch 64: phase form vs nine-tap form rel err %.3e (fp16 engine vs oracle on the parent: %.1e)"
          % (rel, ORACLE_ERR))
    assert torch.isfinite(outs["1"]).all()
    assert not torch.equal(outs["1"], outs["0"]), "the switch changed nothing"
    assert rel < ORACLE_ERR
