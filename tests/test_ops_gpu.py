"""Per-kernel parity: HIP op (through the C ABI) vs the fp32 torch CPU statement of the same op.
Tolerances: fp32 engine rel-err <= 2e-5 of the output scale (f32 MFMA == fmaf chain); fp16 engine
(fp16 operands, fp32 accumulate) <= 4e-3 of the output scale."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DT = {"fp32": 0, "fp16": 1, "bf16": 2}
TOL = {"fp32": 2e-5, "fp16": 4e-3, "bf16": 3e-2}


_KEEP = []


def dev(t):
    """device copy that stays alive until the next test (raw pointers are handed to the C ABI)"""
    d = t.detach().float().contiguous().cuda()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _clear_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def check(lib, rc):
    assert rc == 0, lib.tango_last_error().decode()


def close(out, ref, dtype, what=""):
    ref = ref.float().cpu()
    out = out.float().cpu()
    scale = ref.abs().max().item() + 1e-6
    err = (out - ref).abs().max().item() / scale
    assert err <= TOL[dtype], "%s: rel err %.3e > %.1e (scale %.3f)" % (what, err, TOL[dtype], scale)


def quant(t, dtype):
    """round operands to the engine storage dtype so the test isolates kernel arithmetic"""
    if dtype == "fp16":
        return t.half().float()
    if dtype == "bf16":
        return t.bfloat16().float()
    return t


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("M,N,K", [(200, 320, 320), (128, 128, 64), (77, 48, 96), (300, 640, 1280), (64, 24, 32), (130, 8, 64)])
def test_linear(lib, dtype, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = quant(torch.randn(M, K, generator=g), dtype)
    w = quant(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    r = quant(torch.randn(M, N, generator=g), dtype)
    out = torch.empty(M, N, device="cuda")
    check(lib, lib.tango_op_linear(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)), ptr(out), M, N, K, 0, 0, 0, None))
    close(out, F.linear(x, w, b) + r, dtype, "linear")
    # silu prologue + lrelu-free epilogue silu
    check(lib, lib.tango_op_linear(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), None, ptr(out), M, N, K, 1, 1, 0, None))
    close(out, F.silu(F.linear(quant(F.silu(x), dtype), w, b)), dtype, "linear+silu")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("M,N,K", [(128, 1280, 5120), (512, 640, 2560), (100, 320, 1280)])
def test_linear_splitk(lib, dtype, M, N, K):
    """small-M problems take the deterministic split-K path (partials + fixed-order reduce + epilogue)"""
    g = torch.Generator().manual_seed(M + N)
    x = quant(torch.randn(M, K, generator=g), dtype)
    w = quant(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    r = quant(torch.randn(M, N, generator=g), dtype)
    out = torch.empty(M, N, device="cuda")
    out2 = torch.empty(M, N, device="cuda")
    check(lib, lib.tango_op_linear(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)), ptr(out), M, N, K, 0, 1, 0, None))
    check(lib, lib.tango_op_linear(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)), ptr(out2), M, N, K, 0, 1, 0, None))
    close(out, F.silu(F.linear(x, w, b)) + r, dtype, "linear split-K")
    assert torch.equal(out, out2), "split-K must be run-to-run deterministic"


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_conv2d_splitk(lib, dtype):
    B, Cin, Cout, H, W = 2, 1280, 320, 8, 2
    g = torch.Generator().manual_seed(77)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x, w, b, padding=1)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_conv2d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Cin, H, W, Cout, 1, 0, None))
    close(out, ref, dtype, "conv2d split-K")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("M,C", [(150, 64), (1000, 320), (520, 640)])   # the larger two reach the LDS-DMA kernel when forced
def test_linear_geglu(lib, dtype, M, C):
    g = torch.Generator().manual_seed(5 + M)
    x = quant(torch.randn(M, C, generator=g), dtype)
    w = quant(torch.randn(8 * C, C, generator=g) / C ** 0.5, dtype)
    b = torch.randn(8 * C, generator=g)
    out = torch.empty(M, 4 * C, device="cuda")
    check(lib, lib.tango_op_linear(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), None, ptr(out), M, 8 * C, C, 0, 0, 1, None))
    h = F.linear(x, w, b)
    val, gate = h.chunk(2, dim=-1)
    close(out, val * F.gelu(gate), dtype, "geglu")


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("M,N,K,geglu,res", [(4128, 320, 320, 0, 1), (8192, 960, 320, 0, 0), (4100, 2560, 320, 1, 0), (4096, 640, 640, 0, 1),
                                             (5000, 1920, 640, 0, 0), (4096, 320, 1280, 0, 1), (300, 320, 320, 0, 0)])
def test_linear_layernorm_fused(lib, dtype, M, N, K, geglu, res):
    """weight-stationary streaming linear (K*sizeof(T) in {640,1280} B, M >= 4096) with LayerNorm folded into the
    weights vs LayerNorm -> Linear (-> GEGLU) (+ residual); other shapes take the LN-kernel + GEMM fallback"""
    g = torch.Generator().manual_seed(M + N + K)
    x = quant(torch.randn(M, K, generator=g) * 1.3 + 0.7, dtype)
    w = quant(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    ga, be = 1 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    No = N // 2 if geglu else N
    r = quant(torch.randn(M, No, generator=g), dtype) if res else None
    h = F.linear(F.layer_norm(x, (K,), ga, be, 1e-5), w, b)
    if geglu:
        v, gt = h.chunk(2, dim=-1)
        h = v * F.gelu(gt)
    ref = h + r if res else h
    out = torch.empty(M, No, device="cuda")
    check(lib, lib.tango_op_linear_ln(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(ga)), ptr(dev(be)),
                                      ptr(dev(r)) if res else None, ptr(out), M, N, K, geglu, 1e-5, None))
    ref = ref.float()
    scale = ref.abs().max().item()
    err = (out.cpu() - ref).abs().max().item() / scale
    # the folded form keeps x un-normalised in T: its rounding is relative to |x| (not |x - mean|), so allow 2x
    assert err <= 2 * TOL[dtype], "linear_ln rel err %.3e" % err


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_linear_stream_plain(lib, dtype):
    """same kernel without LayerNorm: bias + residual, M not a multiple of 32"""
    M, N, K = 4130, 320, 320
    g = torch.Generator().manual_seed(9)
    x = quant(torch.randn(M, K, generator=g), dtype)
    w = quant(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    r = quant(torch.randn(M, N, generator=g), dtype)
    out = torch.empty(M, N, device="cuda")
    check(lib, lib.tango_op_linear(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)), ptr(out), M, N, K, 0, 0, 0, None))
    close(out, F.linear(x, w, b) + r, dtype, "linear stream")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("Cin,Cout,H,W,stride,ups", [(64, 64, 16, 8, 1, 0), (64, 96, 16, 8, 2, 0), (64, 32, 8, 4, 1, 1),
                                                    (8, 64, 16, 16, 1, 0), (128, 160, 6, 2, 1, 0), (32, 8, 16, 4, 1, 0)])
def test_conv2d(lib, dtype, Cin, Cout, H, W, stride, ups):
    if dtype == "fp16" and (Cin * 2) % 64 and Cin != 8:
        pytest.skip("Cin*2 bytes must be a 64-byte multiple")
    B = 3
    g = torch.Generator().manual_seed(Cin * Cout + H)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
    ref = F.conv2d(xin, w, b, stride=stride, padding=1)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_conv2d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Cin, H, W, Cout, stride, ups, None))
    close(out, ref, dtype, "conv2d")


# Halo-reuse 3x3 conv (conv_halo.hip): tile counts >= 256 select it without any env switch.  Geometries: 16-wide rows
# (UNet level 0), 8- and 4-wide (levels 1, 2: fragments straddle image rows), 64-wide (VAE), whole-image segments
# (8x8 images, 4 per tile: the 400-row LDS maximum), BN = 160 and 128, several channel chunks.
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,Cin,Cout,H,W", [(16, 64, 640, 64, 16), (32, 128, 640, 64, 8), (64, 192, 640, 64, 4),
                                            (32, 64, 512, 8, 64), (256, 64, 512, 8, 8), (2, 64, 1280, 256, 16)])
def test_conv2d_halo(lib, dtype, B, Cin, Cout, H, W):
    _conv2d_halo_case(lib, dtype, B, Cin, Cout, H, W, 0)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("B,Cin,Cout,H,W", [(16, 64, 640, 32, 8), (32, 128, 640, 32, 4), (8, 64, 512, 16, 32)])
def test_conv2d_halo_upsampled(lib, dtype, B, Cin, Cout, H, W):
    """nearest x2 upsample fused into the halo gather (Upsample2D, diffusers resnet.py:90-137): H, W are the SOURCE dims"""
    _conv2d_halo_case(lib, dtype, B, Cin, Cout, H, W, 1)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("B,Cin,Cout,H,W", [(16, 320, 8, 256, 16), (64, 64, 4, 64, 16), (32, 128, 32, 64, 8), (1024, 64, 24, 8, 8)])
def test_conv2d_halo_narrow_output(lib, dtype, B, Cin, Cout, H, W):
    """the UNet's conv_out (320 -> 8 channels; unet_2d_condition.py conv_out) and other narrow outputs on the halo kernel's 256 x 32 tile (round 6: weight
    rows beyond N come from the zero page) -- against torch, and against the 256 x 16 / 256 x 32 tile kernels it replaces (TANGO_NO_HALO_NARROW=1)"""
    import os
    _conv2d_halo_case(lib, dtype, B, Cin, Cout, H, W, 0)
    g = torch.Generator().manual_seed(Cin * Cout + H + W)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    outs = []
    for off in ("0", "1"):
        os.environ["TANGO_NO_HALO_NARROW"] = off
        lib.tango_tuning_reload()
        try:
            out = torch.empty(B, Cout, H, W, device="cuda")
            check(lib, lib.tango_op_conv2d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Cin, H, W, Cout, 1, 0, None))
            outs.append(out.cpu())
        finally:
            os.environ.pop("TANGO_NO_HALO_NARROW", None)
            lib.tango_tuning_reload()
    d = (outs[0] - outs[1]).abs().max().item() / outs[1].abs().max().item()
    assert d <= (4e-3 if dtype == "fp16" else 2e-2), "halo 256 x 32 tile vs the tile kernel: %.3e" % d


def _conv2d_halo_case(lib, dtype, B, Cin, Cout, H, W, ups):
    g = torch.Generator().manual_seed(Cin * Cout + H + W)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if ups else x
    ref = F.conv2d(xin, w, b, padding=1)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_conv2d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Cin, H, W, Cout, 1, ups, None))
    close(out, ref, dtype, "conv2d halo")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("C,Co,L,k,d", [(32, 32, 301, 3, 1), (32, 32, 301, 7, 3), (64, 64, 200, 11, 5), (64, 128, 77, 7, 1), (32, 1, 500, 7, 1)])
def test_conv1d(lib, dtype, C, Co, L, k, d):
    B = 2
    g = torch.Generator().manual_seed(C + L + k)
    x = quant(torch.randn(B, C, L, generator=g), dtype)
    w = quant(torch.randn(Co, C, k, generator=g) / (C * k) ** 0.5, dtype)
    b = torch.randn(Co, generator=g)
    r = quant(torch.randn(B, Co, L, generator=g), dtype)
    ref = F.leaky_relu(F.conv1d(quant(F.leaky_relu(x, 0.1), dtype), w, b, dilation=d, padding=d * (k - 1) // 2), 0.1) + r
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_conv1d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)), ptr(out), B, C, L, Co, k, d,
                                   2, 0.1, 2, 0.1, None))
    close(out, ref, dtype, "conv1d")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("Ci,Co,L,k,u", [(64, 32, 50, 16, 5), (64, 32, 53, 16, 4), (32, 32, 40, 8, 2), (64, 32, 31, 4, 2)])
def test_conv_transpose1d(lib, dtype, Ci, Co, L, k, u):
    B = 2
    p = (k - u) // 2
    g = torch.Generator().manual_seed(Ci + L + k)
    x = quant(torch.randn(B, Ci, L, generator=g), dtype)
    w = quant(torch.randn(Ci, Co, k, generator=g) / (Ci * k / u) ** 0.5, dtype)
    b = torch.randn(Co, generator=g)
    ref = F.conv_transpose1d(quant(F.leaky_relu(x, 0.1), dtype), w, b, stride=u, padding=p)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_conv_transpose1d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Ci, L, Co, k, u, p,
                                             2, 0.1, None))
    close(out, ref, dtype, "conv_transpose1d")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("C,HW,eps,act", [(320, 512, 1e-5, 1), (64, 4096, 1e-6, 0), (512, 100, 1e-6, 1), (2560, 64, 1e-5, 1), (1920, 33, 1e-5, 0), (128, 7000, 1e-6, 1),
                                              (320, 16384, 1e-5, 1), (640, 6000, 1e-5, 0)])  # last two: multi-kernel (large) path
def test_groupnorm(lib, dtype, C, HW, eps, act):
    B = 3
    g = torch.Generator().manual_seed(C + HW)
    x = quant(torch.randn(B, C, HW, generator=g) * 1.7 + 0.4, dtype)
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x, 32, ga, be, eps)
    if act:
        ref = F.silu(ref)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_groupnorm(DT[dtype], ptr(dev(x)), ptr(dev(ga)), ptr(dev(be)), ptr(out), B, C, HW, 32, eps, act, None))
    close(out, ref, dtype, "groupnorm")


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rows,C", [(100, 320), (37, 1280), (513, 64), (16, 640)])
def test_layernorm(lib, dtype, rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x = quant(torch.randn(rows, C, generator=g) * 2 - 0.3, dtype)
    ga, be = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x, (C,), ga, be, 1e-5)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_layernorm(DT[dtype], ptr(dev(x)), ptr(dev(ga)), ptr(dev(be)), ptr(out), rows, C, 1e-5, None))
    close(out, ref, dtype, "layernorm")


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B,heads,Sq,Skv,masked", [(2, 2, 256, 256, False), (2, 3, 64, 64, False), (3, 1, 200, 7, True),
                                                   (2, 2, 1024, 64, True), (1, 5, 130, 130, False)])
def test_attention(lib, dtype, B, heads, Sq, Skv, masked):
    g = torch.Generator().manual_seed(Sq + Skv)
    C_ = heads * 64
    q = quant(torch.randn(B, Sq, C_, generator=g), dtype)
    k = quant(torch.randn(B, Skv, C_, generator=g), dtype)
    v = quant(torch.randn(B, Skv, C_, generator=g), dtype)
    bias = None
    if masked:
        m = torch.ones(B, Skv)
        m[0, 1:] = 0
        if B > 1:
            m[1, Skv // 2:] = 0
        bias = (1 - m) * -10000.0
    qh = q.view(B, Sq, heads, 64).transpose(1, 2)
    kh = k.view(B, Skv, heads, 64).transpose(1, 2)
    vh = v.view(B, Skv, heads, 64).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) * 0.125
    if bias is not None:
        s = s + bias[:, None, None, :]
    ref = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, Sq, C_)
    out = torch.empty(ref.shape, device="cuda")
    check(lib, lib.tango_op_attention(DT[dtype], ptr(dev(q)), ptr(dev(k)), ptr(dev(v)), ptr(dev(bias)) if bias is not None else None,
                                      ptr(out), B, heads, Sq, Skv, 0.125, None))
    close(out, ref, dtype, "attention")


@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
def test_sched_step_bit_exact(lib, pred):
    """fused CFG + DDPM step == oracle scheduler step, bit for bit (fp32, unfused mul/add order)."""
    from oracle import tango_oracle as O
    cfg = dict(O.SD21_SCHEDULER, prediction_type=pred)
    sch = O.DDPMOracle(**cfg)
    sch.set_timesteps(200)
    B, Cc, HW = 2, 8, 4096
    g = torch.Generator().manual_seed(3)
    for t in (995, 500, 5, 0):
        lat = torch.randn(B, Cc, 256, 16, generator=g)
        mo = torch.randn(2 * B, Cc, 256, 16, generator=g)
        nz = torch.randn(B, Cc, 256, 16, generator=g)
        u, c = mo.chunk(2)
        guided = u + 3.0 * (c - u)
        ref = sch.step(guided, t, lat, noise=nz)
        coef = np.asarray(sch.coefficients(t) + [0, 0, 0], dtype=np.float32)
        lat_d = dev(lat)
        check(lib, lib.tango_op_sched_step(ptr(lat_d), ptr(dev(mo)), ptr(dev(nz)), coef.ctypes.data_as(C.c_void_p), B, Cc, HW, 1, 3.0,
                                           {"epsilon": 0, "v_prediction": 2}[pred], 0, 0, 1.0, None))
        assert torch.equal(lat_d.cpu(), ref), "t=%d max diff %g" % (t, (lat_d.cpu() - ref).abs().max())


@pytest.mark.parametrize("rule", ["ddpm", "ddim"])
@pytest.mark.parametrize("pred", ["v_prediction", "epsilon"])
def test_sched_step_clip_bit_exact(lib, pred, rule):
    """clip_sample through tango_op_sched_step == the oracle's DDPM / DDIM step with clip_sample=True, bit for bit, with and without
    CFG, at an early and a late timestep.  HW = 300: two workgroups per sample pair, the last one partly empty.  The range is 1.0
    except for epsilon at t = 995, where x0 = (x - sqrt(1 - abar) v) / sqrt(abar) with sqrt(abar) = 0.068 has a spread of about 15
    (55 with CFG) and a range of 1.0 would clip nearly everything: 16.0 there.  Each case first shows on the oracle alone that the
    clip changes between 10 % and 90 % of the result."""
    from oracle import tango_oracle as O
    from tango_amd.scheduler import DDIMScheduler
    B, Cc, HW, N = 2, 8, 300, 200
    base = dict(O.SD21_SCHEDULER, prediction_type=pred)
    cls = O.DDPMOracle if rule == "ddpm" else O.DDIMOracle
    ddim_rows = None
    if rule == "ddim":
        host = DDIMScheduler(**{k: v for k, v in base.items() if k != "variance_type"})
        host.set_timesteps(N)
        ddim_rows = dict(zip(host.timesteps.tolist(), host.coef_table()))
    g = torch.Generator().manual_seed(17)
    for cfg_on in (True, False):
        for t in (995, 5):
            rng = 16.0 if (pred == "epsilon" and t == 995) else 1.0
            sch, plain = cls(**dict(base, clip_sample=True, clip_sample_range=rng)), cls(**dict(base, clip_sample=False))
            sch.set_timesteps(N)
            plain.set_timesteps(N)
            lat = torch.randn(B, Cc, HW, generator=g)
            mo = torch.randn(2 * B if cfg_on else B, Cc, HW, generator=g)
            nz = torch.randn(B, Cc, HW, generator=g)
            model = mo.chunk(2)[0] + 3.0 * (mo.chunk(2)[1] - mo.chunk(2)[0]) if cfg_on else mo
            ref, unclipped = sch.step(model, t, lat, noise=nz), plain.step(model, t, lat, noise=nz)
            changed = (ref != unclipped).float().mean().item()
            assert 0.1 <= changed <= 0.9, "cfg %s t=%d: the clip changes %.0f %% of the reference" % (cfg_on, t, 100 * changed)
            row = np.asarray(sch.coefficients(t) + [0, 0, 0], dtype=np.float32) if rule == "ddpm" else np.ascontiguousarray(ddim_rows[t])
            lat_d = dev(lat)
            check(lib, lib.tango_op_sched_step(ptr(lat_d), ptr(dev(mo)), ptr(dev(nz)), row.ctypes.data_as(C.c_void_p), B, Cc, HW,
                                               1 if cfg_on else 0, 3.0, {"epsilon": 0, "v_prediction": 2}[pred],
                                               0 if rule == "ddpm" else 1, 1, rng, None))
            got = lat_d.cpu()
            assert torch.equal(got, ref), "cfg %s t=%d max diff %g" % (cfg_on, t, (got - ref).abs().max())
            assert not torch.equal(got, unclipped)
