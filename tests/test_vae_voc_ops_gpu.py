"""Per-operator parity of the gather-GEMM modes, epilogues and elementwise kernels that only the mel-VAE and HiFi-GAN plans use (and the
large-batch routes of stride-2 / conv1d problems), each against the torch-CPU statement of the op on operands rounded to the engine dtype.
The end-to-end VAE / vocoder tests see these kernels at B = 2 through whole-tensor tolerances; here every case is the smallest shape that
reaches the kernel and its edges, and every case that claims a kernel first asserts the route (tests/test_vae_voc_routes.py holds the
shape tables and the host-side queries).  Tolerances are those of tests/test_ops_gpu.py: fp32 2e-5, fp16 4e-3, bf16 3e-2 of the output scale."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_duo_gpu import tuning
from test_ops_gpu import DT, TOL, _clear_keep, check, close, dev, ptr, quant  # noqa: F401  (_clear_keep: autouse fixture that frees dev() copies)
from test_vae_voc_routes import (CONV_OUT_BIG, CONV_OUT_SMALL, DMA_CONV1D, DMA_CONV1D_FP32, DMA_CONV2D, DMA_CONVT, FORCED, TILE_PAD,
                                 conv1d_route, conv2d_route, convt_phase_routes, tile_pad_expect)

pytestmark = pytest.mark.gpu

ALL = ["fp32", "fp16", "bf16"]
EPS = {"fp32": 2.0 ** -23, "fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
EPV = {"fp32": 4, "fp16": 8, "bf16": 8}          # elements per 16-byte vector


def down_ref(x, w, b, pad):
    """pad 1: Conv2d(k3, s2, p1); pad 0: the VAE Downsample, F.pad(x, (0,1,0,1)) + Conv2d(k3, s2, p0)"""
    return F.conv2d(x, w, b, stride=2, padding=1) if pad else F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


def conv2d_ex(lib, dtype, x, w, b, r, stride, pad, e_act=0, e_slope=0.0, out_f32=0):
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H + pad - 2) // stride + 1, (W + pad - 2) // stride + 1
    out = torch.zeros(B, Cout, Ho, Wo, device="cuda")
    check(lib, lib.tango_op_conv2d_ex(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)) if r is not None else None, ptr(out),
                                      B, Cin, H, W, Cout, stride, pad, e_act, e_slope, out_f32, None))
    return out


# ---- a. gemm_dma_kernel<MODE_CONV2D>: stride 2, pad 1 and pad 0 ----
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("case", DMA_CONV2D)
def test_dma_conv2d_stride2(lib, dtype, case):
    B, Cin, H, W, Cout, pad, res = case
    g = torch.Generator().manual_seed(B + H + W + Cout + pad)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    ref = down_ref(x, w, b, pad)
    r = quant(torch.randn(ref.shape, generator=g), dtype) if res else None
    if res:
        ref = ref + r
    with tuning(lib, **FORCED):
        assert conv2d_route(lib, dtype, B, Cin, H, W, Cout, 2, pad, res) == ("dma", 1)
        out = conv2d_ex(lib, dtype, x, w, b, r, 2, pad)
    close(out, ref, dtype, "DMA conv2d stride 2 pad %d" % pad)
    # the far edge on its own: with pad 0 the last output row / column is where a tap leaves the image
    close(out[:, :, -1, :], ref[:, :, -1, :], dtype, "last output row")
    close(out[:, :, :, -1], ref[:, :, :, -1], dtype, "last output column")
    close(out[:, :, 0, :], ref[:, :, 0, :], dtype, "first output row")


# ---- b. gemm_kernel<MODE_CONV2D> with both paddings at tiny shapes ----
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("Cout,H,W", TILE_PAD)
def test_tile_conv2d_pad(lib, dtype, pad, Cout, H, W):
    B, Cin = 3, 64
    g = torch.Generator().manual_seed(Cout + 10 * H + W)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    ref = down_ref(x.double(), w.double(), b.double(), pad)
    other = down_ref(x.double(), w.double(), b.double(), 1 - pad)
    assert (ref - other).abs().max() > 0.1, "the two paddings must differ on this input, or a mix-up would pass"
    assert conv2d_route(lib, dtype, B, Cin, H, W, Cout, 2, pad) == tile_pad_expect(dtype, Cout)
    out = conv2d_ex(lib, dtype, x, w, b, None, 2, pad)
    close(out, ref, dtype, "tile conv2d stride 2 pad %d" % pad)


# ---- c. gemm_dma_kernel<MODE_CONV1D>: dilated conv1d with residual / leaky-ReLU epilogue ----
def _conv1d_case(lib, dtype, case, a_act, want):
    Cin, Cout, L, k, d, res, e_act = case
    B = 2
    g = torch.Generator().manual_seed(Cin + Cout + L + k + d)
    x = quant(torch.randn(B, Cin, L, generator=g), dtype)
    w = quant(torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5, dtype)
    b = torch.randn(Cout, generator=g)
    r = quant(torch.randn(B, Cout, L, generator=g), dtype) if res else None
    xin = quant(F.leaky_relu(x, 0.1), dtype) if a_act else x
    ref = F.conv1d(xin.double(), w.double(), b.double(), dilation=d, padding=d * (k - 1) // 2)
    if e_act:
        ref = F.leaky_relu(ref, 0.1)
    if res:
        ref = ref + r.double()
    out = torch.zeros(B, Cout, L, device="cuda")
    with tuning(lib, **FORCED):
        assert conv1d_route(lib, dtype, B, Cin, L, Cout, k, d, a_act, res, e_act) == want
        check(lib, lib.tango_op_conv1d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(dev(r)) if res else None, ptr(out), B, Cin, L, Cout,
                                       k, d, a_act, 0.1, e_act, 0.1, None))
    close(out, ref, dtype, "conv1d k=%d d=%d on %s" % (k, d, want[0]))
    pad = min(d * (k - 1) // 2, L)
    close(out[:, :, :pad], ref[:, :, :pad], dtype, "left border")
    close(out[:, :, L - pad:], ref[:, :, L - pad:], dtype, "right border")


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("case", DMA_CONV1D)
def test_dma_conv1d(lib, dtype, case):
    _conv1d_case(lib, dtype, case, 0, ("dma", 1))


@pytest.mark.parametrize("case", DMA_CONV1D_FP32)
def test_dma_conv1d_fp32_narrow_cin(lib, case):
    _conv1d_case(lib, "fp32", case, 0, ("dma", 1))


@pytest.mark.parametrize("dtype", ALL)
def test_conv1d_prologue_runs_on_the_tile_kernel(lib, dtype):
    _conv1d_case(lib, dtype, DMA_CONV1D[0], 2, ("tile", 1))


# ---- d. gemm_dma_kernel<MODE_CONV1D> through the transposed-conv phase decomposition (tap_step -1, in_off, out_mul, out_off) ----
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("k,u,L", DMA_CONVT)
def test_dma_conv_transpose1d(lib, dtype, k, u, L):
    B, Ci, Co = 2, 128, 128
    pd = (k - u) // 2
    g = torch.Generator().manual_seed(L + k + u)
    x = quant(torch.randn(B, Ci, L, generator=g), dtype)
    w = quant(torch.randn(Ci, Co, k, generator=g) / (Ci * k / u) ** 0.5, dtype)
    b = torch.randn(Co, generator=g)
    ref = F.conv_transpose1d(x.double(), w.double(), b.double(), stride=u, padding=pd)
    out = torch.zeros(ref.shape, device="cuda")
    with tuning(lib, **FORCED):
        phases = convt_phase_routes(lib, dtype, B, Ci, L, Co, k, u)
        assert len(phases) == u and all(p[2:] == ("dma", 1) for p in phases), phases
        check(lib, lib.tango_op_conv_transpose1d(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Ci, L, Co, k, u, pd, 0, 0.0, None))
    close(out, ref, dtype, "conv_transpose1d k=%d u=%d on the DMA kernel" % (k, u))
    close(out[:, :, :k], ref[:, :, :k], dtype, "left border")
    close(out[:, :, -k:], ref[:, :, -k:], dtype, "right border")


# ---- e. batched GEMM: the three shapes of Builder::vae_attn ----
def gemm_batched(lib, dtype, a, w, bias, shape, K, lda, ldw, w_col_off=0, a_shared=0, alpha=1.0, bias_rows=0):
    batch, M, N = shape
    out = torch.zeros(batch, M, N, device="cuda")
    check(lib, lib.tango_op_gemm_batched(DT[dtype], ptr(dev(a)), ptr(dev(w)) if w is not None else None, ptr(dev(bias)) if bias is not None else None,
                                         ptr(out), batch, M, N, K, lda, ldw, w_col_off, a_shared, alpha, bias_rows, None))
    return out


def _attn_operands(dtype, C_, HW, batch):
    g = torch.Generator().manual_seed(C_ + HW)
    hn = quant(torch.randn(batch, HW, C_, generator=g), dtype)
    wv = quant(torch.randn(C_, C_, generator=g) / C_ ** 0.5, dtype)
    bv = torch.randn(C_, generator=g)
    qk = quant(torch.randn(batch, HW, 2 * C_, generator=g), dtype)
    return hn, wv, bv, qk


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("C_", [96, 160])
def test_batched_gemm_vae_attn_shapes(lib, dtype, C_):
    HW, batch = 224, 3
    hn, wv, bv, qk = _attn_operands(dtype, C_, HW, batch)
    # V^T[b] = Wv hn[b]^T + bv (per output ROW): one A shared by the batch (sA = 0), bias_rows
    vt = gemm_batched(lib, dtype, wv, hn, bv, (batch, C_, HW), C_, C_, C_, a_shared=1, bias_rows=1)
    vt_ref = wv.double() @ hn.double().transpose(1, 2) + bv.double()[None, :, None]
    close(vt, vt_ref, dtype, "V^T (shared A, bias_rows)")
    # scores[b] = C^-0.5 q[b] k[b]^T: q and k are the two column halves of one buffer (lda = ldw = 2C, W = A + C columns)
    alpha = 1.0 / C_ ** 0.5
    sc = gemm_batched(lib, dtype, qk, None, None, (batch, HW, HW), C_, 2 * C_, 2 * C_, w_col_off=C_, alpha=alpha)
    q, k = qk.double()[:, :, :C_], qk.double()[:, :, C_:]
    sc_ref = q @ k.transpose(1, 2) * float(np.float32(alpha))
    close(sc, sc_ref, dtype, "scores (alpha, W inside A)")
    # out[b] = P[b] V[b]: K = HW
    p = quant(sc_ref.float().softmax(-1), dtype)
    vtq = quant(vt_ref.float(), dtype)
    ao = gemm_batched(lib, dtype, p, vtq, None, (batch, HW, C_), HW, HW, HW)
    close(ao, p.double() @ vtq.double().transpose(1, 2), dtype, "P.V")
    # every batch item must have used ITS operands: the items differ
    assert (sc_ref[0] - sc_ref[1]).abs().max() > 0.5


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("C_", [96, 160])
def test_vae_attention_chain(lib, dtype, C_):
    """the four launches of Builder::vae_attn between the q | k projection and proj_out, chained on the engine-dtype intermediates, against
    single-head attention of head dim C in fp64 (audioldm modules.py AttnBlock)"""
    HW, batch = 224, 3
    hn, wv, bv, qk = _attn_operands(dtype, C_, HW, batch)
    vt = gemm_batched(lib, dtype, wv, hn, bv, (batch, C_, HW), C_, C_, C_, a_shared=1, bias_rows=1)
    sc = gemm_batched(lib, dtype, qk, None, None, (batch, HW, HW), C_, 2 * C_, 2 * C_, w_col_off=C_, alpha=1.0 / C_ ** 0.5)
    pr = torch.zeros(batch * HW, HW, device="cuda")
    check(lib, lib.tango_op_softmax_rows(DT[dtype], ptr(sc), ptr(pr), batch * HW, HW, 1.0, None))
    ao = gemm_batched(lib, dtype, pr.view(batch, HW, HW).cpu(), vt.cpu(), None, (batch, HW, C_), HW, HW, HW)
    q, k = qk.double()[:, :, :C_], qk.double()[:, :, C_:]
    v = hn.double() @ wv.double().t() + bv.double()
    ref = (q @ k.transpose(1, 2) / C_ ** 0.5).softmax(-1) @ v
    close(ao, ref, dtype, "vae attention chain")


# ---- f. softmax_rows ----
def _softmax_inputs(rows, cols, g):
    """(name, x, scale); scales are non-unit.  The rows around -10000 use scale 0.5: x * scale is then exact in fp32, so the fp64 reference and the
    kernel exponentiate the same numbers (a rounded product of magnitude 7000 would move the exponent by up to 2.4e-4)"""
    rnd = torch.randn(rows, cols, generator=g) * 3
    spike = torch.randn(rows, cols, generator=g)
    spike[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] += 30.0
    return [("random", rnd, 0.7),
            ("all equal", torch.full((rows, cols), 1.25) * torch.arange(1, rows + 1)[:, None], 0.7),
            ("one element 30 above", spike, 1.3),
            ("around -10000", -10000.0 + 8 * torch.randn(rows, cols, generator=g), 0.5)]


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("cols", ["vec", 2400, 4096])
def test_softmax_rows(lib, dtype, rows, cols):
    cols = EPV[dtype] if cols == "vec" else cols
    g = torch.Generator().manual_seed(rows + cols)
    for name, x, scale in _softmax_inputs(rows, cols, g):
        x = quant(x, dtype)
        ref = (x.double() * float(np.float32(scale))).softmax(-1)
        out = torch.zeros(rows, cols, device="cuda")
        check(lib, lib.tango_op_softmax_rows(DT[dtype], ptr(dev(x)), ptr(out), rows, cols, scale, None))
        out = out.cpu()
        for r in (0, rows - 1):       # close() scales by the tensor's maximum: rows have their own
            close(out[r], ref[r], dtype, "softmax_rows %s, row %d" % (name, r))
        close(out, ref, dtype, "softmax_rows %s" % name)
        dev1 = (out.double().sum(-1) - 1).abs().max().item()
        assert dev1 <= cols * EPS[dtype], "softmax_rows %s: a row sums to 1 %+.3e (bound %.3e)" % (name, dev1, cols * EPS[dtype])
    bad = torch.zeros(1, cols + 1, device="cuda")
    assert lib.tango_op_softmax_rows(DT[dtype], ptr(bad), ptr(bad), 1, cols + 1, 1.0, None) != 0, "cols must be whole 16-byte vectors"


# ---- g. conv_post: EPI_I16 + tanh + out_scale 32768 at N = 1 ----
def _conv_post(lib, dtype, x, w, b):
    B, Cin, L = x.shape
    out = torch.zeros(B, L, dtype=torch.int16, device="cuda")
    check(lib, lib.tango_op_conv1d_i16(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)), ptr(out), B, Cin, L, 1, w.shape[2], 1, None))
    y = F.conv1d(x.double(), w.double(), b.double(), padding=(w.shape[2] - 1) // 2)[:, 0].numpy()
    ref = np.int32(np.trunc(np.tanh(y) * 32768)).astype(np.int16)      # truncation toward zero, int16 wrap
    return out.cpu().numpy(), ref, y


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("L", [500, 77])
def test_conv_post_int16(lib, dtype, L):
    B, Cin, k = 2, 32, 7
    assert conv1d_route(lib, dtype, B, Cin, L, 1, k, 1) == ("tile", 1)
    g = torch.Generator().manual_seed(L)
    x = quant(torch.randn(B, Cin, L, generator=g), dtype)
    w = quant(torch.randn(1, Cin, k, generator=g) / (Cin * k) ** 0.5, dtype)
    b = torch.tensor([0.1])
    out, ref, y = _conv_post(lib, dtype, x, w, b)
    assert np.abs(y).max() <= 4.5 and np.abs(y).max() > 2.0        # tanh(4.5) * 32768 = 32759.9: no sample near the wrap, yet well into the knee
    diff = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    assert diff.max() <= 1, "conv_post %s: %d samples off by more than 1 LSB (max %d)" % (dtype, (diff > 1).sum(), diff.max())
    assert (out < 0).any() and (out > 0).any()
    # truncation toward zero, not rounding and not floor: either would put about half of the samples one LSB off.  The allowed flips are the
    # samples whose scaled value lies within the fp32 error of an integer: |dy| ~ 1e-6 is 0.03 LSB, so at most ~6 % of them
    assert (diff == 0).mean() >= 0.9, "conv_post %s: only %.1f %% of the samples are exact" % (dtype, 100 * (diff == 0).mean())


@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("bias", [30.0, -30.0])
def test_conv_post_saturated(lib, dtype, bias):
    """|y| ~ 30: tanhf is exactly +-1.0f, +32768 wraps to -32768 as the reference's astype(int16) does; -32768 is representable"""
    B, Cin, k, L = 2, 32, 7, 77
    g = torch.Generator().manual_seed(7)
    x = quant(torch.randn(B, Cin, L, generator=g), dtype)
    w = quant(torch.randn(1, Cin, k, generator=g) * 1e-3, dtype)
    out, ref, y = _conv_post(lib, dtype, x, w, torch.tensor([bias]))
    assert (ref == -32768).all() and np.abs(y).min() > 29
    assert (out == ref).all(), "conv_post saturated %+g: %s" % (bias, np.unique(out))


# ---- h. the VAE's conv_out: fp32 output with ldo = 1, N = 1 ----
def _conv_out_case(lib, dtype, B, H, W, want):
    Cin = 128
    g = torch.Generator().manual_seed(B + H + W)
    x = quant(torch.randn(B, Cin, H, W, generator=g), dtype)
    w = quant(torch.randn(1, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, dtype)
    b = torch.randn(1, generator=g)
    ref = F.conv2d(x, w, b, padding=1)
    assert conv2d_route(lib, dtype, B, Cin, H, W, 1, 1, 1, 0, 0, 1) == want
    out = conv2d_ex(lib, dtype, x, w, b, None, 1, 1, out_f32=1)
    close(out, ref, dtype, "conv_out (fp32 output) on %s" % want[0])
    for sl in ((Ellipsis, 0, slice(None)), (Ellipsis, H - 1, slice(None)), (Ellipsis, slice(None), 0), (Ellipsis, slice(None), W - 1)):
        close(out[sl], ref[sl], dtype, "conv_out image border")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_conv_out_f32_halo_narrow(lib, dtype):
    _conv_out_case(lib, dtype, *CONV_OUT_BIG, ("conv_halo", 1))


@pytest.mark.parametrize("dtype,shape", [("fp32", CONV_OUT_BIG), ("fp32", CONV_OUT_SMALL), ("fp16", CONV_OUT_SMALL), ("bf16", CONV_OUT_SMALL)])
def test_conv_out_f32_tile(lib, dtype, shape):
    _conv_out_case(lib, dtype, *shape, ("tile", 1))


# ---- i. avg3_act: one vector, and the grid-strided sweep above 8192 blocks with a partial last pass ----
def _avg3(lib, dtype, n, slopes):
    g = torch.Generator().manual_seed(n % 1000)
    a, b, c = (quant(torch.randn(n, generator=g), dtype) for _ in range(3))
    da, db, dc = dev(a), dev(b), dev(c)
    s3 = ((a + b) + c) / 3          # reference order (hifigan models.py: xs = xs + resblock(x); x = xs / num_kernels), fp32 like the kernel
    for slope in slopes:
        out = torch.zeros(n, device="cuda")
        check(lib, lib.tango_op_avg3_act(DT[dtype], ptr(da), ptr(db), ptr(dc), ptr(out), n, 1.0 / 3.0, 2, slope, None))
        ref = F.leaky_relu(s3, slope)
        out = out.cpu()
        close(out, ref, dtype, "avg3_act n=%d slope %g" % (n, slope))
        close(out[-300 * EPV[dtype]:], ref[-300 * EPV[dtype]:], dtype, "avg3_act tail")
        neg = s3 < -0.5             # the slope itself: negative outputs are small, the whole-tensor scale would hide a wrong one
        if neg.any():
            close(out[neg], ref[neg], dtype, "avg3_act negative side, slope %g" % slope)


@pytest.mark.parametrize("dtype", ALL)
def test_avg3_act_one_vector(lib, dtype):
    _avg3(lib, dtype, EPV[dtype], (0.1, 0.01))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_avg3_act_strided_sweep(lib, dtype):
    """8192 blocks x 256 threads x one vector is one pass of the capped grid; 300 more vectors make the second pass a partial one"""
    _avg3(lib, dtype, (8192 * 256 + 300) * EPV[dtype], (0.1, 0.01))


@pytest.mark.parametrize("dtype", ALL)
def test_avg3_act_refuses_partial_vectors(lib, dtype):
    n = 3 * EPV[dtype] + 1
    z = torch.zeros(n, device="cuda")
    out = torch.full((n,), 7.0, device="cuda")
    assert lib.tango_op_avg3_act(DT[dtype], ptr(z), ptr(z), ptr(z), ptr(out), n, 1.0 / 3.0, 2, 0.1, None) != 0
    assert b"avg3" in lib.tango_last_error()
    assert (out == 7.0).all(), "nothing may be launched"


# ---- j. the VAE's pointwise (1x1, tiny C) kernels ----
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("HW", [100, 4096])
@pytest.mark.parametrize("bias", [True, False])
def test_pointwise_small(lib, dtype, HW, bias):
    """post_quant_conv of z / scale_factor into channels-last engine-dtype rows (8 -> 8 channels, ld = 8)"""
    B, Ci, Co, scale = 3, 8, 8, 1.0 / 0.9227914214134216
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(B, Ci, HW, generator=g)
    w = torch.randn(Co, Ci, generator=g)
    b = torch.randn(Co, generator=g) if bias else None
    ref = torch.einsum("oc,bcp->bpo", w.double(), x.double() * float(np.float32(scale)))
    if bias:
        ref = ref + b.double()
    out = torch.zeros(B * HW, Co, device="cuda")
    check(lib, lib.tango_op_pointwise_small(DT[dtype], ptr(dev(x)), ptr(dev(w)), ptr(dev(b)) if bias else None, ptr(out), B, Ci, Co, HW, 8, scale, None))
    close(out.view(B, HW, Co), ref, dtype, "pointwise_small")
    assert lib.tango_op_pointwise_small(DT[dtype], ptr(dev(x)), ptr(dev(w)), None, ptr(out), 1, 17, Co, 1, 8, scale, None) != 0, "Cin > 16 must be refused"


@pytest.mark.parametrize("HW", [100, 4096])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("ld", [16, 24])
def test_pointwise_out_nchw(lib, HW, bias, ld):
    """quant_conv: fp32 channels-last rows (the first 16 of ld channels) -> 16 channels in the reference's NCHW layout"""
    B, Ci, Co = 3, 16, 16
    g = torch.Generator().manual_seed(HW + ld)
    x = torch.randn(B, HW, ld, generator=g)
    w = torch.randn(Co, Ci, generator=g)
    b = torch.randn(Co, generator=g) if bias else None
    ref = torch.einsum("oc,bpc->bop", w.double(), x.double()[:, :, :Ci])
    if bias:
        ref = ref + b.double()[None, :, None]
    out = torch.zeros(B, Co, HW, device="cuda")
    check(lib, lib.tango_op_pointwise_out_nchw(ptr(dev(x)), ld, ptr(dev(w)), ptr(dev(b)) if bias else None, ptr(out), B, Ci, Co, HW, None))
    close(out, ref, "fp32", "pointwise_out_nchw")


def test_pointwise_out_nchw_refuses_wide_inputs(lib):
    z = torch.zeros(64, 64, device="cuda")
    assert lib.tango_op_pointwise_out_nchw(ptr(z), 40, ptr(z), None, ptr(z), 1, 33, 16, 4, None) != 0
    assert b"Cin > 32" in lib.tango_last_error()
