"""The GEMM epilogue arms only the engine's plan builders set, at op level: the per-step bias table read through a device step counter
(GemmParams::bias2 / bias2_stride / step_ptr: the time-embedding row of every ResNet conv1), the leading-rows vector with its second
output (::rowvec / rowvec_rows / rowvec_per / out_lo / ldo_lo: the single-key cross-attention constant on attn1's to_out), and per-sample
weights (::wb_rows / wb_stride: GroupNorm folded into proj_in).  tango_op_linear_ex / tango_op_conv2d_temb launch exactly what a plan
launches and report the plan name, which every case asserts.

Every case makes two kinds of assertion:
 (a) the whole output against an fp64 statement of the op (operands rounded to the storage type first; bias, bias2 and rowvec are fp32 and
     are not), at the per-op tolerances of tests/test_ops_gpu.py, separately for every block of 64 rows (the granularity at which the
     epilogues pick a rowvec row, an output base and -- per 256 -- a weight matrix): a failure names its blocks.  The bias2 and rowvec rows
     are O(1) and differ by O(1), so the wrong row is an O(1) error in every block it touches.
 (b) exact ones.  *Pre-summed bias*: wide_epilogue (plans wide, wide+pers, duo, conv_wide) forms bias + bias2[step] + rowvec[s] in fp32
     before it meets the accumulator, so the output is bit-equal to the same route run without bias2 / rowvec and that sum, formed on the
     host in the same order, as its bias.  *Per-sample weights*: the rows of sample s are bit-equal to the same rows of a run with W_s as the
     only weight matrix.  *Untouched memory*: out, out_lo and their pitch columns are pre-filled with 768.0 (exact in fp16 and bf16); what
     the launch must not write still holds it.  *Repeat*: a second call is bit-identical.
     Where the bias is not pre-summed by contract (the 4-wave tiles, conv_halo, the LDS-DMA gather GEMM, and every split-K plan, whose
     reduce adds bias and then bias2 to the sum) the exact check is the step difference instead: out(step) - out(step') equals
     bias2[step] - bias2[step'] within the roundings of the two outputs -- a row added twice or not at all misses that by O(1).

Conv shapes: the dispatcher's split-K policy claims a 3x3 conv until the 128-row tiling has more than 341 tiles, so the unsplit routes
need M >= 21888 (N = 320) or 43776 (N <= 160) rows even with the big tiles forced; conv_wide+splitk needs 224 (tile, split) pairs with
at least 128 channels per split.  The batch sizes below are the smallest that land on each route (tango_debug_conv2d_route)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from test_duo_gpu import DUO, tuning

pytestmark = pytest.mark.gpu

DT = {"fp32": 0, "fp16": 1, "bf16": 2}
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
TOL = {"fp32": 2e-5, "fp16": 4e-3, "bf16": 3e-2}          # tests/test_ops_gpu.py TOL: max abs error over the reference's max abs
ULP = {"fp32": 2.0 ** -23, "fp16": 2.0 ** -10, "bf16": 2.0 ** -7}
FILL = 768.0
STEPS = 4
FORCE = dict(TANGO_FORCE_DMA_GEMM=1)
WIDE = dict(FORCE, TANGO_DUO_MAXK=0)
ENV = {"wide": WIDE, "duo": dict(FORCE, **DUO), "wide+pers": dict(TANGO_WIDE_PERS=1), "tile": {}, "tile+splitk": {}, "dma": WIDE}
PRESUMMED = ("wide", "wide+pers", "duo", "conv_wide")      # plans whose epilogue is wide_epilogue


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def quant(t, dtype):
    return t.to(TDT[dtype]).float()


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def rows_table(g, n, N):
    """n fp32 rows of independent N(0, 1) entries around a mean of 1.5 * (row % 4): bounded however many rows (the output scale stays O(10),
    so the tolerances stay well below 1), neighbours 1.5 apart in every column, and any two rows O(1) apart in most columns"""
    return (randn(g, n, N) + 1.5 * (torch.arange(n, device="cuda") % 4).view(n, 1)).contiguous()


def presum(*vecs):
    """the column constant as wide_epilogue forms it: fp32 adds on the host, left to right"""
    acc = vecs[0].cpu().numpy().astype(np.float32)
    for v in vecs[1:]:
        acc = (acc + v.cpu().numpy().astype(np.float32)).astype(np.float32)
    return torch.from_numpy(acc).cuda()


def assert_blocks(got, ref, dtype, what):
    """max error of every 64-row block over the GLOBAL reference maximum, each block asserted; returns the largest"""
    scale = ref.abs().max().item() + 1e-6
    M = ref.shape[0]
    nb = (M + 63) // 64
    err = torch.zeros(nb * 64, dtype=torch.float64, device=ref.device)
    err[:M] = (got.double() - ref).abs().amax(dim=1)
    blk = err.view(nb, 64).amax(dim=1) / scale
    bad = (blk > TOL[dtype]).nonzero().flatten().tolist()
    assert not bad, "%s: %d of %d 64-row blocks above %.1e of the output scale %.2f: %s" % (
        what, len(bad), nb, TOL[dtype], scale, ", ".join("block %d (rows %d-%d) %.3e" % (b, 64 * b, 64 * b + 63, blk[b].item()) for b in bad[:8]))
    return blk.max().item()


def assert_step_difference(out_a, out_b, delta, dtype, mids, what):
    """out_a - out_b == delta (per column, broadcast over rows) within the roundings of the two outputs: one rounding to the storage type each
    (half an ulp each, taken whole as tests/test_upsample_phase_gpu.py does), plus the fp32 roundings on the way -- at most four per output
    (bias + bias2, + accumulator, + residual, reduce), each below 2^-24 of `mids`, the sum of the operands' maxima"""
    d = (out_a.double() - out_b.double() - delta.double()).abs()
    bound = ULP[dtype] * (out_a.abs() + out_b.abs()).double() + 8 * 2.0 ** -24 * mids + 1e-9
    assert (d <= bound).all(), "%s: the step's row is not added exactly once somewhere: max excess %.3e" % (what, (d - bound).max().item())


# ---- linear -------------------------------------------------------------------------------------------------------------------------------
def linear_ex(lib, dtype, x, w, bias, M, N, K, b2=None, step=0, res=None, rv=None, rv_rows=0, rv_per=64, wb=0, pad=0):
    """-> out [M][N + pad], out_lo [M][N + pad + 8 | N] or None (both pre-filled with FILL), plan name"""
    out = torch.full((M, N + pad), FILL, device="cuda")
    out_lo = torch.full((M, N + (pad + 8 if pad else 0)), FILL, device="cuda") if rv is not None else None
    plan = C.create_string_buffer(64)
    rc = lib.tango_op_linear_ex(DT[dtype], ptr(x), ptr(w), ptr(bias), ptr(b2), STEPS if b2 is not None else 0, step, ptr(res), ptr(rv),
                                rv_rows, rv_per, wb, pad, ptr(out), ptr(out_lo), M, N, K, plan, 64, None)
    assert rc == 0, lib.tango_last_error().decode()
    torch.cuda.synchronize()
    return out, out_lo, plan.value.decode()


def linear_problem(dtype, M, N, K, seed, nw=1, res=True):
    g = gen(seed)
    x = quant(randn(g, M, K), dtype)
    w = quant(randn(g, nw * N, K) / K ** 0.5, dtype)
    bias = randn(g, N)
    r = quant(randn(g, M, N), dtype) if res else None
    return g, x, w, bias, r


ROWVEC_GEOMETRIES = [(rows, per) for rows in (0, 64, 192, 256, 320, 1024) for per in (64, 128, 256, 1024)
                     if rows == 0 or rows % per == 0 or per >= rows]


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("route,M,N,K", [("wide", 1024, 640, 64), ("wide", 1024, 320, 320), ("duo", 1024, 480, 96), ("duo", 1024, 160, 320)])
def test_rowvec_with_residual(lib, dtype, route, M, N, K, pad):
    """the range boundary inside the first tile (64, 192), on a tile edge (256), inside the second tile (320), nowhere (0) and at all rows;
    the vector changing at every wave (rowvec_per = 64), inside a tile (128), per tile (256) and never (1024)"""
    t0 = time.perf_counter()
    g, x, w, bias, r = linear_problem(dtype, M, N, K, M + N + K + pad)
    table = rows_table(g, 16, N)
    lin = x.double() @ w.double().t() + r.double()
    worst = 0.0
    with tuning(lib, **ENV[route]):
        plains = {}

        def plain(vec_key, vec):          # the same route with the host-summed constant as its only bias
            if vec_key not in plains:
                o, _, pl = linear_ex(lib, dtype, x, w, vec, M, N, K, res=r, pad=pad)
                assert pl == route, pl
                plains[vec_key] = o
            return plains[vec_key]

        for rows, per in ROWVEC_GEOMETRIES:
            what = "rowvec %s %s M=%d N=%d K=%d pad=%d rows=%d per=%d" % (route, dtype, M, N, K, pad, rows, per)
            ns = (rows + per - 1) // per
            rv = table[:max(ns, 1)].contiguous()
            out, out_lo, plan = linear_ex(lib, dtype, x, w, bias, M, N, K, res=r, rv=rv, rv_rows=rows, rv_per=per, pad=pad)
            assert plan == route, "%s ran as %s" % (what, plan)
            # (a)
            ref = lin + bias.double()
            sample = torch.arange(rows, device="cuda") // per
            ref[:rows] += rv.double()[sample]
            got = torch.cat([out_lo[:rows, :N], out[rows:, :N]])
            worst = max(worst, assert_blocks(got, ref, dtype, what))
            # (b) untouched memory
            assert (out[:rows] == FILL).all(), "%s: rows below rowvec_rows of `out` were written" % what
            assert (out_lo[rows:] == FILL).all(), "%s: rows from rowvec_rows on of `out_lo` were written" % what
            assert (out[:, N:] == FILL).all() and (out_lo[:, N:] == FILL).all(), "%s: pitch columns were written" % what
            # (b) pre-summed bias, per sample on that sample's rows; the rows outside the range against the plain bias
            for s in range(ns):
                lo, hi = s * per, min((s + 1) * per, rows)
                want = plain(("rv", s), presum(bias, rv[s]))
                assert torch.equal(out_lo[lo:hi, :N], want[lo:hi, :N]), "%s: sample %d (rows %d-%d) is not the plain run with bias + rowvec[%d]" % (what, s, lo, hi - 1, s)
            assert torch.equal(out[rows:, :N], plain("bias", bias)[rows:, :N]), "%s: rows outside the range differ from the plain run" % what
            # (b) repeat
            out2, out_lo2, _ = linear_ex(lib, dtype, x, w, bias, M, N, K, res=r, rv=rv, rv_rows=rows, rv_per=per, pad=pad)
            assert torch.equal(out, out2) and torch.equal(out_lo, out_lo2), "%s: a second call differs" % what
    print("ARMS rowvec+residual %s M=%d N=%d K=%d pad=%d: plan %s, %d geometries, fp64 err %.3e (tol %.1e), %.2f s"
          % (dtype, M, N, K, pad, route, len(ROWVEC_GEOMETRIES), worst, TOL[dtype], time.perf_counter() - t0))


def _per_sample_weights(lib, dtype, route, M, N, K, wb, samples):
    t0 = time.perf_counter()
    nw = M // wb
    g, x, w, bias, _ = linear_problem(dtype, M, N, K, M + N + K + wb, nw=nw, res=False)
    rv = rows_table(g, nw, N)
    what = "wb_rows %s %s M=%d N=%d K=%d wb_rows=%d" % (route, dtype, M, N, K, wb)
    with tuning(lib, **ENV[route]):
        out, out_lo, plan = linear_ex(lib, dtype, x, w, bias, M, N, K, rv=rv, rv_rows=M, rv_per=wb, wb=wb)
        assert plan == route, "%s ran as %s" % (what, plan)
        ref = torch.bmm(x.double().view(nw, wb, K), w.double().view(nw, N, K).transpose(1, 2)) + (bias.double() + rv.double()).view(nw, 1, N)
        err = assert_blocks(out_lo, ref.view(M, N), dtype, what)
        scale = ref.abs().max().item()
        del ref
        assert (out == FILL).all(), "%s: `out` was written although every row belongs to out_lo" % what
        for s in samples:
            ws = w[s * N:(s + 1) * N].contiguous()
            want, _, pl = linear_ex(lib, dtype, x, ws, presum(bias, rv[s]), M, N, K)
            assert pl == route, pl
            lo, hi = s * wb, (s + 1) * wb
            assert torch.equal(out_lo[lo:hi], want[lo:hi]), "%s: sample %d (rows %d-%d) is not the plain run with W_%d and bias + rowvec[%d]: %d elements differ" % (
                what, s, lo, hi - 1, s, s, (out_lo[lo:hi] != want[lo:hi]).sum().item())
        del want
        out2, out_lo2, _ = linear_ex(lib, dtype, x, w, bias, M, N, K, rv=rv, rv_rows=M, rv_per=wb, wb=wb)
        assert torch.equal(out_lo, out_lo2) and torch.equal(out, out2), "%s: a second call differs" % what
    print("ARMS wb_rows+rowvec %s M=%d N=%d K=%d wb_rows=%d: plan %s, fp64 err %.3e (tol %.1e) of the output scale %.1f, samples %s bit-equal, %.2f s"
          % (dtype, M, N, K, wb, route, err, TOL[dtype], scale, list(samples), time.perf_counter() - t0))


@pytest.mark.parametrize("wb", [256, 512])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("route", ["wide", "duo"])
def test_per_sample_weights(lib, dtype, route, wb):
    """rowvec over all rows with rowvec_per = wb_rows, as the engine's GroupNorm fold sets it; every sample checked bit for bit"""
    _per_sample_weights(lib, dtype, route, 1024, 320, 320, wb, range(1024 // wb))


@pytest.mark.parametrize("wb", [256, 1024])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_per_sample_weights_persistent(lib, dtype, wb):
    """512 tiles on at most 256 workgroups: every workgroup computes the NEXT tile's weight base while it finishes a tile (wb_rows = 256:
    another matrix at every tile step).  fp64 on every block -- a tile multiplied with another sample's weights, or given another sample's
    rowvec row, is off by O(1) of an O(10) scale; bit-equality (one 131072-row plain run each) on the first, the last, the samples around the
    middle, where the workgroups' second tiles begin, and every 37th in between, which walks through the workgroups and both of their tiles"""
    M = 131072
    nw = M // wb
    _per_sample_weights(lib, dtype, "wide+pers", M, 320, 64, wb, sorted({0, 1, nw // 2 - 1, nw // 2, nw // 2 + 1, nw - 1} | set(range(0, nw, 37))))


# (the fp32 engine has only the two tile routes)
STEP_BIAS_LINEAR = [(route, dtype, M, N, K)
                    for route, M, N, K, dtypes in [("wide", 512, 320, 64, ("fp16", "bf16")), ("duo", 512, 320, 64, ("fp16", "bf16")),
                                                   ("dma", 512, 160, 256, ("fp16", "bf16")), ("tile", 512, 320, 64, ("fp16", "bf16", "fp32")),
                                                   ("tile+splitk", 512, 1280, 1280, ("fp16", "bf16", "fp32"))]
                    for dtype in dtypes]


@pytest.mark.parametrize("route,dtype,M,N,K", STEP_BIAS_LINEAR)
def test_step_bias_linear(lib, dtype, route, M, N, K):
    """bias2[step] through the device step counter: steps 0, 1 and the last of a four-row table; without a step pointer row 0"""
    t0 = time.perf_counter()
    g, x, w, bias, r = linear_problem(dtype, M, N, K, M + N + K)
    b2 = rows_table(g, STEPS, N)
    lin = x.double() @ w.double().t() + bias.double() + r.double()
    mids = (x.double() @ w.double().t()).abs().max().item() + bias.abs().max().item() + b2.abs().max().item() + r.abs().max().item()
    what = "bias2 %s %s M=%d N=%d K=%d" % (route, dtype, M, N, K)
    outs, worst = {}, 0.0
    with tuning(lib, **ENV[route]):
        for step in (0, 1, STEPS - 1):
            out, _, plan = linear_ex(lib, dtype, x, w, bias, M, N, K, b2=b2, step=step, res=r)
            assert plan == route, "%s ran as %s" % (what, plan)
            worst = max(worst, assert_blocks(out, lin + b2[step].double(), dtype, "%s step %d" % (what, step)))
            if route in PRESUMMED:
                want, _, pl = linear_ex(lib, dtype, x, w, presum(bias, b2[step]), M, N, K, res=r)
                assert pl == route and torch.equal(out, want), "%s step %d: not the plain run with bias + bias2[%d]" % (what, step, step)
            out2, _, _ = linear_ex(lib, dtype, x, w, bias, M, N, K, b2=b2, step=step, res=r)
            assert torch.equal(out, out2), "%s step %d: a second call differs" % (what, step)
            outs[step] = out
        nostep, _, _ = linear_ex(lib, dtype, x, w, bias, M, N, K, b2=b2, step=-1, res=r)
        assert torch.equal(nostep, outs[0]), "%s: a table without a step pointer must read row 0" % what
    for step in (1, STEPS - 1):
        assert_step_difference(outs[step], outs[0], b2[step] - b2[0], dtype, mids, "%s step %d vs 0" % (what, step))
    print("ARMS bias2 linear %s M=%d N=%d K=%d: plan %s, fp64 err %.3e (tol %.1e), %s, %.2f s"
          % (dtype, M, N, K, route, worst, TOL[dtype], "bit-equal to the pre-summed bias" if route in PRESUMMED else "step difference only",
             time.perf_counter() - t0))


# ---- conv1 of a ResNet block ----------------------------------------------------------------------------------------------------------------
def conv_temb(lib, dtype, x, w, bias, b2, step, res):
    B, Cin, H, W = x.shape
    out = torch.empty(B, w.shape[0], H, W, device="cuda")
    plan = C.create_string_buffer(64)
    rc = lib.tango_op_conv2d_temb(DT[dtype], ptr(x), ptr(w), ptr(bias), ptr(b2), STEPS, step, ptr(res), ptr(out), B, Cin, H, W, w.shape[0],
                                  plan, 64, None)
    assert rc == 0, lib.tango_last_error().decode()
    torch.cuda.synchronize()
    return out, plan.value.decode()


def conv_plain(lib, dtype, x, w, bias, res):
    """the same conv without bias2 through tango_op_conv2d_ex -> out, and the plan of exactly that call's problem (tango_debug_conv2d_route
    builds what tango_op_conv2d_ex builds, under the switches in force)"""
    B, Cin, H, W = x.shape
    out = torch.empty(B, w.shape[0], H, W, device="cuda")
    plan = lib.tango_debug_conv2d_route(DT[dtype], B, Cin, H, W, w.shape[0], 1, 0, 1, 1 if res is not None else 0, 0, 0, None).decode()
    rc = lib.tango_op_conv2d_ex(DT[dtype], ptr(x), ptr(w), ptr(bias), ptr(res), ptr(out), B, Cin, H, W, w.shape[0], 1, 1, 0, 0.0, 0, None)
    assert rc == 0, lib.tango_last_error().decode()
    torch.cuda.synchronize()
    return out, plan


def conv_ref64(x, w):
    """fp64 3x3 / pad 1 conv as nine matrix products over shifted views of the padded NHWC image -> rows [B*H*W][Cout]"""
    B, Cin, H, W = x.shape
    xp = torch.nn.functional.pad(x.double(), (1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
    w64 = w.double()
    acc = torch.zeros(B, H, W, w.shape[0], dtype=torch.float64, device="cuda")
    for ky in range(3):
        for kx in range(3):
            acc += xp[:, ky:ky + H, kx:kx + W, :] @ w64[:, :, ky, kx].t()
    return acc.view(B * H * W, -1)


def rows_of(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


CONV_CASES = [
    ("conv_wide", FORCE, (86, 64, 16, 16, 320), ("fp16", "bf16")),                                     # the pipelined kernel (TANGO_CONV_PIPE=2, the default)
    ("conv_wide", dict(FORCE, TANGO_CONV_PIPE=0), (86, 64, 16, 16, 320), ("fp16", "bf16")),           # the ping-pong kernel
    ("conv_wide", dict(FORCE, TANGO_CONV_TALL=1), (43, 64, 32, 16, 320), ("fp16", "bf16")),           # its 512 x 160 form
    ("conv_halo", FORCE, (172, 64, 16, 16, 160), ("fp16", "bf16")),                                    # 160-column tiles
    ("conv_halo", FORCE, (172, 64, 16, 16, 128), ("fp16", "bf16")),                                    # 128-column tiles
    ("conv_wide+splitk", {}, (56, 512, 16, 16, 320), ("fp16", "bf16")),                                # 56 tiles x 4 splits
    ("tile", {}, (973, 64, 9, 5, 96), ("fp16", "bf16", "fp32")),                                       # 43785 rows: a partial last tile
    ("tile+splitk", {}, (1, 64, 8, 4, 96), ("fp16", "bf16", "fp32")),
]


@pytest.mark.parametrize("case,dtype", [(i, dtype) for i, c in enumerate(CONV_CASES) for dtype in c[3]])
def test_step_bias_conv(lib, dtype, case):
    """bias + bias2[step] (+ residual) on every conv route, steps 0, 2 and 3 of a four-row table"""
    route, env, (B, Cin, H, W, Cout), _ = CONV_CASES[case]
    t0 = time.perf_counter()
    g = gen(B + Cin + H + W + Cout)
    x = quant(randn(g, B, Cin, H, W), dtype)
    w = quant(randn(g, Cout, Cin, 3, 3) / (9 * Cin) ** 0.5, dtype)
    bias = randn(g, Cout)
    b2 = rows_table(g, STEPS, Cout)
    res_t = quant(randn(g, B, Cout, H, W), dtype)
    conv = conv_ref64(x, w)
    what0 = "conv bias2 %s %s B=%d Cin=%d %dx%d Cout=%d" % (route, dtype, B, Cin, H, W, Cout)
    worst = 0.0
    with tuning(lib, **env):
        for res in (None, res_t):
            what = what0 + (" +res" if res is not None else "")
            lin = conv + bias.double() + (rows_of(res).double() if res is not None else 0.0)
            mids = conv.abs().max().item() + bias.abs().max().item() + b2.abs().max().item() + (res.abs().max().item() if res is not None else 0.0)
            outs = {}
            for step in (0, 2, 3):
                out, plan = conv_temb(lib, dtype, x, w, bias, b2, step, res)
                assert plan == route, "%s ran as %s" % (what, plan)
                worst = max(worst, assert_blocks(rows_of(out), lin + b2[step].double(), dtype, "%s step %d" % (what, step)))
                if route in PRESUMMED:
                    want, pl = conv_plain(lib, dtype, x, w, presum(bias, b2[step]), res)
                    assert pl == route, "%s: the plain run is planned as %s" % (what, pl)
                    assert torch.equal(out, want), "%s step %d: not the plain run with bias + bias2[%d]" % (what, step, step)
                outs[step] = out
            out2, _ = conv_temb(lib, dtype, x, w, bias, b2, 3, res)
            assert torch.equal(out2, outs[3]), "%s: a second call differs" % what
            for step in (2, 3):
                assert_step_difference(rows_of(outs[step]), rows_of(outs[0]), b2[step] - b2[0], dtype, mids, "%s step %d vs 0" % (what, step))
    print("ARMS bias2 conv %s B=%d Cin=%d %dx%d Cout=%d: plan %s, fp64 err %.3e (tol %.1e), %s, %.2f s"
          % (dtype, B, Cin, H, W, Cout, route, worst, TOL[dtype], "bit-equal to the pre-summed bias" if route in PRESUMMED else "step difference only",
             time.perf_counter() - t0))
