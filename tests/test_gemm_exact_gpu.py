"""Every GEMM and conv route on small-integer operands, where the arithmetic is exact: each product and each partial sum is an integer
below 2^24, so fp32 accumulation is exact in any order, through any MFMA shape, split-K partition or LDS staging; the epilogues
(gemm_epilogue_body, gemm_epilogue_staged_body, wide_epilogue, splitk_reduce_kernel) apply alpha, bias (+ bias2) (+ rowvec), the activation
and the residual in fp32 and convert once.  A correct kernel therefore returns exactly round_T(integer result), round to nearest even, and
every GPU assertion here is torch.equal against a reference formed independently of the library -- no tolerance anywhere.

Operands (seeded): x in {+-1, +-2, +-3} and w in {+-1, +-2} for fp32 / fp16, x, w in {+-1} for bf16 -- no zeros, every product counts; bias,
bias2 rows and rowvec rows integers in [-3, 3] (table rows differ pairwise in most columns, asserted); residual in {+-1 .. +-4}; per-sample
weight matrices independent draws.

Reference: the integer result in float64 on the device (matrix products over shifted views for the convs; exact for these integers), a
slice of >= 64 rows x all columns recomputed in int64 on the CPU and asserted equal; then alpha, the bias terms, the activation and the
residual in float64, in that order, and ONE conversion to the storage type (none where the op writes fp32).

Preconditions, asserted on the host for every case (conditions on the inputs): |value| < 2^24 before rounding, and at most 1 % of the outputs
where the spacing of T exceeds the smallest change one product can make (|v| > 2048 u in fp16, 256 u in bf16; u = 1, or alpha / the
leaky-ReLU slope where the case has one), so that a dropped or doubled product stays visible after rounding.  bf16 cases keep K <= 5120.

Every case asks the host-side route / refusal query under its switches first and launches only when the answer is the plan the case was
written for; where the wrapper reports the plan of the launch itself, that is asserted again.  A failure reports the number of differing
elements, the first few (row, column, got, expected), the 64-row x 16-column blocks they fall in and whether the differences are single
product magnitudes.  test_harness_catches_the_bugs_it_is_for (host only) corrupts the reference the ways the kernels could be wrong and
asserts that the comparison fails."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_duo_gpu import DUO, NODUO, tuning

gpu = pytest.mark.gpu

DT = {"fp32": 0, "fp16": 1, "bf16": 2}
TDT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
ALL = ("fp32", "fp16", "bf16")
HALF = ("fp16", "bf16")
XMAG = {"fp32": (1, 2, 3), "fp16": (1, 2, 3), "bf16": (1,)}
WMAG = {"fp32": (1, 2), "fp16": (1, 2), "bf16": (1,)}
RMAG = (1, 2, 3, 4)
COARSE = {"fp16": 2048.0, "bf16": 256.0}      # above this the spacing of T exceeds 1
LRELU, SLOPE = 2, 0.5
STEPS = 4
FORCE = dict(TANGO_FORCE_DMA_GEMM=1)
WIDE = dict(FORCE, TANGO_DUO_MAXK=0)
FDUO = dict(FORCE, **DUO)
PERS = dict(TANGO_WIDE_PERS=1, TANGO_DUO_MAXK=0)


# ---- the harness (host side: the self-check below runs it without a GPU) -------------------------------------------------------------------
def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 12345)


def signed(g, shape, mags):
    """integers of the given magnitudes with random signs (no zero), fp32 on the CPU"""
    m = torch.tensor(mags, dtype=torch.float32)
    return m[torch.randint(0, len(mags), shape, generator=g)] * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def small(g, shape):
    return torch.randint(-3, 4, shape, generator=g).float()


def table(g, n, N):
    """n rows of integers in [-3, 3]; any two rows differ in most columns (asserted)"""
    t = small(g, (n, N))
    for i in range(n):
        for j in range(i + 1, n):
            assert (t[i] != t[j]).float().mean().item() > 0.5, "table rows %d and %d are too similar" % (i, j)
    return t


def products(dtype):
    return sorted({a * b for a in XMAG[dtype] for b in WMAG[dtype]})


def expected(acc, dtype, alpha=1.0, cols=(), slope=None, res=None, out_f32=False, what=""):
    """acc: the integer result [M][N] in float64.  -> round_T(act(acc * alpha + cols...) + res) as fp32, after the two preconditions"""
    assert acc.abs().max().item() < 2 ** 24, "%s: integer result beyond 2^24" % what
    v = acc * alpha
    for c in cols:
        v = v + c.double()
    if slope is not None:
        v = torch.where(v < 0, v * slope, v)
    if res is not None:
        v = v + res.double()
    assert v.abs().max().item() < 2 ** 24, "%s: reference beyond 2^24" % what
    if out_f32 or dtype == "fp32":
        return v.float()
    unit = alpha * (slope if slope is not None else 1.0)
    coarse = (v.abs() > COARSE[dtype] * unit).double().mean().item()
    assert coarse <= 0.01, "%s: %.3f %% of the outputs lie where one product is below the spacing of %s" % (what, 100 * coarse, dtype)
    return v.to(TDT[dtype]).float()


def mismatch(got, exp, what, prods=()):
    """None when bit-equal, else the report"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if torch.equal(got, exp):
        return None
    got2, exp2 = got.reshape(-1, got.shape[-1]), exp.reshape(-1, exp.shape[-1])
    bad = (got2 != exp2).nonzero()
    r, c = bad[:, 0], bad[:, 1]
    d = (got2[r, c].double() - exp2[r, c].double()).abs()
    single = torch.zeros_like(d, dtype=torch.bool)
    for pm in prods:
        single |= d == float(pm)
    first = ", ".join("(%d, %d): got %r, expected %r" % (i, j, got2[i, j].item(), exp2[i, j].item()) for i, j in bad[:6].tolist())
    blocks = torch.unique(torch.stack([r // 64, c // 16], 1), dim=0)
    return ("%s: %d of %d elements differ; first %s; %d blocks of 64 rows x 16 columns, first (row block, column group) %s; "
            "%d of the differences are a single product magnitude %s" % (what, bad.shape[0], got2.numel(), first, blocks.shape[0],
                                                                         blocks[:8].tolist(), int(single.sum().item()), list(prods)))


def assert_exact(got, exp, what, prods=()):
    report = mismatch(got, exp, what, prods)
    assert report is None, report


def lin_acc(x, w, dtype=torch.float64):
    """x [M][K], w [N][K] or per-sample [nw][N][K] -> [M][N]"""
    x, w = x.to(dtype), w.to(dtype)
    if w.dim() == 2:
        return x @ w.t()
    nw = w.shape[0]
    return torch.bmm(x.view(nw, -1, x.shape[1]), w.transpose(1, 2)).reshape(x.shape[0], -1)


def conv2d_acc(x, w, stride=1, pad=1, ups=0, dtype=torch.float64, band=None, shift=None):
    """3x3 conv (after a nearest x2 upsample when ups) as nine matrix products over shifted views of the padded NHWC image ->
    [B][Ho][Wo][Cout]; pad 1: zeros all round, pad 0: a zero row / column at the far edge only (the VAE Downsample: F.pad(x, (0, 1, 0, 1)));
    band = (h0, h1): those output rows only.  shift = (ky, kx, dx): that tap reads dx columns off (the self-check's bug)"""
    x, w = x.to(dtype), w.to(dtype)
    if ups:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    B, Cin, H, W = x.shape
    Ho, Wo = (H + pad - 2) // stride + 1, (W + pad - 2) // stride + 1
    h0, h1 = band if band else (0, Ho)
    extra = 1 if shift else 0
    xp = F.pad(x, (pad, 1 + extra, pad, 1)).permute(0, 2, 3, 1).contiguous()
    acc = torch.zeros(B, h1 - h0, Wo, w.shape[0], dtype=dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            dx = shift[2] if shift and shift[:2] == (ky, kx) else 0
            v = xp[:, ky + stride * h0:ky + stride * (h1 - 1) + 1:stride, kx + dx:kx + dx + stride * (Wo - 1) + 1:stride, :]
            acc += (v.reshape(-1, Cin) @ w[:, :, ky, kx].t()).view(acc.shape)
    return acc


def conv1d_acc(x, w, d, dtype=torch.float64, rows=None):
    """x [B][Cin][L], w [Cout][Cin][k], dilation d, padding d (k - 1) / 2 -> [B][L][Cout]; rows = (l0, l1): those positions only"""
    x, w = x.to(dtype), w.to(dtype)
    B, Cin, L = x.shape
    k = w.shape[2]
    p = d * (k - 1) // 2
    l0, l1 = rows if rows else (0, L)
    xp = F.pad(x, (p, p)).permute(0, 2, 1).contiguous()
    acc = torch.zeros(B, l1 - l0, w.shape[0], dtype=dtype, device=x.device)
    for t in range(k):
        acc += (xp[:, t * d + l0:t * d + l1, :].reshape(-1, Cin) @ w[:, :, t].t()).view(acc.shape)
    return acc


def convt1d_acc(x, w, u, pd, dtype=torch.float64):
    """x [B][Cin][L], w [Cin][Cout][k], stride u, padding pd: out[j] += x[i] w[t] at j = i u + t - pd -> [B][Lo][Cout]"""
    x, w = x.to(dtype), w.to(dtype)
    B, Cin, L = x.shape
    k = w.shape[2]
    full = torch.zeros(B, (L - 1) * u + k, w.shape[1], dtype=dtype, device=x.device)
    xr = x.permute(0, 2, 1).reshape(-1, Cin)
    for t in range(k):
        full[:, t:t + (L - 1) * u + 1:u, :] += (xr @ w[:, :, t]).view(B, L, -1)
    return full[:, pd:pd + (L - 1) * u - 2 * pd + k, :].contiguous()


def rows_of(t):
    """[B][C][...] -> rows [B * ...][C]"""
    return t.movedim(1, -1).reshape(-1, t.shape[1])


def same_ints(acc_rows, int_rows, what):
    assert torch.equal(acc_rows.cpu(), int_rows.double()), "%s: the float64 reference and its int64 recomputation on the CPU differ" % what


# ---- host only: the harness catches what it is for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL)
def test_harness_catches_the_bugs_it_is_for(dtype):
    """one linear (K = 5120, the largest any GPU case below uses, so this is also the sensitivity cap at its worst) and one 3x3 conv per
    dtype; the reference is corrupted the ways a kernel could be wrong and the comparison must fail -- for a dropped last k index and a
    doubled product at >= 99 % of the outputs (all of them are affected)"""
    M, N, K = 64, 256, 5120
    g = gen(M, N, K, DT[dtype])
    x, w = signed(g, (M, K), XMAG[dtype]), signed(g, (N, K), WMAG[dtype])
    bias, b2, r = small(g, (N,)), table(g, STEPS, N), signed(g, (M, N), RMAG)
    acc = lin_acc(x, w)
    same_ints(acc, lin_acc(x, w, torch.int64), "self-check linear")
    good = expected(acc, dtype, cols=(bias, b2[1]), res=r, what="self-check linear")
    assert mismatch(good.clone(), good, "identity") is None
    dropped = expected(acc - x[:, K - 1:].double() @ w[:, K - 1:].double().t(), dtype, cols=(bias, b2[1]), res=r)
    doubled = expected(acc + x[:, 7:8].double() @ w[:, 7:8].double().t(), dtype, cols=(bias, b2[1]), res=r)
    for name, wrong in (("dropped last k", dropped), ("doubled product", doubled)):
        frac = (wrong != good).double().mean().item()
        report = mismatch(wrong, good, name, products(dtype))
        assert report is not None and frac >= 0.99, "%s %s: visible at %.2f %% of the outputs" % (dtype, name, 100 * frac)
        singles = int(report.split(" blocks of 64 rows")[1].split("; ")[1].split(" of the differences")[0])
        assert singles >= 0.99 * M * N, report          # (the few others sit where the spacing of T is 2: the difference shows as 2)
    for step in (0, 2):
        assert mismatch(expected(acc, dtype, cols=(bias, b2[step]), res=r), good, "bias2[step +- 1]") is not None
    # conv: Cin = 512 (K = 4608, the deepest conv below); the tap (ky, kx) = (1, 0) reading one column off changes the left border column
    B, Cin, H, W, Cout = 2, 512, 8, 8, 64
    g = gen(B, Cin, H, W, Cout, DT[dtype])
    x, w = signed(g, (B, Cin, H, W), XMAG[dtype]), signed(g, (Cout, Cin, 3, 3), WMAG[dtype])
    bias = small(g, (Cout,))
    acc = conv2d_acc(x, w)
    same_ints(acc, conv2d_acc(x, w, dtype=torch.int64), "self-check conv")
    good = expected(acc.view(-1, Cout), dtype, cols=(bias,), what="self-check conv")
    wrong = expected(conv2d_acc(x, w, shift=(1, 0, 1)).view(-1, Cout), dtype, cols=(bias,))
    report = mismatch(wrong, good, "shifted border tap", products(dtype))
    assert report is not None
    border = (wrong != good).view(B, H, W, Cout)
    assert border[:, :, 0, :].double().mean().item() >= 0.9, "the shifted tap must show in the border column"
    w_cut = w.clone()
    w_cut[:, Cin - 1, 2, 2] = 0          # the last k index of the conv's K = 9 Cin: tap (2, 2), channel Cin - 1
    dropped = expected(conv2d_acc(x, w_cut).view(-1, Cout), dtype, cols=(bias,))
    interior = (dropped != good).view(B, H, W, Cout)[:, :H - 1, :W - 1, :]
    assert interior.double().mean().item() >= 0.99, "%s conv, dropped last k: visible at %.2f %%" % (dtype, 100 * interior.double().mean().item())


# ---- linear ------------------------------------------------------------------------------------------------------------------------------------
def linear_operands(dtype, M, N, K, nw=1, seed=0):
    g = gen(M, N, K, nw, DT[dtype], seed)
    x = signed(g, (M, K), XMAG[dtype])
    w = signed(g, (nw * N, K), WMAG[dtype])
    return g, x, w, small(g, (N,)), signed(g, (M, N), RMAG)


def linear_reference(x, w, nw, what):
    """integer result on the device, its last 64 rows recomputed in int64 on the CPU"""
    M, N = x.shape[0], w.shape[0] // nw
    w3 = w.view(nw, N, -1) if nw > 1 else w
    acc = lin_acc(x.cuda(), w3.cuda())
    lo = max(0, M - 64)
    same_ints(acc[lo:], lin_acc(x[lo:], w3[-1] if nw > 1 else w3, torch.int64), what)
    return acc


# (plan, switches, (M, N, K), dtypes).  tile: the tilings of launch_tile in turn, then N with a 4-column tail / no multiple of 4 (never split),
# then the 64 x 64 small tile.  K = 32 / 96 elements are 64-byte chunks in 16 bits, 64 / 320 / 1280 are 128-byte chunks.  tile+splitk: 20 (fp32: 40)
# chunks over 6 (13) splits, 80 over 32: uneven last splits.  wide / duo / dma are forced onto test-sized grids; wide+pers, stream and the fp32
# dma case are the planner's own choice at that size
LINEAR = [
    ("tile", {}, (200, 320, 320), HALF), ("tile+splitk", {}, (200, 320, 320), ("fp32",)),      # 128 x 160
    ("tile", {}, (128, 128, 64), ALL),                                                          # 128 x 128
    ("tile", {}, (77, 48, 96), ALL),                                                            # 128 x 64
    ("tile", {}, (64, 24, 32), ALL),                                                            # 256 x 32
    ("tile", {}, (130, 8, 64), ALL),                                                            # 256 x 16
    ("tile", {}, (77, 100, 96), ALL), ("tile", {}, (77, 30, 96), ALL),
    ("tile", {}, (2048, 640, 640), ALL),                                                        # 64 x 64
    ("tile+splitk", {}, (300, 640, 1280), ALL), ("tile+splitk", {}, (100, 320, 1280), ALL), ("tile+splitk", {}, (128, 1280, 5120), ALL),
    ("dma", WIDE, (512, 160, 256), HALF), ("dma", WIDE, (300, 128, 256), HALF), ("dma", {}, (16384, 640, 640), ("fp32",)),
    ("wide", WIDE, (512, 320, 32), HALF), ("wide", WIDE, (512, 320, 64), HALF), ("wide", WIDE, (1024, 320, 320), HALF),
    ("wide+pers", PERS, (131072, 320, 32), HALF),
    ("duo", FDUO, (512, 160, 32), HALF), ("duo", FDUO, (512, 320, 64), HALF), ("duo", FDUO, (1024, 480, 96), HALF),
    ("stream", NODUO, (16400, 320, 320), HALF), ("stream", NODUO, (16384, 80, 640), HALF), ("stream", {}, (16400, 320, 320), ("fp32",)),
]


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(LINEAR) for d in c[3]])
def test_linear_exact(lib, case, dtype):
    """tango_op_linear with bias only and with bias + residual"""
    plan, env, (M, N, K), _ = LINEAR[case]
    _, x, w, bias, r = linear_operands(dtype, M, N, K)
    what = "linear %s %s M=%d N=%d K=%d" % (plan, dtype, M, N, K)
    acc = linear_reference(x, w, 1, what)
    xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), r.cuda()
    with tuning(lib, **env):
        for res in (None, rd):
            got_plan = lib.tango_debug_linear_route(DT[dtype], M, N, K, 0, 0, 1 if res is not None else 0, 0).decode()
            assert got_plan == plan, "%s is planned as %s" % (what, got_plan)
            out = torch.zeros(M, N, device="cuda")
            rc = lib.tango_op_linear(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(res), ptr(out), M, N, K, 0, 0, 0, None)
            assert rc == 0, lib.tango_last_error().decode()
            assert_exact(out, expected(acc, dtype, cols=(bd,), res=res, what=what), what + (" +res" if res is not None else ""), products(dtype))


def linear_ex(lib, dtype, plan, what, x, w, bias, M, N, K, b2=None, step=0, res=None, rv=None, rv_rows=0, rv_per=64, wb=0, pad=0):
    """route / refusal query, then tango_op_linear_ex -> the rows of the result [M][N] (from out_lo below rv_rows)"""
    name = C.create_string_buffer(64)
    why = lib.tango_debug_linear_ex_check(DT[dtype], M, N, K, 1 if res is not None else 0, 1 if b2 is not None else 0, 1 if rv is not None else 0,
                                          rv_rows, rv_per, 1 if rv is not None else 0, wb, pad, 0, name, 64).decode()
    assert why == "" and name.value.decode() == plan, "%s is planned as %s %s" % (what, name.value.decode(), why)
    out = torch.zeros(M, N + pad, device="cuda")
    out_lo = torch.zeros(M, N + (pad + 8 if pad else 0), device="cuda") if rv is not None else None
    xs, rs = x.cuda(), res.cuda() if res is not None else None
    ran = C.create_string_buffer(64)
    rc = lib.tango_op_linear_ex(DT[dtype], ptr(xs), ptr(w), ptr(bias), ptr(b2), STEPS if b2 is not None else 0, step, ptr(rs), ptr(rv), rv_rows,
                                rv_per, wb, pad, ptr(out), ptr(out_lo), M, N, K, ran, 64, None)
    assert rc == 0, lib.tango_last_error().decode()
    torch.cuda.synchronize()
    assert ran.value.decode() == plan, "%s ran as %s" % (what, ran.value.decode())
    return torch.cat([out_lo[:rv_rows, :N], out[rv_rows:, :N]]) if rv is not None else out[:, :N]


STEP_BIAS = [("wide", WIDE, (512, 320, 64), HALF), ("duo", FDUO, (512, 320, 64), HALF), ("dma", WIDE, (512, 160, 256), HALF),
             ("tile", {}, (512, 320, 64), ALL), ("tile+splitk", {}, (512, 1280, 1280), ALL),
             ("wide+pers", dict(TANGO_WIDE_PERS=1), (131072, 320, 64), HALF)]      # 512 tiles: two per workgroup


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(STEP_BIAS) for d in c[3]])
def test_linear_step_bias_exact(lib, case, dtype):
    """bias + bias2[step] + residual, the table read at step 0 and at the last step"""
    plan, env, (M, N, K), _ = STEP_BIAS[case]
    g, x, w, bias, r = linear_operands(dtype, M, N, K, seed=1)
    b2 = table(g, STEPS, N)
    what = "bias2 %s %s M=%d N=%d K=%d" % (plan, dtype, M, N, K)
    acc = linear_reference(x, w, 1, what)
    wd, bd, b2d, rd = w.cuda(), bias.cuda(), b2.cuda(), r.cuda()
    with tuning(lib, **env):
        for step in (0, STEPS - 1):
            out = linear_ex(lib, dtype, plan, what, x, wd, bd, M, N, K, b2=b2d, step=step, res=r)
            assert_exact(out, expected(acc, dtype, cols=(bd, b2d[step]), res=rd, what=what), "%s step %d" % (what, step), products(dtype))


# the boundary nowhere (0 rows), inside the first tile, on a tile edge; the vector changing at every wave and inside a tile
ROWVEC = [(rows, per) for rows in (0, 192, 256) for per in (64, 128)]


@gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("plan,env,M,N,K", [("wide", WIDE, 1024, 320, 320), ("duo", FDUO, 1024, 480, 96)])
def test_linear_rowvec_exact(lib, dtype, plan, env, M, N, K):
    """bias + rowvec[row / per] below the boundary into out_lo, bias alone above it into out, + residual, pitched rows (pad = 24, out_lo 32)"""
    g, x, w, bias, r = linear_operands(dtype, M, N, K, seed=2)
    tab = table(g, 4, N)
    acc = linear_reference(x, w, 1, "rowvec")
    wd, bd, rd = w.cuda(), bias.cuda(), r.cuda()
    with tuning(lib, **env):
        for rows, per in ROWVEC:
            what = "rowvec %s %s M=%d N=%d K=%d rows=%d per=%d" % (plan, dtype, M, N, K, rows, per)
            ns = (rows + per - 1) // per
            rv = tab[:max(ns, 1)].contiguous().cuda()
            out = linear_ex(lib, dtype, plan, what, x, wd, bd, M, N, K, res=r, rv=rv, rv_rows=rows, rv_per=per, pad=24)
            add = torch.zeros(M, N, dtype=torch.float64, device="cuda")
            add[:rows] = rv.double()[torch.arange(rows, device="cuda") // per]
            exp = expected(acc, dtype, cols=(bd, add), res=rd, what=what)
            assert_exact(out, exp, what, products(dtype))


@gpu
@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("plan,env", [("wide", WIDE), ("duo", FDUO)])
def test_linear_per_sample_weights_exact(lib, dtype, plan, env):
    """wb_rows = 256: another, independently drawn weight matrix at every tile; rowvec over all rows with rowvec_per = wb_rows"""
    M, N, K, wb = 1024, 320, 320, 256
    nw = M // wb
    g, x, w, bias, _ = linear_operands(dtype, M, N, K, nw=nw, seed=3)
    rv = table(g, nw, N).cuda()
    what = "wb_rows %s %s M=%d N=%d K=%d wb_rows=%d" % (plan, dtype, M, N, K, wb)
    acc = linear_reference(x, w, nw, what)
    bd = bias.cuda()
    with tuning(lib, **env):
        out = linear_ex(lib, dtype, plan, what, x, w.cuda(), bd, M, N, K, rv=rv, rv_rows=M, rv_per=wb, wb=wb)
    add = rv.double()[torch.arange(M, device="cuda") // wb]
    assert_exact(out, expected(acc, dtype, cols=(bd, add), what=what), what, products(dtype))


# ---- batched -------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("C_", [96, 160])
def test_gemm_batched_exact(lib, dtype, C_):
    """the three forms of the VAE attention block: A shared by the batch with a bias per output ROW; alpha = 0.25 with W inside A (lda = ldw = 2 C > K);
    K = HW = 224.  The batched wrapper has no route query: every other kernel's *_ok() predicate and the split-K policy demand batch == 1
    (gemm_route, gemm_pick_splitk), so the plan of a batch of three is the unsplit tile kernel by construction, and no name is asserted"""
    HW, batch = 224, 3
    g = gen(C_, HW, DT[dtype])

    def run(what, a, w, bias, M, N, K, lda, ldw, col=0, shared=0, alpha=1.0, bias_rows=0):
        out = torch.zeros(batch, M, N, device="cuda")
        rc = lib.tango_op_gemm_batched(DT[dtype], ptr(a), ptr(w), ptr(bias), ptr(out), batch, M, N, K, lda, ldw, col, shared, alpha, bias_rows, None)
        assert rc == 0, lib.tango_last_error().decode()
        return out

    def check(what, out, acc, a_last, w_last, **kw):
        same_ints(acc[-1, -64:], a_last[-64:].long() @ w_last.long().t(), what)
        assert_exact(out.view(-1, out.shape[-1]), expected(acc.view(-1, acc.shape[-1]), dtype, what=what, **kw), what, products(dtype))

    # V^T[b] = Wv hn[b]^T + bv[row]
    wv, hn, bv = signed(g, (C_, C_), XMAG[dtype]), signed(g, (batch, HW, C_), WMAG[dtype]), small(g, (C_,))
    what = "batched %s C=%d shared A, bias_rows" % (dtype, C_)
    out = run(what, wv.cuda(), hn.cuda(), bv.cuda(), C_, HW, C_, C_, C_, shared=1, bias_rows=1)
    acc = wv.cuda().double() @ hn.cuda().double().transpose(1, 2)
    check(what, out, acc, wv, hn[-1], cols=(bv.cuda().view(1, C_, 1).expand(batch, C_, HW).reshape(-1, HW),))
    # scores[b] = 0.25 q[b] k[b]^T, q | k the column halves of one buffer
    qk = torch.cat([signed(g, (batch, HW, C_), XMAG[dtype]), signed(g, (batch, HW, C_), WMAG[dtype])], 2).contiguous()
    what = "batched %s C=%d alpha, W inside A" % (dtype, C_)
    out = run(what, qk.cuda(), None, None, HW, HW, C_, 2 * C_, 2 * C_, col=C_, alpha=0.25)
    acc = qk.cuda().double()[:, :, :C_] @ qk.cuda().double()[:, :, C_:].transpose(1, 2)
    check(what, out, acc, qk[-1, :, :C_], qk[-1, :, C_:], alpha=0.25)
    # out[b] = P[b] V[b]
    pr, vt = signed(g, (batch, HW, HW), XMAG[dtype]), signed(g, (batch, C_, HW), WMAG[dtype])
    what = "batched %s C=%d K=HW" % (dtype, C_)
    out = run(what, pr.cuda(), vt.cuda(), None, HW, C_, HW, HW, HW)
    check(what, out, pr.cuda().double() @ vt.cuda().double().transpose(1, 2), pr[-1], vt[-1])


# ---- q | k | v^T ------------------------------------------------------------------------------------------------------------------------------------
QKV = [("tile", {}, (2, 256, 320, 64), ALL), ("wide", WIDE, (2, 256, 320, 64), HALF), ("duo", FDUO, (2, 256, 160, 96), HALF),
       ("stream", NODUO, (4, 1024, 320, 320), HALF), ("stream", NODUO, (8, 1024, 160, 640), HALF)]


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(QKV) for d in c[3]])
def test_linear_qkv_exact(lib, case, dtype):
    """q | k rows and V^T (gamma = beta = NULL), V^T also with the tokens of every block of 32 in the attention kernel's fragment order"""
    plan, env, (B, S, Ch, K), _ = QKV[case]
    M, N = B * S, 3 * Ch
    _, x, w, _, _ = linear_operands(dtype, M, N, K, seed=4)
    what = "qkv %s %s B=%d S=%d C=%d K=%d" % (plan, dtype, B, S, Ch, K)
    acc = linear_reference(x, w, 1, what)
    exp = expected(acc, dtype, what=what)
    exp_qk = exp[:, :2 * Ch].contiguous()
    exp_vt = exp[:, 2 * Ch:].reshape(B, S, Ch).transpose(1, 2).contiguous()
    s = torch.arange(S)
    pos = ((s & ~31) | ((s & 12) << 1) | ((s & 16) >> 2) | (s & 3)).cuda()      # position 8 g + 4 hi + r holds token 16 hi + 4 g + r
    exp_perm = torch.zeros_like(exp_vt)
    exp_perm[:, :, pos] = exp_vt
    xd, wd = x.cuda(), w.cuda()
    with tuning(lib, **env):
        got_plan = lib.tango_debug_linear_route(DT[dtype], M, N, K, 0, 0, 0, 1).decode()
        assert got_plan == plan, "%s is planned as %s" % (what, got_plan)
        for perm in ((0,) if dtype == "fp32" else (0, 1)):
            qk = torch.zeros(M, 2 * Ch, device="cuda")
            vt = torch.zeros(B, Ch, S, device="cuda")
            rc = lib.tango_op_linear_qkv_perm(DT[dtype], ptr(xd), ptr(wd), None, None, ptr(qk), ptr(vt), B, S, Ch, K, C.c_float(1e-5), perm, None)
            assert rc == 0, lib.tango_last_error().decode()
            assert_exact(qk, exp_qk, "%s perm=%d q|k" % (what, perm), products(dtype))
            assert_exact(vt.view(B * Ch, S), (exp_perm if perm else exp_vt).view(B * Ch, S), "%s perm=%d v^T" % (what, perm), products(dtype))


# ---- conv2d 3x3 ----------------------------------------------------------------------------------------------------------------------------------------
def conv2d_operands(dtype, B, Cin, H, W, Cout, Ho, Wo, seed=0):
    g = gen(B, Cin, H, W, Cout, DT[dtype], seed)
    x = signed(g, (B, Cin, H, W), XMAG[dtype])
    w = signed(g, (Cout, Cin, 3, 3), WMAG[dtype])
    return g, x, w, small(g, (Cout,)), signed(g, (B, Cout, Ho, Wo), RMAG)


def conv2d_reference(x, w, stride, pad, ups, what):
    """integer result rows [B Ho Wo][Cout] on the device; >= 64 rows of it (the bottom rows of the last image, or the last images whole)
    recomputed in int64 on the CPU"""
    acc = conv2d_acc(x.cuda(), w.cuda(), stride, pad, ups)
    B, Ho, Wo, Cout = acc.shape
    if Ho * Wo >= 64:
        nh = (64 + Wo - 1) // Wo
        same_ints(acc[-1:, Ho - nh:], conv2d_acc(x[-1:], w, stride, pad, ups, torch.int64, band=(Ho - nh, Ho)), what)
    else:
        nb = min(B, (64 + Ho * Wo - 1) // (Ho * Wo))
        same_ints(acc[B - nb:], conv2d_acc(x[B - nb:], w, stride, pad, ups, torch.int64), what)
    return acc.view(-1, Cout)


def conv2d_route(lib, dtype, B, Cin, H, W, Cout, stride=1, ups=0, pad=1, res=0, e_act=0, out_f32=0):
    return lib.tango_debug_conv2d_route(DT[dtype], B, Cin, H, W, Cout, stride, ups, pad, res, e_act, out_f32, None).decode()


# (plan, switches, (B, Cin, H, W, Cout), stride, pad, dtypes) through tango_op_conv2d_ex, each without and with a residual.  The split-K policy claims
# a 3x3 conv until the 128-row tiling has more than 341 tiles, so the unsplit routes carry M >= 22016 rows (N = 320) or 44032 (N <= 160)
CONV_EX = [
    ("conv_wide", FORCE, (86, 64, 16, 16, 320), 1, 1, HALF),                                   # the pipelined kernel (TANGO_CONV_PIPE = 2, the default)
    ("conv_wide", dict(FORCE, TANGO_CONV_PIPE=0), (86, 64, 16, 16, 320), 1, 1, HALF),         # the ping-pong kernel
    ("conv_wide", dict(FORCE, TANGO_CONV_TALL=1), (43, 64, 32, 16, 320), 1, 1, HALF),         # its 512 x 160 form
    ("conv_wide", FORCE, (344, 64, 32, 2, 320), 1, 1, HALF),                                    # W = 2: four images per tile
    ("conv_wide", FORCE, (86, 64, 64, 4, 320), 1, 1, HALF), ("conv_wide", FORCE, (22, 64, 128, 8, 320), 1, 1, HALF),       # W = 4: whole-image tiles; W = 8
    ("conv_wide", FORCE, (22, 64, 32, 32, 320), 1, 1, HALF),                                    # W = 32: 8-row tiles
    ("conv_wide", FORCE, (6, 64, 256, 16, 320), 1, 1, HALF),                                    # tall images: 16 tiles each
    ("conv_wide", dict(FORCE, TANGO_CONV_TALL=1), (86, 64, 64, 4, 320), 1, 1, HALF),            # two images per 512-row tile
    ("conv_wide+splitk", {}, (56, 512, 16, 16, 320), 1, 1, HALF),                               # 56 tiles x 4 splits, K = 4608
    ("conv_halo", FORCE, (172, 64, 16, 16, 160), 1, 1, HALF), ("conv_halo", FORCE, (172, 64, 16, 16, 128), 1, 1, HALF),
    ("conv_halo", FORCE, (86, 64, 16, 16, 320), 1, 1, ("fp32",)),
    ("tile", {}, (973, 64, 9, 5, 96), 1, 1, ALL),                                               # 43785 rows: a partial last tile
    ("tile+splitk", {}, (1, 64, 8, 4, 96), 1, 1, ALL),
    ("tile+splitk", {}, (3, 64, 16, 8, 96), 2, 0, ALL), ("tile+splitk", {}, (3, 64, 16, 8, 96), 2, 1, ALL),
    ("tile", {}, (3, 64, 4, 2, 30), 2, 0, ALL), ("tile", {}, (3, 64, 4, 2, 30), 2, 1, ALL),
    ("tile", {}, (2, 8, 16, 16, 64), 1, 1, ALL),                                                # Cin = 8: im2col + the linear tile kernel
    ("wide", FORCE, (2, 8, 16, 16, 320), 1, 1, HALF),                                           # ... + the 256 x 320 GEMM (K = 96: three 64-byte chunks)
    ("dma", FORCE, (6, 64, 128, 64, 640), 2, 0, ALL),                                           # the VAE Downsample: the last tap row / column falls off the image
    ("dma", FORCE, (7, 64, 130, 70, 640), 2, 1, ALL),                                           # 65 x 35 outputs: ragged last tile, tiles straddle images
    ("dma", FORCE, (8, 64, 160, 160, 128), 2, 1, ALL),                                          # the 128-column tile
]


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(CONV_EX) for d in c[5]])
def test_conv2d_exact(lib, case, dtype):
    plan, env, (B, Cin, H, W, Cout), stride, pad, _ = CONV_EX[case]
    Ho, Wo = (H + pad - 2) // stride + 1, (W + pad - 2) // stride + 1
    _, x, w, bias, r = conv2d_operands(dtype, B, Cin, H, W, Cout, Ho, Wo)
    what = "conv2d %s %s B=%d Cin=%d %dx%d Cout=%d stride %d pad %d" % (plan, dtype, B, Cin, H, W, Cout, stride, pad)
    acc = conv2d_reference(x, w, stride, pad, 0, what)
    xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), r.cuda()
    im2col = (Cin * (4 if dtype == "fp32" else 2)) % 64 != 0
    with tuning(lib, **env):
        for res in ((None,) if im2col else (None, rd)):
            got_plan = conv2d_route(lib, dtype, B, Cin, H, W, Cout, stride, 0, pad, 1 if res is not None else 0)
            assert got_plan == plan, "%s is planned as %s" % (what, got_plan)
            out = torch.zeros(B, Cout, Ho, Wo, device="cuda")
            rc = lib.tango_op_conv2d_ex(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(res), ptr(out), B, Cin, H, W, Cout, stride, pad, 0, 0.0, 0, None)
            assert rc == 0, lib.tango_last_error().decode()
            exp = expected(acc, dtype, cols=(bd,), res=rows_of(res) if res is not None else None, what=what)
            assert_exact(rows_of(out), exp, what + (" +res" if res is not None else ""), products(dtype))


# leaky-ReLU (slope 0.5: exact) epilogue and fp32 output rows, the arms of the VAE plans: (plan, switches, shape, e_act, out_f32, dtypes)
CONV_EPI = [
    ("conv_halo", FORCE, (172, 64, 16, 16, 160), LRELU, 0, HALF), ("conv_halo", FORCE, (86, 64, 16, 16, 320), LRELU, 0, ALL),
    ("conv_halo", FORCE, (4, 128, 64, 8, 32), 0, 0, HALF),                                      # the 256 x 32 narrow-output tile
    ("conv_halo", FORCE, (4, 128, 64, 8, 1), 0, 1, HALF),                                       # conv_out: one channel, fp32 rows
    ("tile", {}, (3, 128, 10, 6, 1), 0, 1, ALL),
    ("tile+splitk", {}, (1, 64, 8, 4, 96), LRELU, 0, ALL), ("tile+splitk", {}, (1, 64, 8, 4, 96), LRELU, 1, ALL),
    ("dma", FORCE, (8, 64, 160, 160, 128), LRELU, 0, ALL),
]


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(CONV_EPI) for d in c[5]])
def test_conv2d_epilogue_arms_exact(lib, case, dtype):
    plan, env, (B, Cin, H, W, Cout), e_act, out_f32, _ = CONV_EPI[case]
    stride = 2 if plan == "dma" else 1
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    _, x, w, bias, _ = conv2d_operands(dtype, B, Cin, H, W, Cout, Ho, Wo, seed=1)
    what = "conv2d %s %s B=%d Cin=%d %dx%d Cout=%d e_act=%d out_f32=%d" % (plan, dtype, B, Cin, H, W, Cout, e_act, out_f32)
    acc = conv2d_reference(x, w, stride, 1, 0, what)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    with tuning(lib, **env):
        got_plan = conv2d_route(lib, dtype, B, Cin, H, W, Cout, stride, 0, 1, 0, e_act, out_f32)
        assert got_plan == plan, "%s is planned as %s" % (what, got_plan)
        out = torch.zeros(B, Cout, Ho, Wo, device="cuda")
        rc = lib.tango_op_conv2d_ex(DT[dtype], ptr(xd), ptr(wd), ptr(bd), None, ptr(out), B, Cin, H, W, Cout, stride, 1, e_act, SLOPE, out_f32, None)
        assert rc == 0, lib.tango_last_error().decode()
    exp = expected(acc, dtype, cols=(bd,), slope=SLOPE if e_act else None, out_f32=bool(out_f32), what=what)
    assert_exact(rows_of(out), exp, what, products(dtype))


TEMB = [("conv_wide", FORCE, (86, 64, 16, 16, 320), HALF), ("conv_halo", FORCE, (172, 64, 16, 16, 160), HALF),
        ("conv_wide+splitk", {}, (56, 512, 16, 16, 320), HALF), ("tile", {}, (973, 64, 9, 5, 96), ALL), ("tile+splitk", {}, (1, 64, 8, 4, 96), ALL)]


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(TEMB) for d in c[3]])
def test_conv2d_step_bias_exact(lib, case, dtype):
    """tango_op_conv2d_temb: bias + bias2[step] + residual, steps 0 and 3 of a four-row table"""
    plan, env, (B, Cin, H, W, Cout), _ = TEMB[case]
    g, x, w, bias, r = conv2d_operands(dtype, B, Cin, H, W, Cout, H, W, seed=2)
    b2 = table(g, STEPS, Cout).cuda()
    what = "conv2d_temb %s %s B=%d Cin=%d %dx%d Cout=%d" % (plan, dtype, B, Cin, H, W, Cout)
    acc = conv2d_reference(x, w, 1, 1, 0, what)
    xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), r.cuda()
    with tuning(lib, **env):
        got_plan = conv2d_route(lib, dtype, B, Cin, H, W, Cout, 1, 0, 1, 1)
        assert got_plan == plan, "%s is planned as %s" % (what, got_plan)
        for step in (0, STEPS - 1):
            out = torch.zeros(B, Cout, H, W, device="cuda")
            ran = C.create_string_buffer(64)
            rc = lib.tango_op_conv2d_temb(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(b2), STEPS, step, ptr(rd), ptr(out), B, Cin, H, W, Cout, ran, 64, None)
            assert rc == 0, lib.tango_last_error().decode()
            assert ran.value.decode() == plan, "%s ran as %s" % (what, ran.value.decode())
            exp = expected(acc, dtype, cols=(bd, b2[step]), res=rows_of(rd), what=what)
            assert_exact(rows_of(out), exp, "%s step %d" % (what, step), products(dtype))


# fused nearest x2 upsample: (plan with the phase form asked, plan with nine taps asked, switches, (B, Cin, H, W, Cout), dtypes)
UPS = [("conv_wide+phase", "conv_wide", FORCE, (22, 64, 16, 16, 320), HALF),                    # 22 x 1024 output rows
       ("conv_wide+phase", "conv_wide", FORCE, (22, 64, 64, 4, 320), HALF),                     # 8-wide output of a 4-wide source
       (None, "conv_halo", FORCE, (43, 64, 16, 16, 160), HALF), (None, "tile+splitk", {}, (3, 64, 8, 4, 32), ALL)]


@gpu
@pytest.mark.parametrize("case,dtype", [(i, d) for i, c in enumerate(UPS) for d in c[4]])
def test_conv2d_upsample_exact(lib, case, dtype):
    """tango_op_conv2d_ups_temb as nine taps on the upsampled grid and as four 2x2-tap phase convolutions on the source grid (phase weights
    are sums of at most four integer taps, |sum| <= 8: exact in T), bias2 at the last step; tango_op_conv2d decides by itself"""
    phase_plan, nine_plan, env, (B, Cin, H, W, Cout), _ = UPS[case]
    g, x, w, bias, _ = conv2d_operands(dtype, B, Cin, H, W, Cout, 2 * H, 2 * W, seed=3)
    b2 = table(g, STEPS, Cout).cuda()
    what = "conv2d_ups %s %s B=%d Cin=%d %dx%d Cout=%d" % (phase_plan or nine_plan, dtype, B, Cin, H, W, Cout)
    acc = conv2d_reference(x, w, 1, 1, 1, what)
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    step = STEPS - 1
    exp = expected(acc, dtype, cols=(bd, b2[step]), what=what)
    with tuning(lib, **env):
        auto_plan = conv2d_route(lib, dtype, B, Cin, H, W, Cout, 1, 1, 1)
        assert auto_plan == (phase_plan or nine_plan), "%s is planned as %s" % (what, auto_plan)
        for phases, plan in ((0, nine_plan), (1, phase_plan)):
            if plan is None:
                continue
            out = torch.zeros(B, Cout, 2 * H, 2 * W, device="cuda")
            ran = C.create_string_buffer(64)
            rc = lib.tango_op_conv2d_ups_temb(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(b2), STEPS, step, ptr(out), B, Cin, H, W, Cout, phases, ran, 64, None)
            assert rc == 0, lib.tango_last_error().decode()
            assert ran.value.decode() == plan, "%s phases=%d ran as %s" % (what, phases, ran.value.decode())
            assert_exact(rows_of(out), exp, "%s phases=%d" % (what, phases), products(dtype))
            one = b2[1].contiguous()          # tango_op_conv2d_ups: bias2 as a single row, no step pointer
            out = torch.zeros(B, Cout, 2 * H, 2 * W, device="cuda")
            rc = lib.tango_op_conv2d_ups(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(one), ptr(out), B, Cin, H, W, Cout, phases, None)
            assert rc == 0, lib.tango_last_error().decode()
            assert_exact(rows_of(out), expected(acc, dtype, cols=(bd, one), what=what), "%s phases=%d, one bias2 row" % (what, phases), products(dtype))
        out = torch.zeros(B, Cout, 2 * H, 2 * W, device="cuda")
        rc = lib.tango_op_conv2d(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(out), B, Cin, H, W, Cout, 1, 1, None)
        assert rc == 0, lib.tango_last_error().decode()
        assert_exact(rows_of(out), expected(acc, dtype, cols=(bd,), what=what), what + " tango_op_conv2d", products(dtype))


# ---- conv1d / conv_transpose1d -------------------------------------------------------------------------------------------------------------------------
# (Cin, Cout, L, k, dilation, residual): L no multiple of the 128- / 256-row tiles; the last: five 256-row tiles, the batch boundary inside the third
CONV1D = [(128, 128, 301, 3, 1, 1), (64, 160, 301, 7, 3, 0), (64, 160, 301, 11, 5, 1), (64, 128, 40, 11, 5, 1), (128, 128, 513, 11, 3, 1), (64, 160, 301, 7, 1, 0),
          (128, 128, 301, 3, 5, 0)]


def conv1d_route(lib, dtype, B, Cin, L, Cout, k, d, a_act, res):
    sk = C.c_int(0)
    name = lib.tango_debug_conv1d_route(DT[dtype], B, Cin, L, Cout, k, d, -d * (k - 1) // 2, L, 1, 0, a_act, res, 0, C.byref(sk)).decode()
    return name, sk.value


@gpu
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("plan,env,a_act", [("tile", {}, 0), ("dma", FORCE, 0), ("tile", FORCE, LRELU)])
@pytest.mark.parametrize("case", range(len(CONV1D)))
def test_conv1d_exact(lib, dtype, plan, env, a_act, case):
    """k in {3, 7, 11} x dilation in {1, 3, 5} on the tile and the LDS-DMA kernels; a leaky-ReLU prologue (slope 0.5: halves stay exact in T and
    in the products) keeps a problem on the tile kernel even when the DMA kernel is forced"""
    Cin, Cout, L, k, d, res = CONV1D[case]
    B = 2
    g = gen(Cin, Cout, L, k, d, DT[dtype])
    x, w = signed(g, (B, Cin, L), XMAG[dtype]), signed(g, (Cout, Cin, k), WMAG[dtype])
    bias, r = small(g, (Cout,)), signed(g, (B, Cout, L), RMAG)
    what = "conv1d %s %s Cin=%d Cout=%d L=%d k=%d d=%d a_act=%d" % (plan, dtype, Cin, Cout, L, k, d, a_act)
    xin = torch.where(x < 0, x * SLOPE, x) if a_act else x
    acc = conv1d_acc(xin.cuda(), w.cuda(), d)
    l0 = max(0, L - 64)
    same_ints(acc[-1:, l0:] * 2, conv1d_acc((xin[-1:] * 2), w, d, torch.int64, rows=(l0, L)), what)     # (x 2: the halved inputs as integers)
    xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), r.cuda() if res else None
    with tuning(lib, **env):
        assert conv1d_route(lib, dtype, B, Cin, L, Cout, k, d, a_act, res) == (plan, 1), what
        out = torch.zeros(B, Cout, L, device="cuda")
        rc = lib.tango_op_conv1d(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(rd), ptr(out), B, Cin, L, Cout, k, d, a_act, SLOPE, 0, 0.0, None)
        assert rc == 0, lib.tango_last_error().decode()
    exp = expected(acc.view(-1, Cout) * (2.0 if a_act else 1.0), dtype, alpha=0.5 if a_act else 1.0, cols=(bd,), res=rows_of(rd) if res else None, what=what)
    assert_exact(rows_of(out), exp, what, [pm * (0.5 if a_act else 1.0) for pm in products(dtype)] + (products(dtype) if a_act else []))


@gpu
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("plan,env", [("tile", {}), ("dma", FORCE)])
@pytest.mark.parametrize("k,u", [(16, 8), (16, 5), (8, 2), (4, 2)])
def test_conv_transpose1d_exact(lib, dtype, plan, env, k, u):
    """every phase of the decomposition (u gather problems with tap step -1) against the scatter statement of the transposed conv"""
    B, Ci, Co, L = 2, 128, 128, 53
    pd = (k - u) // 2
    g = gen(k, u, L, DT[dtype])
    x, w, bias = signed(g, (B, Ci, L), XMAG[dtype]), signed(g, (Ci, Co, k), WMAG[dtype]), small(g, (Co,))
    what = "conv_transpose1d %s %s k=%d u=%d L=%d" % (plan, dtype, k, u, L)
    acc = convt1d_acc(x.cuda(), w.cuda(), u, pd)
    same_ints(acc[-1:], convt1d_acc(x[-1:], w, u, pd, torch.int64), what)
    Lo = acc.shape[1]
    xd, wd, bd = x.cuda(), w.cuda(), bias.cuda()
    with tuning(lib, **env):
        phases = 0
        for r in range(u):
            geom = (C.c_int * 6)()
            if not lib.tango_debug_conv_transpose1d_phase(B, Ci, L, Co, k, u, pd, r, geom):
                continue
            sk = C.c_int(0)
            name = lib.tango_debug_conv1d_route(DT[dtype], B, Ci, L, Co, *list(geom), 0, 0, 0, C.byref(sk)).decode()
            assert (name, sk.value) == (plan, 1), "%s: phase %d is planned as %s" % (what, r, name)
            phases += 1
        assert phases == u, what
        out = torch.zeros(B, Co, Lo, device="cuda")
        rc = lib.tango_op_conv_transpose1d(DT[dtype], ptr(xd), ptr(wd), ptr(bd), ptr(out), B, Ci, L, Co, k, u, pd, 0, 0.0, None)
        assert rc == 0, lib.tango_last_error().decode()
    assert_exact(rows_of(out), expected(acc.view(-1, Co), dtype, cols=(bd,), what=what), what, products(dtype))
