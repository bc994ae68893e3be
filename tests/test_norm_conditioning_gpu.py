"""Conditioning of the normalisation statistics: GroupNorm groups and LayerNorm rows that sit on a common offset many times their spread
(the ordinary state of several GroupNorm inputs of trained UNet / VAE checkpoints; every other parity test here feeds mean / sigma <= 3).
A one-pass variance Q/n - mean^2 from fp32 sums of x and x*x loses about (mean / sigma)^2 * 2^-24 of its value, however exactly the last
subtraction is done.  The GroupNorm kernels therefore accumulate x - K about a pivot K of the (sample, group) (norm.hip), the LayerNorm kernels centre a
second pass over registers, and the fp32 streaming linear centres its fragments on the row's first element; the 16-bit in-GEMM row statistics sum x and
x * x as they are (their offsets of +-32 stay on the output-rounding floor here).

Reference: torch's group_norm / layer_norm in float64 applied to the input AFTER it was rounded to the engine's storage type, so that only
the kernel's arithmetic is measured.  Yardstick: torch's own fp32 CPU operator on the same input against the same float64 result (printed
next to the kernel's error for every case; run with -s to see the table).

GroupNorm error measure: per (sample, group) max|out - ref| / max|ref| over that group's elements -- a tensor-wide maximum would let a healthy
group's scale hide a sick one.  Bound per group: max(TOL[dtype], 4 e_ref) with the project's TOL (the one used at mean / sigma = 0) and e_ref the
fp32 CPU operator's error in that group; the factor 4 covers a different summation order and the rounding of the apply step, which grows like
(mean / sigma) 2^-24 (8e-6 at 128: why the sweep ends there)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gn_coop_gpu import DT, TOL, gn, p, q, tuning

pytestmark = pytest.mark.gpu

GROUPS = 32
EPS_ACT = ((1e-5, 1), (1e-6, 0))

# form -> (switches, shapes (samples, channels, rows)); the rule of norm.hip gn_launch that selects the form with these switches:
#   slab      default switches: gn_slab_geom() holds (rows 64 / 256 = 16 x {4, 16}, groups of 40 / 80 channels = whole 16-byte vectors of every
#             dtype, 20 vectors per slab row a multiple of the group's) -> gn_slab_kernel, first rule of gn_launch
#   group     TANGO_GN_SLAB=0; rows < 1024 and no TANGO_GN_COOP_ALL, so not the cooperative kernel; even groups of rows x cg / 2 <= 24576 pairs and
#             a tensor below TANGO_GN_SMALL_MB (8 MiB) -> gn_fused_small_kernel, one workgroup per (sample, group)
#   coop      TANGO_GN_SLAB=0, TANGO_GN_COOP_ALL=1 lifts the size rule; <= 256 vectors per row, the grid fits the chip -> gn_coop_kernel
#   coop_fb   the same plus TANGO_GN_COOP_FORCE_FALLBACK=1: every workgroup re-reduces its sample without the rendezvous; bit-identical to coop
#   two       TANGO_NO_GN_COOP=1, TANGO_GN_SMALL_MB=0 (no tensor is "small"), TANGO_GN_SLAB=0 -> gn_stats_kernel + gn_apply_kernel; chunks of 16
#             rows: 1024 = 64 chunks, 4100 = 256 + a 4-row tail chunk, 33 = 2 + a 1-row tail chunk (fp32 C = 1920: two vectors per thread and row)
# No (form, shape, dtype) of this table has to be skipped: the cooperative kernel cannot take fp32 rows of more than 1024 channels, and its
# two shapes have 320 and 640.
FORMS = {
    "slab": (dict(), [(3, 1280, 64), (2, 2560, 256)]),
    "group": (dict(TANGO_GN_SLAB=0), [(3, 320, 256), (2, 64, 777)]),
    "coop": (dict(TANGO_GN_SLAB=0, TANGO_GN_COOP_ALL=1), [(2, 320, 1024), (2, 640, 1024)]),
    "coop_fb": (dict(TANGO_GN_SLAB=0, TANGO_GN_COOP_ALL=1, TANGO_GN_COOP_FORCE_FALLBACK=1), [(2, 320, 1024), (2, 640, 1024)]),
    "two": (dict(TANGO_NO_GN_COOP=1, TANGO_GN_SMALL_MB=0, TANGO_GN_SLAB=0), [(2, 320, 1024), (1, 128, 4100), (2, 1920, 33)]),
}
FAMILIES = ["offset0", "offset8", "offset32", "offset128", "offset-128", "one_bad_group", "small_spread", "constant_group"]
DTYPES = ["fp32", "fp16", "bf16"]
GN_SHAPES = sorted({s for _, shapes in FORMS.values() for s in shapes})
# ordered so that the forms sharing a shape run next to each other: the float64 reference of an input is computed once and the caches stay small
GN_CASES = [(f, s, d) for s in GN_SHAPES for d in DTYPES for f in FORMS if s in FORMS[f][1]]
GN_FAMILY_CASES = [(f, s, fam, d) for s in GN_SHAPES for fam in FAMILIES for d in DTYPES for f in FORMS if s in FORMS[f][1]]


# what tango_debug_groupnorm_form must report for the form (the forced fallback is a mode of the cooperative kernel)
FORM_NAME = {"slab": "slab", "group": "group", "coop": "coop", "coop_fb": "coop", "two": "two"}


def assert_form(lib, form, dtype, shape):
    """inside tuning(): the dispatcher really picks the kernel this case is about (a declined cooperative launch would otherwise pass as another form)"""
    B, Cc, HW = shape
    got = lib.tango_debug_groupnorm_form(DT[dtype], B, Cc, HW, GROUPS).decode()
    assert got == FORM_NAME[form], "groupnorm %s %s %s: dispatched to %r, this case is about %r" % (form, shape, dtype, got, FORM_NAME[form])


def _id(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else v for v in c)


def _seed(*a):
    return sum((i + 1) * 7919 * abs(int(v)) for i, v in enumerate(a)) % (2 ** 31)


@functools.lru_cache(maxsize=2)
def gn_input(family, shape, dtype):
    """x (rounded to the storage type), gamma, beta on the CPU; shared by every form that runs this shape and never modified"""
    B, Cc, HW = shape
    cg = Cc // GROUPS
    g = torch.Generator().manual_seed(_seed(B, Cc, HW, len(family), ord(family[-1])))
    x = torch.randn(B, Cc, HW, generator=g)
    if family.startswith("offset"):
        x = x + float(family[len("offset"):])
    elif family == "one_bad_group":
        x[0, 5 * cg:6 * cg] += 128.0
        x[B - 1, 31 * cg:] -= 128.0
    elif family == "small_spread":
        # true variance below / near eps: a cancelled variance moves rstd by percent.  16-bit: sigma = 2^-6 so that the rounded data keeps several levels
        x = 1.0 + x * (1e-3 if dtype == "fp32" else 2.0 ** -6)
    elif family == "constant_group":
        x[B - 1, 7 * cg:8 * cg] = 3.0
    x = q(x, dtype)
    ga, be = 1.0 + 0.2 * torch.randn(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g)
    return x, ga, be


@functools.lru_cache(maxsize=4)
def gn_reference(family, shape, dtype, eps, act):
    """float64 reference, and per (sample, group): its scale max|ref| and the error e_ref of torch's fp32 CPU operator"""
    x, ga, be = gn_input(family, shape, dtype)
    ref = F.group_norm(x.double(), GROUPS, ga.double(), be.double(), eps)
    r32 = F.group_norm(x, GROUPS, ga, be, eps)
    if act:
        ref, r32 = F.silu(ref), F.silu(r32)
    B = shape[0]
    scale = ref.abs().reshape(B, GROUPS, -1).amax(-1)
    e_ref = (r32.double() - ref).abs().reshape(B, GROUPS, -1).amax(-1) / scale
    return ref, scale, e_ref


def group_errors(out, ref, scale):
    return (out.double().cpu() - ref).abs().reshape(ref.shape[0], GROUPS, -1).amax(-1) / scale


def check_groups(what, out, family, shape, dtype, eps, act):
    ref, scale, e_ref = gn_reference(family, shape, dtype, eps, act)
    assert torch.isfinite(out).all(), "%s: output not finite" % what
    e = group_errors(out, ref, scale)
    bound = torch.clamp(4.0 * e_ref, min=TOL[dtype])
    worst = int(torch.argmax(e / bound))
    b, grp = divmod(worst, GROUPS)
    ek, er, bd = e[b, grp].item(), e_ref[b, grp].item(), bound[b, grp].item()
    print("groupnorm %s eps=%g act=%d: worst (sample %d, group %d) e_kernel %.3e e_ref %.3e bound %.3e | max over groups e_kernel %.3e e_ref %.3e"
          % (what, eps, act, b, grp, ek, er, bd, e.max().item(), e_ref.max().item()))
    assert ek <= bd, "groupnorm %s eps=%g act=%d: sample %d group %d: e_kernel %.3e > bound %.3e (torch fp32 CPU: %.3e)" % (what, eps, act, b, grp, ek, bd, er)


@pytest.mark.parametrize("form,shape,family,dtype", GN_FAMILY_CASES, ids=[_id(c) for c in GN_FAMILY_CASES])
def test_groupnorm_statistics_on_offset_inputs(lib, form, shape, family, dtype):
    x, ga, be = gn_input(family, shape, dtype)
    xg, gg, bg = x.cuda(), ga.cuda(), be.cuda()
    what = "%s %s %s %s" % (form, "x".join(map(str, shape)), dtype, family)
    for eps, act in EPS_ACT:
        with tuning(lib, **FORMS[form][0]):
            assert_form(lib, form, dtype, shape)
            out = gn(lib, dtype, xg, gg, bg, eps, act)
            assert torch.equal(gn(lib, dtype, xg, gg, bg, eps, act), out), "%s: second run differs" % what
        check_groups(what, out, family, shape, dtype, eps, act)
        if form == "coop_fb":
            with tuning(lib, **FORMS["coop"][0]):
                assert_form(lib, "coop", dtype, shape)
                assert torch.equal(gn(lib, dtype, xg, gg, bg, eps, act), out), "%s: the forced fallback differs from the rendezvous result" % what


@pytest.mark.parametrize("form,shape,dtype", GN_CASES, ids=[_id(c) for c in GN_CASES])
def test_groupnorm_batch_invariance_with_a_badly_conditioned_sample(lib, form, shape, dtype):
    """the 'one bad group' tensor: the first and the last sample carry a group at +-128 sigma; each run alone must equal its slice of the batch"""
    x, ga, be = gn_input("one_bad_group", shape, dtype)
    xg, gg, bg = x.cuda(), ga.cuda(), be.cuda()
    B = shape[0]
    for eps, act in EPS_ACT:
        with tuning(lib, **FORMS[form][0]):
            assert_form(lib, form, dtype, shape)
            assert_form(lib, form, dtype, (1,) + shape[1:])
            full = gn(lib, dtype, xg, gg, bg, eps, act)
            for b in sorted({0, B - 1}):
                alone = gn(lib, dtype, xg[b:b + 1].contiguous(), gg, bg, eps, act)
                assert torch.equal(alone, full[b:b + 1]), "%s %s %s: sample %d alone differs from its slice of the batch" % (form, shape, dtype, b)


# ------------------------------------------------------------------------------------------
# LayerNorm, plain and folded into the linear that consumes it.  Rows are m_r + randn with m_r cycling through {0, +8, -8, +32, -32} ROW BY ROW, so that
# every 16- or 32-row MFMA fragment mixes well- and ill-conditioned rows; one row is exactly constant.  Reference: float64 layer_norm -> linear (-> GEGLU)
# (+ residual) on the rounded operands.  Bound: 2 TOL[dtype] of the output scale (as test_ops_gpu.test_linear_layernorm_fused), taken PER ROW.
# ------------------------------------------------------------------------------------------
LN_MEANS = (0.0, 8.0, -8.0, 32.0, -32.0)
CONST_ROW = 7


def ln_rows(g, M, K, dtype):
    x = torch.randn(M, K, generator=g) + torch.tensor(LN_MEANS).repeat(M // len(LN_MEANS) + 1)[:M, None]
    x[CONST_ROW % M] = 2.5
    return q(x, dtype)


def ln_affine(g, K):
    return 1 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)


def check_rows(what, dtype, outs_refs):
    """outs_refs: (name, kernel output, float64 reference, torch fp32 CPU result); rows along dim 0"""
    worst = None
    for name, out, ref, r32 in outs_refs:
        out = out.double().cpu()
        assert torch.isfinite(out).all(), "%s %s: output not finite" % (what, name)
        scale = ref.abs().flatten(1).amax(-1)
        e = (out - ref).abs().flatten(1).amax(-1) / scale
        er = (r32.double() - ref).abs().flatten(1).amax(-1) / scale
        r = int(torch.argmax(e))
        print("%s %s %s: worst row %d (mean offset %+g) e_kernel %.3e e_ref there %.3e | max over rows e_ref %.3e | bound %.1e"
              % (what, dtype, name, r, LN_MEANS[r % len(LN_MEANS)], e[r].item(), er[r].item(), er.max().item(), 2 * TOL[dtype]))
        if worst is None or e[r].item() > worst[0]:
            worst = (e[r].item(), name, r)
    assert worst[0] <= 2 * TOL[dtype], "%s %s %s: row %d: e_kernel %.3e > %.1e" % (what, dtype, worst[1], worst[2], worst[0], 2 * TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,K", [(37, 1280), (100, 320)])
def test_layernorm_rows_on_offsets(lib, dtype, rows, K):
    g = torch.Generator().manual_seed(rows + K)
    x = ln_rows(g, rows, K, dtype)
    ga, be = ln_affine(g, K)
    ref = F.layer_norm(x.double(), (K,), ga.double(), be.double(), 1e-5)
    r32 = F.layer_norm(x, (K,), ga, be, 1e-5)
    xg, gg, bg = x.cuda(), ga.cuda(), be.cuda()
    out = torch.zeros(rows, K, device="cuda")
    rc = lib.tango_op_layernorm(DT[dtype], p(xg), p(gg), p(bg), p(out), rows, K, 1e-5, None)
    assert rc == 0, lib.tango_last_error().decode()
    check_rows("layernorm %dx%d" % (rows, K), dtype, [("y", out, ref, r32)])


def ln_linear_reference(x, w, b, ga, be, r, geglu, dt):
    K = x.shape[1]
    c = lambda t: None if t is None else t.to(dt)   # noqa: E731
    h = F.linear(F.layer_norm(c(x), (K,), c(ga), c(be), 1e-5), c(w), c(b))
    if geglu:
        v, gt = h.chunk(2, dim=-1)
        h = v * F.gelu(gt)
    return h + c(r) if r is not None else h


FORCE = dict(TANGO_FORCE_DMA_GEMM=1)
WIDE_PING = dict(FORCE, TANGO_WIDE_PIPE=0, TANGO_WIDE_PERS=0, TANGO_DUO_MAXK=0)
DUO = dict(TANGO_DUO_MAXK=100000, TANGO_DUO_MIN_TILES=1, TANGO_DUO_MASK=15)
# (name, switches, M, N, K, geglu, residual, dtypes, route the dispatcher must report for the 16-bit types / for fp32)
LINEAR_LN_CASES = [
    # default switches, the shapes of test_ops_gpu.test_linear_layernorm_fused: weight-stationary streaming kernel (rows of 640 / 1280 bytes, M >= 4096; it
    # carries a per-row shift), else the two-pass LayerNorm kernel + a plain GEMM
    ("stream-k320", dict(), 4128, 320, 320, 0, 1, DTYPES, "stream", "stream"),
    ("stream-k640", dict(), 4096, 640, 640, 0, 1, DTYPES, "stream", "layernorm+"),
    ("fallback", dict(), 300, 320, 320, 0, 0, DTYPES, "layernorm+", "layernorm+"),
    ("stream-geglu", dict(), 4100, 2560, 320, 1, 0, DTYPES, "stream", "layernorm+"),
    # ln_stats_kernel (two-pass) + the 256 x 320 GEMM reading the row statistics (XS): the engine's route for the GEGLU projections of levels 1-2
    ("wide-xstats", WIDE_PING, 512, 2560, 640, 1, 0, DTYPES[1:], "wide+xstats", None),
    # in-kernel row statistics of the 256 x 320 GEMM, in each of its main loops (test_wide_pipe_gpu.py: ping-pong, pipelined, pipelined in lockstep) ...
    ("wide-ping", WIDE_PING, 768, 640, 640, 0, 1, DTYPES[1:], "wide", None),
    ("wide-pipe1", dict(WIDE_PING, TANGO_WIDE_PIPE=1), 768, 640, 640, 0, 1, DTYPES[1:], "wide", None),
    ("wide-pipe2", dict(WIDE_PING, TANGO_WIDE_PIPE=2), 512, 320, 320, 0, 0, DTYPES[1:], "wide", None),
    # ... and of the 256 x 160 GEMM (test_duo_gpu.py)
    ("duo", DUO, 512, 320, 320, 0, 1, DTYPES[1:], "duo", None),
    ("duo-k640", DUO, 512, 480, 640, 0, 0, DTYPES[1:], "duo", None),
]


LINEAR_LN_PARAMS = [c[:7] + (d,) + c[8:] for c in LINEAR_LN_CASES for d in c[7]]


@pytest.mark.parametrize("name,env,M,N,K,geglu,res,dtype,route16,route32", LINEAR_LN_PARAMS, ids=["%s-%s" % (c[0], c[7]) for c in LINEAR_LN_PARAMS])
def test_linear_ln_rows_on_offsets(lib, name, env, M, N, K, geglu, res, dtype, route16, route32):
    g = torch.Generator().manual_seed(M + N + K)
    x = ln_rows(g, M, K, dtype)
    w = q(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    ga, be = ln_affine(g, K)
    No = N // 2 if geglu else N
    r = q(torch.randn(M, No, generator=g), dtype) if res else None
    ref = ln_linear_reference(x, w, b, ga, be, r, geglu, torch.float64)
    r32 = ln_linear_reference(x, w, b, ga, be, r, geglu, torch.float32)
    dev = [t.cuda() if t is not None else None for t in (x, w, b, ga, be, r)]
    out = torch.zeros(M, No, device="cuda")
    with tuning(lib, **env):
        route = lib.tango_debug_linear_route(DT[dtype], M, N, K, geglu, 1, res, 0).decode()
        want = route32 if dtype == "fp32" else route16
        assert route.startswith(want), "linear_ln %s %s: dispatched to %r, this case is about %r" % (name, dtype, route, want)
        rc = lib.tango_op_linear_ln(DT[dtype], *[p(t) if t is not None else None for t in dev], p(out), M, N, K, geglu, 1e-5, None)
        assert rc == 0, lib.tango_last_error().decode()
    check_rows("linear_ln %s (%s) M=%d N=%d K=%d" % (name, route, M, N, K), dtype, [("y", out, ref, r32)])


# shapes where a materialised LayerNorm is followed by a split-K GEMM: the wrapper, its route query and the engine plan one way (gemm.hip plan_linear)
LN_SPLITK_CASES = [(300, 320, 320, "fp32"), (512, 1280, 1280, "fp16"), (512, 1280, 1280, "bf16")]


@pytest.mark.parametrize("M,N,K,dtype", LN_SPLITK_CASES, ids=["%dx%dx%d-%s" % c for c in LN_SPLITK_CASES])
def test_linear_ln_wrapper_equals_its_query_and_its_parts(lib, M, N, K, dtype):
    """LayerNorm, no GEGLU, no residual: the query names layernorm + split-K tile GEMM, and tango_op_linear_ln runs exactly those two launches, so its
    output is bit-identical to tango_op_linear(tango_op_layernorm(x)).  (Before the wrapper shared the engine's planner it ran the GEMM unsplit
    while the query said split: max |wrapper - parts| was 3.3e-6 in fp32, 3.9e-3 in fp16 and 1.6e-2 in bf16 on outputs of scale 6.5, all three cases failing.)"""
    g = torch.Generator().manual_seed(M + N + K)
    x = ln_rows(g, M, K, dtype)
    w = q(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b = torch.randn(N, generator=g)
    ga, be = ln_affine(g, K)
    xg, wg, bg, gg, eg = (t.cuda() for t in (x, w, b, ga, be))
    route = lib.tango_debug_linear_route(DT[dtype], M, N, K, 0, 1, 0, 0).decode()
    assert route == "layernorm+tile+splitk", route
    fused = torch.zeros(M, N, device="cuda")
    rc = lib.tango_op_linear_ln(DT[dtype], p(xg), p(wg), p(bg), p(gg), p(eg), None, p(fused), M, N, K, 0, 1e-5, None)
    assert rc == 0, lib.tango_last_error().decode()
    xn = torch.zeros(M, K, device="cuda")
    rc = lib.tango_op_layernorm(DT[dtype], p(xg), p(gg), p(eg), p(xn), M, K, 1e-5, None)
    assert rc == 0, lib.tango_last_error().decode()
    parts = torch.zeros(M, N, device="cuda")
    rc = lib.tango_op_linear(DT[dtype], p(xn), p(wg), p(bg), None, p(parts), M, N, K, 0, 0, 0, None)
    assert rc == 0, lib.tango_last_error().decode()
    diff = (fused - parts).abs().max().item()
    print("linear_ln %dx%dx%d %s (%s): max |wrapper - parts| = %.3e of scale %.3e" % (M, N, K, dtype, route, diff, parts.abs().max().item()))
    assert torch.equal(fused, parts)


# tango_op_qkv_stat (the activation-stationary kernel) takes the 16-bit types only: (qkv_stat, fp32) is the one combination left out
QKV_CASES = [("qkv_stat", d) for d in DTYPES[1:]] + [("linear_qkv", d) for d in DTYPES]


@pytest.mark.parametrize("op,dtype", QKV_CASES, ids=["%s-%s" % c for c in QKV_CASES])
def test_qkv_rows_on_offsets(lib, op, dtype):
    """norm1 + [to_q | to_k | to_v^T]: the activation-stationary kernel (tango_op_qkv_stat mode 0) and the GEMM route (tango_op_linear_qkv), at the smallest
    shape of test_qkv_stat_gpu.py"""
    B, S, Ch = 1, 256, 320
    g = torch.Generator().manual_seed(B * S + 1)
    x = ln_rows(g, B * S, Ch, dtype)
    w = q(torch.randn(3 * Ch, Ch, generator=g) / Ch ** 0.5, dtype)
    ga, be = ln_affine(g, Ch)
    h = ln_linear_reference(x, w, None, ga, be, None, 0, torch.float64)
    h32 = ln_linear_reference(x, w, None, ga, be, None, 0, torch.float32)
    xg, wg, gg, bg = x.cuda(), w.cuda(), ga.cuda(), be.cuda()
    qk = torch.zeros(B * S, 2 * Ch, device="cuda")
    vt = torch.zeros(B, Ch, S, device="cuda")
    if op == "qkv_stat":
        rc = lib.tango_op_qkv_stat(DT[dtype], p(xg), p(wg), p(gg), p(bg), p(qk), p(vt), B, S, Ch, 1e-5, 0, 0, None, None)
    else:
        rc = lib.tango_op_linear_qkv(DT[dtype], p(xg), p(wg), p(gg), p(bg), p(qk), p(vt), B, S, Ch, Ch, 1e-5, None)
    assert rc == 0, lib.tango_last_error().decode()
    # rows of v^T are channels: back to [token][channel] so that every measure is per token row, against the scale of the token's whole q | k | v row
    got = torch.cat([qk, vt.transpose(1, 2).reshape(B * S, Ch)], dim=1)
    check_rows("%s B=%d S=%d" % (op, B, S), dtype, [("q|k|v", got, h, h32)])


@pytest.mark.parametrize("dtype", DTYPES[1:])
def test_ff_fused_rows_on_offsets(lib, dtype):
    """x + ff.net.2(GEGLU(ff.net.0.proj(LayerNorm(x)))) in one launch, at the smallest shape of test_ff_fused_gpu.py"""
    M, Cc, H = 128, 320, 1280
    g = torch.Generator().manual_seed(M + 4)
    x = ln_rows(g, M, Cc, dtype)
    w1 = q(torch.randn(2 * H, Cc, generator=g) / Cc ** 0.5, dtype)
    b1 = 0.3 * torch.randn(2 * H, generator=g)
    w2 = q(torch.randn(Cc, H, generator=g) / H ** 0.5, dtype)
    b2 = 0.3 * torch.randn(Cc, generator=g)
    ga, be = ln_affine(g, Cc)

    def branch(dt):
        h = ln_linear_reference(x, w1, b1, ga, be, None, 1, dt)
        return F.linear(h, w2.to(dt), b2.to(dt))

    b64, b32 = branch(torch.float64), branch(torch.float32)
    dev = [t.cuda() for t in (x, w1, b1, ga, be, w2, b2)]
    out = torch.zeros(M, Cc, device="cuda")
    rc = lib.tango_op_ff_fused(DT[dtype], *[p(t) for t in dev], p(out), M, Cc, H, 1e-5, 0, 0, None, None)
    assert rc == 0, lib.tango_last_error().decode()
    check_rows("ff_fused M=%d" % M, dtype, [("out", out, x.double() + b64, x + b32)])


@pytest.mark.parametrize("dtype", DTYPES[1:])
@pytest.mark.parametrize("single_key", [False, True])
def test_xattn_block_rows_on_offsets(lib, dtype, single_key):
    """norm2 -> attn2 -> + residual in one launch (xattn.hip); `single_key`: sample 0 sees one live text token (the T5("") row)"""
    B, HW, L, C_ = 2, 256, 64, 320
    g = torch.Generator().manual_seed(B * 1000 + HW + L)
    x = ln_rows(g, B * HW, C_, dtype)
    ga, be = ln_affine(g, C_)
    wq = q(torch.randn(C_, C_, generator=g) / C_ ** 0.5, dtype)
    wo = q(torch.randn(C_, C_, generator=g) / C_ ** 0.5, dtype)
    bo = torch.randn(C_, generator=g)
    k = q(torch.randn(B * L, C_, generator=g), dtype)
    v = q(torch.randn(B * L, C_, generator=g), dtype)
    bias = None
    if single_key:
        m = torch.ones(B, L)
        m[0, 1:] = 0
        bias = (1 - m) * -10000.0

    def block(dt):
        c = lambda t: t.to(dt)   # noqa: E731
        xn = F.layer_norm(c(x), (C_,), c(ga), c(be), 1e-5)
        qh = (xn @ c(wq).t()).view(B, HW, 5, 64).transpose(1, 2)
        kh = c(k).view(B, L, 5, 64).transpose(1, 2)
        vh = c(v).view(B, L, 5, 64).transpose(1, 2)
        s = qh @ kh.transpose(-1, -2) * 0.125
        if bias is not None:
            s = s + c(bias)[:, None, None, :]
        a = (s.softmax(-1) @ vh).transpose(1, 2).reshape(B * HW, C_)
        return c(x) + a @ c(wo).t() + c(bo)

    ref, r32 = block(torch.float64), block(torch.float32)
    dev = [t.cuda() if t is not None else None for t in (x, ga, be, wq, k, v, bias, wo, bo)]
    out = torch.zeros(B * HW, C_, device="cuda")
    rc = lib.tango_op_xattn_block(DT[dtype], *[p(t) if t is not None else None for t in dev], p(out), B, HW, L, 1e-5, None)
    assert rc == 0, lib.tango_last_error().decode()
    check_rows("xattn_block B=%d HW=%d L=%d single_key=%s" % (B, HW, L, single_key), dtype, [("out", out, ref, r32)])
