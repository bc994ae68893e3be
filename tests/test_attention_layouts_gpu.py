"""attn_kernel on the memory layouts its callers hand it, through the test hook tango_op_attention_view (csrc/ops_abi.hip).

tango_op_attention[_ex] always builds dense q, k and o rows (pitch heads * 64), ldvt = round8(Skv), zeroed V^T pads, no position bias and a
key bias that is 0 or -10000.  No caller in the product does: Builder::transformer reads q | k as slices of one buffer of pitch 2C, the
unfused cross-attention q from that buffer and the hoisted k at pitch C, build_t5 the same slicing with scale 1 and a [heads][L][L]
position bias.  This file runs

  (a) every kernel form in those layouts (L1 self, L2 cross), in a contract layout with odd pitches (L3) and with an output row that is
      8- but not 16-byte aligned (L4, the direct-store branch of the masked form): bit for bit the dense result, every element of the
      output buffer outside the result still the pad value;
  (b) the masked forms with a key bias that is neither 0 nor -10000 (the kernel scales it by log2 e);
  (c) the position-bias form as the text encoder calls it;
  (d) the hook's own refusals.

V of head h is scaled by 16^-h and the error is taken per (sample, head) block against that block's own maximum, so that a wrong offset
for one quiet head cannot hide behind a loud one.  Bounds per block: test_ops_gpu.TOL (each block is an attention problem with the
statistics of the cases there).  References are fp64 on the rounded operands.  Pads hold -7.0 (exact in every type), never NaN or Inf:
the V^T contract is "zero / finite" and the hook refuses anything else."""
import ctypes as C
import functools

import pytest
import torch

from test_duo_gpu import tuning
from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

DT = {"fp32": 0, "fp16": 1, "bf16": 2}
PAD = -7.0
F8_TOL = 8e-2          # of the global maximum, as test_attention_fp8_gpu.py
# every attention switch the planner reads, at its default: a case states what it changes
BASE_ENV = dict(TANGO_ATTN_MSUM=1, TANGO_ATTN_DEFER=0, TANGO_ATTN_KDMA=1, TANGO_ATTN_X8_QB=2, TANGO_ATTN_QB2_MIN_WGS=512)


def quant(t, dtype):
    return t.half().float() if dtype == "fp16" else t.bfloat16().float() if dtype == "bf16" else t


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def r8(n):
    return (n + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def operands(B, heads, Sq, Skv, dtype, seed=0):
    """q, k: randn; v: 1.5 randn + 0.3 with head h scaled by 16^-h; all rounded to the storage type (fp32 tensors holding those values)"""
    assert heads <= 3
    g = torch.Generator().manual_seed(1000 * Sq + 10 * Skv + heads + seed)
    C_ = heads * 64
    q = torch.randn(B, Sq, C_, generator=g)
    k = torch.randn(B, Skv, C_, generator=g)
    v = (torch.randn(B, Skv, C_, generator=g) * 1.5 + 0.3).view(B, Skv, heads, 64)
    v = v * (16.0 ** -torch.arange(heads, dtype=torch.float32)).view(1, 1, heads, 1)
    return quant(q, dtype), quant(k, dtype), quant(v.reshape(B, Skv, C_), dtype)


def ref64(q, k, v, heads, scale, bias=None, pos_bias=None):
    """fp64 softmax(q k^T scale + bias[b, kv] + pos_bias[h, q, kv]) v on [B, S, heads * 64] operands -> [B, Sq, heads * 64] fp64"""
    B, Sq, C_ = q.shape
    Skv = k.shape[1]
    qh, kh, vh = (t.double().view(B, -1, heads, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias.double().view(B, 1, 1, Skv)
    if pos_bias is not None:
        s = s + pos_bias.double().view(1, heads, Sq, Skv)
    return (s.softmax(-1) @ vh).transpose(1, 2).reshape(B, Sq, C_)


def block_diff(a, b, heads):
    """per (sample, head) block: max |a - b| over the block / max |b| of that block -> [B, heads]"""
    B, Sq, _ = b.shape
    d = (a.double() - b.double()).abs().view(B, Sq, heads, 64).amax(dim=(1, 3))
    m = b.double().abs().view(B, Sq, heads, 64).amax(dim=(1, 3))
    assert (m > 0).all()
    return d / m


def assert_blocks(what, out, ref, heads, dtype):
    e = block_diff(out, ref, heads)
    print("%s %s: per-block error vs fp64 max %.3e min %.3e (bound %.1e)" % (what, dtype, e.max().item(), e.min().item(), TOL[dtype]))
    assert torch.isfinite(out).all()
    assert e.max().item() <= TOL[dtype], (what, dtype, e)


def assert_moves(what, other, ref, heads):
    """a perturbed REFERENCE differs from the reference by at least 10 % of every block's own maximum: the test can see the perturbation"""
    e = block_diff(other, ref, heads)
    assert e.min().item() >= 0.10, (what, e)


def layout(name, dtype, heads, Sq, Skv):
    C_ = heads * 64
    f32 = dtype == "fp32"
    if name == "L1":      # Builder::transformer self-attention, build_t5: q | k slices of one buffer
        assert Sq == Skv
        return dict(ldq=2 * C_, ldk=2 * C_, k_col0=C_, ldvt=r8(Skv), ldo=C_, o_col0=0)
    if name == "L2":      # unfused cross-attention: q from the q | k buffer, the hoisted k
        return dict(ldq=2 * C_, ldk=C_, k_col0=-1, ldvt=r8(Skv), ldo=C_, o_col0=0)
    if name == "L3":      # what AttnParams allows: every pitch its own, 16-byte rows
        return (dict(ldq=C_ + 4, ldk=C_ + 12, k_col0=-1, ldvt=r8(Skv) + 4, ldo=C_ + 4, o_col0=0) if f32 else
                dict(ldq=C_ + 8, ldk=C_ + 24, k_col0=-1, ldvt=r8(Skv) + 8, ldo=C_ + 8, o_col0=0))
    if name == "L4":      # L2 with output rows that are 8- but not 16-byte aligned
        return dict(ldq=2 * C_, ldk=C_, k_col0=-1, ldvt=r8(Skv), ldo=C_ + (2 if f32 else 4), o_col0=2 if f32 else 4)
    raise KeyError(name)


def route_ld(lib, dtype, B, heads, Sq, Skv, masked, pos_bias, flags, lay):
    fp8 = 2 if flags & 2 else flags & 1
    return lib.tango_debug_attention_route_ld(DT[dtype], B, heads, Sq, Skv, int(masked), int(pos_bias), fp8, 1 if flags & 4 else 0,
                                              lay["ldq"], lay["ldk"], lay["ldvt"], lay["ldo"]).decode()


def run_dense(lib, dtype, q, k, v, bias, heads, scale, flags):
    B, Sq, C_ = q.shape
    out = torch.empty(B, Sq, C_, device="cuda")
    dev = [t.cuda() if t is not None else None for t in (q, k, v, bias)]
    rc = lib.tango_op_attention_ex(DT[dtype], p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(out), B, heads, Sq, k.shape[1], scale, flags, None)
    assert rc == 0, lib.tango_last_error().decode()
    return out.cpu()


def run_view(lib, dtype, q, k, v, bias, pos_bias, heads, scale, flags, lay):
    """-> (result [B, Sq, C], mask of the result's columns [ldo], the whole output buffer [B*Sq, ldo])"""
    B, Sq, C_ = q.shape
    Skv = k.shape[1]
    buf = torch.full((B * Sq, lay["ldo"]), 123.0, device="cuda")
    dev = [t.contiguous().cuda() if t is not None else None for t in (q, k, v, bias, pos_bias)]
    rc = lib.tango_op_attention_view(DT[dtype], p(dev[0]), p(dev[1]), p(dev[2]), p(dev[3]), p(dev[4]), p(buf), B, heads, Sq, Skv, scale, flags,
                                     lay["ldq"], lay["ldk"], lay["k_col0"], lay["ldvt"], lay["ldo"], lay["o_col0"], PAD, None)
    assert rc == 0, lib.tango_last_error().decode()
    buf = buf.cpu()
    cols = torch.zeros(lay["ldo"], dtype=torch.bool)
    cols[lay["o_col0"]:lay["o_col0"] + C_] = True
    return buf[:, cols].reshape(B, Sq, C_), cols, buf


def perm_rows(v):
    """the rows of v in the kernel's fragment order inside every block of 32 keys: row vt_perm_pos(s) holds key s (flags bit 2)"""
    s = torch.arange(v.shape[1])
    pos = (s & ~31) | ((s & 12) << 1) | ((s & 16) >> 2) | (s & 3)
    vp = torch.empty_like(v)
    vp[:, pos] = v
    return vp


def mask_bias(B, Skv):
    """the -10000 key mask of test_ops_gpu.test_attention: sample 0 keeps one key, sample 1 the first half"""
    m = torch.ones(B, Skv)
    m[0, 1:] = 0
    if B > 1:
        m[1, Skv // 2:] = 0
    return (1 - m) * -10000.0


def finite_bias(B, Skv, seed):
    g = torch.Generator().manual_seed(77 + seed)
    return -8.0 * torch.rand(B, Skv, generator=g)


# ---- (a) ----
H16 = ("fp16", "bf16")
ALL = ("fp32", "fp16", "bf16")
# name -> (route, (B, heads, Sq, Skv), switches, flags, dtypes, -10000 mask)
FORMS = {
    "msum_qb1": ("qb1:msum", (2, 3, 256, 256), {}, 0, H16, False),
    "msum_qb2": ("qb2:msum", (2, 3, 128, 128), dict(TANGO_ATTN_QB2_MIN_WGS=1), 0, H16, False),
    "kdma": ("qb2:msum+kdma", (1, 2, 576, 576), {}, 0, H16, False),
    "kvdma": ("qb2:msum+kdma+vdma", (1, 2, 576, 576), {}, 4, H16, False),
    "msum_defer": ("qb1:msum+defer", (2, 3, 256, 256), dict(TANGO_ATTN_DEFER=1), 0, H16, False),
    "defer": ("qb1:defer", (2, 3, 256, 256), dict(TANGO_ATTN_MSUM=0, TANGO_ATTN_DEFER=1), 0, H16, False),
    "plain16": ("qb1:plain", (2, 3, 256, 256), dict(TANGO_ATTN_MSUM=0), 0, H16, False),
    "plain32_qb1": ("qb1:plain", (2, 2, 64, 64), {}, 0, ("fp32",), False),
    "plain32_qb2": ("qb2:plain", (1, 2, 576, 576), {}, 0, ("fp32",), False),
    "f8": ("qb1:f8", (2, 2, 256, 256), dict(TANGO_ATTN_MSUM=0), 1, H16, False),
    "f8_msum": ("qb1:f8+msum", (2, 2, 256, 256), {}, 1, H16, False),
    "x8_qb2": ("qb2:x8", (2, 2, 256, 256), dict(TANGO_ATTN_X8_QB=2), 3, H16, False),
    "x8_qb1": ("qb1:x8", (2, 2, 256, 256), dict(TANGO_ATTN_X8_QB=1), 3, H16, False),
    "masked_200x7": ("qb1:masked", (3, 1, 200, 7), {}, 0, ALL, True),
    "masked_130": ("qb1:masked", (1, 3, 130, 130), {}, 0, ALL, False),
    "masked_256x64": ("qb1:masked", (2, 2, 256, 64), {}, 0, ALL, True),
    "masked_qb2": ("qb2:masked", (2, 2, 128, 64), dict(TANGO_ATTN_QB2_MIN_WGS=1), 0, ALL, True),
}
MASKED_FORMS = [n for n in FORMS if n.startswith("masked")]
LAYOUT_CASES = [(n, d, l) for n, f in FORMS.items() for d in f[4] for l in ("L1", "L2", "L3", "L4") if l != "L1" or f[1][2] == f[1][3]]

_DENSE = {}


def dense_case(lib, name, dtype):
    """operands, -10000 mask or None, the dense op's result and the fp64 reference of a form: computed once per (form, dtype)"""
    if (name, dtype) not in _DENSE:
        route, (B, heads, Sq, Skv), env, flags, _, masked = FORMS[name]
        q, k, v = operands(B, heads, Sq, Skv, dtype)
        bias = mask_bias(B, Skv) if masked else None
        vin = perm_rows(v) if flags & 4 else v
        with tuning(lib, **dict(BASE_ENV, **env)):
            dense = run_dense(lib, dtype, q, k, vin, bias, heads, 0.125, flags)
        _DENSE[(name, dtype)] = (q, k, v, vin, bias, dense, ref64(q, k, v, heads, 0.125, bias))
    return _DENSE[(name, dtype)]


@pytest.mark.parametrize("name,dtype,lname", LAYOUT_CASES)
def test_layout_changes_no_bit(lib, name, dtype, lname):
    route, (B, heads, Sq, Skv), env, flags, _, masked = FORMS[name]
    lay = layout(lname, dtype, heads, Sq, Skv)
    dense_lay = dict(ldq=heads * 64, ldk=heads * 64, ldvt=r8(Skv), ldo=heads * 64)
    with tuning(lib, **dict(BASE_ENV, **env)):
        # the named kernel is the one both runs launch
        assert route_ld(lib, dtype, B, heads, Sq, Skv, masked, False, flags, dense_lay).split()[0] == route
        assert route_ld(lib, dtype, B, heads, Sq, Skv, masked, False, flags, lay).split()[0] == route
        q, k, v, vin, bias, dense, ref = dense_case(lib, name, dtype)
        out, cols, buf = run_view(lib, dtype, q, k, vin, bias, None, heads, 0.125, flags, lay)
    assert torch.equal(out, dense), "layout %s: max |diff| %.3e" % (lname, (out - dense).abs().max().item())
    assert (buf[:, ~cols] == PAD).all(), "layout %s: the kernel wrote outside its result columns" % lname
    if lname in ("L1", "L2"):
        if flags & 1:
            e = ((out.double() - ref).abs().max() / ref.abs().max()).item()
            print("%s %s %s: fp8 P.V error vs fp64 %.3e of the global maximum (bound %.1e)" % (name, lname, dtype, e, F8_TOL))
            assert torch.isfinite(out).all() and e <= F8_TOL, e
        else:
            assert_blocks("%s %s" % (name, lname), out, ref, heads, dtype)


# ---- (b) ----
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("name", MASKED_FORMS)
def test_finite_key_bias(lib, name, dtype):
    """an additive key bias uniform in [-8, 0] per (sample, key), at L2: the kernel's bias * log2(e), and the bias row of the right sample"""
    route, (B, heads, Sq, Skv), env, flags, _, _ = FORMS[name]
    q, k, v = operands(B, heads, Sq, Skv, dtype)
    bias = finite_bias(B, Skv, Sq + Skv)
    ref = ref64(q, k, v, heads, 0.125, bias)
    # on the reference alone: this bias matters, in each way the kernel could get it wrong
    assert_moves("bias * ln 2", ref64(q, k, v, heads, 0.125, bias * 0.6931471805599453), ref, heads)
    assert_moves("bias dropped", ref64(q, k, v, heads, 0.125, None), ref, heads)
    if B > 1:
        assert_moves("the other sample's bias", ref64(q, k, v, heads, 0.125, bias.roll(1, 0)), ref, heads)
    lay = layout("L2", dtype, heads, Sq, Skv)
    with tuning(lib, **dict(BASE_ENV, **env)):
        assert route_ld(lib, dtype, B, heads, Sq, Skv, True, False, 0, lay).split()[0] == route
        out, cols, buf = run_view(lib, dtype, q, k, v, bias, None, heads, 0.125, 0, lay)
    assert (buf[:, ~cols] == PAD).all()
    assert_blocks("%s finite bias" % name, out, ref, heads, dtype)


# ---- (c) ----
@pytest.mark.parametrize("dtype", ALL)
@pytest.mark.parametrize("key_bias", ["ragged_mask", "finite"])
@pytest.mark.parametrize("B,heads,S", [(2, 2, 37), (1, 3, 64), (2, 2, 130), (1, 2, 200)])
def test_position_bias_as_the_text_encoder_calls_it(lib, B, heads, S, key_bias, dtype):
    """build_t5's call: q | k slices of one buffer of pitch 2 * inner (L1), scale 1 (q carries the 1/8 here so the logits stay O(1)), a
    [heads][S][S] position bias shared by the batch, a key bias per sample.  Tails in the query and the key direction (37, 130, 200),
    exactly one tile (64), several tiles."""
    q, k, v = operands(B, heads, S, S, dtype, seed=3)
    q = quant(q * 0.125, dtype)                          # exact: a power of two
    g = torch.Generator().manual_seed(S + heads)
    pb = torch.randn(heads, S, S, generator=g)
    if key_bias == "ragged_mask":
        bias = torch.zeros(B, S)
        bias[B - 1, S - S // 3:] = -10000.0               # the last sample (sample 1 of a batch of two) is shorter
    else:
        bias = finite_bias(B, S, S)
    ref = ref64(q, k, v, heads, 1.0, bias, pb)
    assert_moves("table dropped", ref64(q, k, v, heads, 1.0, bias, None), ref, heads)
    assert_moves("table transposed", ref64(q, k, v, heads, 1.0, bias, pb.transpose(1, 2)), ref, heads)
    assert_moves("the next head's table", ref64(q, k, v, heads, 1.0, bias, pb.roll(-1, 0)), ref, heads)
    lay = layout("L1", dtype, heads, S, S)
    with tuning(lib, **BASE_ENV):
        assert route_ld(lib, dtype, B, heads, S, S, True, True, 0, lay).split()[0] == "qb1:posbias"
        out, cols, buf = run_view(lib, dtype, q, k, v, bias, pb, heads, 1.0, 0, lay)
    assert cols.all()
    assert_blocks("posbias B=%d heads=%d S=%d %s" % (B, heads, S, key_bias), out, ref, heads, dtype)


def test_position_bias_with_fp8_is_refused(lib):
    B, heads, S = 1, 2, 128
    q, k, v = (t.cuda() for t in operands(B, heads, S, S, "fp16"))
    pb = torch.zeros(heads, S, S, device="cuda")
    lay = layout("L1", "fp16", heads, S, S)
    for flags in (1, 3):
        assert "fp8" in route_ld(lib, "fp16", B, heads, S, S, False, True, flags, lay)          # the planner's own refusal
        buf = torch.full((B * S, lay["ldo"]), 123.0, device="cuda")
        rc = lib.tango_op_attention_view(1, p(q), p(k), p(v), None, p(pb), p(buf), B, heads, S, S, 1.0, flags, lay["ldq"], lay["ldk"], lay["k_col0"],
                                         lay["ldvt"], lay["ldo"], lay["o_col0"], PAD, None)
        assert rc != 0 and "pos_bias with an fp8" in lib.tango_last_error().decode()
        assert (buf == 123.0).all()


# ---- (d) ----
def view_refusals(C_, S):
    """(dtype, overrides of a good L3-like call, part of the message): every refusal of tango_op_attention_view that guards a buffer"""
    nan, inf = float("nan"), float("inf")
    return [
        ("fp16", dict(pad=nan), "pad_value must be finite"), ("fp32", dict(pad=inf), "pad_value must be finite"), ("bf16", dict(pad=-inf), "pad_value must be finite"),
        ("fp16", dict(ldq=C_ - 8), "at least heads * 64"), ("fp16", dict(ldk=C_ - 8), "at least heads * 64"), ("fp32", dict(ldo=C_ - 2), "at least heads * 64"),
        ("fp16", dict(ldq=2 * C_, ldk=2 * C_, k_col0=C_ + 8), "exceeds ldq"),
        ("fp16", dict(ldq=2 * C_, ldk=2 * C_, k_col0=C_ - 8), "inside the columns of q"),
        ("fp16", dict(ldq=2 * C_, ldk=C_, k_col0=C_), "needs Sq == Skv and ldk == ldq"),
        ("bf16", dict(ldo=C_ + 8, o_col0=16), "exceeds ldo"), ("fp32", dict(o_col0=-4), "o_col0 is negative"),
        ("fp16", dict(ldvt=r8(S) - 8), "at least round8(Skv)"), ("fp32", dict(ldvt=r8(S) - 4), "at least round8(Skv)"),
        ("fp16", dict(ldq=2 * C_ + 8, ldk=2 * C_ + 8, k_col0=C_ + 4), "16-byte aligned"),      # 8 bytes into a 16-byte piece
        ("fp32", dict(ldq=2 * C_ + 4, ldk=2 * C_ + 4, k_col0=C_ + 2), "16-byte aligned"),
        ("fp16", dict(ldo=C_ + 4, o_col0=2), "8-byte aligned"), ("bf16", dict(ldo=C_ + 4, o_col0=1), "8-byte aligned"),
        ("fp32", dict(ldo=C_ + 2, o_col0=1), "8-byte aligned"),
        ("fp16", dict(ldq=C_ + 4), "ld alignment"), ("fp32", dict(ldvt=r8(S) + 2), "ld alignment"), ("fp16", dict(ldo=C_ + 2), "ld alignment"),
        ("fp16", dict(ldk=1 << 20), "beyond 65536"),
        ("fp16", dict(flags=1, pos_bias=True), "pos_bias with an fp8"), ("bf16", dict(flags=3, pos_bias=True), "pos_bias with an fp8"),
        ("fp16", dict(flags=1, bias=True), "unmasked problems"), ("fp16", dict(flags=2), "rides on"), ("fp16", dict(flags=8), "unknown flags"),
    ]


def call_refused(lib, dtype, over, ptrs, B, heads, S):
    """one refused call of the hook; ptrs: (q, k, v, bias, pos_bias, out) as addresses"""
    C_ = heads * 64
    a = dict(ldq=C_ + 8, ldk=C_ + 8, k_col0=-1, ldvt=r8(S) + 8, ldo=C_ + 8, o_col0=0, pad=PAD, flags=0, bias=False, pos_bias=False)
    a.update(over)
    q, k, v, bias, pb, out = ptrs
    rc = lib.tango_op_attention_view(DT[dtype], q, k, v, bias if a["bias"] else None, pb if a["pos_bias"] else None, out, B, heads, S, S, 0.125, a["flags"],
                                     a["ldq"], a["ldk"], a["k_col0"], a["ldvt"], a["ldo"], a["o_col0"], a["pad"], None)
    return rc, lib.tango_last_error().decode()


def test_view_hook_refusals(lib):
    """everything that could take the kernel outside the staged buffers is refused with its message, and nothing is launched: the output
    buffer keeps its fill"""
    B, heads, S = 1, 2, 64
    C_ = heads * 64
    x = torch.randn(B, S, C_, device="cuda")
    bias = torch.zeros(B, S, device="cuda")
    pb = torch.zeros(heads, S, S, device="cuda")
    out = torch.full((B * S, 4 * C_), 123.0, device="cuda")
    ptrs = (p(x), p(x), p(x), p(bias), p(pb), p(out))
    rc, _ = call_refused(lib, "fp16", {}, ptrs, B, heads, S)
    assert rc == 0, lib.tango_last_error().decode()          # the call every row below changes in one place is a good one
    out.fill_(123.0)
    for dtype, over, part in view_refusals(C_, S):
        rc, msg = call_refused(lib, dtype, over, ptrs, B, heads, S)
        assert rc != 0 and part in msg, (dtype, over, msg)
    assert (out == 123.0).all()
    rc = lib.tango_op_attention_view(1, None, p(x), p(x), None, None, p(out), B, heads, S, S, 0.125, 0, C_, C_, -1, S, C_, 0, PAD, None)
    assert rc != 0 and "required" in lib.tango_last_error().decode()
