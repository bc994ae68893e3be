"""The attention planner's routes (csrc/attention.hip plan_attention), pinned on the UNet's and the text encoder's sites through the host-side
query tango_debug_attention_route -- no GPU needed.  The expectations are what the if-chain this planner replaced launched for the same
arguments (compared once over the full cross product of dtypes, shapes, flags and switches: no difference), so they also pin its
precedences: TANGO_ATTN_DEFER=1 drops the LDS-DMA K tile, TANGO_ATTN_KDMA needs TANGO_ATTN_MSUM, a vt_perm site reads no switch.  A change
that flips one of them changes which kernel a site or an A/B arm runs and should come with its own measurement."""
import os

import pytest

from tango_amd import _lib

SWITCHES = ["TANGO_ATTN_MSUM", "TANGO_ATTN_DEFER", "TANGO_ATTN_KDMA", "TANGO_ATTN_VDMA", "TANGO_ATTN_X8_QB", "TANGO_ATTN_QB2_MIN_WGS"]
F32, F16, BF16 = 0, 1, 2


@pytest.fixture()
def route():
    lib = _lib.load()
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    lib.tango_tuning_reload()

    def ask(B, heads, Sq, Skv, masked=0, pos_bias=0, fp8=0, vt_perm=0, dtype=F16, **env):
        os.environ.update({k: str(v) for k, v in env.items()})
        lib.tango_tuning_reload()
        try:
            return lib.tango_debug_attention_route(dtype, B, heads, Sq, Skv, masked, pos_bias, fp8, vt_perm).decode()
        finally:
            for k in env:
                del os.environ[k]
            lib.tango_tuning_reload()

    yield ask
    os.environ.update(saved)
    lib.tango_tuning_reload()


# (B, heads, Sq, Skv, flags) -> "qb<n>:<form> <grid>": the sites of a B = 32 step (64 samples with CFG; the shared front runs on 32)
SITES = [
    ((32, 5, 4096, 4096, dict(vt_perm=1)), "qb2:msum+kdma+vdma 32x5x32"),   # level-0 self, v^T in fragment order
    ((32, 5, 4096, 4096, {}), "qb2:msum+kdma 32x5x32"),
    ((64, 10, 1024, 1024, dict(vt_perm=1)), "qb2:msum+kdma+vdma 8x10x64"),  # level-1 self
    ((64, 20, 256, 256, {}), "qb2:msum 2x20x64"),                           # level-2 self: 2560 workgroups >= 512 -> 32 rows per wave
    ((2, 20, 256, 256, {}), "qb1:msum 4x20x2"),                             # ... at B = 1: 80 workgroups
    ((64, 20, 64, 64, {}), "qb1:msum 1x20x64"),                             # level 3: 64 is no multiple of 128
    ((32, 10, 1024, 64, dict(masked=1)), "qb2:masked 8x10x32"),             # cross-attention, levels 1 - 3
    ((32, 20, 256, 64, dict(masked=1)), "qb2:masked 2x20x32"),
    ((32, 20, 64, 64, dict(masked=1)), "qb1:masked 1x20x32"),
    ((2, 5, 4096, 72, {}), "qb2:masked 32x5x2"),                            # Skv % 64 != 0 is masked whatever the caller says
    ((2, 5, 256, 72, {}), "qb1:masked 4x5x2"),
    ((2, 12, 77, 77, dict(pos_bias=1, masked=1, dtype=F32)), "qb1:posbias 2x12x2"),    # T5
    ((64, 12, 1024, 1024, dict(pos_bias=1, dtype=F32)), "qb1:posbias 16x12x64"),       # ... never 32 rows per wave
    ((2, 5, 4096, 4096, dict(fp8=1)), "qb2:f8+msum 32x5x2"),
    ((2, 5, 4096, 4096, dict(fp8=1, TANGO_ATTN_MSUM=0)), "qb2:f8 32x5x2"),
    ((2, 5, 4096, 4096, dict(fp8=2)), "qb2:x8 32x5x2"),                     # MX fp8: Sq / 128 blocks
    ((2, 5, 4096, 4096, dict(fp8=2, TANGO_ATTN_X8_QB=1)), "qb1:x8 64x5x2"),  # ... Sq / 64
    ((2, 5, 4096, 4096, dict(fp8=2, TANGO_ATTN_MSUM=0)), "qb2:x8 32x5x2"),  # ... attn_msum is not consulted
    ((2, 5, 192, 128, dict(fp8=2)), "qb1:x8 3x5x2"),                        # Sq % 128 != 0
    ((2, 5, 4096, 4096, dict(dtype=F32)), "qb2:plain 32x5x2"),
    ((2, 5, 4096, 4096, dict(dtype=F32, TANGO_ATTN_DEFER=1)), "qb2:plain 32x5x2"),     # fp32 reads no switch
]
# the A/B arms at Sq = Skv = 4096, and the level-2 site without the short-sequence rule
ARMS = [
    ((2, 5, 4096, 4096, dict(TANGO_ATTN_DEFER=1)), "qb2:msum+defer 32x5x2"),                    # DEFER beats KDMA
    ((2, 5, 4096, 4096, dict(TANGO_ATTN_DEFER=1, vt_perm=1)), "qb2:msum+kdma+vdma 32x5x2"),    # vt_perm ignores the switches
    ((2, 5, 4096, 4096, dict(TANGO_ATTN_MSUM=0, TANGO_ATTN_KDMA=0, vt_perm=1)), "qb2:msum+kdma+vdma 32x5x2"),
    ((2, 5, 4096, 4096, dict(TANGO_ATTN_MSUM=0)), "qb2:plain 32x5x2"),                         # KDMA needs MSUM
    ((2, 5, 4096, 4096, dict(TANGO_ATTN_MSUM=0, TANGO_ATTN_DEFER=1)), "qb2:defer 32x5x2"),
    ((2, 5, 4096, 4096, dict(TANGO_ATTN_KDMA=0)), "qb2:msum 32x5x2"),
    ((64, 20, 256, 256, dict(TANGO_ATTN_QB2_MIN_WGS=0)), "qb1:msum 4x20x64"),
    ((64, 20, 256, 256, dict(TANGO_ATTN_DEFER=1)), "qb2:msum+defer 2x20x64"),
    ((4, 20, 256, 256, dict(TANGO_ATTN_QB2_MIN_WGS=160)), "qb2:msum 2x20x4"),                  # exactly n workgroups
    ((4, 20, 256, 256, dict(TANGO_ATTN_QB2_MIN_WGS=161)), "qb1:msum 4x20x4"),
    ((64, 20, 192, 192, dict(TANGO_ATTN_QB2_MIN_WGS=1)), "qb1:msum 3x20x64"),                  # Sq % 128 != 0
]


@pytest.mark.parametrize("args,want", SITES + ARMS)
def test_attention_route(route, args, want):
    B, heads, Sq, Skv, kw = args
    assert route(B, heads, Sq, Skv, **kw) == want
    if kw.get("dtype", F16) == F16:
        assert route(B, heads, Sq, Skv, **dict(kw, dtype=BF16)) == want      # bf16 takes the same kernels


REFUSALS = [
    (dict(Sq=256, Skv=256, vt_perm=1), "attention: vt_perm needs an unmasked 16-bit site with Sq > 512, Skv % 64 == 0, no fp8 P.V"),
    (dict(Sq=4096, Skv=4096, vt_perm=1, masked=1), "attention: vt_perm needs an unmasked 16-bit site with Sq > 512, Skv % 64 == 0, no fp8 P.V"),
    (dict(Sq=4096, Skv=72, vt_perm=1), "attention: vt_perm needs an unmasked 16-bit site with Sq > 512, Skv % 64 == 0, no fp8 P.V"),
    (dict(Sq=4096, Skv=4096, vt_perm=1, fp8=1), "attention: vt_perm needs an unmasked 16-bit site with Sq > 512, Skv % 64 == 0, no fp8 P.V"),
    (dict(Sq=4096, Skv=4096, vt_perm=1, dtype=F32), "attention: vt_perm needs an unmasked 16-bit site with Sq > 512, Skv % 64 == 0, no fp8 P.V"),
    (dict(Sq=4096, Skv=4096, fp8=1, dtype=F32), "attention: fp8 P.V needs a 16-bit engine (Q.K^T stays in the engine dtype)"),
    (dict(Sq=1024, Skv=64, fp8=1, masked=1), "attention: fp8 P.V is implemented for unmasked sites with Skv % 64 == 0 only"),
    (dict(Sq=1024, Skv=72, fp8=1), "attention: fp8 P.V is implemented for unmasked sites with Skv % 64 == 0 only"),
    (dict(Sq=1024, Skv=1024, fp8=2, pos_bias=1), "attention: fp8 P.V is implemented for unmasked sites with Skv % 64 == 0 only"),
    (dict(Sq=192, Skv=192, fp8=2), "attention: MX fp8 P.V (128 keys per MFMA) needs Skv % 128 == 0"),
    (dict(Sq=64, Skv=64, dtype=3), "attention: bad dtype"),
]


@pytest.mark.parametrize("kw,why", REFUSALS)
def test_attention_refusal(route, kw, why):
    """what launch_attention refuses, with the message it fails with (the ld-alignment refusal is asked through
    tango_debug_attention_route_ld below: this query builds the op wrapper's dense, aligned rows)"""
    assert route(2, 5, **kw) == why


def dense_ld(heads, Skv):
    C_ = heads * 64
    return dict(ldq=C_, ldk=C_, ldvt=(Skv + 7) // 8 * 8, ldo=C_)


@pytest.fixture()
def route_ld(route):
    """tango_debug_attention_route_ld under the `route` fixture's clean switches: pitches by keyword, dense where not given"""
    lib = _lib.load()

    def ask(B, heads, Sq, Skv, masked=0, pos_bias=0, fp8=0, vt_perm=0, dtype=F16, ldq=None, ldk=None, ldvt=None, ldo=None, **env):
        d = dense_ld(heads, Skv)
        ld = [d[n] if v is None else v for n, v in (("ldq", ldq), ("ldk", ldk), ("ldvt", ldvt), ("ldo", ldo))]
        os.environ.update({k: str(v) for k, v in env.items()})
        lib.tango_tuning_reload()
        try:
            return lib.tango_debug_attention_route_ld(dtype, B, heads, Sq, Skv, masked, pos_bias, fp8, vt_perm, *ld).decode()
        finally:
            for k in env:
                del os.environ[k]
            lib.tango_tuning_reload()

    return ask


# q, k and v^T rows are read in 16-byte pieces, output rows stored in 8-byte ones: the smallest step off the dense pitch that breaks that,
# and next to each the smallest one that keeps it (which must plan like the dense rows)
LD_REFUSED = [
    (F16, dict(ldq=321)), (F16, dict(ldq=324)), (F16, dict(ldk=321)), (F16, dict(ldk=324)), (F16, dict(ldvt=260)), (F16, dict(ldo=321)), (F16, dict(ldo=322)),
    (BF16, dict(ldq=321)), (BF16, dict(ldk=324)), (BF16, dict(ldvt=257)), (BF16, dict(ldo=322)),
    (F32, dict(ldq=321)), (F32, dict(ldq=322)), (F32, dict(ldk=322)), (F32, dict(ldvt=258)), (F32, dict(ldo=321)),
]
LD_ACCEPTED = [
    (F16, dict(ldq=328)), (F16, dict(ldk=328)), (F16, dict(ldvt=264)), (F16, dict(ldo=324)), (BF16, dict(ldo=324)), (BF16, dict(ldvt=264)),
    (F32, dict(ldq=324)), (F32, dict(ldk=324)), (F32, dict(ldvt=260)), (F32, dict(ldo=322)),
]


@pytest.mark.parametrize("dtype,ld", LD_REFUSED)
def test_attention_ld_alignment_refusal(route_ld, dtype, ld):
    assert route_ld(2, 5, 256, 256, dtype=dtype, **ld) == "attention: ld alignment"
    assert route_ld(2, 5, 256, 72, masked=1, dtype=dtype, **dict(ld, ldvt=ld.get("ldvt", 72))) == "attention: ld alignment"


@pytest.mark.parametrize("dtype,ld", LD_ACCEPTED)
def test_attention_ld_alignment_accepted(route, route_ld, dtype, ld):
    assert route_ld(2, 5, 256, 256, dtype=dtype, **ld) == route(2, 5, 256, 256, dtype=dtype)


def test_attention_vt_perm_with_odd_ldvt(route_ld):
    """a fragment-order V^T whose pitch is no multiple of 8 is never planned.  The planner's vt_perm rule names ldvt % 8 itself; for the
    16-bit types, the only ones that read a vt_perm V^T, the 16-byte rule for rows says the same thing first"""
    perm = "attention: vt_perm needs an unmasked 16-bit site with Sq > 512, Skv % 64 == 0, no fp8 P.V"
    assert route_ld(2, 5, 4096, 4096, vt_perm=1, dtype=F32, ldvt=4100) == perm      # 16-byte rows in fp32, 4100 % 8 != 0
    for dtype in (F16, BF16):
        assert route_ld(2, 5, 4096, 4096, vt_perm=1, dtype=dtype, ldvt=4100) == "attention: ld alignment"
        assert route_ld(2, 5, 4096, 4096, vt_perm=1, dtype=dtype, ldvt=4104) == "qb2:msum+kdma+vdma 32x5x2"


@pytest.mark.parametrize("args,want", SITES + ARMS)
def test_attention_route_with_engine_pitches(route, route_ld, args, want):
    """the engine hands the kernel q | k slices of one buffer of pitch 2C (self-attention, text encoder) or q from that buffer and the hoisted
    k at pitch C (cross-attention): the same kernel and grid as on dense rows -- the planner reads pitches for alignment only"""
    B, heads, Sq, Skv, kw = args
    C_ = heads * 64
    cross = Sq != Skv
    dtypes = (F16, BF16) if kw.get("dtype", F16) == F16 else (kw["dtype"],)
    for dtype in dtypes:
        k = dict(kw, dtype=dtype)
        dense = route(B, heads, Sq, Skv, **k)
        assert dense == want
        assert route_ld(B, heads, Sq, Skv, ldq=2 * C_, ldk=C_ if cross else 2 * C_, **k) == dense
        assert route_ld(B, heads, Sq, Skv, ldq=2 * C_, ldk=C_ if cross else 2 * C_, ldvt=(Skv + 7) // 8 * 8 + 8, ldo=C_ + 8, **k) == dense
        assert route_ld(B, heads, Sq, Skv, **k) == dense                             # dense pitches spelled out


def test_attention_view_hook_refuses_before_any_gpu_call():
    """tango_op_attention_view answers each of its refusals (the rows of tests/test_attention_layouts_gpu.py) from its host checker before it
    allocates or launches anything: the same messages on a machine without a GPU, from pointers that are never dereferenced"""
    import ctypes as C

    from test_attention_layouts_gpu import call_refused, view_refusals
    lib = _lib.load()
    B, heads, S = 1, 2, 64
    ptrs = tuple(C.c_void_p(0x10000 * (i + 1)) for i in range(6))
    rows = view_refusals(heads * 64, S)
    assert len(rows) >= 25
    for dtype, over, part in rows:
        rc, msg = call_refused(lib, dtype, over, ptrs, B, heads, S)
        assert rc != 0 and part in msg, (dtype, over, msg)
