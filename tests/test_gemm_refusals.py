"""What launch_gemm refuses on the host for the epilogue arms only the engine's plan builders set (GemmParams::rowvec / out_lo, ::wb_rows),
asked through tango_debug_linear_ex_check -- the problem tango_op_linear_ex builds, on never-dereferenced aligned pointers, no GPU needed.

Two of these were silent before: rowvec with a null out_lo (wide_epilogue would have stored through a null base) and a wb_rows that is
no multiple of the 256-row tile or does not divide M (a tile would have multiplied rows of two samples with one sample's weights, or read
past the last weight matrix).  They are refused here and never launched: no GPU test passes them to a kernel."""
import ctypes as C
import os

import pytest

from tango_amd import _lib

SWITCHES = ["TANGO_DUO_MAXK", "TANGO_DUO_MIN_TILES", "TANGO_DUO_MASK", "TANGO_WIDE_PERS", "TANGO_NO_WIDE_GEMM", "TANGO_NO_STREAM",
            "TANGO_NO_DMA_GEMM", "TANGO_FORCE_DMA_GEMM", "TANGO_NO_SMALL_TILE"]
WIDE = dict(TANGO_FORCE_DMA_GEMM="1", TANGO_DUO_MAXK="0")
DUO = dict(TANGO_FORCE_DMA_GEMM="1", TANGO_DUO_MAXK="100000", TANGO_DUO_MIN_TILES="1", TANGO_DUO_MASK="15")
FORCED = {"wide": WIDE, "duo": DUO}


@pytest.fixture()
def check():
    """check(env, M, N, K, **arms) -> (plan name, refusal message or "")"""
    lib = _lib.load()
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}

    def ask(env, M, N, K, dtype=1, residual=0, bias2=0, rowvec=0, rowvec_rows=0, rowvec_per=64, out_lo=0, wb_rows=0, pad=0, geglu=0):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        lib.tango_tuning_reload()
        plan = C.create_string_buffer(64)
        why = lib.tango_debug_linear_ex_check(dtype, M, N, K, residual, bias2, rowvec, rowvec_rows, rowvec_per, out_lo, wb_rows, pad, geglu,
                                              plan, 64)
        return plan.value.decode(), why.decode()

    yield ask
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(saved)
    lib.tango_tuning_reload()


@pytest.mark.parametrize("route", ["wide", "duo"])
@pytest.mark.parametrize("dtype", [1, 2])
def test_the_arms_are_accepted_on_their_routes(check, route, dtype):
    """the problems tests/test_gemm_engine_arms_gpu.py launches: accepted, on the route it names"""
    env = FORCED[route]
    for pad in (0, 24):
        assert check(env, 1024, 320, 320, dtype=dtype, residual=1, rowvec=1, rowvec_rows=192, rowvec_per=64, out_lo=1, pad=pad) == (route, "")
    assert check(env, 1024, 320, 320, dtype=dtype, rowvec=1, rowvec_rows=1024, rowvec_per=256, out_lo=1, wb_rows=256) == (route, "")
    assert check(env, 1024, 320, 320, dtype=dtype, rowvec=1, rowvec_rows=1024, rowvec_per=512, out_lo=1, wb_rows=512) == (route, "")
    assert check(env, 1024, 320, 320, dtype=dtype, wb_rows=1024) == (route, "")
    assert check(env, 512, 320, 64, dtype=dtype, bias2=1) == (route, "")


def test_the_persistent_form_takes_per_sample_weights(check):
    for wb in (256, 1024):
        assert check(dict(TANGO_WIDE_PERS="1"), 131072, 320, 64, rowvec=1, rowvec_rows=131072, rowvec_per=wb, out_lo=1, wb_rows=wb) == ("wide+pers", "")


@pytest.mark.parametrize("route", ["wide", "duo"])
def test_rowvec_without_out_lo_is_refused(check, route):
    plan, why = check(FORCED[route], 1024, 320, 320, residual=1, rowvec=1, rowvec_rows=192, rowvec_per=64, out_lo=0)
    assert plan == route and "rowvec" in why and "out_lo" in why, (plan, why)
    # ... also when no row would take it: the epilogue's store base must never be null where rowvec is set
    plan, why = check(FORCED[route], 1024, 320, 320, rowvec=1, rowvec_rows=0, rowvec_per=64, out_lo=0)
    assert "out_lo" in why, (plan, why)


@pytest.mark.parametrize("route", ["wide", "duo"])
def test_rowvec_over_no_rows_stays_legal(check, route):
    assert check(FORCED[route], 1024, 320, 320, residual=1, rowvec=1, rowvec_rows=0, rowvec_per=64, out_lo=1) == (route, "")


@pytest.mark.parametrize("route", ["wide", "duo"])
@pytest.mark.parametrize("arms", [dict(rowvec_rows=96), dict(rowvec_rows=192, rowvec_per=96), dict(rowvec_rows=192, rowvec_per=0),
                                  dict(rowvec_rows=1088), dict(rowvec_rows=-64), dict(rowvec_rows=192, pad=4)])
def test_rowvec_geometry_the_epilogue_cannot_index_is_refused(check, route, arms):
    """a wave's 64 rows lie on one side of rowvec_rows and in one rowvec_per block; rowvec_per = 0 would divide by zero; ldo_lo % 8"""
    a = dict(residual=1, rowvec=1, rowvec_per=64, out_lo=1)
    a.update(arms)
    plan, why = check(FORCED[route], 1024, 320, 320, **a)
    assert "rowvec" in why, (arms, plan, why)


def test_rowvec_off_its_two_kernels_is_refused(check):
    a = dict(rowvec=1, rowvec_rows=192, rowvec_per=64, out_lo=1)
    for env, M, N, K, extra in [({}, 512, 320, 64, {}),                      # the 4-wave tiles
                                ({}, 512, 1280, 1280, {}),                   # split-K
                                (WIDE, 1024, 640, 320, dict(geglu=1))]:      # an epilogue other than the plain one, on the 256 x 320 kernel itself
        plan, why = check(env, M, N, K, **a, **extra)
        assert "rowvec" in why, (plan, why)
    assert check(WIDE, 1024, 640, 320, geglu=1) == ("wide", "")             # (the same problem without rowvec is fine)


@pytest.mark.parametrize("route", ["wide", "duo"])
@pytest.mark.parametrize("wb_rows", [64, 128, 384, 768, 2048, -256])
def test_wb_rows_that_split_a_tile_or_do_not_divide_m_are_refused(check, route, wb_rows):
    """M = 1024: 128 puts two samples into every 256-row tile; 768 and 2048 are tile multiples that do not divide M"""
    plan, why = check(FORCED[route], 1024, 320, 320, wb_rows=wb_rows)
    assert plan == route and "wb_rows" in why, (plan, why)


def test_wb_rows_off_its_two_kernels_is_refused(check):
    plan, why = check({}, 512, 320, 64, wb_rows=256)
    assert plan == "tile" and "per-sample weights" in why, (plan, why)
