"""Which kernel takes the gather-GEMM problems that only the mel-VAE and HiFi-GAN plans (and the large-batch UNet downsampler) pose:
the shapes of tests/test_vae_voc_ops_gpu.py, pinned through the host-side queries tango_debug_conv2d_route / tango_debug_conv1d_route
-- no GPU needed.  The queries, the tango_op_* wrappers and the engine's plan builders build their GemmParams with the same constructors
(csrc/problem.h) and take split-K, route and phase form from the same planner (csrc/gemm.hip plan_gemm / plan_conv3x3), so the answer is
the wrapper's route and the plan's; the GPU tests assert the same table again, under the same switches, before they run a case.

Why these shapes (csrc/gemm_dma.hip gemm_dma_ok, csrc/gemm.hip gemm_pick_splitk):
  * gemm_dma_kernel takes convs from 448 tiles of 256 rows on, or any number under TANGO_FORCE_DMA_GEMM=1; it is the only 8-wave kernel
    for stride 2, pad 0 and every conv1d.  The wrappers' split-K policy looks at 128-row tiles first: a conv2d with fewer than 400 of
    them is split (in practice: fewer than 342) and goes to the 4-wave tile kernel, so the DMA cases carry >= 400 tiles of 128 x (160 | 128).
  * conv1d / transposed-conv phases are never split, and a leaky-ReLU prologue (a_act) keeps a problem off the DMA kernel."""
import ctypes as C
import os

import pytest

from tango_amd import _lib
from test_duo_gpu import tuning
from test_routing import SWITCHES

DT = {"fp32": 0, "fp16": 1, "bf16": 2}
FORCED = dict(TANGO_FORCE_DMA_GEMM=1)
UNFORCED = {}


def conv2d_route(lib, dtype, B, Cin, H, W, Cout, stride, pad=1, residual=0, e_act=0, out_f32=0, ups=0):
    sk = C.c_int(0)
    name = lib.tango_debug_conv2d_route(DT[dtype], B, Cin, H, W, Cout, stride, ups, pad, residual, e_act, out_f32, C.byref(sk))
    return name.decode(), sk.value


def conv1d_route(lib, dtype, B, Cin, L, Cout, k, d, a_act=0, residual=0, e_act=0):
    """the problem tango_op_conv1d(k, dilation d) poses"""
    sk = C.c_int(0)
    name = lib.tango_debug_conv1d_route(DT[dtype], B, Cin, L, Cout, k, d, -d * (k - 1) // 2, L, 1, 0, a_act, residual, e_act, C.byref(sk))
    return name.decode(), sk.value


def convt_phase_routes(lib, dtype, B, Cin, L, Cout, k, u, a_act=0):
    """(taps, rows per batch item, route, split-K) of every phase tango_op_conv_transpose1d(k, stride u, padding (k - u) / 2) launches"""
    out = []
    for r in range(u):
        g = (C.c_int * 6)()
        if not lib.tango_debug_conv_transpose1d_phase(B, Cin, L, Cout, k, u, (k - u) // 2, r, g):
            continue
        taps, tap_step, in_off, rows_pb, out_mul, out_off = list(g)
        sk = C.c_int(0)
        name = lib.tango_debug_conv1d_route(DT[dtype], B, Cin, L, Cout, taps, tap_step, in_off, rows_pb, out_mul, out_off, a_act, 0, 0, C.byref(sk))
        out.append((taps, rows_pb, name.decode(), sk.value))
    return out


# ---- a. stride-2 convs on gemm_dma_kernel<MODE_CONV2D> (forced): (B, Cin, H, W, Cout, pad, residual) ----
DMA_CONV2D = [
    (8, 64, 128, 64, 640, 0, 0),      # the VAE Downsample: even dims, the last tap row / column falls off the image; 512 tiles of 128 x 160
    (8, 64, 128, 64, 640, 1, 0),      # the UNet downsampler's padding on the same grid
    (7, 64, 130, 70, 640, 1, 0),      # Ho x Wo = 65 x 35, M = 15925: ragged last tile, tile rows straddle images; 500 tiles
    (8, 64, 160, 160, 128, 0, 1),     # BN = 128 instantiation with a residual; M = 51200 = 400 tiles of 128 x 128
    (8, 64, 160, 160, 128, 1, 1),
]

# ---- b. the 4-wave tile kernel with both paddings at tiny shapes, stride 2, B = 3, Cin = 64: (Cout, H, W) ----
TILE_PAD = [(Cout, H, W) for Cout in (96, 32, 30) for (H, W) in ((16, 8), (4, 2), (2, 2))]


def tile_pad_expect(dtype, Cout):
    """one tile of 128 (or 256) rows: the split-K policy splits K = 576 into chunks of 128 bytes, at least three per split -- 18 / 3 splits in fp32,
    9 / 3 in 16 bits.  N = 30 is no multiple of 4: never split (the reduce kernel stores four columns at a time)"""
    if Cout % 4:
        return "tile", 1
    return "tile+splitk", (6 if dtype == "fp32" else 3)


# ---- c. conv1d on gemm_dma_kernel<MODE_CONV1D> (forced): (Cin, Cout, L, k, d, residual, e_act) ----
DMA_CONV1D = [
    (64, 128, 301, 7, 1, 1, 0),       # HiFi-GAN resblock c2: residual, no activation
    (64, 160, 301, 7, 3, 0, 2),       # dilation 3, leaky-ReLU epilogue, BN = 160
    (64, 160, 301, 11, 5, 1, 2),      # k = 11, d = 5: 25 rows of padding on each side
    (64, 128, 40, 11, 5, 1, 2),       # L shorter than the dilated span (51): the outer taps never hit the signal
    (64, 160, 40, 7, 1, 0, 0),
    (128, 128, 513, 11, 3, 1, 0),     # M = 1026: five 256-row tiles, two rows in the last, the batch boundary inside the third
]
DMA_CONV1D_FP32 = [(32, 128, 301, 7, 3, 1, 2)]      # Cin = 32 is a whole 128-byte chunk only in fp32

# ---- d. transposed-conv phases on gemm_dma_kernel<MODE_CONV1D> (forced), Cin = Cout = 128: (k, u) x L ----
DMA_CONVT = [(k, u, L) for (k, u) in ((16, 5), (16, 4), (8, 2), (4, 2)) for L in (53, 31)]

# ---- h. the VAE's conv_out (Cin 128 -> 1 channel, fp32 output with ldo = 1): (B, H, W) ----
CONV_OUT_BIG = (4, 256, 64)           # 256 tiles of 256 rows: the halo kernel's 256 x 32 tile, unforced, in 16 bits
CONV_OUT_SMALL = (3, 10, 6)           # M = 180: the 256 x 16 tile kernel


@pytest.fixture()
def lib():
    lib = _lib.load()
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    lib.tango_tuning_reload()
    yield lib
    os.environ.update(saved)
    lib.tango_tuning_reload()


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", DMA_CONV2D)
def test_dma_conv2d_routes(lib, dtype, case):
    B, Cin, H, W, Cout, pad, res = case
    with tuning(lib, **FORCED):
        assert conv2d_route(lib, dtype, B, Cin, H, W, Cout, 2, pad, res) == ("dma", 1)
    # unforced, these test-sized problems stay on the tile kernel: 448 tiles of 256 rows are B >= 7 at the VAE encoder's first Downsample
    assert conv2d_route(lib, dtype, B, Cin, H, W, Cout, 2, pad, res)[0] == "tile"


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_dma_conv2d_small_grids_are_split_instead(lib, dtype):
    """gemm_pick_splitk aims at two workgroups per CU, (512 + tiles / 2) / tiles splits: from 342 tiles of 128 x 160 on that is one (400 and
    more return early), so DMA_CONV2D[0] may lose two of its eight images; with five (320 tiles) the wrappers split K in two and the problem
    runs on the tile kernel even when the DMA kernel is forced"""
    with tuning(lib, **FORCED):
        assert conv2d_route(lib, dtype, 6, 64, 128, 64, 640, 2, 0) == ("dma", 1)        # 384 tiles
        assert conv2d_route(lib, dtype, 5, 64, 128, 64, 640, 2, 0) == ("tile+splitk", 2)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("Cout,H,W", TILE_PAD)
def test_tile_pad_routes(lib, dtype, pad, Cout, H, W):
    for env in (FORCED, UNFORCED):           # too small for every other kernel, switch or not
        with tuning(lib, **env):
            assert conv2d_route(lib, dtype, 3, 64, H, W, Cout, 2, pad) == tile_pad_expect(dtype, Cout)


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("case", DMA_CONV1D)
def test_dma_conv1d_routes(lib, dtype, case):
    Cin, Cout, L, k, d, res, e_act = case
    with tuning(lib, **FORCED):
        assert conv1d_route(lib, dtype, 2, Cin, L, Cout, k, d, 0, res, e_act) == ("dma", 1)
    assert conv1d_route(lib, dtype, 2, Cin, L, Cout, k, d, 0, res, e_act) == ("tile", 1)


def test_dma_conv1d_fp32_routes(lib):
    for Cin, Cout, L, k, d, res, e_act in DMA_CONV1D_FP32:
        with tuning(lib, **FORCED):
            assert conv1d_route(lib, "fp32", 2, Cin, L, Cout, k, d, 0, res, e_act) == ("dma", 1)
            assert conv1d_route(lib, "fp16", 2, Cin, L, Cout, k, d, 0, res, e_act) == ("tile", 1)     # 64-byte rows: half a chunk


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_conv1d_prologue_stays_on_the_tile_kernel(lib, dtype):
    """the LDS-DMA gather cannot apply leaky_relu on the way in: HiFi-GAN's c1 convs and upsamplers (a_act) never reach gemm_dma_kernel"""
    Cin, Cout, L, k, d, res, e_act = DMA_CONV1D[0]
    with tuning(lib, **FORCED):
        assert conv1d_route(lib, dtype, 2, Cin, L, Cout, k, d, 2, res, e_act) == ("tile", 1)
        assert all(r[2:] == ("tile", 1) for r in convt_phase_routes(lib, dtype, 2, 128, 53, 128, 16, 4, a_act=2))


@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("k,u,L", DMA_CONVT)
def test_dma_convt_phase_routes(lib, dtype, k, u, L):
    with tuning(lib, **FORCED):
        phases = convt_phase_routes(lib, dtype, 2, 128, L, 128, k, u)
    assert len(phases) == u
    assert sorted({p[0] for p in phases}) == {(16, 5): [3, 4], (16, 4): [4], (8, 2): [4], (4, 2): [2]}[(k, u)]      # taps per phase
    assert all(p[2:] == ("dma", 1) for p in phases), phases


def test_conv_out_routes(lib):
    B, H, W = CONV_OUT_BIG
    for dtype in ("fp16", "bf16"):
        assert conv2d_route(lib, dtype, B, 128, H, W, 1, 1, 1, 0, 0, 1) == ("conv_halo", 1)
        assert conv2d_route(lib, dtype, B - 1, 128, H, W, 1, 1, 1, 0, 0, 1) == ("tile", 1)        # 192 tiles: below the halo kernel's 256
        assert conv2d_route(lib, dtype, *((CONV_OUT_SMALL[0], 128) + CONV_OUT_SMALL[1:]), 1, 1, 1, 0, 0, 1) == ("tile", 1)
    assert conv2d_route(lib, "fp32", B, 128, H, W, 1, 1, 1, 0, 0, 1) == ("tile", 1)               # the narrow halo tile is 16-bit only


# (query arguments, (route, split-K)): the product batch sizes at which the DMA kernel starts to take these convs, unforced
PRODUCT_THRESHOLDS = [
    # UNet level-0 downsampler (320 -> 320, 256 x 16 -> 128 x 8): 2 x 1024 / 256 tiles per sample of the CFG batch -> 448 tiles at 2B = 56
    (("conv2d", 56, 320, 256, 16, 320, 2, 1), ("dma", 1)),
    (("conv2d", 55, 320, 256, 16, 320, 2, 1), ("tile", 1)),
    # VAE encoder, first Downsample (128 -> 128 at 1024 x 64 -> 512 x 32, pad 0): 64 tiles of 256 rows per sample -> B = 7
    (("conv2d", 7, 128, 1024, 64, 128, 2, 0), ("dma", 1)),
    (("conv2d", 6, 128, 1024, 64, 128, 2, 0), ("tile", 1)),
]


@pytest.mark.parametrize("args,want", PRODUCT_THRESHOLDS)
def test_product_batch_thresholds(lib, args, want):
    kind, B, Cin, H, W, Cout, stride, pad = args
    assert conv2d_route(lib, "fp16", B, Cin, H, W, Cout, stride, pad) == want


def test_vocoder_batch_thresholds(lib):
    """HiFi-GAN at 1024 mel frames (rates 5, 4, 2, 2, 2 from 1024 channels): the first resblock c2 convs (512 channels, L = 5120: 20 x 4 tiles of
    256 x 128 per sample) and the third upsampler's phases (256 -> 128 channels, 20480 rows per phase: 80 tiles per sample) reach the DMA
    kernel at B = 6; in the engine neither carries a prologue (the leaky_relu in front of them is the previous kernel's epilogue)"""
    for k, d in ((3, 1), (7, 1), (11, 1)):
        assert conv1d_route(lib, "fp16", 6, 512, 5120, 512, k, d, 0, 1, 0) == ("dma", 1)
        assert conv1d_route(lib, "fp16", 5, 512, 5120, 512, k, d, 0, 1, 0) == ("tile", 1)
    assert all(r[2:] == ("dma", 1) for r in convt_phase_routes(lib, "fp16", 6, 256, 20480, 128, 8, 2))
    assert all(r[2:] == ("tile", 1) for r in convt_phase_routes(lib, "fp16", 5, 256, 20480, 128, 8, 2))
