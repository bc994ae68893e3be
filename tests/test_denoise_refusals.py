"""Every refusal of the denoise loop's argument checks (check_denoise_args and check_guidance_args, through
tango_debug_denoise_guided_check), word for word, with their precedence, and a handful of calls they accept.  No GPU.

The hook answers tango_last_error()'s text.  set_error() stores its argument as it is (no prefix); TANGO_FAIL appends
" at <file>:<line>" to the message it is given.  The message proper is therefore the answer without that suffix, and that is what
is compared here, in full."""
import ctypes as C
import re

import numpy as np
import pytest

from tango_amd import _lib

DDPM, DDIM, MULTISTEP = 0, 1, 2

M_STEPS = "denoise: num_steps must be positive"
M_RULE = "denoise: unknown rule"
M_WIDTH_MS = "denoise: the multistep rule takes 16-float coefficient rows (coef_width 16)"
M_WIDTH_8 = "denoise: DDPM / DDIM take 8-float coefficient rows (coef_width 0 or 8)"
M_MS_NOISE = "denoise: the multistep rule is deterministic: noise must be NULL"
M_MS_CLIP = "denoise: clip_sample is not supported by the multistep rule"
M_MS_ALGO = "denoise: multistep table column 11 (algorithm) must be 0 or 1"
M_MS_ORDER = "denoise: multistep table row with a bad order"
M_MASK_PAIR = "denoise: known_latents and latent_mask go together"
M_MASK_COEF = "denoise: a masked call needs blend_coef [num_steps][2]"
M_MASK_STRAY = "denoise: blend_coef / blend_noise need known_latents and latent_mask"
M_RESCALE = "denoise: guidance rescale must be in [0, 1]"
M_RESCALE_CFG = "denoise: guidance rescale needs classifier-free guidance (guidance_scale > 1 or a guidance table)"
M_TABLE_BATCH = "denoise: a guidance table needs batch > 0"
M_TABLE_ENTRY = "denoise: guidance table entries must be finite and >= 0"

_SUFFIX = re.compile(r" at [^ ]+:\d+$")
_BUF = np.zeros(64, dtype=np.float32)          # stands for any device pointer: the checks only ask whether it is null
PTR = _BUF.ctypes.data


def ms_table(orders, algo=0.0):
    """a multistep coefficient table [len(orders)][16] with the order column (10) and the algorithm column (11) set"""
    t = np.zeros((len(orders), 16), dtype=np.float32)
    t[:, 10] = orders
    t[:, 11] = algo
    return t


def check(lib, guidance_scale=3.0, table=None, rescale=None, steps=2, batch=2, coef=None, **fields):
    """the message proper ("" = accepted); a guidance block is passed when `table` or `rescale` is given"""
    a = _lib.DenoiseArgs()
    a.num_steps, a.batch, a.guidance_scale = steps, batch, guidance_scale
    keep_c = np.ascontiguousarray(coef, dtype=np.float32) if coef is not None else None
    if keep_c is not None:
        a.coef = keep_c.ctypes.data
    for k, v in fields.items():
        setattr(a, k, v)
    g = None
    keep_t = np.ascontiguousarray(table, dtype=np.float32) if table is not None else None
    if table is not None or rescale is not None:
        g = _lib.GuidanceArgs()
        g.table = keep_t.ctypes.data if keep_t is not None else None
        g.rescale = 0.0 if rescale is None else rescale
    got = lib.tango_debug_denoise_guided_check(C.byref(a), C.byref(g) if g is not None else None).decode()
    return _SUFFIX.sub("", got)


def ms(lib, orders=(1, 2, 3, 3), algo=0.0, **kw):
    kw.setdefault("steps", len(orders))
    kw.setdefault("coef_width", 16)
    return check(lib, rule=MULTISTEP, coef=ms_table(orders, algo), **kw)


def test_suffix_is_all_that_is_stripped(lib):
    a = _lib.DenoiseArgs(num_steps=0, batch=1)
    raw = lib.tango_debug_denoise_guided_check(C.byref(a), None).decode()
    assert raw.startswith(M_STEPS + " at ") and _SUFFIX.search(raw) and _SUFFIX.sub("", raw) == M_STEPS


def test_accepted(lib):
    for rule in (DDPM, DDIM):
        for w in (0, 8):
            assert check(lib, rule=rule, coef_width=w) == ""
        assert check(lib, rule=rule, noise=PTR, clip_sample=1, clip_sample_range=1.0) == ""
    assert ms(lib) == "" and ms(lib, algo=1.0) == "" and ms(lib, orders=(1,)) == "" and ms(lib, orders=(1, 1, 2, 1, 3)) == ""
    assert check(lib, known_latents=PTR, latent_mask=PTR, blend_coef=PTR) == ""
    assert check(lib, known_latents=PTR, latent_mask=PTR, blend_coef=PTR, blend_noise=PTR) == ""
    assert ms(lib, known_latents=PTR, latent_mask=PTR, blend_coef=PTR) == ""
    assert check(lib, rescale=0.0) == "" and check(lib, rescale=0.7) == "" and check(lib, rescale=1.0) == ""
    assert check(lib, guidance_scale=1.0, rescale=0.0) == ""
    assert check(lib, guidance_scale=1.0, table=[[0, 1], [2, 3]], rescale=0.5) == ""
    assert check(lib, table=[[0.0, 7.5], [3.0, 0.0]]) == ""
    assert ms(lib, table=np.full((4, 2), 3.0), rescale=0.7) == ""


def test_denoise_refusals_verbatim(lib):
    assert check(lib, steps=0) == M_STEPS and check(lib, steps=-3) == M_STEPS
    for rule in (-1, 3, 7):
        assert check(lib, rule=rule) == M_RULE
    for w in (16, 4, 1):
        assert check(lib, rule=DDPM, coef_width=w) == M_WIDTH_8 and check(lib, rule=DDIM, coef_width=w) == M_WIDTH_8
    for w in (0, 8, 32):
        assert ms(lib, coef_width=w) == M_WIDTH_MS
    assert ms(lib, noise=PTR) == M_MS_NOISE
    assert ms(lib, clip_sample=1) == M_MS_CLIP
    for algo in (2.0, -1.0, 0.5):
        assert ms(lib, algo=algo) == M_MS_ALGO
    assert ms(lib, orders=(2, 1, 1)) == M_MS_ORDER, "order 2 at row 0"
    assert ms(lib, orders=(1, 3, 1)) == M_MS_ORDER, "order 3 at row 1"
    assert ms(lib, orders=(1, 2, 3, 4)) == M_MS_ORDER, "order 4"
    assert ms(lib, orders=(1, 2, 0)) == M_MS_ORDER and ms(lib, orders=(1, 1.5)) == M_MS_ORDER
    assert check(lib, known_latents=PTR) == M_MASK_PAIR and check(lib, latent_mask=PTR) == M_MASK_PAIR
    assert check(lib, known_latents=PTR, latent_mask=PTR) == M_MASK_COEF
    assert check(lib, known_latents=PTR, latent_mask=PTR, blend_noise=PTR) == M_MASK_COEF
    assert check(lib, blend_coef=PTR) == M_MASK_STRAY and check(lib, blend_noise=PTR) == M_MASK_STRAY


def test_guidance_refusals_verbatim(lib):
    for r in (-0.1, 1.5, float("nan"), float("inf")):
        assert check(lib, rescale=r) == M_RESCALE
    for gs in (1.0, 0.0):
        assert check(lib, guidance_scale=gs, rescale=0.5) == M_RESCALE_CFG
    for batch in (0, -2):
        assert check(lib, table=[[3, 1], [2, 2]], batch=batch) == M_TABLE_BATCH
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert check(lib, table=[[3, 1], [2, bad]]) == M_TABLE_ENTRY
        assert check(lib, table=[[bad, 1], [2, 3]]) == M_TABLE_ENTRY


def test_precedence(lib):
    """where two rules fire at once, the earlier `if` speaks"""
    assert check(lib, steps=0, rule=7) == M_STEPS
    assert check(lib, rule=7, coef_width=5) == M_RULE
    assert check(lib, rule=DDPM, coef_width=16, known_latents=PTR) == M_WIDTH_8
    assert ms(lib, coef_width=8, noise=PTR) == M_WIDTH_MS
    assert ms(lib, noise=PTR, clip_sample=1) == M_MS_NOISE
    assert ms(lib, clip_sample=1, algo=2.0) == M_MS_CLIP
    assert ms(lib, orders=(2, 1), algo=2.0) == M_MS_ALGO
    assert ms(lib, orders=(2, 1), known_latents=PTR) == M_MS_ORDER
    assert check(lib, known_latents=PTR, blend_noise=PTR) == M_MASK_PAIR, "before the blend_coef rules"
    assert check(lib, latent_mask=PTR, blend_coef=PTR) == M_MASK_PAIR
    # the checks of the call come before those of the guidance block
    assert check(lib, steps=0, rescale=1.5) == M_STEPS
    assert check(lib, blend_coef=PTR, rescale=1.5) == M_MASK_STRAY
    assert ms(lib, orders=(1, 3), table=[[3, -1], [2, 2]]) == M_MS_ORDER
    # inside the guidance block
    assert check(lib, guidance_scale=1.0, rescale=1.5) == M_RESCALE
    assert check(lib, rescale=-0.5, table=[[3, 1], [2, 2]], batch=0) == M_RESCALE
    assert check(lib, guidance_scale=1.0, rescale=0.5, table=[[3, 1], [2, 2]], batch=0) == M_TABLE_BATCH, "a table is guidance"
    assert check(lib, table=[[3, float("nan")], [2, 2]], batch=0) == M_TABLE_BATCH


def test_all_fifteen_are_covered():
    msgs = [v for k, v in globals().items() if k.startswith("M_")]
    assert len(msgs) == 15 and len(set(msgs)) == 15 and all(m.startswith("denoise: ") for m in msgs)
