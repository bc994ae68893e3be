"""Audio-to-audio editing on the engine (AudioLDM style_transfer, audioldm/pipeline.py:145-247): the inverse and truncated loops at op
level against the fork's (tests/golden/edit_ref.npz), the fused latent encode launch (bitwise part, sampled part, Philox streams),
truncated / inverted / regional loops on the tiny UNet against the fp32 oracle, plan-cache isolation and the Tango entry points."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_inpaint_gpu as TI  # noqa: E402  (shared engines, inputs, oracle adapters and the synthetic Tango stack)
from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd.inpaint import latent_mask  # noqa: E402
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMInverseScheduler, DDIMScheduler  # noqa: E402

ROOT = TI.ROOT
PRED, RULE = TI.PRED, TI.RULE
vp = TI.vp
_cache = {}


def _tool():
    spec = importlib.util.spec_from_file_location("make_golden_edit", os.path.join(ROOT, "tools", "make_golden_edit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _tool()


def fixture():
    if "fix" not in _cache:
        with np.load(os.path.join(ROOT, "tests", "golden", "edit_ref.npz")) as z:
            _cache["fix"] = {k: z[k] for k in z.files}
    return _cache["fix"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- 1. op level: the fused one-step kernel replays the fork's inverse loops from the inverse table, bit for bit ------------------------
@pytest.mark.parametrize("pred,cfg", G.INVERSE_GRID)
def test_op_inverse_loop_bitwise(lib, pred, cfg):
    """tango_op_sched_step with rule 1 (DDIM) and the inverse table: no update kernel of its own is needed.  The table is the
    fixture's (the engine's coef_table() where the fixture was made, pinned there by tests/test_edit_host.py)."""
    f = fixture()
    key = G.inv_key(pred, cfg)
    coef = np.ascontiguousarray(f["tab/inv|%s/coef" % pred], dtype=np.float32)
    x, outs = G.inverse_inputs(int(f["seed/inv/" + key]), G.LOOP_STEPS, cfg)
    B, Cc, H, Wd = G.SHAPE
    lat = x.clone().cuda()
    for i in range(G.LOOP_STEPS):
        mod = outs[i].contiguous().cuda()
        row = np.ascontiguousarray(coef[i])
        rc = lib.tango_op_sched_step(vp(lat), vp(mod), None, hp(row), B, Cc, H * Wd, 1 if cfg else 0, G.GUIDANCE, PRED[pred], 1, 0, 1.0,
                                     None)
        assert rc == 0, lib.tango_last_error().decode()
    got, ref = lat.cpu().numpy(), f["inv/" + key]
    assert np.array_equal(bits(got), bits(ref)), "%s: max diff %g" % (key, np.abs(got - ref).max())


@pytest.mark.parametrize("rule,pred,cfg", G.TRUNC_GRID)
def test_op_truncated_loop_bitwise(lib, rule, pred, cfg):
    """the truncated tables drive the fused kernels through the fork's loop over timesteps[start:] (the multistep solver from
    order 1), bit for bit"""
    f = fixture()
    key = G.trunc_key(rule, pred, cfg)
    kind = G.I.RULES[rule][0]
    coef = np.ascontiguousarray(f["tab/%s|%s/coef" % (rule, pred)], dtype=np.float32)
    n = G.LOOP_STEPS - G.START
    assert coef.shape[0] == n
    x, outs, zn = G.trunc_inputs(int(f["seed/trunc/" + key]), n, cfg)
    B, Cc, H, Wd = G.SHAPE
    HW = H * Wd
    lat = x.clone().cuda()
    ring = torch.zeros(3, B, Cc, HW, device="cuda")
    for j in range(n):
        mod = outs[j].contiguous().cuda()
        if kind == "dpmsolver":
            rc = lib.tango_op_sched_multistep(vp(lat), vp(mod), vp(ring), hp(coef), j, B, Cc, HW, 1 if cfg else 0, G.GUIDANCE, PRED[pred],
                                              0, None)
        else:
            row = np.ascontiguousarray(coef[j])
            rc = lib.tango_op_sched_step(vp(lat), vp(mod), vp(zn[j].contiguous().cuda()), hp(row), B, Cc, HW, 1 if cfg else 0, G.GUIDANCE,
                                         PRED[pred], RULE[kind], 0, 1.0, None)
        assert rc == 0, lib.tango_last_error().decode()
    got, ref = lat.cpu().numpy(), f["trunc/" + key]
    assert np.array_equal(bits(got), bits(ref)), "%s: max diff %g" % (key, np.abs(got - ref).max())


# ---- the fused latent encode launch ---------------------------------------------------------------------------------------------------
SCALE = 0.9227914214134216           # the released checkpoint's scale_factor magnitude; any fp32-representable value would do
TRIGGER, RANGE = 1e2, 10.0


def encode(lib, mom, B, sa, sb, mode, eps=None, noise=None, seed=0, offset=0, want_z0=True, trigger=TRIGGER, rng=RANGE, scale=SCALE,
           expect=0):
    """tango_op_latent_encode on moments [Bm, 2C, HW] (cuda) -> (xt, z0) on the host"""
    Bm, C2, HW = mom.shape
    Cc = C2 // 2
    xt = torch.full((B, Cc, HW), float("nan"), device="cuda")
    z0 = torch.full((B, Cc, HW), float("nan"), device="cuda") if want_z0 else None
    rc = lib.tango_op_latent_encode(vp(mom), Bm, vp(z0), vp(xt), vp(eps), vp(noise), B, Cc, HW, scale, trigger, rng, sa, sb,
                                    1 if mode else 0, seed, offset, None)
    torch.cuda.synchronize()
    if expect:
        assert rc != 0
        return lib.tango_last_error().decode()
    assert rc == 0, lib.tango_last_error().decode()
    return xt.cpu(), (z0.cpu() if want_z0 else None)


def f32(x):
    return float(np.float32(x))


SA, SB = f32(0.6180339887), f32(0.7861513778)


# ---- 2. bitwise part: posterior mode, injected noise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Bm,Cc,HW", [(3, 1, 8, 4096), (2, 2, 8, 100), (2, 2, 6, 37)])
def test_encode_mode_bitwise(lib, B, Bm, Cc, HW):
    """xt == sa * (scale * mean) + sb * n and z0 == scale * mean in torch fp32, bit for bit; any HW (100 and 37 are no multiple of
    the block or of 4), C % 4 != 0 allowed when both draws are injected"""
    g = torch.Generator().manual_seed(100 + HW)
    mom = torch.randn(Bm, 2 * Cc, HW, generator=g) * 2.0
    n = torch.randn(B, Cc, HW, generator=g)
    xt, z0 = encode(lib, mom.cuda(), B, SA, SB, True, noise=n.cuda())
    mean = mom[:, :Cc].expand(B, Cc, HW)
    z = SCALE * mean
    ref = torch.tensor(SA) * z + torch.tensor(SB) * n
    assert torch.equal(z0, z)
    assert np.array_equal(bits(xt.numpy()), bits(ref.numpy())), (xt - ref).abs().max()
    # without the z0 output the same xt
    xt2, _ = encode(lib, mom.cuda(), B, SA, SB, True, noise=n.cuda(), want_z0=False)
    assert torch.equal(xt, xt2)


def test_encode_clip_is_per_sample_and_bitwise(lib):
    """a sample whose largest |z| is just above clip_trigger is clamped to +-clip_range, its neighbour just below is untouched"""
    B, Cc, HW = 2, 8, 4096
    g = torch.Generator().manual_seed(5)
    mom = torch.randn(B, 2 * Cc, HW, generator=g) * 8.0               # many |z| above the clip range of 10, none near 100
    assert (SCALE * mom[:, :Cc]).abs().max() < 60
    sc, trig = np.float32(SCALE), np.float32(TRIGGER)
    hi = trig / sc                                   # an fp32 mean whose scaled value is the first above the trigger ...
    while not np.float32(sc * hi) > trig:
        hi = np.nextafter(hi, np.float32(np.inf))
    lo = hi                                          # ... and the nearest below it whose scaled value is not
    while np.float32(sc * lo) > trig:
        lo = np.nextafter(lo, np.float32(0))
    mom[0, 3, 4000] = -float(hi)                     # the last block of the sample, negative sign
    mom[1, 5, 77] = float(lo)
    n = torch.randn(B, Cc, HW, generator=g)
    xt, z0 = encode(lib, mom.cuda(), B, SA, SB, True, noise=n.cuda())
    z = SCALE * mom[:, :Cc]
    assert z[0].abs().max() > TRIGGER and z[1].abs().max() <= TRIGGER and z[1].abs().max() > 99.99
    zref = torch.stack([z[0].clamp(-RANGE, RANGE), z[1]])
    assert torch.equal(z0, zref)
    assert z0[0].abs().max() == RANGE and z0[0, 3, 4000] == -RANGE and z0[1].abs().max() > 99.99
    ref = torch.tensor(SA) * zref + torch.tensor(SB) * n
    assert np.array_equal(bits(xt.numpy()), bits(ref.numpy()))


def test_encode_argument_errors(lib):
    mom = torch.zeros(2, 16, 64, device="cuda")
    n = torch.zeros(3, 8, 64, device="cuda")
    assert "moments_batch" in encode(lib, mom, 3, 1.0, 0.0, True, noise=n, expect=1)            # Bm = 2, B = 3
    m6 = torch.zeros(1, 12, 64, device="cuda")                                                   # C = 6
    n6 = torch.zeros(2, 6, 64, device="cuda")
    assert "multiple of 4" in encode(lib, m6, 2, SA, SB, True, expect=1)                        # Philox n
    xt, z0 = encode(lib, m6 + 1.5, 2, SA, 0.0, True)                                            # sb = 0: no n is drawn, any C
    assert torch.equal(z0, torch.tensor(SCALE) * torch.full((2, 6, 64), 1.5)) and torch.equal(xt, torch.tensor(SA) * z0)
    assert "multiple of 4" in encode(lib, m6, 2, 1.0, 0.0, False, noise=n6, expect=1)           # Philox eps
    encode(lib, m6, 2, 1.0, 0.0, False, eps=n6, noise=n6)                                       # both injected: fine
    rc = lib.tango_op_latent_encode(vp(mom), 2, None, None, None, None, 2, 8, 64, 1.0, 1e2, 10.0, 1.0, 0.0, 1, 0, 0, None)
    assert rc != 0
    out = torch.zeros(2, 8, 64, device="cuda")
    assert lib.tango_op_philox_normal_encode(vp(out), 2, 8, 64, 2, 0, 0, None) != 0
    assert lib.tango_op_philox_normal_encode(None, 2, 8, 64, 0, 0, 0, None) != 0
    assert lib.tango_op_philox_normal_encode(vp(out), 2, 0, 64, 0, 0, 0, None) != 0
    assert lib.tango_op_philox_normal_encode(vp(out), 2, 8, 64, 0, 0, -1, None) != 0


# ---- 3. sampled part: against the oracle's posterior + the scheduler's add_noise, exp being the only inexact operation -------------------
def test_encode_sampled_vs_oracle(lib):
    """fp64 value of the expression; the torch fp32 composition's error against it is the reference's own error; the kernel's error
    must stay within 2x that (a one-to-two-ulp difference between two correct expf implementations).
    Measured on the MI355X: see DESIGN.md, "Audio-to-audio editing"."""
    B, Cc, HW = 2, 8, 4096
    g = torch.Generator().manual_seed(9)
    mom = torch.randn(B, 2 * Cc, HW, generator=g)
    mom[:, Cc:] = torch.rand(B, Cc, HW, generator=g) * 60.0 - 35.0          # logvar in [-35, 25): past the clamp on both sides
    assert (mom[:, Cc:] < -30).any() and (mom[:, Cc:] > 20).any()
    eps, n = torch.randn(B, Cc, HW, generator=g), torch.randn(B, Cc, HW, generator=g)
    sch = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    start, t_enc = sch.edit_plan(20, 0.5)
    sa, sb = (float(v) for v in sch.blend_table(start=start - 1)[0])
    cfg = dict(scale_factor=SCALE)
    m4, e4, n4 = (t.view(B, -1, 256, 16) for t in (mom, eps, n))
    z32 = O.vae_get_first_stage_encoding(m4, cfg, noise=e4)
    ref32 = sch.add_noise(z32, n4, torch.full((B,), t_enc, dtype=torch.int64)).view(B, Cc, HW)
    md = mom.double()
    sd, ac = torch.exp(0.5 * md[:, Cc:].clamp(-30.0, 20.0)), sch.alphas_cumprod.double()[t_enc]
    z64 = float(np.float32(SCALE)) * (md[:, :Cc] + sd * eps.double())
    ref64 = float(np.float32(sa)) * z64 + float(np.float32(sb)) * n.double()
    assert abs(float(ac) ** 0.5 - sa) < 1e-6
    # no clip here: the oracle's composition has none (the trigger is out of reach)
    xt, z0 = encode(lib, mom.cuda(), B, sa, sb, False, eps=eps.cuda(), noise=n.cuda(), trigger=3e38)
    err_ref = (ref32.double() - ref64).abs().max().item()
    err_k = (xt.double() - ref64).abs().max().item()
    zerr_ref = (z32.view(B, Cc, HW).double() - z64).abs().max().item()
    zerr_k = (z0.double() - z64).abs().max().item()
    print("encode sampled: |ref64| max %.4g; xt error torch fp32 %.4g, kernel %.4g; z0 error torch fp32 %.4g, kernel %.4g"
          % (ref64.abs().max().item(), err_ref, err_k, zerr_ref, zerr_k))
    assert err_k <= 2 * err_ref
    assert zerr_k <= 2 * zerr_ref


# ---- 4. the two Philox streams ---------------------------------------------------------------------------------------------------------
def _draws(lib, B, which, seed, offset, HW=4096):
    out = torch.empty(B, 8, HW, device="cuda")
    assert lib.tango_op_philox_normal_encode(vp(out), B, 8, HW, which, seed, offset, None) == 0, lib.tango_last_error().decode()
    return out


@pytest.mark.parametrize("Bm", [1, 2])
def test_encode_injected_draws_equal_philox_and_batch_split(lib, Bm):
    B, Cc, HW, seed = 2, 8, 4096, 4711
    g = torch.Generator().manual_seed(21)
    mom = (torch.randn(Bm, 2 * Cc, HW, generator=g) * 1.5).cuda()
    eps, n = _draws(lib, B, 0, seed, 0), _draws(lib, B, 1, seed, 0)
    inj = encode(lib, mom, B, SA, SB, False, eps=eps, noise=n)
    phx = encode(lib, mom, B, SA, SB, False, seed=seed)
    assert torch.equal(inj[0], phx[0]) and torch.equal(inj[1], phx[1])
    half = encode(lib, mom, B, SA, SB, False, eps=eps, seed=seed)           # eps injected, n from Philox
    assert torch.equal(half[0], phx[0])
    assert not torch.equal(phx[0], encode(lib, mom, B, SA, SB, False, seed=seed + 1)[0])
    # B = 2 at offset 0 == two B = 1 calls at offsets 0 and 1
    parts = [encode(lib, mom[i:i + 1] if Bm == 2 else mom, 1, SA, SB, False, seed=seed, offset=i) for i in range(2)]
    assert torch.equal(phx[0], torch.cat([p[0] for p in parts])) and torch.equal(phx[1], torch.cat([p[1] for p in parts]))
    # posterior mode draws only n
    mode = encode(lib, mom, B, SA, SB, True, seed=seed)
    assert torch.equal(mode[0], encode(lib, mom, B, SA, SB, True, noise=n)[0])


@pytest.mark.parametrize("seed", [1, 77, 31337])
def test_encode_draws_independent_of_each_other_and_of_the_loop_streams(lib, seed):
    """test_blend_draws_independent_of_step_draws's checks and bounds (|corr|, |mean|, |std - 1| < 0.02 on 65 536 values) for the two
    new streams against each other and against the step and blend streams"""
    e = _draws(lib, 2, 0, seed, 0).flatten().double()
    n = _draws(lib, 2, 1, seed, 0).flatten().double()
    others = {"n": n}
    for step in (0, 1, 3, 19):
        others["step%d" % step] = TI._philox(lib, 2, step, seed, 0, False).flatten().double()
        others["blend%d" % step] = TI._philox(lib, 2, step, seed, 0, True).flatten().double()
    for name, a in (("eps", e), ("n", n)):
        mean, std = a.mean().item(), a.std().item()
        print("seed %d %s: mean %.4f std %.4f" % (seed, name, mean, std))
        assert abs(mean) < 0.02 and abs(std - 1) < 0.02
        for other, s in others.items():
            if other == name:
                continue
            corr = torch.corrcoef(torch.stack([a, s]))[0, 1].item()
            assert abs(corr) < 0.02, (name, other, corr)


# ---- tiny-UNet loops through the public entry points -----------------------------------------------------------------------------------
def _model(dtype):
    """AudioDiffusion on the tiny UNet (fp16: the one of the synthetic Tango stack)"""
    if dtype == "fp16":
        return TI._tango().model
    if "m32" not in _cache:
        from tango_amd.models import AudioDiffusion
        m = AudioDiffusion(unet_config=O.UNET_CONFIG_TINY, dtype="fp32")
        m.engine.load_synthetic(1234)
        _cache["m32"] = m
    return _cache["m32"]


def _inputs(N=20, L=9, seed=41):
    """one sample (the oracle's UNet is most of these tests' time; the op-level tests above cover B > 1): [uncond; cond] text rows
    with a one-token unconditional mask and a partly masked prompt, start latents, known latents, a mask with a time span and a mel
    band, step and blend noise"""
    if ("in", N) not in _cache:
        cfg = O.UNET_CONFIG_TINY
        g = torch.Generator().manual_seed(seed)
        enc = torch.randn(2, L, cfg["cross_attention_dim"], generator=g)
        mask = torch.ones(2, L, dtype=torch.bool)
        mask[0, 1:] = False
        mask[1, L - 2:] = False
        lat0 = torch.randn(1, 8, 256, 16, generator=g)
        known = torch.randn(1, 8, 256, 16, generator=g) * 0.8
        noises = torch.randn(N, 1, 8, 256, 16, generator=g)
        bnoise = torch.randn(N, 1, 8, 256, 16, generator=g)
        _cache[("in", N)] = (enc, mask, lat0, known, latent_mask(1, (0.10, 0.15), (0.5, 0.75)), noises, bnoise)
    return _cache[("in", N)]


class _Truncated:
    """the oracle loop's scheduler over timesteps[start:]: set_timesteps installs the tail of the full schedule"""

    def __init__(self, sch, start):
        self.s, self.start = sch, start

    def __getattr__(self, k):
        return getattr(self.s, k)

    def set_timesteps(self, n):
        self.s.set_timesteps(n)
        self.timesteps = self.s.timesteps[self.start:]


class _Inverse:
    """O.denoise_loop's scheduler interface on DDIMInverseScheduler (its step() is pinned to the fork's by tests/test_edit_host.py)"""

    def __init__(self, sch, count):
        self.s, self.count = sch, count

    def __getattr__(self, k):
        return getattr(self.s, k)

    def set_timesteps(self, n):
        self.s.set_timesteps(n)
        self.timesteps = self.s.timesteps[:self.count]

    def step(self, out, t, lat, noise=None):
        return self.s.step(out, t, lat).prev_sample


def _trunc_oracle(rule, N, inputs):
    key = ("trunc", rule, N)
    if key not in _cache:
        enc, mask, lat0, _, _, noises, _ = inputs
        with torch.no_grad():
            _cache[key] = O.denoise_loop(TI.unet_sd(), O.UNET_CONFIG_TINY, _Truncated(TI._oracle_sched(rule), N // 2), enc, mask,
                                         lat0.clone(), N, 3.0, noises=None if rule == "dpmpp_2m" else list(noises), prefix="unet.")
    return _cache[key]


def _edit_run(m, rule, N, inputs, use_graph=True, **kw):
    enc, mask, lat0, _, _, noises, _ = inputs
    k = N - N // 2
    m.use_graph = use_graph
    try:
        out = m.edit_from_embeddings(enc.cuda(), mask.cuda(), TI._sched(rule), N, 3.0, start_latents=lat0, strength=0.5,
                                     noise=None if rule == "dpmpp_2m" else noises[:k], seed=3, **kw)
        torch.cuda.synchronize()
    finally:
        m.use_graph = True
    return out.cpu()


# ---- 5. truncated loops against the fp32 oracle; graph / eager / k-step agree bit for bit ------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("N", [10, 20])
@pytest.mark.parametrize("rule", TI.RULES3)
def test_truncated_loop_vs_oracle(lib, rule, N, dtype):
    inputs = _inputs()
    ref = _trunc_oracle(rule, N, inputs)
    m = _model(dtype)
    g = _edit_run(m, rule, N, inputs, use_graph=True)
    x = _edit_run(m, rule, N, inputs, use_graph=False)
    assert torch.equal(g, x), "hipGraph replay and eager launches must agree bit for bit"
    with TI.tuning(lib, TANGO_GRAPH_STEPS=3):
        k = _edit_run(m, rule, N, inputs, use_graph=True)
    assert torch.equal(g, k), "the k-step graph must equal the one-step graph"
    err = (g - ref).abs().max().item()
    print("truncated %s N=%d start=%d %s max abs err %.3e (|ref| max %.2f)" % (rule, N, N // 2, dtype, err, ref.abs().max()))
    assert err <= (1e-2 if dtype == "fp32" else 1e-1)


# ---- 6. invert, then decode: 10 inverse steps and 10 DDIM (eta 0) steps without CFG ------------------------------------------------------
def _invert_decode_oracle(enc, mask, z):
    if "invdec" not in _cache:
        inv = DDIMInverseScheduler.from_scheduler(DDIMScheduler(**SD21_SCHEDULER_CONFIG))
        with torch.no_grad():
            x = O.denoise_loop(TI.unet_sd(), O.UNET_CONFIG_TINY, _Inverse(inv, 10), enc, mask, z.clone(), 10, 1.0, prefix="unet.")
            y = O.denoise_loop(TI.unet_sd(), O.UNET_CONFIG_TINY, O.DDIMOracle(**SD21_SCHEDULER_CONFIG, eta=0.0), enc, mask, x.clone(), 10,
                               1.0, prefix="unet.")
        _cache["invdec"] = (x, y)
    return _cache["invdec"]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_invert_then_decode_vs_oracle(lib, dtype):
    """compared with the same two loops on the oracle, not with the source latents: the reconstruction error is the method's"""
    enc2, mask2, _, known, *_ = _inputs()
    enc, mask = enc2[1:], mask2[1:]                       # the conditional row: no CFG
    z = known * 0.5
    rx, ry = _invert_decode_oracle(enc, mask, z)
    m = _model(dtype)
    ddim = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    x = m.invert_from_embeddings(enc.cuda(), mask.cuda(), ddim, 10, latents=z, count=10)
    y = m.inference_from_embeddings(enc.cuda(), mask.cuda(), ddim, 10, 1.0, latents=x, seed=0)
    ex, ey = (x.cpu() - rx).abs().max().item(), (y.cpu() - ry).abs().max().item()
    print("invert 10 + decode 10, %s: inverted max abs err %.3e (|ref| max %.2f), decoded %.3e (|ref| max %.2f)"
          % (dtype, ex, rx.abs().max(), ey, ry.abs().max()))
    tol = 1e-2 if dtype == "fp32" else 1e-1
    assert ex <= tol and ey <= tol
    # a partial inversion runs the first `count` rows only, and an inverse scheduler object is taken as it is
    inv = DDIMInverseScheduler.from_scheduler(ddim)
    a = m.invert_from_embeddings(enc.cuda(), mask.cuda(), inv, 10, latents=z, count=4)
    b = m.invert_from_embeddings(enc.cuda(), mask.cuda(), ddim, 10, latents=z, count=4)
    assert torch.equal(a, b) and not torch.equal(a, x)
    with pytest.raises(ValueError):
        m.invert_from_embeddings(enc.cuda(), mask.cuda(), ddim, 10, latents=z, count=11)


# ---- 7. regional edit: DPM++ 2M, known latents kept outside the mask, over a truncated schedule -------------------------------------------
def test_regional_edit_vs_masked_oracle(lib):
    N, start = 10, 5
    inputs = _inputs()
    enc, mask, lat0, known, lm, _, bnoise = inputs
    bl = TI._sched("dpmpp_2m")
    bl.set_timesteps(N)
    ts = bl.timesteps[start:]
    k = N - start
    x = bl.add_noise(known, bnoise[0], ts[0:1]) * lm + (1.0 - lm) * lat0

    def cb(i, t, lat):
        if i + 1 < k:
            lat.copy_(bl.add_noise(known, bnoise[i + 1], ts[i + 1:i + 2]) * lm + (1.0 - lm) * lat)

    with torch.no_grad():
        ref = O.denoise_loop(TI.unet_sd(), O.UNET_CONFIG_TINY, _Truncated(TI._oracle_sched("dpmpp_2m"), start), enc, mask, x, N, 3.0,
                             prefix="unet.", callback=cb)
    got = _edit_run(_model("fp32"), "dpmpp_2m", N, inputs, known_latents=known, latent_mask=lm, blend_noise=bnoise[:k])
    err = (got - ref).abs().max().item()
    print("regional DPM++ 2M edit N=10 start=5 fp32 max abs err %.3e" % err)
    assert err <= 1e-2
    assert not torch.equal(got, _edit_run(_model("fp32"), "dpmpp_2m", N, inputs))


# ---- 7b. the Music forms, and inversion on a DPM-Solver sampler's grid ---------------------------------------------------------------------
def test_music_edit_and_dpm_grid_inversion_vs_oracle(lib):
    """MusicAudioDiffusion.edit_from_embeddings (DPM++ 2M, 3 of 6 steps, CFG) and invert_from_embeddings handed the DPM-Solver sampler
    (3 inverse steps up the sampler's own timesteps, no CFG) against the oracle's loops with the beat / chord streams"""
    from oracle.make_golden import music_inputs
    from tango_amd import weights as W
    from tango_amd.models import MusicAudioDiffusion
    cfg = O.UNET_CONFIG_MUSIC_TINY
    m = MusicAudioDiffusion(unet_config=cfg, dtype="fp32")
    sd = W.synth_state_dict(W.unet_param_shapes(cfg), 1234)
    m.load_state_dict({"unet." + k: v for k, v in sd.items()})
    N, start = 6, 3
    _, enc, beat, chord, em, bm, cm = music_inputs(cfg, 2, 11)            # [uncond; cond] rows of one sample
    lat0 = torch.randn(1, 8, 256, 16, generator=torch.Generator().manual_seed(12))
    streams = dict(encoded_beats=beat, beat_mask=bm, encoded_chords=chord, chord_mask=cm)
    music = dict(beat_features=beat, chord_features=chord, beat_attention_mask=bm, chord_attention_mask=cm)
    got = m.edit_from_embeddings(enc, em, TI._sched("dpmpp_2m"), N, 3.0, start_latents=lat0, strength=0.5, seed=3, **streams).cpu()
    with torch.no_grad():
        ref = O.denoise_loop(sd, cfg, _Truncated(TI._oracle_sched("dpmpp_2m"), start), enc, em, lat0.clone(), N, 3.0, music=music)
    err = (got - ref).abs().max().item()
    # the conditional rows alone: no CFG
    cond = {k: v[1:] for k, v in streams.items()}
    dpm = TI._sched("dpmpp_2m")
    inv = DDIMInverseScheduler.from_scheduler(dpm)
    z = lat0 * 0.4
    x = m.invert_from_embeddings(enc[1:], em[1:], dpm, N, latents=z, count=N - start, **cond).cpu()
    with torch.no_grad():
        rx = O.denoise_loop(sd, cfg, _Inverse(inv, N - start), enc[1:], em[1:], z.clone(), N, 1.0,
                            music={k: v[1:] for k, v in music.items()})
    ex = (x - rx).abs().max().item()
    print("Music truncated DPM++ 2M 3 of 6 max abs err %.3e; 3 inverse steps on the DPM grid %s max abs err %.3e"
          % (err, inv.timesteps.tolist()[:4], ex))
    assert err <= 1e-2 and ex <= 1e-2
    assert int(inv.timesteps[N - start]) == dpm.edit_plan(N, 0.5)[1]       # the inversion ended on the sampler's encode timestep
    with pytest.raises(ValueError):
        m.edit_from_embeddings(enc, em, TI._sched("dpmpp_2m"), N, 3.0, start_latents=lat0, strength=0.5)
    with pytest.raises(NotImplementedError):
        m.edit(["x"], lat0, dpm)


# ---- 8. an edit does not disturb the cached plans / graphs of a full generation ---------------------------------------------------------
@pytest.mark.parametrize("rule", ["ddpm", "dpmpp_2m"])
def test_generation_edit_generation(lib, rule):
    m = _model("fp32")
    inputs = TI._inputs(N=6)
    enc, mask, lat0, *_ = inputs

    def gen():
        return m.inference_from_embeddings(enc.cuda(), mask.cuda(), TI._sched(rule), 6, 3.0, latents=lat0, seed=5).cpu()

    a = gen()
    e = m.edit_from_embeddings(enc.cuda(), mask.cuda(), TI._sched(rule), 6, 3.0, start_latents=lat0, strength=0.5, seed=5).cpu()
    b = gen()
    assert torch.equal(a, b)
    assert not torch.equal(a, e)


# ---- 9. Tango.edit_from_embeddings end to end ---------------------------------------------------------------------------------------------
def test_tango_edit_end_to_end_matches_hand_composed_chain(lib):
    t = TI._tango()
    enc, mask, *_ = TI._inputs(B=2, N=1)
    audio = TI._clip()
    w1 = t.edit_from_embeddings(enc.cuda(), mask.cuda(), audio, strength=0.5, steps=6, guidance=3, samples=2, seed=7)
    assert w1.dtype == np.int16 and w1.shape == (2, 163872)
    mom = t.encode_moments(audio)
    assert tuple(mom.shape) == (1, 16, 256, 16)
    start, t_enc = t.scheduler.edit_plan(6, 0.5)
    sa, sb = t.scheduler.blend_table(start=start - 1)[0]
    x = t.vae.encode_start_latents(mom, float(sa), float(sb), 2, seed=7)
    assert tuple(x.shape) == (2, 8, 256, 16) and not torch.equal(x[0], x[1])          # one clip, two draws
    lat = t.model.edit_from_embeddings(enc.cuda(), mask.cuda(), t.scheduler, 6, 3, start_latents=x, strength=0.5, seed=7)
    w2 = t.vae.decode_to_waveform(t.vae.decode_first_stage(lat))
    assert np.array_equal(w1, w2)
    assert np.abs(w1.astype(np.float32)).max() > 0
    # a regional edit: the clean latents are the known latents, the named time span is the region of the edit
    w3 = t.edit_from_embeddings(enc.cuda(), mask.cuda(), audio, strength=0.5, steps=6, guidance=3, samples=2, seed=7,
                                time_range=(0.25, 0.5))
    x2, z0 = t.vae.encode_start_latents(mom, float(sa), float(sb), 2, seed=7, want_clean=True)
    assert torch.equal(x, x2)
    lat3 = t.model.edit_from_embeddings(enc.cuda(), mask.cuda(), t.scheduler, 6, 3, start_latents=x2, strength=0.5, seed=7,
                                        known_latents=z0, latent_mask=latent_mask(2, (0.25, 0.5), (1.0, 1.0)))
    assert np.array_equal(w3, t.vae.decode_to_waveform(t.vae.decode_first_stage(lat3)))
    assert not np.array_equal(w1, w3)


def test_tango_edit_invert_mode_and_errors(lib):
    from tango_amd.tango import Tango
    t = TI._tango()
    enc, mask, *_ = TI._inputs(B=2, N=1)
    audio = TI._clip()
    with pytest.raises(ValueError):                                  # the default scheduler is DDPM: stochastic
        t.edit_from_embeddings(enc.cuda(), mask.cuda(), audio, steps=6, samples=2, mode="invert", source_embeds=enc[2:].cuda(),
                               source_mask=mask[2:].cuda())
    bare = Tango.from_components(t.model, t.vae)                      # no stft
    with pytest.raises(RuntimeError):
        bare.edit_from_embeddings(enc.cuda(), mask.cuda(), audio, steps=6, samples=2)
    ddim = DDIMScheduler(**SD21_SCHEDULER_CONFIG)
    td = Tango.from_components(t.model, t.vae, scheduler=ddim, stft=t.stft)
    w = [td.edit_from_embeddings(enc.cuda(), mask.cuda(), audio, strength=0.5, steps=6, guidance=3, samples=2, mode="invert",
                                 source_embeds=enc[2:].cuda(), source_mask=mask[2:].cuda(), seed=s) for s in (1, 2)]
    assert w[0].dtype == np.int16 and w[0].shape == (2, 163872) and np.abs(w[0].astype(np.float32)).max() > 0
    assert np.array_equal(w[0], w[1])                                 # deterministic: no draw reaches the result
    # the hand-composed chain: posterior mode -> 3 inverse steps under the source text -> the last 3 DDIM steps under the prompt
    z = td.vae.encode_start_latents(td.encode_moments(audio), 1.0, 0.0, 2, posterior="mode")
    assert torch.equal(z[0], z[1])
    x = td.model.invert_from_embeddings(enc[2:].cuda(), mask[2:].cuda(), ddim, 6, latents=z, count=3)
    lat = td.model.edit_from_embeddings(enc.cuda(), mask.cuda(), ddim, 6, 3, start_latents=x, strength=0.5, seed=1)
    assert np.array_equal(w[0], td.vae.decode_to_waveform(td.vae.decode_first_stage(lat)))
