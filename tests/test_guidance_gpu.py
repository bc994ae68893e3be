"""Guidance tables, guidance rescale and negative prompts on the GPU: the statistics launch and the guided update kernels through
tango_op_sched_guided (scale accuracy, bit-exactness of everything after the scale, defaults, batch independence, zero spread, the
masked variants), the tiny-UNet loop against a reference built from the oracle's UNet and scheduler steps (graph replay, one engine
serving default and guided calls in turn), and the string entry points of Tango with a negative prompt."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tango_oracle as O  # noqa: E402  (checker only)
from tango_amd import weights as W  # noqa: E402
from tango_amd.engine import Engine  # noqa: E402
from tango_amd.scheduler import SD21_SCHEDULER_CONFIG, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler  # noqa: E402

SD21 = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
_DDPM_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}
RULE = {"ddpm": 0, "ddim": 1, "dpmsolver": 2}
_cache = {}


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def hp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
N_OP = 4            # steps of the op-level schedules; the DDPM / DDIM cases run loop index 0, the multistep case 0 and then 1 (order 2)


class Case:
    """one rule and prediction type: the engine's table and a torch step on the same host (the oracle's for DDPM / DDIM, the
    engine scheduler's own multistep step(), as the existing bit-exact tests pair them)"""

    def __init__(self, rule, pred):
        self.rule, self.pred = rule, pred
        if rule == "ddpm":
            self.sch = DDPMScheduler.from_config(dict({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS}, prediction_type=pred))
            self.ora = O.DDPMOracle(**dict(O.SD21_SCHEDULER, prediction_type=pred))
        elif rule == "ddim":
            self.sch = DDIMScheduler(**dict(SD21_SCHEDULER_CONFIG, prediction_type=pred), eta=1.0)
            self.ora = O.DDIMOracle(**dict(SD21_SCHEDULER_CONFIG, prediction_type=pred), eta=1.0)
        else:
            self.sch = DPMSolverMultistepScheduler(**SD21, solver_order=2, prediction_type=pred, algorithm_type="dpmsolver++")
            self.ora = None
        self.sch.set_timesteps(N_OP)
        if self.ora is not None:
            self.ora.set_timesteps(N_OP)
        self.coef = np.ascontiguousarray(self.sch.coef_table(), dtype=np.float32)
        self.bc = np.ascontiguousarray(self.sch.blend_table(), dtype=np.float32)
        self.ms = rule == "dpmsolver"
        self.steps = (0, 1) if self.ms else (0,)

    def fresh(self):
        """a scheduler with no multistep history"""
        if self.ms:
            self.sch = DPMSolverMultistepScheduler(**SD21, solver_order=2, prediction_type=self.pred, algorithm_type="dpmsolver++")
            self.sch.set_timesteps(N_OP)

    def torch_step(self, v, i, x, noise):
        t = self.sch.timesteps[i]
        if self.ms:
            return self.sch.step(v, t, x).prev_sample
        return self.ora.step(v, int(t), x, noise=noise)


CASES = [(r, p) for r in ("ddpm", "ddim", "dpmsolver") for p in ("epsilon", "v_prediction")]


def op_inputs(B, HW, off, seed, steps=2):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(B, 8, HW, 1, generator=g)
    outs, noises = [], []
    for _ in range(steps):
        u = torch.randn(B, 8, HW, 1, generator=g) + off
        c = u + 0.3 * torch.randn(B, 8, HW, 1, generator=g)
        outs.append(torch.cat([u, c]))
        noises.append(torch.randn(B, 8, HW, 1, generator=g))
    return lat, outs, torch.stack(noises)


def guided_step(lib, case, lat_d, mo_d, noise_d, ring_d, i, row, phi, masked=None, guided=True):
    """one call of the guided hook (or of tango_op_sched_masked with `guided` False); returns scale_out"""
    B, Cc, HW = lat_d.shape[0], lat_d.shape[1], lat_d.shape[2] * lat_d.shape[3]
    scale = np.full(B, -7.0, dtype=np.float32)
    known, lm, bn = masked if masked is not None else (None, None, None)
    head = (vp(lat_d), vp(mo_d), None if case.ms else vp(noise_d), vp(ring_d) if case.ms else None, hp(case.coef), case.coef.shape[1], i,
            N_OP, vp(known), vp(lm), hp(case.bc) if masked is not None else None, vp(bn), 0, 0, B, Cc, HW, 1, 3.0, PRED[case.pred],
            RULE[case.rule])
    if guided:
        rowa = np.ascontiguousarray(row, dtype=np.float32)
        rc = lib.tango_op_sched_guided(*head, hp(rowa), float(phi), hp(scale), None)
    else:
        rc = lib.tango_op_sched_masked(*head, None)
    assert rc == 0, lib.tango_last_error().decode()
    return scale


def formula(u, c, row, s, phi):
    """cfg, r, v in fp32 in the written order; 1 - phi is an fp32 subtraction"""
    g = torch.tensor(row, dtype=torch.float32).view(-1, 1, 1, 1)
    d = c - u
    cfg = u + g * d
    if not phi > 0:
        return cfg
    r = cfg * torch.as_tensor(s, dtype=torch.float32).view(-1, 1, 1, 1)
    p32 = torch.tensor(phi, dtype=torch.float32)
    return p32 * r + (torch.tensor(1.0) - p32) * cfg


def scale_refs(u, c, row):
    """(float64 formula, torch's own fp32 evaluation) of s_b on the same fp32 inputs"""
    g64 = torch.tensor(row, dtype=torch.float32).double().view(-1, 1, 1, 1)
    u64, c64 = u.double(), c.double()
    cfg64 = u64 + g64 * (c64 - u64)
    s64 = c64.flatten(1).std(1) / cfg64.flatten(1).std(1)
    cfg32 = formula(u, c, row, None, 0.0)
    s32 = c.flatten(1).std(1) / cfg32.flatten(1).std(1)
    return s64, s32


ROW = (3.0, 1.0, 7.5)
worst = {"kernel": 0.0, "torch": 0.0}


@pytest.mark.parametrize("HW", [300, 1024, 8192])
@pytest.mark.parametrize("rule,pred", CASES)
def test_op_scale_accuracy_and_bitwise_rest(lib, rule, pred, HW):
    """(a) scale_out against the float64 formula: relative error <= max(32 x the error of torch's own fp32 evaluation, 1e-6);
    (b) given that scale, the latents equal torch fp32 evaluating cfg, r, v in the written order and then the scheduler step"""
    case = Case(rule, pred)
    B = 3
    for off in (0.0, 64.0):
        for phi in (0.7, 1.0):
            case.fresh()
            lat, outs, noises = op_inputs(B, HW, off, seed=1000 + HW + int(off))
            lat_d, noise_d = lat.clone().cuda(), noises.cuda()
            ring = torch.zeros(3, B, 8, HW, device="cuda")
            x = lat.clone()
            for i in case.steps:
                u, c = outs[i].chunk(2)
                scale = guided_step(lib, case, lat_d, outs[i].cuda(), noise_d, ring, i, ROW, phi)
                s64, s32 = scale_refs(u, c, ROW)
                ek = ((torch.from_numpy(scale).double() - s64).abs() / s64).max().item()
                et = ((s32.double() - s64).abs() / s64).max().item()
                worst["kernel"], worst["torch"] = max(worst["kernel"], ek), max(worst["torch"], et)
                print("%s %s HW %d off %g phi %g step %d: s_b rel err kernel %.3e torch-fp32 %.3e (worst so far %.3e / %.3e)"
                      % (rule, pred, HW, off, phi, i, ek, et, worst["kernel"], worst["torch"]))
                assert ek <= max(32 * et, 1e-6)
                x = case.torch_step(formula(u, c, ROW, scale, phi), i, x, noises[i])
                got = lat_d.cpu()
                assert torch.equal(got, x), "step %d: max diff %g" % (i, (got - x).abs().max())


@pytest.mark.parametrize("rule,pred", CASES)
def test_op_defaults_equal_the_scalar_kernels(lib, rule, pred):
    """(c) phi = 0 with a uniform row of 3.0 is tango_op_sched_step / tango_op_sched_multistep, bit for bit"""
    case = Case(rule, pred)
    B, HW = 3, 300
    lat, outs, noises = op_inputs(B, HW, 0.0, seed=5)
    a, b = lat.clone().cuda(), lat.clone().cuda()
    ring_a, ring_b = torch.zeros(3, B, 8, HW, device="cuda"), torch.zeros(3, B, 8, HW, device="cuda")
    noise_d = noises.cuda()
    for i in case.steps:
        mo = outs[i].cuda()
        scale = guided_step(lib, case, a, mo, noise_d, ring_a, i, (3.0, 3.0, 3.0), 0.0)
        assert scale.tolist() == [1.0] * B
        if case.ms:
            rc = lib.tango_op_sched_multistep(vp(b), vp(mo), vp(ring_b), hp(case.coef), i, B, 8, HW, 1, 3.0, PRED[pred], 0, None)
        else:
            row = np.ascontiguousarray(case.coef[i])
            rc = lib.tango_op_sched_step(vp(b), vp(mo), vp(noise_d[i]), hp(row), B, 8, HW, 1, 3.0, PRED[pred], RULE[rule], 0, 1.0, None)
        assert rc == 0, lib.tango_last_error().decode()
        assert torch.equal(a.cpu(), b.cpu()), "step %d" % i
        assert torch.equal(ring_a.cpu(), ring_b.cpu())


@pytest.mark.parametrize("HW", [300, 8192])
@pytest.mark.parametrize("rule,pred", [("ddpm", "v_prediction"), ("dpmsolver", "epsilon")])
def test_op_batch_independence(lib, rule, pred, HW):
    """(d) sample 1 run alone gives the same s_b bits and the same latents bits as inside B = 3"""
    case = Case(rule, pred)
    lat, outs, noises = op_inputs(3, HW, 64.0, seed=9)
    full, one = lat.clone().cuda(), lat[1:2].clone().cuda()
    ring3, ring1 = torch.zeros(3, 3, 8, HW, device="cuda"), torch.zeros(3, 1, 8, HW, device="cuda")
    for i in case.steps:
        u, c = outs[i].chunk(2)
        s3 = guided_step(lib, case, full, outs[i].cuda(), noises.cuda(), ring3, i, ROW, 0.7)
        s1 = guided_step(lib, case, one, torch.cat([u[1:2], c[1:2]]).cuda(), noises[:, 1:2].contiguous().cuda(), ring1, i, ROW[1:2], 0.7)
        assert s3.view(np.uint32)[1] == s1.view(np.uint32)[0]
        assert torch.equal(full[1:2].cpu(), one.cpu())


@pytest.mark.parametrize("rule,pred", [("ddpm", "v_prediction"), ("ddim", "epsilon"), ("dpmsolver", "v_prediction")])
def test_op_zero_spread(lib, rule, pred):
    """(e) a constant model output has std(cfg) = 0: s_b = 1 (the one deviation from the formula) and finite latents"""
    case = Case(rule, pred)
    B, HW = 3, 300
    lat, _, noises = op_inputs(B, HW, 0.0, seed=11)
    for uval, cval in ((0.25, 0.25), (0.5, -1.5), (0.0, 0.0)):
        mo = torch.cat([torch.full((B, 8, HW, 1), uval), torch.full((B, 8, HW, 1), cval)])
        lat_d = lat.clone().cuda()
        ring = torch.zeros(3, B, 8, HW, device="cuda")
        scale = guided_step(lib, case, lat_d, mo.cuda(), noises.cuda(), ring, 0, ROW, 0.7)
        assert scale.tolist() == [1.0] * B
        got = lat_d.cpu()
        assert torch.isfinite(got).all()
        u, c = mo.chunk(2)
        case.fresh()
        assert torch.equal(got, case.torch_step(formula(u, c, ROW, scale, 0.7), 0, lat.clone(), noises[0]))


@pytest.mark.parametrize("rule,pred", CASES)
def test_op_masked_variant(lib, rule, pred):
    """(f) a 0 / 1 mask with injected blend noise: rows with m = 0 equal the unmasked guided result, rows with m = 1 equal
    tango_op_sched_masked's, bit for bit"""
    case = Case(rule, pred)
    B, HW = 3, 300
    lat, outs, noises = op_inputs(B, HW, 0.0, seed=13)
    g = torch.Generator().manual_seed(14)
    known = torch.randn(B, 8, HW, 1, generator=g).cuda()
    bn = torch.randn(N_OP, B, 8, HW, 1, generator=g).cuda()
    m = (torch.rand(B, HW, generator=g) < 0.5).float()
    mo, noise_d = outs[0].cuda(), noises.cuda()
    res = {}
    for name, masked, guided in (("guided", None, True), ("guided+mask", (known, m.cuda(), bn), True), ("mask", (known, m.cuda(), bn), False)):
        x = lat.clone().cuda()
        ring = torch.zeros(3, B, 8, HW, device="cuda")
        res[name] = (guided_step(lib, case, x, mo, noise_d, ring, 0, ROW, 0.7, masked=masked, guided=guided), x.cpu())
    assert np.array_equal(res["guided"][0], res["guided+mask"][0])
    keep = (m == 1).view(B, 1, HW, 1).expand(B, 8, HW, 1)
    assert keep.any() and (~keep).any()
    gm = res["guided+mask"][1]
    assert torch.equal(gm[~keep], res["guided"][1][~keep])
    assert torch.equal(gm[keep], res["mask"][1][keep])
    assert not torch.equal(gm, res["guided"][1]) and not torch.equal(gm, res["mask"][1])


def test_op_refusals(lib):
    case = Case("ddpm", "v_prediction")
    lat, outs, noises = op_inputs(2, 300, 0.0, seed=3)
    x, mo, nz = lat.cuda(), outs[0].cuda(), noises.cuda()

    def call(row, phi, cfg=1):
        rowa = np.ascontiguousarray(row, dtype=np.float32)
        return lib.tango_op_sched_guided(vp(x), vp(mo), vp(nz), None, hp(case.coef), 8, 0, N_OP, None, None, None, None, 0, 0, 2, 8, 300, cfg,
                                         3.0, 2, 0, hp(rowa), phi, None, None)

    assert call((3, 5), 0.5) == 0
    for row, phi, cfg in (((3, -1), 0.5, 1), ((3, float("nan")), 0.0, 1), ((3, 5), 1.5, 1), ((3, 5), float("nan"), 1), ((3, 5), 0.5, 0)):
        assert call(row, phi, cfg) != 0
        assert b"op_sched_guided" in lib.tango_last_error()


# ---- loop level -------------------------------------------------------------------------------------------------------------------------
H_LOOP, B_LOOP, N_LOOP = 64, 2, 3


def unet_engine(dtype):
    if dtype not in _cache:
        e = Engine(unet=O.UNET_CONFIG_TINY, dtype=dtype)
        e.load_synthetic(1234)
        _cache[dtype] = e
    return _cache[dtype]


def unet_sd():
    if "sd" not in _cache:
        _cache["sd"] = W.synth_state_dict(W.unet_param_shapes(O.UNET_CONFIG_TINY, "unet."), 1234)
    return _cache["sd"]


def loop_inputs():
    if "in" not in _cache:
        g = torch.Generator().manual_seed(41)
        L = 9
        enc = torch.randn(2 * B_LOOP, L, O.UNET_CONFIG_TINY["cross_attention_dim"], generator=g)
        mask = torch.ones(2 * B_LOOP, L, dtype=torch.bool)
        mask[0, 5:] = False          # the negative half keeps >= 2 keys per row: the whole-batch plan, no single-key prefix
        mask[1, 2:] = False
        mask[3, 4:] = False
        lat0 = torch.randn(B_LOOP, 8, H_LOOP, 16, generator=g)
        noises = torch.randn(N_LOOP, B_LOOP, 8, H_LOOP, 16, generator=g)
        _cache["in"] = (enc, mask, lat0, noises)
    return _cache["in"]


def loop_sched(rule):
    if rule == "ddpm":
        return DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS}), O.DDPMOracle(**O.SD21_SCHEDULER)
    s = DPMSolverMultistepScheduler(**SD21, solver_order=2, prediction_type="v_prediction", algorithm_type="dpmsolver++")
    return s, None


GUIDES = {"row": (0.7, np.array([3.0, 5.0], np.float32)),
          "schedule": (0.3, np.array([[7.5, 1.0], [4.0, 0.0], [2.0, 6.0]], np.float32))}


def loop_reference(rule, which):
    """the loop of models.py:224-249 with the table and the rescale: the oracle's UNet, the formula in torch fp32, the oracle's step"""
    key = ("ref", rule, which)
    if key not in _cache:
        enc, mask, lat0, noises = loop_inputs()
        phi, tab = GUIDES[which]
        tab = np.broadcast_to(tab, (N_LOOP, B_LOOP))
        sch, ora = loop_sched(rule)
        sch.set_timesteps(N_LOOP)
        if ora is not None:
            ora.set_timesteps(N_LOOP)
        x = lat0.clone()
        with torch.no_grad():
            for i, t in enumerate(sch.timesteps):
                out = O.unet_forward(unet_sd(), O.UNET_CONFIG_TINY, torch.cat([x, x]), t, enc, mask, "unet.")
                u, c = out.chunk(2)
                g = torch.tensor(tab[i].tolist(), dtype=torch.float32).view(-1, 1, 1, 1)
                cfg = u + g * (c - u)
                sd_cfg = cfg.flatten(1).std(1)
                s = torch.where(sd_cfg == 0, torch.ones_like(sd_cfg), c.flatten(1).std(1) / sd_cfg).view(-1, 1, 1, 1)
                v = phi * (cfg * s) + (1 - phi) * cfg
                x = ora.step(v, int(t), x, noise=noises[i]) if ora is not None else sch.step(v, t, x).prev_sample
        _cache[key] = x
    return _cache[key]


def loop_run(e, rule, guidance=3.0, which=None, use_graph=True):
    enc, mask, lat0, noises = loop_inputs()
    sch, _ = loop_sched(rule)
    sch.set_timesteps(N_LOOP)
    kw = {}
    if which is not None:
        phi, tab = GUIDES[which]
        kw = dict(guidance_table=np.ascontiguousarray(np.broadcast_to(tab, (N_LOOP, B_LOOP))), guidance_rescale=phi)
    lat = lat0.clone().cuda()
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), guidance, prediction_type="v_prediction", rule=sch.rule,
              noise=noises.cuda() if rule == "ddpm" else None, use_graph=use_graph, latent_h=H_LOOP, **kw)
    torch.cuda.synchronize()
    return lat.cpu()


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("rule", ["ddpm", "dpmsolver"])
def test_loop_guided_default_guided_on_one_engine(lib, rule, dtype):
    """a rescaled call, a default call, a rescaled call with another phi and table, on one engine and plan: the default call equals
    the one made before any guided call bit for bit (no statistics launch leaked into its graph, nothing left in the parameter
    block), each guided call meets its own reference (phi and the table are read per call, not baked in at capture), and graph
    replay equals eager launches bit for bit"""
    e = unet_engine(dtype)
    tol = 1e-2 if dtype == "fp32" else 1e-1
    d0 = loop_run(e, rule)
    r1 = loop_run(e, rule, which="row")
    d1 = loop_run(e, rule)
    r2 = loop_run(e, rule, which="schedule")
    d2 = loop_run(e, rule)
    assert torch.equal(d0, d1) and torch.equal(d0, d2)
    for got, which in ((r1, "row"), (r2, "schedule")):
        ref = loop_reference(rule, which)
        err = (got - ref).abs().max().item()
        print("%s %s %s: max abs err vs the reference loop %.3e (|ref| max %.2f)" % (rule, dtype, which, err, ref.abs().max()))
        assert err <= tol
        assert torch.equal(got, loop_run(e, rule, which=which, use_graph=False)), "hipGraph replay and eager launches must agree bit for bit"
    assert not torch.equal(r1, r2) and not torch.equal(r1, d0)
    # a rescale alone (scalar guidance) is the table filled with the scalar
    enc, mask, lat0, noises = loop_inputs()
    sch, _ = loop_sched(rule)
    sch.set_timesteps(N_LOOP)
    outs = []
    for kw in (dict(guidance_rescale=0.7), dict(guidance_rescale=0.7, guidance_table=np.full((N_LOOP, B_LOOP), 3.0, np.float32))):
        lat = lat0.clone().cuda()
        e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 3.0, prediction_type="v_prediction", rule=sch.rule,
                  noise=noises.cuda() if rule == "ddpm" else None, latent_h=H_LOOP, **kw)
        outs.append(lat.cpu())
    assert torch.equal(outs[0], outs[1])
    # a table of the scalar with phi = 0 is the default call
    lat = lat0.clone().cuda()
    e.denoise(lat, enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), 1.0, prediction_type="v_prediction", rule=sch.rule,
              noise=noises.cuda() if rule == "ddpm" else None, latent_h=H_LOOP, guidance_table=np.full((N_LOOP, B_LOOP), 3.0, np.float32))
    assert torch.equal(lat.cpu(), d0)


def test_loop_argument_errors(lib):
    e = unet_engine("fp32")
    enc, mask, lat0, noises = loop_inputs()
    sch, _ = loop_sched("ddpm")
    sch.set_timesteps(N_LOOP)

    def call(guidance=3.0, **kw):
        e.denoise(lat0.clone().cuda(), enc.cuda(), mask.cuda(), sch.timesteps.numpy(), sch.coef_table(), guidance, latent_h=H_LOOP, **kw)

    with pytest.raises(ValueError):
        call(guidance_table=np.ones((N_LOOP, B_LOOP + 1), np.float32))
    with pytest.raises(ValueError):
        call(guidance_table=np.ones(B_LOOP, np.float32))
    with pytest.raises(ValueError):
        call(guidance_rescale=1.5)
    with pytest.raises(ValueError):
        call(guidance_table=np.array([[3, 1], [2, -1], [1, 1]], np.float32))
    with pytest.raises(ValueError):
        e.denoise(lat0.clone().cuda(), enc[B_LOOP:].cuda(), mask[B_LOOP:].cuda(), sch.timesteps.numpy(), sch.coef_table(), 1.0,
                  latent_h=H_LOOP, guidance_rescale=0.5)


# ---- string level -----------------------------------------------------------------------------------------------------------------------
class WhitespaceTokenizer:
    """Tokenizer double with the transformers call surface models.py uses"""
    model_max_length = 512
    pad_token_id, eos_token_id = 0, 1

    def __call__(self, texts, max_length=None, padding=True, truncation=True, return_tensors="pt"):
        rows = [[2 + (sum(ord(ch) * (i + 1) for i, ch in enumerate(w)) % 126) for w in t.split()] + [1] for t in texts]
        if truncation and max_length:
            rows = [r[:max_length] for r in rows]
        width = max_length if padding == "max_length" else max(len(r) for r in rows)
        ids = torch.zeros((len(rows), width), dtype=torch.long)
        am = torch.zeros((len(rows), width), dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            am[i, :len(r)] = 1
        return type("BatchEncoding", (), {"input_ids": ids, "attention_mask": am})()


def _tango():
    """the synthetic stack of the inpainting tests (tiny UNet, full VAE with encoder, vocoder, STFT) with a text side: a random
    tiny transformers T5 encoder and the tokenizer double"""
    if "tango" not in _cache:
        from transformers import T5Config, T5EncoderModel
        from oracle import stft_oracle as S
        from tango_amd.autoencoder import AutoencoderKL
        from tango_amd.models import AudioDiffusion
        from tango_amd.stft import TacotronSTFT
        from tango_amd.tango import Tango
        torch.manual_seed(111)
        t5 = T5EncoderModel(T5Config(vocab_size=128, d_model=O.UNET_CONFIG_TINY["cross_attention_dim"], d_kv=64, d_ff=128, num_layers=2,
                                     num_heads=2, feed_forward_proj="gated-gelu", tie_word_embeddings=False)).eval().cuda()
        model = AudioDiffusion(unet_config=O.UNET_CONFIG_TINY, dtype="fp16", text_encoder=t5, tokenizer=WhitespaceTokenizer())
        model.engine.load_synthetic(1234)
        vae = AutoencoderKL(ddconfig=dict(O.VAE_CONFIG, resolution=256, in_channels=1, double_z=True, attn_resolutions=[], dropout=0.0),
                            embed_dim=8, scale_factor=O.VAE_CONFIG["scale_factor"], dtype="fp16", with_encoder=True)
        vae.engine.load_synthetic(1234)
        _cache["tango"] = Tango.from_components(model, vae, stft=TacotronSTFT(**S.AUDIOLDM_STFT_CONFIG))
    return _cache["tango"]


PROMPT, NEG = "a dog barks twice", "low quality noise speech hiss hum clicks distortion"     # the negative prompt is the longer one


def hand_encoded(t, samples=1):
    """[T5(q); T5(p)] at the common length, made by hand"""
    tok, te = t.model.tokenizer, t.model.text_encoder
    nb = tok([NEG], max_length=512)
    cb = tok([PROMPT], max_length=nb.input_ids.shape[1], padding="max_length")
    assert nb.input_ids.shape[1] == 9 and int(cb.attention_mask.sum()) == 5
    with torch.no_grad():
        ne = te(input_ids=nb.input_ids.cuda(), attention_mask=nb.attention_mask.cuda())[0]
        ce = te(input_ids=cb.input_ids.cuda(), attention_mask=cb.attention_mask.cuda())[0]
    pe = torch.cat([ne.repeat_interleave(samples, 0), ce.repeat_interleave(samples, 0)]).float()
    pm = torch.cat([nb.attention_mask.repeat_interleave(samples, 0), cb.attention_mask.repeat_interleave(samples, 0)]) == 1
    return pe, pm.cuda()


def _clip():
    t = np.arange(2 * 16000) / 16000.0
    g = np.random.default_rng(17)
    return (0.3 * np.sin(2 * np.pi * 330 * t) + 0.05 * g.standard_normal(t.shape) + 0.1).astype(np.float32)


def test_tango_generate_negative_prompt(lib):
    t = _tango()
    pe, pm = hand_encoded(t)
    kw = dict(steps=3, guidance=3, duration=2.5)
    torch.manual_seed(21)
    w = t.generate(PROMPT, negative_prompt=NEG, **kw)
    torch.manual_seed(21)
    w_hand = t.generate_from_embeddings(pe, pm, **kw)[0]
    assert w.dtype == np.int16 and np.array_equal(w, w_hand) and np.abs(w.astype(np.float32)).max() > 0
    outs = []
    for extra in ({}, dict(negative_prompt=None), dict(negative_prompt="")):
        torch.manual_seed(21)
        outs.append(t.generate(PROMPT, **kw, **extra))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert not np.array_equal(outs[0], w), "the negative prompt changes the result"
    # rescale and a per-sample table reach the loop through the string path
    torch.manual_seed(21)
    wr = t.generate(PROMPT, negative_prompt=NEG, guidance_rescale=0.7, **kw)
    torch.manual_seed(21)
    wr_hand = t.generate_from_embeddings(pe, pm, guidance_rescale=0.7, **kw)[0]
    assert np.array_equal(wr, wr_hand) and not np.array_equal(wr, w)
    torch.manual_seed(21)
    w2 = t.generate(PROMPT, steps=3, guidance=[3.0, 6.0], samples=2, duration=2.5, negative_prompt=NEG)
    assert w2.shape == w.shape      # generate returns the first sample; row 0 has the scalar call's guidance but another batch's draws
    outs = t.generate_for_batch([PROMPT, "rain", "wind"], steps=2, guidance=np.array([3.0, 4.0, 5.0]), batch_size=2, duration=2.5,
                                negative_prompt=[NEG, "hiss", "hum"], guidance_rescale=0.5)
    assert len(outs) == 3 and all(o.dtype == np.int16 for o in outs)


def test_tango_edit_and_inpaint_negative_prompt(lib):
    t = _tango()
    pe, pm = hand_encoded(t)
    audio = _clip()
    kw = dict(strength=0.5, steps=4, guidance=3, samples=1, seed=5, duration=2.5)
    e1 = t.edit(PROMPT, audio, negative_prompt=NEG, **kw)
    e2 = t.edit_from_embeddings(pe, pm, audio, **kw)
    e0 = t.edit(PROMPT, audio, **kw)
    assert e1.dtype == np.int16 and np.array_equal(e1, e2) and not np.array_equal(e1, e0)
    kw = dict(steps=3, guidance=3, samples=1, duration=2.5)
    torch.manual_seed(31)
    i1 = t.inpaint(PROMPT, audio, negative_prompt=NEG, **kw)
    torch.manual_seed(31)
    i2 = t.inpaint_from_embeddings(pe, pm, audio, **kw)
    torch.manual_seed(31)
    i0 = t.inpaint(PROMPT, audio, **kw)
    assert i1.dtype == np.int16 and np.array_equal(i1, i2) and not np.array_equal(i1, i0)
