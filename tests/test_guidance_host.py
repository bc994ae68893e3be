"""Negative prompts, guidance tables and guidance rescale: everything that needs no GPU -- the classifier-free text encoder with a
negative prompt (bare AudioDiffusion, whitespace tokenizer double, tiny T5), the guidance-table helper, the engine's argument checks
through tango_debug_denoise_guided_check, the Tango / data-parallel refusals and the C ABI."""
import ctypes as C
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tango_amd import _lib
from tango_amd.models import AudioDiffusion, MusicAudioDiffusion
from tango_amd.scheduler import (SD21_SCHEDULER_CONFIG, DDPMScheduler, cfg_enabled, check_guidance_rescale, guidance_is_table,
                                 guidance_table)
from tango_amd.tango import Tango

_DDPM_KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")


class WhitespaceTokenizer:
    """Tokenizer double with the transformers call surface models.py uses: one id per word, then EOS"""
    model_max_length = 512
    pad_token_id, eos_token_id = 0, 1

    def __init__(self, vocab_size=128):
        self.vocab_size = vocab_size
        self.calls = []

    def _ids(self, text):
        return [2 + (sum(ord(ch) * (i + 1) for i, ch in enumerate(w)) % (self.vocab_size - 2)) for w in text.split()] + [self.eos_token_id]

    def __call__(self, texts, max_length=None, padding=True, truncation=True, return_tensors="pt"):
        self.calls.append((list(texts), max_length, padding))
        rows = [self._ids(t) for t in texts]
        if truncation and max_length:
            rows = [r[:max_length] for r in rows]
        width = max_length if padding == "max_length" else max(len(r) for r in rows)
        ids = torch.full((len(rows), width), self.pad_token_id, dtype=torch.long)
        am = torch.zeros((len(rows), width), dtype=torch.long)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = torch.tensor(r)
            am[i, :len(r)] = 1
        return SimpleNamespace(input_ids=ids, attention_mask=am)


def tiny_t5(seed=5):
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(seed)
    return T5EncoderModel(T5Config(vocab_size=128, d_model=32, d_kv=16, d_ff=64, num_layers=1, num_heads=2,
                                   feed_forward_proj="gated-gelu", tie_word_embeddings=False)).eval()


@pytest.fixture(scope="module")
def model():
    """an AudioDiffusion without an engine: only the text side is exercised"""
    m = AudioDiffusion.__new__(AudioDiffusion)
    m.device = torch.device("cpu")
    m.text_encoder, m.tokenizer, m._text_sd, m.bucket_text_len = tiny_t5(), WhitespaceTokenizer(), None, True
    return m


def todays_encoder(m, prompt, n):
    """_encode_text_classifier_free as it was before negative prompts (models.py:266-305 of the reference, plus the host mask)"""
    batch = m.tokenizer(prompt, max_length=m.tokenizer.model_max_length, padding=True, truncation=True, return_tensors="pt")
    with torch.no_grad():
        pe = m.text_encoder(input_ids=batch.input_ids, attention_mask=batch.attention_mask)[0].repeat_interleave(n, 0)
    ub = m.tokenizer([""] * len(prompt), max_length=pe.shape[1], padding="max_length", truncation=True, return_tensors="pt")
    with torch.no_grad():
        ne = m.text_encoder(input_ids=ub.input_ids, attention_mask=ub.attention_mask)[0].repeat_interleave(n, 0)
    host = torch.cat([ub.attention_mask.repeat_interleave(n, 0), batch.attention_mask.repeat_interleave(n, 0)]) == 1
    return torch.cat([ne, pe]), host


PROMPTS = ["a dog barks twice", "rain"]


# ---- encoder ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_encoder_default_is_todays(model, n):
    want_e, want_m = todays_encoder(model, PROMPTS, n)
    for got in (model._encode_text_classifier_free(PROMPTS, n), model._encode_text_classifier_free(PROMPTS, n, None),
                model._encode_text_classifier_free(PROMPTS, n, negative_prompt=None)):
        pe, pm, host = got
        assert torch.equal(pe, want_e) and torch.equal(pm, want_m) and torch.equal(host, want_m)
        assert host.dtype == torch.bool and not host.is_cuda
        assert host[:len(PROMPTS) * n].sum(1).tolist() == [1] * (len(PROMPTS) * n)      # T5(""): one key -> the single-key plan
    pe2, pm2 = model.encode_text_classifier_free(PROMPTS, n)
    assert torch.equal(pe2, want_e) and torch.equal(pm2, want_m)
    # the empty negative prompt is the same batch: same ids, same mask
    pe3, pm3, host3 = model._encode_text_classifier_free(PROMPTS, n, "")
    assert torch.equal(pe3, want_e) and torch.equal(pm3, want_m) and torch.equal(host3, want_m)


def test_encoder_long_negative_is_not_truncated(model):
    neg = "low quality noise speech hiss hum clicks distortion"          # 8 words + EOS = 9 > the prompts' 5
    pe, pm, host = model._encode_text_classifier_free(PROMPTS, 1, neg)
    assert pe.shape[0] == 4 and pe.shape[1] == 9 and pm.shape == (4, 9)
    assert host[:2].sum(1).tolist() == [9, 9] and host[2:].sum(1).tolist() == [5, 2]
    tok = WhitespaceTokenizer()
    nb = tok([neg, neg], max_length=512)
    cb = tok(PROMPTS, max_length=9, padding="max_length")
    with torch.no_grad():
        ne = model.text_encoder(input_ids=nb.input_ids, attention_mask=nb.attention_mask)[0]
        ce = model.text_encoder(input_ids=cb.input_ids, attention_mask=cb.attention_mask)[0]
    assert torch.equal(pe, torch.cat([ne, ce])), "order is [negative; cond], each half encoded at the common length"
    assert torch.equal(host, torch.cat([nb.attention_mask, cb.attention_mask]) == 1)


def test_encoder_short_negative_is_padded_to_the_prompt(model):
    pe, pm, host = model._encode_text_classifier_free(PROMPTS, 1, "hiss hum")
    assert pe.shape[1] == 5 and host[:2].sum(1).tolist() == [3, 3] and host[2:].sum(1).tolist() == [5, 2]
    assert torch.equal(pm, host)


def test_encoder_str_list_order_and_repeat(model):
    negs = ["hiss", "low quality speech"]
    a = model._encode_text_classifier_free(PROMPTS, 2, negs)
    assert a[0].shape[0] == 8
    one = [model._encode_text_classifier_free(PROMPTS, 1, negs)[i] for i in range(3)]
    # repeat_interleave inside each half: rows [n0, n0, n1, n1, c0, c0, c1, c1]
    idx = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3])
    for got, base in zip(a, one):
        assert torch.equal(got, base[idx])
    # a str is that text for every prompt
    s = model._encode_text_classifier_free(PROMPTS, 1, "hiss")
    lst = model._encode_text_classifier_free(PROMPTS, 1, ["hiss", "hiss"])
    for x, y in zip(s, lst):
        assert torch.equal(x, y)
    # the list is per prompt: swapping it swaps the negative rows only
    sw = model._encode_text_classifier_free(PROMPTS, 1, negs[::-1])
    assert torch.equal(sw[2][:2], one[2][:2].flip(0)) and torch.equal(sw[2][2:], one[2][2:])
    for bad in (["hiss"], ["a", "b", "c"], []):
        with pytest.raises(ValueError):
            model._encode_text_classifier_free(PROMPTS, 1, bad)


# ---- the table helper -----------------------------------------------------------------------------------------------------------------
def test_guidance_table_helper():
    for scalar in (3, 3.0, np.float32(2.5), np.array(4.0), torch.tensor(1.5)):
        assert guidance_table(scalar, 4, 3) is None and not guidance_is_table(scalar)
    assert cfg_enabled(3) and not cfg_enabled(1.0) and not cfg_enabled(torch.tensor(0.5)) and cfg_enabled([0.0, 0.0])
    for row in ([3, 1, 7.5], (3, 1, 7.5), np.array([3, 1, 7.5]), torch.tensor([3, 1, 7.5], dtype=torch.float64)):
        t = guidance_table(row, 4, 3)
        assert t.dtype == np.float32 and t.shape == (4, 3) and t.flags["C_CONTIGUOUS"]
        assert all(np.array_equal(t[i], np.array([3, 1, 7.5], np.float32)) for i in range(4))
    full = np.arange(12, dtype=np.float64).reshape(4, 3) / 2
    t = guidance_table(full, 4, 3)
    assert t.dtype == np.float32 and np.array_equal(t, full.astype(np.float32))
    assert np.array_equal(guidance_table(torch.from_numpy(full), 4, 3), t)
    assert guidance_table([0.0, 1.0, 0.0], 2, 3).tolist() == [[0, 1, 0], [0, 1, 0]]
    for bad in ([3, 1], np.zeros((3, 4)), np.zeros((4, 3, 1)), np.zeros((1, 3)), np.zeros((4, 1))):
        with pytest.raises(ValueError):
            guidance_table(bad, 4, 3)
    for bad in ([3, -1, 2], [3, float("nan"), 2], [3, float("inf"), 2]):
        with pytest.raises(ValueError):
            guidance_table(bad, 4, 3)


# ---- the engine's refusals, without a GPU ---------------------------------------------------------------------------------------------
def _check(lib, guidance_scale=3.0, table=None, rescale=0.0, steps=2, batch=2, **fields):
    a = _lib.DenoiseArgs()
    a.num_steps, a.batch, a.guidance_scale = steps, batch, guidance_scale
    for k, v in fields.items():
        setattr(a, k, v)
    g = _lib.GuidanceArgs()
    keep = np.ascontiguousarray(table, dtype=np.float32) if table is not None else None
    g.table = keep.ctypes.data if keep is not None else None
    g.rescale = rescale
    return lib.tango_debug_denoise_guided_check(C.byref(a), C.byref(g)).decode()


def test_guided_refusals(lib):
    assert _check(lib) == "" and _check(lib, rescale=0.7) == "" and _check(lib, rescale=1.0) == ""
    assert _check(lib, guidance_scale=1.0, table=[[0, 1], [2, 3]], rescale=0.5) == "", "a table is guidance: rescale is allowed"
    assert lib.tango_debug_denoise_guided_check(C.byref(_lib.DenoiseArgs(num_steps=1, batch=1)), None).decode() == ""
    for r in (-0.1, 1.5, float("nan"), float("inf")):
        assert "rescale must be in [0, 1]" in _check(lib, rescale=r)
    for gs in (1.0, 0.0):
        assert "rescale needs classifier-free guidance" in _check(lib, guidance_scale=gs, rescale=0.5)
    for bad in (-1.0, float("nan"), float("inf")):
        assert "finite and >= 0" in _check(lib, table=[[3, 1], [2, bad]])
    # tango_engine_denoise's own checks still speak
    assert "num_steps must be positive" in _check(lib, steps=0)
    assert "unknown rule" in _check(lib, rule=7)


def test_python_rescale_checks():
    assert check_guidance_rescale(3, 0) == 0.0 and check_guidance_rescale(3, 0.7) == pytest.approx(0.7)
    assert check_guidance_rescale([1.0, 0.5], 1.0) == 1.0
    for g, r in ((3, -0.1), (3, 1.01), (3, float("nan")), (1.0, 0.5), (0, 0.5), (torch.tensor(1.0), 0.2)):
        with pytest.raises(ValueError):
            check_guidance_rescale(g, r)


# ---- Tango and the data-parallel path -------------------------------------------------------------------------------------------------
def _bare_tango():
    sch = DDPMScheduler.from_config({k: SD21_SCHEDULER_CONFIG[k] for k in _DDPM_KEYS})
    return Tango.from_components(SimpleNamespace(), SimpleNamespace(), scheduler=sch)


def test_tango_argument_checks():
    t = _bare_tango()
    audio = np.zeros(16000, dtype=np.float32)
    for kw in (dict(guidance_rescale=-0.5), dict(guidance_rescale=1.5), dict(guidance=1.0, guidance_rescale=0.5),
               dict(guidance=0.5, guidance_rescale=1.0)):
        with pytest.raises(ValueError):
            t.generate("rain", steps=3, **kw)
        with pytest.raises(ValueError):
            t.generate_for_batch(["rain"], steps=3, **kw)
        with pytest.raises(ValueError):
            t.generate_for_batch_dp(["rain"], steps=3, **kw)
        with pytest.raises(ValueError):
            t.inpaint("rain", audio, steps=3, **kw)
        with pytest.raises(ValueError):
            t.edit("rain", audio, steps=10, **kw)
    with pytest.raises(ValueError, match="negative_prompt"):
        t.generate_for_batch(["rain", "wind"], steps=3, negative_prompt=["hiss"])
    with pytest.raises(ValueError, match="guidance table"):
        t.generate_for_batch(["rain", "wind"], steps=3, samples=2, guidance=np.array([3.0, 4.0]))


def test_dp_refuses_a_table():
    t = _bare_tango()
    for table in ([3.0, 5.0], np.full((3, 2), 3.0), torch.tensor([3.0, 5.0])):
        with pytest.raises(ValueError, match="table"):
            t.generate_for_batch_dp(["rain", "wind"], steps=3, guidance=table)


def test_per_batch_slices():
    s = Tango._slice_per_batch
    assert s(["a", "b", "c"], 1, 2) == ["b", "c"] and s("x", 1, 2) == "x" and s(None, 0, 2) is None and s(3.0, 2, 2) == 3.0
    g = np.arange(6.0)
    assert s(g, 1, 1, 2).tolist() == [2, 3] and s(np.stack([g, g + 10]), 2, 1, 2).tolist() == [[4, 5], [14, 15]]


def test_generate_and_save_passes_new_keywords_only_when_set(tmp_path):
    from tango_amd.batch_inference import generate_and_save, parse_args
    seen = []

    class Old:                                     # a duck-typed generator from before these keywords
        def generate_for_batch(self, prompts, steps, guidance, samples, batch_size):
            seen.append("old")
            return [np.zeros(16, np.int16) for _ in prompts]

    class New:
        def generate_for_batch(self, prompts, steps, guidance, samples, batch_size, **kw):
            seen.append(kw)
            return [np.zeros(16, np.int16) for _ in prompts]

    generate_and_save(Old(), ["a"], 2, 3, out_root=str(tmp_path), exp_id="x")
    generate_and_save(New(), ["a"], 2, 3, out_root=str(tmp_path), exp_id="y")
    generate_and_save(New(), ["a"], 2, 3, out_root=str(tmp_path), exp_id="z", negative_prompt="hiss", guidance_rescale=0.7)
    assert seen == ["old", {}, {"negative_prompt": "hiss", "guidance_rescale": 0.7}]
    a = parse_args(["--model", "m", "--negative_prompt", "low quality", "--guidance_rescale", "0.5"])
    assert a.negative_prompt == "low quality" and a.guidance_rescale == 0.5
    assert parse_args(["--model", "m"]).negative_prompt == ""


def test_predict_passes_negative_prompt(tmp_path):
    from tango_amd.predict import Predictor
    calls = []

    class Gen:
        def generate(self, prompt, steps, guidance, **kw):
            calls.append(kw)
            return np.zeros(16, np.int16)

    p = Predictor()
    p.models = {"tango2": Gen()}
    p.predict("rain", "tango2", 2, 3.0, out=str(tmp_path / "a.wav"))
    p.predict("rain", "tango2", 2, 3.0, negative_prompt="hiss", out=str(tmp_path / "b.wav"))
    assert calls == [{}, {"negative_prompt": "hiss"}]


# ---- surface and ABI ------------------------------------------------------------------------------------------------------------------
def test_keywords_exist_everywhere():
    def has(fn, *names):
        ps = inspect.signature(fn).parameters
        return all(n in ps for n in names)

    for fn in (AudioDiffusion.inference, AudioDiffusion.inpaint, AudioDiffusion.edit, Tango.generate, Tango.generate_for_batch,
               Tango.generate_for_batch_dp, Tango.inpaint, Tango.edit):
        assert has(fn, "negative_prompt", "guidance_rescale"), fn
    for cls in (AudioDiffusion, MusicAudioDiffusion):
        for name in ("inference_from_embeddings", "inpaint_from_embeddings", "edit_from_embeddings"):
            assert has(getattr(cls, name), "guidance_rescale"), (cls, name)
    assert has(AudioDiffusion._denoise, "guidance_rescale")
    assert has(AudioDiffusion._encode_text_classifier_free, "negative_prompt")
    assert has(AudioDiffusion.encode_text_classifier_free, "negative_prompt")
    from tango_amd.engine import Engine
    assert has(Engine.denoise, "guidance_table", "guidance_rescale")


def test_abi(lib):
    assert _lib.DenoiseArgs._fields_[-1][0] == "latent_h" and len(_lib.DenoiseArgs._fields_) == 30
    assert [f[0] for f in _lib.GuidanceArgs._fields_] == ["table", "rescale"]
    assert C.sizeof(_lib.GuidanceArgs) == 16 and _lib.GuidanceArgs.rescale.offset == 8
    for s in ("tango_engine_denoise", "tango_engine_denoise_guided", "tango_debug_denoise_guided_check", "tango_op_sched_guided"):
        assert hasattr(lib, s) and s in _lib.SYMBOLS
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib.__file__), "..", "include", "tango_engine.h")).read()
    for s in ("tango_guidance_args_t", "tango_engine_denoise_guided", "tango_debug_denoise_guided_check", "tango_op_sched_guided"):
        assert s in header
