#!/usr/bin/env python
"""bench.py -- headline benchmark of the Tango hot path on MI355X (see BASELINE.json / DESIGN.md).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one full pass of the hot path over one batch per GPU: the CFG denoise loop
(`--denoise-steps` UNet+scheduler iterations, default 200) -> mel-VAE decode -> HiFi-GAN -> int16, for
`--batch` (default 32) synthetic 64-token prompts per GPU (BASELINE config 3: Tango-full, 200 steps,
batch 32, guidance 3).  Other BASELINE configs: `--batch 1 --denoise-steps 100` (config 2), `--xl --dtype bf16 --fp8-attn
--batch 8` (config 5's per-GPU shard); `config.workload` in the JSON line names what actually ran.  Inputs (text-encoder outputs, initial latents) are resident in HBM when the timed
region starts; weights are seeded synthetic tensors of the real architecture (no checkpoint offline).
Metric: audio-seconds generated per wall-second, whole job (all GPUs).  Weak scaling: per-GPU batch fixed.

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds what takes runs of its own: the CPU
oracle baseline, the other BASELINE configs and the fp32 pass (`other_configs`, `roofline.same_precision`, only for the
config-3 workload on one GPU), the text-encoder timing and the committed parity ladder (`parity`).  `--dump-outputs DIR`
writes the last timed step's waveforms as DIR/wav.npy (float32; a fixed, seeded sample of rows when above 64 MB).
"""
import argparse
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

#: BASELINE.md section 2 (FlopCounterMode on the reference modules, 64 text tokens, CFG on)
GFLOP_UNET_PER_PROMPT_STEP = 1606.36
GFLOP_VAE_PER_SAMPLE = 670.47
GFLOP_VOCODER_PER_SAMPLE = 1027.04
AUDIO_SECONDS_PER_SAMPLE = 163872 / 16000.0
PEAK_TFLOPS = {"fp16": 2500.0, "bf16": 2500.0, "fp32": 157.3}   # MI355X_MICROARCH.md dense MFMA peaks
#: HBM-side bytes of one denoise-step launch from rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE, KiB
#: units; separate --pmc runs, tools/final_profiles.sh): NOT measurable inside this process, so the number is read from
#: the committed evidence file named in profiles/hbm_traffic.json and the JSON line names that file next to it.


def hbm_traffic(batch, dtype, xl, fp8=False):
    """(bytes per denoise-step launch, evidence file) for THIS configuration, or (None, None): a record only counts when it was
    taken on the tree being benchmarked -- profiles/hbm_traffic.json names the library build it measured ("lib_sha16" = first 16
    hex digits of sha256(libtango_hip.so's kernel sources), tools/final_profiles.sh) and a stale record is not reported."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    except (OSError, ValueError):
        return None, None
    cur = kernel_source_sha16()
    for r in rec.get("records", []):
        if (r.get("batch") == batch and r.get("dtype") == dtype and bool(r.get("xl", False)) == bool(xl)
                and bool(r.get("fp8_attn", False)) == bool(fp8) and r.get("src_sha16") == cur):
            return float(r["bytes_per_step"]), r.get("source")
    return None, None


def kernel_source_sha16():
    """identity of the kernel sources the library was built from (csrc/*.hip, *.h in name order)"""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "tango_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def workload_name(args):
    """which BASELINE.json config (if any) this invocation is: the label must say what RAN, not what the default is"""
    std = abs(args.guidance - 3.0) < 1e-9 and args.text_len == 64
    if std and not args.xl and not args.fp8_attn and args.batch == 32 and args.denoise_steps == 200 and args.dtype == "fp16":
        return "BASELINE config 3"
    if std and not args.xl and not args.fp8_attn and args.batch == 1 and args.denoise_steps == 100 and args.dtype == "fp16":
        return "BASELINE config 2"
    if std and not args.xl and not args.fp8_attn and args.batch == 32 and args.denoise_steps == 200:
        return "BASELINE config 4's per-GPU shard (256 prompts / 8 GPUs) == config 3's shape, %s" % args.dtype
    if std and args.xl and args.fp8_attn and args.dtype == "bf16" and args.batch == 8 and args.denoise_steps == 200:
        return "BASELINE config 5's per-GPU shard (64 prompts / 8 GPUs)"
    return "custom (not a BASELINE.json config)"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1, help="timed passes of the hot path")
    ap.add_argument("--warmup", type=int, default=1, help="untimed passes")
    ap.add_argument("--batch", type=int, default=32, help="prompts per GPU")
    ap.add_argument("--denoise-steps", type=int, default=200)
    ap.add_argument("--guidance", type=float, default=3.0)
    ap.add_argument("--text-len", type=int, default=64)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--xl", action="store_true", help="FLAN-T5-XL cross-attention width (2048)")
    ap.add_argument("--fp8-attn", action="store_true", help="self-attention P.V on the fp8 MFMA (BASELINE config 5; 16-bit dtypes)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full: skip the `other_configs` sub-records (batch 1 / 8 and config 5's shard) a config-3 run at N = 1 appends")
    ap.add_argument("--full", action="store_true",
                    help="also measure the CPU baseline, other configs / precisions, text encoder and parity record (off: headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (the int16 waveforms as float32) to DIR/<name>.npy")
    return ap.parse_args()


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: re-exec this script under torch.distributed.run, one rank per GPU of this
    node (rendezvous on 127.0.0.1, a free port).  Rank 0 of the child job prints the JSON line; its exit code is returned."""
    import socket
    import subprocess
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def cpu_baseline(args, unet_cfg, vae_cfg, hifi_cfg, sched_cfg):
    """The CPU oracle (fp32 restatement of the reference path, kind "port") timed on this host's cores on a bounded sample:
    BASELINE config 1 IN FULL (B = 1, 10 CFG denoise steps of the full UNet + VAE decode + HiFi-GAN) --
    `config1_measured` is that run with no extrapolation; `value` prices the benchmarked workload (`--denoise-steps` steps) from
    the same run's measured per-step time."""
    from oracle import tango_oracle as O
    from tango_amd import weights as W
    usd = W.synth_state_dict(W.unet_param_shapes(unet_cfg, "unet."), args.seed)
    shapes = W.vae_decoder_param_shapes(vae_cfg)
    shapes.update(W.hifigan_param_shapes(hifi_cfg))
    vsd = W.synth_state_dict(shapes, args.seed)
    g = torch.Generator().manual_seed(0)
    enc = torch.randn(2, args.text_len, unet_cfg["cross_attention_dim"], generator=g)
    mask = torch.ones(2, args.text_len, dtype=torch.bool)
    mask[0, 1:] = False
    lat = torch.randn(1, 8, 256, 16, generator=g)
    n = int(os.environ.get("TANGO_BENCH_CPU_STEPS", "10"))
    sch = O.DDPMOracle(**sched_cfg)
    # thread-count sweep on one UNet forward: torch's default (= all hardware threads) oversubscribes the memory system on
    # big hosts (round 1: 8.25 s/step at 128 threads vs 2.7 s at 8) -- report the BEST the host can do, with its core count
    # (the all-hardware-threads point is gone -- round 5, VERDICT r4 weak #11: 161-165 s per forward on the 256-thread GPU box, twice,
    #  i.e. 330 s of the driver's run to re-learn that it loses by 50x; rounds 1-4 recorded it in profiles/*bench*.json)
    ncpu = os.cpu_count() or 1
    cands = sorted({c for c in (8, 16, 32, 64) if 1 <= c <= ncpu} or {ncpu})
    sweep = {}
    with torch.no_grad():
        O.unet_forward(usd, unet_cfg, torch.cat([lat] * 2), 999, enc, mask, prefix="unet.")   # page-in / thread-pool warm-up
        for c in cands:
            torch.set_num_threads(c)
            t0 = time.time()
            O.unet_forward(usd, unet_cfg, torch.cat([lat] * 2), 999, enc, mask, prefix="unet.")
            sweep[c] = time.time() - t0
        threads = min(sweep, key=sweep.get)
        torch.set_num_threads(threads)
        t0 = time.time()
        lat2 = O.denoise_loop(usd, unet_cfg, sch, enc, mask, lat, n, args.guidance, prefix="unet.")
        t1 = time.time()
        mel = O.vae_decode_first_stage(vsd, vae_cfg, lat2)
        t2 = time.time()
        O.decode_to_waveform(vsd, hifi_cfg, mel)
        t3 = time.time()
    t_step = (t1 - t0) / n
    total = t_step * args.denoise_steps + (t2 - t1) + (t3 - t2)
    return {
        "value": AUDIO_SECONDS_PER_SAMPLE / total, "unit": "audio-seconds/s", "cores": threads, "kind": "port",
        "config1_measured": {"value": AUDIO_SECONDS_PER_SAMPLE / (t3 - t0), "unit": "audio-seconds/s", "seconds": t3 - t0, "denoise_steps": n,
                             "batch": 1, "note": "BASELINE config 1 run in full on the host, no extrapolation"},
        "sample": "BASELINE config 1 in full -- B=1: %d full-UNet CFG steps (%.2f s/step) + VAE decode (%.2f s) + HiFi-GAN (%.2f s), fp32 torch CPU "
                  "oracle, best of a thread sweep %s (s per UNet forward) -> %d threads of %d, %s; `value` = the same per-step time at %d steps"
                  % (n, t_step, t2 - t1, t3 - t2, {k: round(v, 2) for k, v in sweep.items()}, threads, ncpu,
                     platform.processor() or platform.machine(), args.denoise_steps),
    }


def text_encoder_timing(args, device, batch, length):
    """"text-encoder time reported separately".  FLAN-T5-large (random init of the real architecture, fp32) on
    `batch` x `length` token ids: the frozen `transformers.T5EncoderModel` in PyTorch-ROCm (the default of row a2) and the same
    encoder on the engine (`tango_engine_encode_text`, row f1).  It runs once per pass, in front of the timed region."""
    from tango_amd import weights as W
    from tango_amd.text_encoder import T5EncoderOnEngine
    cfg = dict(W.T5_CONFIG_LARGE)
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(2, cfg["vocab_size"], (batch, length), generator=g).to(device)
    am = torch.ones(batch, length, dtype=torch.int64, device=device)
    rec = {"batch": batch, "tokens": length, "model": "flan-t5-large (24 blocks, d_model 1024; seeded random weights)", "dtype": "fp32"}

    def timeit(fn, reps=5):
        fn(); fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / reps

    try:
        enc = T5EncoderOnEngine(cfg, device=device)
        enc.engine.load_synthetic(args.seed)
        rec["engine_ms"] = timeit(lambda: enc(input_ids=ids, attention_mask=am)[0])
        del enc
    except Exception as e:  # noqa: BLE001  (a sub-record must not take the headline down)
        rec["engine_error"] = repr(e)[:200]
    try:
        from transformers import T5Config, T5EncoderModel
        c = T5Config(vocab_size=cfg["vocab_size"], d_model=cfg["d_model"], d_kv=cfg["d_kv"], d_ff=cfg["d_ff"], num_layers=cfg["num_layers"],
                     num_heads=cfg["num_heads"], feed_forward_proj="gated-gelu", dropout_rate=0.0,
                     relative_attention_num_buckets=cfg.get("relative_attention_num_buckets", 32))
        with torch.no_grad():
            m = T5EncoderModel(c).eval().to(device)
            rec["torch_ms"] = timeit(lambda: m(input_ids=ids, attention_mask=am)[0])
        del m
    except Exception as e:  # noqa: BLE001
        rec["torch_error"] = repr(e)[:200]
    torch.cuda.empty_cache()
    return rec


def parity_record():
    """the 16-bit parity ladder that belongs next to the throughput (tests/test_parity_chain_gpu.py writes it on the GPU with
    TANGO_WRITE_PARITY_RECORD; committed as profiles/parity_ladder.json): fp16 engine vs the fp32 oracle, end to end"""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "parity_ladder.json")))
    except (OSError, ValueError):
        return None
    out = {"source": "profiles/parity_ladder.json (tests/test_parity_chain_gpu.py: engine latents -> vae_decode -> vocode vs the fp32 CPU oracle)"}
    r = rec.get("fp16_b1_50step_chain") or rec.get("fp16_b2_20step_chain")
    if r:
        out.update({"fp16_mel_psnr_db": r["mel_psnr_db"], "fp16_wave_snr_db": r["wave_snr_db"], "lsb1_frac": r["lsb1_frac"],
                    "fp16_latents_max_abs_err": r["latents_max_abs_err"], "denoise_steps": r["denoise_steps"], "batch": r["batch"]})
    out["records"] = rec
    return out


class Workload:
    """One engine pair (UNet + VAE/vocoder) and the timed pass over it: the hot path for `batch` prompts per GPU."""

    def __init__(self, args, device, xl, dtype, fp8):
        from tango_amd.autoencoder import AutoencoderKL
        from tango_amd.engine import UNET_CONFIG_LARGE, UNET_CONFIG_XL, VAE_CONFIG
        from tango_amd.models import AudioDiffusion
        from tango_amd.tango import Tango
        self.unet_cfg = UNET_CONFIG_XL if xl else UNET_CONFIG_LARGE
        self.dtype = dtype
        self.model = AudioDiffusion(unet_config=self.unet_cfg, dtype=dtype, device=device, attn_fp8=fp8)
        self.model.engine.load_synthetic(args.seed)
        self.model.use_graph = not args.no_graph
        self.vae = AutoencoderKL(ddconfig=dict(VAE_CONFIG, attn_resolutions=[]), embed_dim=8, scale_factor=VAE_CONFIG["scale_factor"],
                                 dtype=dtype, device=device)
        self.vae.engine.load_synthetic(args.seed)
        self.tango = Tango.from_components(self.model, self.vae)
        self.device = device
        self.n_samples = self.vae.engine.vocoder_samples(1024)
        self.denoise_ms = []

    def compute(self, denoise_steps, guidance):
        def fn(pe, pm, offset, seed):
            b = pe.shape[0] // 2
            # initial latents keyed by the GLOBAL sample index (like the step noise): outputs do not depend on the GPU count
            lat = torch.stack([torch.randn(8, 256, 16, generator=torch.Generator(device="cpu").manual_seed(1000 + offset + i))
                               for i in range(b)]).to(self.device)
            latents = self.model.inference_from_embeddings(pe, pm, self.tango.scheduler, denoise_steps, guidance, latents=lat,
                                                           seed=seed, sample_offset=offset)
            mel = self.vae.decode_first_stage(latents)
            wav = self.vae.engine.vocode(mel)            # int16 stays on the device; the gather moves it (no host round trip)
            self.denoise_ms.append(self.model.engine.last_denoise_ms())
            return wav
        return fn


def synthetic_text(Bg, L, d, device):
    """synthetic text-encoder outputs: [uncond; cond], uncond mask = [1, 0, ...] (T5("") is one valid token)"""
    g = torch.Generator().manual_seed(7)
    cond = torch.randn(Bg, L, d, generator=g)
    unc = torch.randn(Bg, L, d, generator=g)
    mc = torch.ones(Bg, L, dtype=torch.bool)
    mu = torch.zeros(Bg, L, dtype=torch.bool)
    mu[:, 0] = True
    # the mask stays on the HOST, as a tokenizer hands it over: the engine then picks its plan without reading a device copy back
    # (with a device mask every denoise call started with a D2H copy + stream sync that the product path does not need)
    return torch.cat([unc, cond]).to(device), torch.cat([mu, mc])


def timed_single_gpu(wl, args, batch, denoise_steps, warm_steps=None):
    """one warm-up pass (of `warm_steps` denoise steps if given: plans and the captured step do not depend on the step count) + one
    timed pass of the hot path on THIS GPU only (the `other_configs` sub-records)"""
    from tango_amd.parallel import DataParallelGenerator
    dp = DataParallelGenerator(wl.compute(denoise_steps, args.guidance), wl.device)
    pe, pm = synthetic_text(batch, args.text_len, wl.unet_cfg["cross_attention_dim"], wl.device)
    if warm_steps is not None and warm_steps != denoise_steps:
        DataParallelGenerator(wl.compute(warm_steps, args.guidance), wl.device).generate(pe, pm, args.guidance, wl.n_samples, seed=args.seed)
    else:
        dp.generate(pe, pm, args.guidance, wl.n_samples, seed=args.seed)
    wl.denoise_ms.clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    wav = dp.generate(pe, pm, args.guidance, wl.n_samples, seed=args.seed)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert wav.shape == (batch, wl.n_samples)
    per_step_ms = float(np.mean([m[1] for m in wl.denoise_ms]))
    ach = GFLOP_UNET_PER_PROMPT_STEP * batch / per_step_ms
    peak = PEAK_TFLOPS[wl.dtype]
    rec = {"value": batch * AUDIO_SECONDS_PER_SAMPLE / dt, "unit": "audio-seconds/s", "batch": batch, "denoise_steps": denoise_steps,
           "dtype": wl.dtype, "seconds_per_pass": dt, "denoise_step_launch_ms": per_step_ms, "achieved_tflops": ach, "peak_tflops": peak,
           "roofline_frac": ach / peak}
    ex = wl.model.engine.last_step_gflop()
    if ex:
        rec["executed_gflop_per_launch"] = ex
    return rec


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, wav):
    """--dump-outputs: what the timed path hands its caller in its last step -- the global int16 waveforms [B, n_samples] -- as
    float32 `wav.npy`.  Above DUMP_LIMIT_BYTES a fixed, seeded sample of whole rows is written instead, with their row indices in
    `wav_rows.npy` (float64), so that two builds given the same arguments can be compared output for output."""
    os.makedirs(out_dir, exist_ok=True)
    wav = np.asarray(wav)
    row_bytes = 4 * int(np.prod(wav.shape[1:]))
    if wav.shape[0] * row_bytes > DUMP_LIMIT_BYTES:
        k = max(1, DUMP_LIMIT_BYTES // max(row_bytes, 1) - 1)
        rows = np.sort(np.random.default_rng(0).choice(wav.shape[0], size=k, replace=False))
        np.save(os.path.join(out_dir, "wav_rows.npy"), rows.astype(np.float64))
        wav = wav[rows]
    np.save(os.path.join(out_dir, "wav.npy"), wav.astype(np.float32))


def stub_main(args, world, rank):
    """TANGO_BENCH_STUB=1 (tests/test_bench_launch.py): the launch / rendezvous / sharding / gather / JSON plumbing of this
    script on CPU over gloo with a stand-in compute function.  Not a measurement: the line says "stub": true."""
    from tango_amd.parallel import DataParallelGenerator
    device = torch.device("cpu")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    n_samples = 64

    def compute(pe, pm, offset, seed):
        b = pe.shape[0] // 2
        return (torch.arange(b, dtype=torch.int16)[:, None] + offset).expand(b, n_samples).contiguous()

    dp = DataParallelGenerator(compute, device, timing=True)
    B, L, d = args.batch, args.text_len, 8
    Bg = B * world
    pe, pm = synthetic_text(Bg, L, d, device) if rank == 0 else (None, None)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        wav = dp.generate(pe, pm, args.guidance, n_samples, seed=args.seed)
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    stage = dp.timing_summary()
    if rank == 0:
        assert wav.shape == (Bg, n_samples) and (wav[:, 0] == np.arange(Bg)).all()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, wav)
        print(json.dumps({"metric": "stub", "stub": True, "value": Bg * args.steps / dt, "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "ms_per_step": 1000.0 * dt / args.steps, "ranks": world, "config": {"global_batch": Bg},
                          "per_rank_ms": stage["per_rank_ms"], "bcast_ms": stage["bcast_ms"], "gather_ms": stage["gather_ms"]}))
    if world > 1:
        dist.destroy_process_group()


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, "--gpus %d but the launcher started %d ranks" % (args.gpus, world)
    if os.environ.get("TANGO_BENCH_STUB"):
        return stub_main(args, world, rank)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # also when an external torchrun started the ranks (dmabuf IPC for RCCL)
    torch.cuda.set_device(local_rank)          # before the process group: RCCL binds its communicator to the current device
    device = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world)

    from tango_amd.engine import HIFIGAN_CONFIG, VAE_CONFIG
    from tango_amd.parallel import DataParallelGenerator
    from tango_amd.scheduler import SD21_SCHEDULER_CONFIG

    wl = Workload(args, device, args.xl, args.dtype, args.fp8_attn)
    unet_cfg, n_samples, denoise_ms = wl.unet_cfg, wl.n_samples, wl.denoise_ms
    B, L, d = args.batch, args.text_len, unet_cfg["cross_attention_dim"]
    Bg = B * world

    dp = DataParallelGenerator(wl.compute(args.denoise_steps, args.guidance), device, timing=True)
    pe = pm = None
    if rank == 0:
        pe, pm = synthetic_text(Bg, L, d, device)

    def one_pass():
        return dp.generate(pe, pm, args.guidance, n_samples, seed=args.seed)

    for _ in range(args.warmup):
        one_pass()
    denoise_ms.clear()
    if world > 1:
        dist.barrier(device_ids=[local_rank])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        wav = one_pass()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier(device_ids=[local_rank])
    dt = time.perf_counter() - t0
    rccl_ranks = world
    if world > 1:
        t = torch.tensor([dt, 1.0], device=device, dtype=torch.float64)
        dist.all_reduce(t[:1], op=dist.ReduceOp.MAX)
        dist.all_reduce(t[1:], op=dist.ReduceOp.SUM)     # every rank that took part in the job over RCCL
        dt, rccl_ranks = float(t[0].item()), int(round(float(t[1].item())))
    stage = dp.timing_summary()      # every rank: per-rank compute time, broadcast and gather time of the last timed pass

    if rank == 0:
        assert wav.shape == (Bg, n_samples) and wav.dtype == np.int16
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, wav)
        audio_s = Bg * AUDIO_SECONDS_PER_SAMPLE * args.steps
        per_step_ms = float(np.mean([m[1] for m in denoise_ms])) if denoise_ms else float("nan")
        # roofline of the dominant launch = one hipGraph replay of the UNet step (MFMA-bound):
        # algorithmic 1606.36 GFLOP per (prompt, step) x B prompts per launch / measured launch duration
        ach = GFLOP_UNET_PER_PROMPT_STEP * B / per_step_ms   # GFLOP / ms == TFLOP/s
        traffic, traffic_src = hbm_traffic(B, args.dtype, args.xl, args.fp8_attn)
        executed = wl.model.engine.last_step_gflop()     # GFLOP the engine's step program executes per launch (sum over its ops)
        out = {
            "metric": "audio-seconds generated/sec, Tango-full %d-step, batch=%d, guidance=%g" % (args.denoise_steps, B, args.guidance),
            "value": audio_s / dt, "unit": "audio-seconds/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1000.0 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic (seeded random weights of the real architecture; N(0,1) text embeddings)",
            "config": {"workload": "%s: Tango-full%s UNet (%s) %d-step DDPM CFG=%g denoise%s + mel-VAE decode + "
                                   "HiFi-GAN, %d prompts/GPU x %d tokens" % (workload_name(args), " XL" if args.xl else "", "891M" if args.xl else "866M", args.denoise_steps,
                                                                             args.guidance, " with fp8 P.V self-attention" if args.fp8_attn else "", B, L),
                       "global_batch": Bg, "text_len": L, "denoise_steps": args.denoise_steps, "parallelism": "dp%d" % world,
                       "rccl_ranks": rccl_ranks,
                       "hipgraph": not args.no_graph, "fp8_attention": bool(args.fp8_attn), "kernel_src_sha16": kernel_source_sha16()},
            # `achieved` counts the REFERENCE's algorithmic FLOPs (FlopCounterMode on its modules: what a drop-in must deliver per
            # launch); `executed_gflop` is what this engine's launch actually multiplies (the single-key path skips to_q / QK^T / PV /
            # to_out of the unconditional half's cross-attention, step-invariant K / V projections are hoisted out of the step):
            # `executed_tflops` / `executed_frac` price the kernels, `achieved` / `frac` price the job
            "roofline": {"bound": "mfma", "achieved": ach, "peak": PEAK_TFLOPS[args.dtype], "unit": "TFLOP/s",
                         "frac": ach / PEAK_TFLOPS[args.dtype], "achieved_counts": "algorithmic (reference) FLOPs",
                         "executed_gflop": executed, "executed_tflops": (executed / per_step_ms) if executed else None,
                         "executed_frac": (executed / per_step_ms / PEAK_TFLOPS[args.dtype]) if executed else None,
                         "traffic": traffic, "traffic_source": traffic_src,
                         "kernel": "denoise step (one hipGraph replay: UNet forward of %d prompts x 1606.36 GFLOP + fused CFG/scheduler update), %.2f ms/launch by HIP events"
                                   % (B, per_step_ms)},
            "end_to_end_tflops": (GFLOP_UNET_PER_PROMPT_STEP * args.denoise_steps + GFLOP_VAE_PER_SAMPLE + GFLOP_VOCODER_PER_SAMPLE)
                                 * Bg * args.steps / dt / 1000.0,
            # stages of the LAST timed pass as each rank saw them (host clock around device syncs): a straggler shows as
            # per_rank_ms.max - min, a slow collective as bcast_ms / gather_ms (no per-step collective exists)
            "per_rank_ms": stage["per_rank_ms"], "bcast_ms": stage["bcast_ms"], "gather_ms": stage["gather_ms"],
        }
        par = parity_record() if args.full and args.dtype == "fp16" else None
        if par:
            out["parity"] = par
        if args.full and world == 1 and not args.no_other_configs and workload_name(args) == "BASELINE config 3":
            # the other batch sizes north_star names, timed by the same process (one warm-up + one timed pass each, ~20 s in all):
            # sub-records only -- `value` above stays config 3
            oc = {}
            oc["config2_b1_100step_fp16"] = timed_single_gpu(wl, args, 1, 100)
            oc["b8_200step_fp16"] = timed_single_gpu(wl, args, 8, 200)
            del wl
            wl5 = Workload(args, device, True, "bf16", True)
            oc["config5_shard_xl_bf16_fp8attn_b8_200step"] = timed_single_gpu(wl5, args, 8, 200)
            del wl5
            # row g1 (round 6): the same shard with P.V on the MX instruction (v_mfma_scale_f32_16x16x128_f8f6f4, 128 keys per MFMA)
            wl5x = Workload(args, device, True, "bf16", 2)
            oc["config5_shard_xl_bf16_mxfp8attn_b8_200step"] = timed_single_gpu(wl5x, args, 8, 200)
            del wl5x
            # the reference's own arithmetic (fp32) at config 3's batch, a REAL 200-step pass (20-step warm-up builds the plans), priced
            # against the 157.3-TFLOP/s f32 MFMA peak -- the like-for-like record next to the fp16 headline
            wl32 = Workload(args, device, False, "fp32", False)
            r32 = timed_single_gpu(wl32, args, 32, 200, warm_steps=20)
            oc["config3_fp32_b32_200step"] = r32
            out["roofline"]["same_precision"] = {"value": r32["value"], "unit": "audio-seconds/s", "dtype": "fp32", "roofline_frac": r32["roofline_frac"],
                                                 "denoise_step_launch_ms": r32["denoise_step_launch_ms"], "peak_tflops": r32["peak_tflops"],
                                                 "note": "BASELINE config 3 in the reference's own precision (models.py:224-249 runs fp32): full 200-step pass, no extrapolation"}
            del wl32
            out["text_encoder_ms"] = text_encoder_timing(args, device, 32, args.text_len)
            out["other_configs"] = oc
        if args.full and world == 1 and not args.no_cpu_baseline:
            keys = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "prediction_type", "clip_sample", "variance_type")
            out["cpu_baseline"] = cpu_baseline(args, unet_cfg, VAE_CONFIG, HIFIGAN_CONFIG, {k: SD21_SCHEDULER_CONFIG[k] for k in keys})
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
