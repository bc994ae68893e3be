"""bench.py's launch contract on CPU: `python bench.py --gpus N` with no launcher around it must re-exec
itself under torch.distributed.run (one rank per GPU, rendezvous on 127.0.0.1) and still print exactly ONE JSON line from rank 0;
under a launcher (WORLD_SIZE set) it must not re-exec.  TANGO_BENCH_STUB=1 swaps the engine for a stand-in compute function and
RCCL for gloo: what runs here is the launch / sharding / gather / JSON plumbing, not a measurement."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, extra_env=None):
    env = dict(os.environ, TANGO_BENCH_STUB="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    return json.loads(lines[0])


def test_bench_self_launches_for_gpus_2():
    out = _run([sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "0", "--batch", "3"])
    assert out["stub"] is True and out["n_gpus"] == 2 and out["ranks"] == 2 and out["steps"] == 2
    assert out["config"]["global_batch"] == 6          # weak scaling: 3 prompts per rank
    # the line shows a straggler rank or a slow collective, not one number
    pr = out["per_rank_ms"]
    assert len(pr["all"]) == 2 and 0.0 <= pr["min"] <= pr["max"] and out["bcast_ms"] >= 0.0 and out["gather_ms"] >= 0.0


def test_bench_single_process_default():
    out = _run([sys.executable, "bench.py", "--steps", "1", "--warmup", "0", "--batch", "2"])
    assert out["n_gpus"] == 1 and out["config"]["global_batch"] == 2


def test_bench_under_an_external_launcher_does_not_relaunch():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(port), "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0", "--batch", "1"])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 2


def test_bench_dump_outputs_and_ms_per_step(tmp_path):
    """--dump-outputs DIR writes the last timed step's waveforms as float32 DIR/wav.npy, identical across runs with the same
    arguments; --steps sets the timed steps and the line carries ms_per_step"""
    import numpy as np
    dumps = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        out = _run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--batch", "2", "--dump-outputs", str(d)])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0.0
        w = np.load(d / "wav.npy")
        assert w.dtype == np.float32 and w.shape == (2, 64) and (w[:, 0] == np.arange(2)).all()
        dumps.append(w)
    assert np.array_equal(dumps[0], dumps[1])


def test_bench_dump_outputs_samples_rows_above_the_limit(tmp_path, monkeypatch):
    """above 64 MB the dump is a fixed, seeded sample of whole rows, with their indices"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 4 * 8)
    wav = (np.arange(40, dtype=np.int16)[:, None] + np.zeros((1, 8), np.int16))
    for run in range(2):
        bench.dump_outputs(str(tmp_path / str(run)), wav)
    a, rows = np.load(tmp_path / "0" / "wav.npy"), np.load(tmp_path / "0" / "wav_rows.npy")
    assert a.dtype == np.float32 and rows.dtype == np.float64 and a.nbytes <= bench.DUMP_LIMIT_BYTES
    assert len(rows) == a.shape[0] > 0 and (a[:, 0] == rows).all() and (np.diff(rows) > 0).all()
    assert np.array_equal(a, np.load(tmp_path / "1" / "wav.npy"))
