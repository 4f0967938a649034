"""bench.py's launch contract on CPU (no GPU call): --gpus N means N ranks."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_world_size_mismatch_fails_before_any_gpu_call():
    env = dict(os.environ, WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--gpus 2 but WORLD_SIZE=1" in r.stderr


def test_gpus_n_launches_n_ranks(monkeypatch):
    import bench
    seen = {}

    def fake_run(cmd, *a, **k):
        seen["cmd"] = cmd

        class R:
            returncode = 0
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    a = type("A", (), {"gpus": 4})()
    assert bench.launch_ranks(a) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")


def test_phases_needs_full_and_fails_before_any_gpu_call():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--phases"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--full" in r.stderr and r.stdout == ""


def test_dump_outputs_writes_float32_within_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import torch as th
    import bench
    small = th.arange(6, dtype=th.float32)
    big = th.arange(1000, dtype=th.float64).reshape(10, 100)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4 * 100)   # a share of 100 floats for each of the two
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(s, small.numpy())
    # the tensor past its share: a sample of its elements, in order, the same one in every run
    assert b.shape == (100,) and np.all(np.diff(b) > 0) and np.all(b == np.round(b)) and b.max() < 1000
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert s.nbytes + b.nbytes <= 2 * 4 * 100


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """A plain run: K timed steps, no survey / roofline / baselines, and --dump-outputs writes the last timed step's
    stats, parameters, optimiser state and gradient."""
    import json
    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["rollout_baseline"] is None
    assert d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    _, n, _, _, _, T, B, _ = __import__("bench").CONFIGS["cfg2"]
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 - B * T * n) <= 1e-6 * B * T * n
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["grad.npy", "params.npy", "square_avg.npy", "stats.npy", "target_params.npy"]
    assert all(v.dtype == np.float32 and v.ndim == 1 and np.isfinite(v).all() for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    P = got["params.npy"].size
    assert P > 0 and all(got[k].size == P for k in ("grad.npy", "square_avg.npy", "target_params.npy"))
    loss, grad_norm = got["stats.npy"][:2]
    assert got["stats.npy"].size >= 6 and loss > 0 and grad_norm > 0
    assert got["square_avg.npy"].min() >= 0 and got["square_avg.npy"].max() > 0
    assert np.abs(got["params.npy"] - got["target_params.npy"]).max() > 0   # 4 steps in: no target update yet


def test_stale_pmc_summary_is_not_reported(tmp_path, monkeypatch):
    import json
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "zz_pmc_cfg2.json").write_text(json.dumps({"source_sha256": "0" * 64,
                                                       "cfg2": {"gru_bwd": {"hbm_bytes_per_launch": 1e8}}}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_hash", lambda: "1" * 64)
    v, why = bench.pmc_traffic("cfg2", "gru_bwd")
    assert v is None and "stale" in why
    monkeypatch.setattr(bench, "kernel_source_hash", lambda: "0" * 64)
    v, why = bench.pmc_traffic("cfg2", "gru_bwd")
    assert v == 1e8 and "zz_pmc_cfg2.json" in why
