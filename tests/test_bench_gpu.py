"""bench.py on the device at --gpus 1: a plain run does what its headline figure needs and nothing else, `--full` adds
the CPU baseline to the same line."""
import json
import os
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
OVERHEAD_BOUND_S = 30.0          # a plain run outside its warm-up and timed steps, whole process from start to exit


def _bench(*args, timeout=600):
    """-> (the JSON line, seconds from starting the process to its exit)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    if torch.cuda.is_initialized():
        torch.cuda.empty_cache()             # the headline ring takes 173 GB: hand back what earlier tests left cached
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    return json.loads(lines[0]), wall


def test_plain_headline_run_is_lean():
    """The headline workload (4096 actors, history 2000) as every pull request's plain run starts it: the whole process
    less its (steps + warmup) x ms_per_step stays within OVERHEAD_BOUND_S, and the line carries no CPU baseline."""
    steps, warmup = 5, 2
    out, wall = _bench("--steps", str(steps), "--warmup", str(warmup))
    assert all(k in out for k in HEADLINE_KEYS) and out["value"] > 0 and out["higher_is_better"] is True
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert "cpu_baseline" not in out
    assert out["roofline"]["launches"] > 0               # HIP-event timed inside the timed steps: no run of its own
    outside = wall - (steps + warmup) * out["ms_per_step"] * 1e-3
    print("plain run: %.1f s in all, %.2f ms per step, %.1f s outside its steps" % (wall, out["ms_per_step"], outside))
    assert outside <= OVERHEAD_BOUND_S, (wall, out["ms_per_step"], outside)


def test_full_adds_the_cpu_baseline_to_the_same_line():
    small = ("--steps", "2", "--warmup", "1", "--actors", "64", "--history", "60")
    plain, _ = _bench(*small)
    full, _ = _bench(*small, "--full", "--cpu-seconds", "2", "--cpu-threads", "2")
    assert "cpu_baseline" not in plain
    assert set(full) == set(plain) | {"cpu_baseline"}
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert full[k] == plain[k], k
    cb = full["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "env-steps/s" and cb["cores"] == 2 and cb["value"] > 0
    assert [r["threads"] for r in cb["by_threads"]][:2] == [1, 2] and all(r["env_steps"] > 0 for r in cb["by_threads"])
    skipped, _ = _bench(*small, "--full", "--no-cpu-baseline")
    assert "cpu_baseline" not in skipped
