"""bench.py's result line: a plain run carries the headline figure and nothing that takes a run of its own; --full adds the
other measurements to the same line."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "step_mode", "config"}
# what only --full measures: eager steps and their per-launch events, extra steps, other modes / configurations, the host's oracle
FULL_ONLY = {"eager", "roofline", "non_gemm", "forward_only", "graph_replay", "comm", "parity", "bf16_mode", "c2a_b8", "c2a_train",
             "c2b", "c1", "c3", "c4_train", "cpu_baseline"}


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"] + list(args)
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_full_is_an_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_is_the_timed_steps_and_the_line():
    """the flagship step (C2a, 64 windows, fp16, HIP-graph replay) as every plain run times it: the headline keys, no leg that
    --full owns, and at most 30 s of the process's life outside its warm-up and timed steps"""
    d, wall = _bench()
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d), sorted(d)
    assert d["steps"] == 5 and d["warmup"] == 2 and d["step_mode"].startswith("hip_graph_replay"), d
    assert d["unit"] == "interval-queries/s" and d["higher_is_better"] is True and d["dtype"] == "fp16"
    assert d["value"] > 0 and abs(d["value"] - 64 * 25 / (d["ms_per_step"] / 1e3)) / d["value"] < 1e-2
    assert d["repeat_ms"] == [d["ms_per_step"]]          # the timed set only
    assert wall - (5 + 2) * d["ms_per_step"] / 1e3 <= 30.0, wall


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements():
    """--full on one GPU (less its two slowest legs, the secondary configurations and the host's oracle): the same headline keys,
    and the eager steps, the roofline events of their last step, the repeat sets and the forward-only loop beside them"""
    d, _ = _bench("--full", "--no-secondary", "--no-cpu-baseline")
    assert HEADLINE <= set(d) and {"eager", "roofline", "non_gemm", "forward_only"} <= set(d), sorted(d)
    assert d["step_mode"].startswith("hip_graph_replay") and d["eager"]["ms_per_step"] > 0
    # the 51 launches of the encoder layers (tests/test_gpu_bench_ranks.py) + the two outside them that reach the events' 1e10-FLOP
    # threshold at 64 windows, as in the recorded lines (BENCH_r06.json)
    assert d["roofline"]["launches_timed"] == 53 and d["roofline"]["achieved"] > 0 and d["roofline"]["per_shape_isolated"]
    assert len(d["repeat_ms"]) == 5 and d["repeat_ms"][0] == d["ms_per_step"]
    assert not {"parity", "bf16_mode", "c2b", "cpu_baseline"} & set(d)
