"""bench.py --dump-outputs: the files by which two builds of the project are compared output for output - what they hold, how
large they may get, and that the same arguments give the same inputs (weights, batch, cotangents, dropout masks) in every run."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(str(d), "*.npy")))}


def test_dump_outputs_names_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    import bench
    g = torch.Generator().manual_seed(0)
    m = torch.nn.Linear(300, 200)
    m.weight.grad = torch.randn(200, 300, generator=g)          # (the bias has no gradient: no file)
    out = {"cls": [torch.randn(50, 400, generator=g).half(), None], "ids": torch.arange(7), "loss": torch.tensor(1.5)}
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 4000)   # four arrays: 1000 float32 elements each
    bench.dump_outputs(str(tmp_path / "a"), out, m)
    a = _load(tmp_path / "a")
    assert sorted(a) == ["grad.weight", "out_cls_0", "out_ids", "out_loss"]
    assert a["out_ids"].dtype == np.float64 and a["out_ids"].tolist() == list(range(7))
    assert a["out_loss"].dtype == np.float32 and a["out_loss"].tolist() == [1.5]
    for k, full in (("grad.weight", m.weight.grad), ("out_cls_0", out["cls"][0])):
        assert a[k].dtype == np.float32 and a[k].shape == (1000,)
        assert np.isin(a[k], full.float().numpy()).all()
    assert sum(v.nbytes for v in a.values()) <= 4 * 4000
    # the sample sits at the same positions whatever the values are
    m.weight.grad = m.weight.grad * 2
    out["cls"][0] = out["cls"][0] * 2
    bench.dump_outputs(str(tmp_path / "b"), out, m)
    b = _load(tmp_path / "b")
    assert np.array_equal(b["grad.weight"], 2 * a["grad.weight"]) and np.array_equal(b["out_cls_0"], 2 * a["out_cls_0"])


@pytest.mark.gpu
def test_two_runs_with_the_same_arguments_dump_the_same_step(tmp_path):
    """the timed path of the default mode (HIP-graph replay, fp16, train-mode dropout) twice: K timed steps as asked for, the same
    files both times, every array finite and the two runs equal up to the order of floating-point sums - a different batch,
    cotangent or dropout draw would move the logits by their own size"""
    runs = []
    for tag in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
               "--no-roofline", "--no-secondary", "--no-cpu-baseline", "--no-extra-step", "--no-repeat",
               "--dump-outputs", str(tmp_path / tag)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["step_mode"].startswith("hip_graph_replay"), d
        runs.append(_load(tmp_path / tag))
        assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / tag / "*"))) <= 64 * 10 ** 6
    a, b = runs
    assert sorted(a) == sorted(b)
    assert {"out_verb", "out_noun", "out_action", "out_audio", "out_feats"} <= set(a)
    import bench
    from tim_amd.config import named_config
    names = [k for k, _ in bench.build_model(named_config("C2a"), "fp16", "cpu")[0].named_parameters()]
    # every parameter got its gradient, but for the MLP of the auxiliary DRLoc loss, which the fixed-cotangent step does not run
    assert sorted(k[5:] for k in a if k.startswith("grad.")) == sorted(k for k in names if not k.startswith("drloc_mlp."))
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == b[k].shape and a[k].size > 0, k
        assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), k
        assert np.abs(a[k] - b[k]).max() <= 1e-3 * max(np.abs(a[k]).max(), 1e-30), k
    assert np.abs(a["out_action"]).max() > 0
