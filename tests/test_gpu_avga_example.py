"""examples/train_ave_synthetic.py runs at its --tiny shape: an AVE-shaped model with the AVGA pooling on the device route
trains for a few steps on one fixed batch; the loss is finite and goes down."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_ave_synthetic_example_trains(monkeypatch):
    from tim_amd import avga
    monkeypatch.delenv("TIM_AMD_AVGA", raising=False)
    calls = []
    real = avga.pool_forward
    monkeypatch.setattr(avga, "pool_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    import train_ave_synthetic
    hist = train_ave_synthetic.main(["--tiny", "--steps", "12", "--batch", "8", "--windows", "8"])
    assert len(hist) == 12 and all(math.isfinite(x) for x in hist)
    assert sum(hist[-3:]) / 3 < 0.9 * hist[0]
    assert len(calls) >= 12                     # the pooling went through the device route at every step
