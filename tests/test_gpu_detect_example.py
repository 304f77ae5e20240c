"""examples/detect_synthetic.py runs: synthetic windows through the detection model and the collector, detections per video."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_detect_synthetic_example_returns_detections():
    import detect_synthetic
    res = detect_synthetic.main(["--videos", "3", "--windows", "3", "--batch", "4"])
    assert sorted(res) == ["video_00", "video_01", "video_02"]
    n = 0
    for vid, dets in res.items():
        scores = [d["score"] for d in dets]
        assert scores == sorted(scores, reverse=True)
        for d in dets:
            assert math.isfinite(d["score"]) and 0.0 < d["score"] <= 1.0
            assert all(math.isfinite(x) for x in d["segment"]) and d["segment"][1] > d["segment"][0]
            assert isinstance(d["action"], int) and d["action"] >= 0
        n += len(dets)
    assert n > 0
