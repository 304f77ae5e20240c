"""examples/query_windows_synthetic.py runs: windows encoded once, the pyramid and a second set of intervals scored from the same
cache, both collected into detections per video."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_query_windows_synthetic_example_collects_both_query_sets():
    import query_windows_synthetic
    out = query_windows_synthetic.main(["--videos", "2", "--windows", "3", "--proposals", "24"])
    res = out["results"]
    assert sorted(res) == ["video_00", "video_01"]
    first, both = out["candidates"]
    assert 0 < first < both                      # the second query set added candidates of its own
    assert out["cache_bytes"] > 0
    n = 0
    for dets in res.values():
        scores = [d["score"] for d in dets]
        assert scores == sorted(scores, reverse=True)
        for d in dets:
            assert math.isfinite(d["score"]) and 0.0 < d["score"] <= 1.0
            assert all(math.isfinite(x) for x in d["segment"]) and d["segment"][1] > d["segment"][0]
        n += len(dets)
    assert n > 0
