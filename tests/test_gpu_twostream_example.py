"""examples/twostream_synthetic.py runs: synthetic windows through a verb model and a noun model, the two-stream collector and
the scorer; (verb, noun) detections per video and three sets of mAP."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_twostream_synthetic_example_returns_detections_and_maps():
    import twostream_synthetic
    maps, res = twostream_synthetic.main(["--videos", "3", "--windows", "3", "--batch", "4"])
    assert sorted(maps) == ["action", "noun", "verb"]
    for mAP, avg in maps.values():
        assert len(mAP) == 5 and all(math.isfinite(m) and 0.0 <= m <= 1.0 for m in mAP) and 0.0 < avg < 1.0
    assert set(res) <= {"video_00", "video_01", "video_02"} and len(res) > 0
    n = 0
    for vid, dets in res.items():
        scores = [d["score"] for d in dets]
        assert scores == sorted(scores, reverse=True)
        for d in dets:
            assert math.isfinite(d["score"]) and 0.0 < d["score"] <= 1.0
            assert all(math.isfinite(x) for x in d["segment"]) and d["segment"][1] > d["segment"][0]
            assert 0 <= d["verb"] < 7 and 0 <= d["noun"] < 11 and d["action"] == "%d,%d" % (d["verb"], d["noun"])
        n += len(dets)
    assert n > 0
