"""examples/eval_synthetic.py runs: overlapping synthetic windows through the recognition model and the collector."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_eval_synthetic_example_prints_accuracies():
    import eval_synthetic
    res = eval_synthetic.main(["--videos", "3", "--actions", "6", "--batch", "4"])
    assert sorted(res["accuracies"]) == ["action", "audio", "mt_action", "noun", "verb"]
    for top1, top5 in res["accuracies"].values():
        assert math.isfinite(top1) and 0.0 <= top1 <= top5 <= 100.0
    assert res["seen"].max() >= 2                           # windows overlap: some action is seen more than once
    assert res["seen"].shape == (res["num_actions"],) and (res["seen"] > 0).sum() >= res["num_actions"] // 2
