"""examples/query_maps_synthetic.py runs once: C2a windows encoded once, two interval sets asked of the cache, and per printed
interval the span of its most attended feature tokens and the shares of the visual tokens, the audio tokens and the query itself,
which add up to 1."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_query_maps_example_runs(capsys):
    import query_maps_synthetic
    res = query_maps_synthetic.main(["--windows", "2", "--sets", "2", "--intervals", "3"])
    maps = res["last"]["maps"]
    assert res["last"]["window_index"] == [0, 1, 0]              # the second set: three groups on two windows
    assert maps.layers == [5] and (maps.F, maps.S, maps.s0) == (100, 109, 100)
    assert tuple(maps.weights[5].shape) == (3, 9, 101)           # three rows (verb, noun, action) per visual interval
    assert tuple(maps.for_head("action").shape) == (3, 3, 101)
    assert res["cache"].W == 2 and len(res["intervals"]) == 2 * 3
    for q in res["intervals"]:
        assert abs(sum(q["share"]) - 1.0) <= 1e-5 and len(q["top"]) == 5
        assert q["interval"][0] < q["interval"][1] and q["span"][0] < q["span"][1]
    out = capsys.readouterr().out
    assert "encoded once" in out and "set 1: 3 groups x 3 intervals" in out and "tokens span" in out
