"""examples/attention_maps_synthetic.py runs once: C2a on synthetic features, the maps of the last layer, and per printed query
the shares of the visual tokens, the audio tokens and the query itself, which add up to 1."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_attention_maps_example_runs(capsys):
    import attention_maps_synthetic
    res = attention_maps_synthetic.main(["--windows", "2", "--queries", "2"])
    maps = res["maps"]
    assert maps.layers == [5] and (maps.F, maps.S, maps.s0) == (100, 155, 100)
    assert tuple(maps.weights[5].shape) == (2, 55, 101)
    assert len(res["queries"]) == 2
    for q in res["queries"]:
        assert abs(sum(q["share"]) - 1.0) <= 1e-5 and len(q["top"]) == 5 and q["interval"][0] < q["interval"][1]
    out = capsys.readouterr().out
    assert "action query 0" in out and "weight" in out
