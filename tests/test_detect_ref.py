"""tests/detect_ref.py (the numpy restatement of the detection inference tail) against tests/golden/detect_small.npz, which
tests/golden/make_golden_detect.py recorded from the reference's own FeatureMeter and format_predictions.main.  CPU only."""
import os

import numpy as np

from tests import detect_ref as D
from tests import helpers as H


def _fixture():
    return np.load(os.path.join(H.GOLDEN, "detect_small.npz"))


def _collect(g, order=None):
    col = D.Collector(g["logits"].shape[2], float(g["threshold"]))
    B = g["window_start"].shape[1]
    qt = np.tile(g["queries"][None], (B, 1, 1))
    for b in (range(g["logits"].shape[0]) if order is None else order):
        col.update(g["logits"][b], g["reg"][b], qt, list(g["video_ids"][b]), g["window_start"][b], float(g["window_size"]))
    return col


def _ulp_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_fixture_covers_the_cases_it_names():
    g = _fixture()
    nq = int(g["num_queries"])
    assert g["logits"].shape == (3, 2 * nq, 23) and nq == 19
    assert len(set(g["video_ids"].ravel())) == 3 and g["video_ids"][0, 1] == g["video_ids"][1, 0]     # one video spans batches
    mt = g["queries"].max()
    assert (g["reg"] < 0).any() and (g["reg"] > mt).any()                                             # both clamps
    assert (np.abs(g["window_start"] * 1000 - np.rint(g["window_start"] * 1000)) > 1e-4).any()         # > 3 decimals
    seg, ok = D.decode(g["reg"][0], g["window_start"][0], float(g["window_size"]), mt, nq)
    assert not ok[1] and not ok[2] and ok[3]                                                          # zero width, reversed
    assert tuple(seg[3]) == (3.062, 4.062)                                                            # x.0625 -> half-even
    s = 1.0 / (1.0 + np.exp(-g["logits"].astype(np.float64)))
    assert not (np.abs(s - float(g["threshold"])) < 1e-5).any()


def test_proposals_are_the_references_float64_values():
    g = _fixture()
    nq = int(g["num_queries"])
    mt = g["queries"].max()
    ws32 = np.float32(float(g["window_size"]))
    got = []
    for b in range(3):
        p = np.minimum(np.maximum(g["reg"][b], np.float32(0)), mt)
        got.append((p * ws32).astype(np.float32).astype(np.float64) + np.repeat(g["window_start"][b], nq)[:, None])
    assert g["v_proposals"].dtype == np.float64
    assert np.array_equal(np.concatenate(got), g["v_proposals"])                  # unrounded, bit for bit
    seg = np.concatenate([D.decode(g["reg"][b], g["window_start"][b], float(g["window_size"]), mt, nq)[0] for b in range(3)])
    assert np.array_equal(seg, np.round(g["v_proposals"], 3))


def test_candidates_match_the_reference_in_membership_and_order():
    g = _fixture()
    col = _collect(g)
    c = col.candidates()
    names = list(g["video_names"])
    n = 0
    for v, vid in enumerate(col.video_ids):                    # per video, in collection order: what the NMS is handed
        m = c["video"] == v
        r = g["cand_video"] == names.index(vid)
        assert m.sum() == r.sum() and m.sum() > 0
        assert np.array_equal(c["cls"][m], g["cand_class"][r])
        assert np.array_equal(c["seg"][m].astype(np.float64), g["cand_seg"][r].astype(np.float32).astype(np.float64))
        # torch's CPU sigmoid (what the fixture holds) is not correctly rounded: 29 % of its values are 1 ulp and 0.13 %
        # 2 ulp from the rounded float64 value (2e6 normal logits), never more
        assert _ulp_apart(c["score"][m], g["cand_score"][r]).max() <= 2
        n += int(m.sum())
    assert n == len(g["cand_class"]) == len(c["score"])
    assert np.array_equal(c["key"], c["video"] * 23 + c["cls"])
    assert col.video_ids == ["P03_01", "P01_07", "P02_05"]     # first-seen order


def test_results_match_the_reference_submission():
    g = _fixture()
    col = _collect(g)
    res = col.results(sigma=float(g["sigma"]))
    names = list(g["video_names"])
    assert sorted(res) == sorted(names)
    for vid, entries in res.items():
        r = g["res_video"] == names.index(vid)
        want = {(int(a), float(s0), float(s1)): float(sc)
                for a, s0, s1, sc in zip(g["res_class"][r], g["res_seg"][r, 0], g["res_seg"][r, 1], g["res_score"][r])}
        got = {(e["action"], e["segment"][0], e["segment"][1]): e["score"] for e in entries}
        assert len(got) == len(entries) == int(r.sum())
        assert set(got) == set(want)
        for k in got:
            assert abs(got[k] - want[k]) <= 2e-5 * max(abs(want[k]), 1e-3), (vid, k)
        sc = [e["score"] for e in entries]
        assert sc == sorted(sc, reverse=True)


def test_sigmoid32_is_the_rounded_float64_value():
    x = np.array([-120.0, -104.0, -103.0, -87.5, -4.6, 0.0, 3.0, 17.0, 40.0, np.inf, -np.inf], np.float32)
    s = D.sigmoid32(x)
    assert s.dtype == np.float32 and s[0] == 0.0 and s[5] == 0.5 and s[8] == 1.0 and s[9] == 1.0 and s[10] == 0.0
    assert s[2] > 0.0                                           # an fp32 denormal, not flushed
    assert np.all(np.diff(s[:10]) >= 0)
