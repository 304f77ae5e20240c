"""tests/twostream_ref.py (the numpy restatement of the two-stream detection fusion) against
tests/golden/twostream_small.npz, which tests/golden/make_golden_twostream.py recorded from the reference's own FeatureMeter
and format_two_stream_predictions_epic.main.  CPU only."""
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import twostream_ref as T
from tests.detect_ref import sigmoid32

SETS = ("k1", "k3", "k2a")       # top_k 1 and 3 at verb_alpha 0.65; top_k 2 at 1.3 (the fused score can fail there)


def _fixture():
    return np.load(os.path.join(H.GOLDEN, "twostream_small.npz"))


def _collect(g, tag, sizes=None):
    col = T.Collector(g["verb_logits"].shape[2], g["noun_logits"].shape[2], float(g["threshold"]), float(g[tag + "_alpha"]),
                      int(g[tag + "_top_k"]))
    B = g["window_start"].shape[1]
    qt = np.tile(g["queries"][None], (B, 1, 1))
    for b in range(g["verb_logits"].shape[0]):
        col.update(g["verb_logits"][b], g["noun_logits"][b], g["verb_reg"][b], g["noun_reg"][b], qt, list(g["video_ids"][b]),
                   g["window_start"][b], float(g["window_size"]))
    return col


def _ulp_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_fixture_covers_the_cases_it_names():
    g = _fixture()
    nq = int(g["num_queries"])
    assert g["verb_logits"].shape == (3, 2 * nq, 11) and g["noun_logits"].shape == (3, 2 * nq, 23) and nq == 19
    assert len(set(g["video_ids"].ravel())) == 3 and g["video_ids"][0, 1] == g["video_ids"][1, 0]     # one video spans batches
    assert [int(g[t + "_top_k"]) for t in SETS] == [1, 3, 2] and [float(g[t + "_alpha"]) for t in SETS] == [0.65, 0.65, 1.3]
    assert str(g["numpy_version"]).split(".")[0] >= "2" and int(g["max_ulp_vs_reference"]) >= 0
    mt, thr = g["queries"].max(), np.float32(float(g["threshold"]))
    for reg in (g["verb_reg"], g["noun_reg"]):
        assert (reg < 0).any() and (reg > mt).any()                                                   # both clamps
    assert (g["window_start"] > 3000).any()
    # batch 0 at top_k 1: the crafted rows
    c = T.batch_candidates(g["verb_logits"][0], g["noun_logits"][0], g["verb_reg"][0], g["noun_reg"][0], g["window_start"][0],
                           float(g["window_size"]), mt, [0, 0], thr, 0.65, 1)
    vs, ns, ok, seg = c["sel_score"][:, 0, 0], c["sel_score"][:, 1, 0], c["pair_ok"][:, 0], c["pair_seg"][:, 0]
    assert vs[0] > thr and not ns[0] > thr and not ok[0]                                              # only the verb passes
    assert not vs[1] > thr and ns[1] > thr and not ok[1]                                              # only the noun passes
    assert vs[2] > thr and ns[2] > thr and c["pair_score"][2, 0] > thr and ok[2]
    assert ok[3]                                                                                      # both clamps
    for r in (4, 6):                                                                                  # the blend is reversed
        assert vs[r] > thr and ns[r] > thr and c["pair_score"][r, 0] > thr and seg[r, 1] < seg[r, 0] and not ok[r]
    assert vs[5] > thr and ns[5] > thr and c["pair_score"][5, 0] > thr and seg[5, 1] == seg[5, 0] and not ok[5]   # zero width
    # ... and at verb_alpha 1.3 both scores of row 2 pass and the fused one does not
    c = T.batch_candidates(g["verb_logits"][0], g["noun_logits"][0], g["verb_reg"][0], g["noun_reg"][0], g["window_start"][0],
                           float(g["window_size"]), mt, [0, 0], thr, 1.3, 2)
    assert c["sel_score"][2, 0, 0] > thr and c["sel_score"][2, 1, 0] > thr and not c["pair_score"][2, 0] > thr
    assert not c["pair_ok"][2, 0]
    # the margins the maker asserted, on the restatement's values
    for lg in (g["verb_logits"], g["noun_logits"]):
        s = 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))
        assert not (np.abs(s - float(g["threshold"])) < 1e-5).any()


def test_proposals_are_the_references_float64_values():
    g = _fixture()
    nq, mt, ws = int(g["num_queries"]), g["queries"].max(), float(g["window_size"])
    for reg, want in ((g["verb_reg"], g["verb_proposals"]), (g["noun_reg"], g["noun_proposals"])):
        got = np.concatenate([T.proposals(reg[b], g["window_start"][b], ws, mt, nq) for b in range(3)])
        assert want.dtype == np.float64 and np.array_equal(got, want)                 # unrounded, bit for bit


@pytest.mark.parametrize("tag", SETS)
def test_candidates_match_the_reference_row_by_row(tag):
    """per video the reference lists its candidates proposal by proposal, as the restatement does; inside a proposal its order
    is argpartition's, so each row is compared as a set of (verb, noun)"""
    g = _fixture()
    col = _collect(g, tag)
    names = list(g["video_names"])
    bound = 2 * int(g["max_ulp_vs_reference"])
    nq = int(g["num_queries"])
    rows = np.concatenate([ch["row"].astype(np.int64) + b * 2 * nq for b, ch in enumerate(col.chunks)])
    c = col.candidates()
    n = 0
    for v, vid in enumerate(col.video_ids):
        m = np.nonzero(c["video"] == v)[0]
        r = np.nonzero(g[tag + "_cand_video"] == names.index(vid))[0]
        assert len(m) == len(r) and len(m) > 0
        for row in np.unique(rows[m]):                          # rows ascending on both sides: the same slice of either list
            at = np.nonzero(rows[m] == row)[0]
            got = {(int(c["verb"][m[i]]), int(c["noun"][m[i]])): i for i in at}
            want = {(int(g[tag + "_cand_verb"][r[i]]), int(g[tag + "_cand_noun"][r[i]])): i for i in at}
            assert len(got) == len(at) and set(got) == set(want), (vid, row)
            for pair, i in got.items():
                j = want[pair]
                assert np.array_equal(c["seg64"][m[i]], g[tag + "_cand_seg"][r[j]]), (vid, row, pair)     # exactly equal
                assert _ulp_apart(c["score"][m[i]], g[tag + "_cand_score"][r[j]]) <= bound, (vid, row, pair)
        n += len(m)
    assert n == len(g[tag + "_cand_verb"]) == len(c["score"])
    assert np.array_equal(c["key"], c["video"] * (11 * 23) + c["verb"] * 23 + c["noun"])
    assert col.video_ids == ["P03_01", "P01_07", "P02_05"]     # first-seen order


@pytest.mark.parametrize("tag", SETS)
def test_results_match_the_reference_submission(tag):
    g = _fixture()
    col = _collect(g, tag)
    res = col.results(sigma=float(g["sigma"]))
    names = list(g["video_names"])
    assert sorted(res) == sorted(names[i] for i in np.unique(g[tag + "_res_video"]))
    for vid, entries in res.items():
        r = g[tag + "_res_video"] == names.index(vid)
        want = [(int(a), int(n), float(s0), float(s1)) for a, n, s0, s1 in
                zip(g[tag + "_res_verb"][r], g[tag + "_res_noun"][r], g[tag + "_res_seg"][r, 0], g[tag + "_res_seg"][r, 1])]
        got = [(e["verb"], e["noun"], e["segment"][0], e["segment"][1]) for e in entries]
        assert got == want                                                                     # the same list, the same order
        assert all(e["action"] == "%d,%d" % (e["verb"], e["noun"]) for e in entries)
        for e, w in zip(entries, g[tag + "_res_score"][r]):
            assert abs(e["score"] - w) <= 2e-5 * max(abs(w), 1e-3), (vid, e)
    for task, f in (("verb", lambda l: l // 23), ("noun", lambda l: l % 23)):
        a, t = col.detections(sigma=float(g["sigma"])), col.detections(sigma=float(g["sigma"]), task=task)
        assert np.array_equal(t[2], f(a[2])) and all(np.array_equal(x, y) for x, y in zip(a[:2] + a[3:], t[:2] + t[3:]))


def test_selection_is_argpartitions_set_and_takes_a_nan():
    rng = np.random.default_rng(5)
    s = sigmoid32(rng.normal(-3, 2, size=(10000, 37)).astype(np.float32))
    for k in (1, 3, 8):
        d = -np.sort(-s, axis=1)
        rows = d[:, k - 1] != d[:, k]                                   # no tie at the boundary: the set is defined
        assert rows.sum() > 9900
        got = T.select_top_k(s, k)
        want = np.stack([np.argpartition(row, -k)[-k:] for row in s])
        assert np.array_equal(np.sort(got[rows], axis=1), np.sort(want[rows], axis=1))
        picked = np.take_along_axis(s, got, 1)
        assert (np.diff(picked, axis=1) <= 0).all()                     # by descending score
    t = s[:50].copy()
    t[:, 11] = np.nan
    for k in (1, 3):
        got = T.select_top_k(t, k)
        assert (got[:, 0] == 11).all()                                  # a NaN ranks above every number, as numpy sorts it
        assert all(11 in np.argpartition(row, -k)[-k:] for row in t)
    u = np.array([[0.25, 0.5, 0.5, 0.125, 0.5]], np.float32)            # equal scores: the lower class first
    assert T.select_top_k(u, 2).tolist() == [[1, 2]] and T.select_top_k(u, 4).tolist() == [[1, 2, 4, 0]]


def test_exponents_are_rounded_after_the_double_subtraction():
    a, b = T.exponents(0.65)
    assert a == np.float32(0.65) and b == np.float32(1.0 - 0.65) and a.dtype == b.dtype == np.float32
    assert T.exponents(1.0) == (np.float32(1), np.float32(0)) and T.exponents(0.0) == (np.float32(0), np.float32(1))
