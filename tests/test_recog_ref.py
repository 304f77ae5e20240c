"""tests/recog_ref.py (the numpy restatement of the recognition inference tail) against the fixture recorded
from the reference's own InferenceMeter, FeatureMeter and metrics.py (tests/golden/make_golden_recog.py ->
tests/golden/recog_small.npz).  Accumulators, seen counts, labels and every accuracy float are equal to the reference's.

The probabilities are the reference's torch-fp32 softmax against the float64 softmax rounded to fp32: the reference against
arithmetic, not against the code under test.  Measured by the recorder over this fixture: at most 6 ulp (C = 7; 4 to 5 ulp
at the other widths).  The bound is twice that, 12 ulp, since torch's vectorised exp varies by host."""
import os

import numpy as np

from tests import helpers as H
from tests import recog_ref as RR

MAX_ULP_MEASURED = 6
HEADS = ("verb", "noun", "action", "audio")


def load():
    return np.load(os.path.join(H.GOLDEN, "recog_small.npz"))


def replay(g, splits=None):
    classes = dict(zip(HEADS, (int(c) for c in g["classes"])))
    col = RR.Collector(classes, int(g["num_actions"]))
    for b in range(g["v_ids"].shape[0]):
        col.update({h: g["logits_" + h][b] for h in HEADS}, g["v_ids"][b], g["a_ids"][b], g["v_labels"][b], g["a_labels"][b])
    return col


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_fixture_covers_what_it_claims():
    g = load()
    v, a = g["v_ids"], g["a_ids"]
    assert int(g["max_ulp"]) == MAX_ULP_MEASURED
    assert (v == -1).any() and (a == -1).any()                                   # padded rows
    assert (a == -1).all(axis=1).any()                                           # a batch without a valid audio row
    assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in v)                  # duplicates inside one batch
    only_one_modality = np.concatenate([g["seen"][:int(a[a >= 0].min())], g["seen"][int(g["last_visual"]):]])
    assert set(only_one_modality.astype(int)) == {1, 2, 3, 4, 5}
    assert set(v[v >= 0]) & set(a[a >= 0])                                       # ids both modalities see: one seen count


def test_accumulators_seen_and_labels_equal_the_reference():
    g, col = load(), None
    col = replay(g)
    assert not col.err
    for h in HEADS:
        grp = col.groups["audio" if h == "audio" else "visual"]
        acc = grp["acc"][grp["heads"].index(h)]
        assert acc.dtype == np.float32 and np.array_equal(acc.view(np.int32), g["sum_" + h].view(np.int32)), h
    assert np.array_equal(col.seen, g["seen"])
    assert np.array_equal(col.groups["visual"]["labels"], g["state_v_labels"])
    assert np.array_equal(col.groups["audio"]["labels"][:, 0], g["state_a_labels"])
    assert np.array_equal(col.groups["visual"]["touched"] != 0, g["state_v_labels"][:, 2] != -1)
    assert np.array_equal(col.groups["audio"]["touched"] != 0, g["state_a_labels"] != -1)


def test_accuracy_floats_equal_the_reference():
    g = load()
    acc = replay(g).accuracies()
    assert sorted(acc) == ["action", "audio", "mt_action", "noun", "verb"]
    for h, got in acc.items():
        assert tuple(got) == tuple(float(x) for x in g["acc_" + h]), (h, got, g["acc_" + h])


def test_ranks_agree_with_the_reference_probabilities():
    """the fixture has no tie at a boundary, so the rank on the mean logits and the position in the reference's fp32
    probabilities put every label on the same side of top-1 and top-5"""
    g = load()
    col = replay(g)
    for h, (rank, ids) in col.ranks().items():
        prob = g["prob_" + h]
        lab = (g["state_a_labels"] if h == "audio" else g["state_v_labels"][:, HEADS.index(h)])[ids]
        above = np.array([(p > p[l]).sum() for p, l in zip(prob, lab)])
        for k in (1, 5):
            assert np.array_equal(rank < k, above < k), (h, k)


def test_probabilities_within_twice_the_measured_distance():
    g = load()
    worst = 0
    preds = replay(g).predictions()
    for h in HEADS:
        prob, ids = preds[h]
        assert prob.dtype == np.float32 and prob.shape == g["prob_" + h].shape
        d = ulps(prob, g["prob_" + h])
        print("%s: at most %d ulp from the reference's fp32 softmax" % (h, d.max()))
        worst = max(worst, int(d.max()))
        # FeatureMeter.finalize_metrics: visual actions are the ids below last_visual, audio actions the rest
        lv = int(g["last_visual"])
        sel = ids < lv if h != "audio" else ids >= lv
        feat = g["feat_prob_" + h][ids[sel] - (0 if h != "audio" else lv)]
        assert ulps(prob[sel], feat).max() <= 2 * MAX_ULP_MEASURED
    assert worst <= 2 * MAX_ULP_MEASURED


def test_batch_split_does_not_change_the_restatement():
    g = load()
    a = replay(g)
    classes = dict(zip(HEADS, (int(c) for c in g["classes"])))
    b = RR.Collector(classes, int(g["num_actions"]))
    flat = lambda x: x.reshape((-1,) + x.shape[2:])
    b.update({h: flat(g["logits_" + h]) for h in HEADS}, flat(g["v_ids"]), flat(g["a_ids"]), flat(g["v_labels"]), flat(g["a_labels"]))
    for name in a.groups:
        for x, y in zip(a.groups[name]["acc"], b.groups[name]["acc"]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert np.array_equal(a.seen, b.seen)


def test_out_of_range_id_is_skipped_and_reported():
    col = RR.Collector({"audio": 3}, 4, modality="audio")
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    col.update({"audio": x}, a_ids=np.array([1, 7, -1, 1]), a_labels=np.array([2, 0, -1, 2]))
    assert col.err and col.seen.tolist() == [0, 2, 0, 0]
    assert np.array_equal(col.groups["audio"]["acc"][0][1], x[0] + x[3])
