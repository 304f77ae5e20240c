"""The numpy restatement of the detection scoring (tests/detmap_ref.py) against what the reference's own scoring script
computed (tests/golden/detmap_small.npz, recorded by tests/golden/make_golden_map.py), and the host side of
`tim_amd.DetectionScorer` that needs no GPU."""
import os
import re

import numpy as np
import pytest
import torch

import tim_amd
from tests import detmap_ref as R
from tests import helpers as H
from tim_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"timhip_det_match", "timhip_det_ap"}


@pytest.fixture(scope="module")
def small():
    g = np.load(os.path.join(H.GOLDEN, "detmap_small.npz"))
    tp, lock, ap, tab = R.evaluate(g["gt_video"], g["gt_seconds"], g["gt_label"], g["pred_video"], g["pred_seg"],
                                   g["pred_score"], g["pred_label"], g["thresholds"])
    return g, tp, lock, ap, tab


def test_fixture_has_the_shapes_it_was_made_for(small):
    g, tp, lock, ap, tab = small
    sizes = np.diff(tab["gt_off"])
    assert sizes.max() > 128 and sizes.min() == 1 and 64 in sizes and 65 in sizes
    assert len(tab["classes"]) == 7 and len(np.unique(g["pred_label"])) == 8
    assert not np.isin(g["pred_label"], tab["classes"]).all()                    # labels the ground truth does not have
    assert (np.diff(tab["class_off"]) == 0).sum() == 1                           # a class without predictions
    assert not np.isin(g["pred_video"], g["gt_video"]).all()                     # a video without ground truth
    assert 350 <= len(g["gt_label"]) <= 450 and 2700 <= len(g["pred_label"]) <= 3000
    assert tp[0].sum() > 100 and tp[-1].sum() < tp[0].sum()


def test_ap_equals_the_reference(small):
    """AP is a sum of at most npos <= 2^13 positive terms totalling at most 1: any order of summation stays within
    npos * 2^-53 < 1e-12"""
    g, tp, lock, ap, tab = small
    assert ap.shape == g["ap"].shape == (5, 7)
    print("max |ap - reference|", np.abs(ap - g["ap"]).max())
    assert np.abs(ap - g["ap"]).max() <= 1e-12
    assert np.abs(ap.mean(axis=1) - g["mAP"]).max() <= 1e-12
    assert abs(ap.mean(axis=1).mean() - float(g["average_mAP"])) <= 1e-12
    assert ap[:, np.diff(tab["class_off"]) == 0].max() == 0.0


def test_matches_equal_the_reference(small):
    """every prediction's recorded matched_gt / iou is the segment the lock table names at the last threshold at which
    the prediction matched (the reference overwrites both threshold after threshold)"""
    g, tp, lock, ap, tab = small
    N = tab["pred_seg"].shape[0]
    assert g["cp_score"].shape[0] == N
    assert np.array_equal(g["cp_score"], tab["pred_score"])                      # the same order: class, descending score
    assert np.array_equal(g["cp_action"], tab["classes"][tab["pred_cls"]])
    gt_cls = np.searchsorted(tab["classes"], g["gt_label"])
    n_matched = 0
    for pos in range(N):
        ts = np.nonzero(tp[:, pos])[0]
        if len(ts) == 0:
            assert g["cp_matched_gt"][pos] == -1 and g["cp_iou"][pos] == 0.0
            continue
        c = tab["pred_cls"][pos]
        rows = np.nonzero((lock[ts[-1]] == pos - tab["class_off"][c]) & (gt_cls == c))[0]
        assert len(rows) == 1
        r = rows[0]
        assert g["gt_narration"][r] == g["cp_matched_gt"][pos]
        assert g["gt_video"][r] == g["pred_video"][tab["pred_input_row"][pos]]
        assert R.tiou(tab["pred_seg"][pos, 0], tab["pred_seg"][pos, 1], g["gt_seconds"][r, 0], g["gt_seconds"][r, 1]) \
            == g["cp_iou"][pos]
        n_matched += 1
    assert n_matched == int(tp.any(axis=0).sum()) > 100
    # every lock entry names a true positive of its class, once
    for t in range(tp.shape[0]):
        taken = lock[t] >= 0
        assert int(taken.sum()) == int(tp[t].sum())
        pos = tab["class_off"][gt_cls[taken]] + lock[t][taken]
        assert len(np.unique(pos)) == len(pos) and tp[t, pos].all()


def test_ties_fixture_is_the_restatement(small):
    g = np.load(os.path.join(H.GOLDEN, "detmap_ties.npz"))
    tp, lock, ap, tab = R.evaluate(g["gt_video"], g["gt_seg"], g["gt_label"], g["pred_video"], g["pred_seg"], g["pred_score"],
                                   g["pred_label"], g["thresholds"])
    assert np.array_equal(tp, g["tp"]) and np.array_equal(lock, g["lock"]) and np.array_equal(ap, g["ap"])
    assert np.array_equal(tp[2], tp[3])                                          # the repeated threshold
    sc = tab["pred_score"]
    same = (np.diff(sc) == 0) & (np.diff(tab["pred_cls"]) == 0)
    assert same.sum() > 100
    assert (np.diff(tab["pred_input_row"])[same] < 0).all()                      # equal scores: reverse input order


def test_rounding_identity():
    """rint(x * 1000) / 1000 in float64 is Python's round(x, 3) for fp32-origin values (what DetectionCollector.results()
    writes into the file the reference reads): x * 1000 is exact in double for them"""
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(0, 4000, 100000), rng.uniform(0, 40, 60000),
                        np.arange(40000) / 16.0]).astype(np.float32).astype(np.float64)
    assert x.shape[0] == 200000
    got = R.round_segments(x)
    want = np.asarray([round(float(v), 3) for v in x])
    assert np.array_equal(got, want)
    assert np.array_equal((torch.round(torch.from_numpy(x) * 1000) / 1000).numpy(), want)
    assert np.array_equal(R.round_segments(want), want)                          # and it leaves rounded values alone


def test_timestamp_to_seconds(small):
    from tim_amd.detmap import timestamp_to_seconds
    g = small[0]
    sec = np.asarray([[timestamp_to_seconds(a), timestamp_to_seconds(b)] for a, b in zip(g["gt_start"], g["gt_stop"])])
    assert np.array_equal(sec, g["gt_seconds"])
    assert timestamp_to_seconds("01:02:03.25") == 1.0 * 3600 + 2.0 * 60 + 3.25


def test_scorer_host_side():
    assert "DetectionScorer" not in vars(tim_amd)
    from tim_amd.detmap import DetectionScorer
    assert tim_amd.DetectionScorer is DetectionScorer
    seg = np.asarray([[0.0, 1.0], [2.0, 3.0], [0.5, 4.0]])
    sc = DetectionScorer(["b", "a", "b"], seg, [7, 3, 7])
    assert sc.classes.tolist() == [3, 7] and sc.tiou_thresholds.shape == (5,) and sc.round_segments
    assert sc._host["gt_off"].tolist() == [0, 1, 3] and sc._host["npos"].tolist() == [1, 2]
    with pytest.raises(ValueError):
        DetectionScorer(["b", "a", "b"], seg, [7, 3, 7], tiou_thresholds=np.linspace(0.1, 0.9, 17))
    with pytest.raises(ValueError):
        DetectionScorer(["b", "a", "b"], seg, [7, 3, 7], tiou_thresholds=[])
    with pytest.raises(ValueError):
        DetectionScorer(["b", "a"], seg, [7, 3, 7])
    with pytest.raises(ValueError):
        DetectionScorer([], np.zeros((0, 2)), [])
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        sc.evaluate(torch.zeros(2, 2), torch.zeros(2), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), ["a"])
    if not torch.cuda.is_available():
        with pytest.raises(_lib.TimHipError):
            sc.evaluate_results({"a": []})


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    declared = set(re.findall(r"\b(timhip_det_(?:match|ap))\s*\(", hdr))
    assert declared == NAMES <= set(_lib.exported_symbols())
    assert len(_lib._SIGS["timhip_det_match"][1]) == 16 and len(_lib._SIGS["timhip_det_ap"][1]) == 8
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert re.search(r"^SRCS\s*=.*\bdetmap\.hip\b", open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read(), re.M)
    lib = _lib.load()
    for n in NAMES:
        assert hasattr(lib, n)
