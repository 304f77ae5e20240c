"""tests/det_batch_ref.py (the numpy restatement of the reference's detection `__getitem__` + collate that the GPU tests hold
the device path against) against the reference's own outputs, tests/golden/det_batch_{av,visual,audio}.npz
(tests/golden/make_golden_det_batch.py).  Bit for bit; zeros are compared by ==, so the sign of a zero is no part of the
contract.  The fixture must carry the witnesses that tell torch's fp32 rounding from its two plausible misstatements, and the
same comparison must reject both."""
import os

import numpy as np
import pytest

from tests import det_batch_ref as R
from tests.golden.det_batch_inputs import MAX_A, MAX_V, NF, make_tables, round3_f32, round3_f64, round3_mul

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [("av", 81, "audio_visual"), ("visual", 82, "visual"), ("audio", 83, "audio")]


def load(name):
    return np.load(os.path.join(HERE, "golden", "det_batch_%s.npz" % name))


def same(got, want):
    """bit for bit, except that +0.0 == -0.0"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(np.array_equal(got, want))


def windows_match(tb, g, round3):
    """-> the number of times / segment elements over all windows that differ from the golden file"""
    bad = 0
    for i in range(int(g["n"])):
        it = R.getitem(tb, i, g["va%d" % i] if g["va%d" % i].size else None, g["aa%d" % i] if g["aa%d" % i].size else None, 2, round3)
        for got, key in ((it["times"], "t"), (it["v_gt_segments"], "vseg"), (it["a_gt_segments"], "aseg")):
            want = g["%s%d" % (key, i)]
            assert got.shape == want.shape and got.dtype == want.dtype == np.float32
            bad += int((got != want).sum())
    return bad


@pytest.mark.parametrize("name,seed,modality", CASES)
def test_restatement_is_the_references_getitem(name, seed, modality):
    g, tb = load(name), make_tables(seed, modality)
    assert int(g["seed"]) == seed and str(g["modality"]) == modality and int(g["n"]) == len(tb["windows"])
    for i in range(int(g["n"])):
        va, aa = g["va%d" % i], g["aa%d" % i]
        for col in (0, 1, 2):
            it = R.getitem(tb, i, va if va.size else None, aa if aa.size else None, col)
            assert same(it["v"], g["v%d" % i]) and same(it["a"], g["a%d" % i]) and same(it["times"], g["t%d" % i])
            assert same(it["v_gt_segments"], g["vseg%d" % i]) and same(it["a_gt_segments"], g["aseg%d" % i])
            assert same(it["verb"], g["verb%d" % i]) and same(it["noun"], g["noun%d" % i]) and same(it["class_id"], g["class_id%d" % i])
            assert same(it["action"], g["action%d_c%d" % (i, col)])
            assert it["window_start"] == float(g["start%d" % i]) and tb["window_size"] == float(g["size%d" % i])
            assert it["video_id"] == str(g["vid%d" % i])
        assert it["times"].shape == ((2 if modality == "audio_visual" else 1) * NF, 2)
    assert R.action_column("epic", False, True) == 0 and R.action_column("epic", False, False) == 1
    assert R.action_column("epic", True, True) == R.action_column("epic", True, False) == R.action_column("thumos", False, True) == 2


@pytest.mark.parametrize("name,seed,modality", CASES)
def test_restated_collate_is_default_collate(name, seed, modality):
    g, tb = load(name), make_tables(seed, modality)
    idx = g["c_index"].tolist()
    assert len(set(idx)) < len(idx) and idx != sorted(idx)            # windows repeat and arrive out of order
    va = np.stack([g["va%d" % i] for i in idx]) if "visual" in modality else None
    aa = np.stack([g["aa%d" % i] for i in idx]) if "audio" in modality else None
    v, a, t, label, meta = R.batch(tb, idx, va, aa, 2)
    assert same(v, g["c_v"]) and same(a, g["c_a"]) and same(t, g["c_t"])
    assert sorted(label) == sorted(R.LABEL_KEYS)
    for k in R.LABEL_KEYS:
        assert same(label[k], g["c_" + k]), k
    assert same(meta["window_start"], g["c_start"]) and meta["window_start"].dtype == np.float64
    assert same(meta["window_size"], g["c_size"]) and meta["video_id"] == [str(s) for s in g["c_vid"]]
    assert [tb["video_ids"][j] for j in meta["video_index"]] == meta["video_id"] and meta["video_index"].dtype == np.int32
    # rows the sampler marks absent: -1 labels, zero segments, everything else kept
    valid = np.array([1, 0, 1, 1, 0], np.uint8)
    v2, a2, t2, l2, m2 = R.batch(tb, idx, va, aa, 2, valid=valid)
    assert same(v2, v) and same(t2, t) and same(m2["window_start"], meta["window_start"])
    for k in R.LABEL_KEYS:
        assert np.array_equal(l2[k][valid != 0], label[k][valid != 0])
        assert bool((l2[k][valid == 0] == (0.0 if k.endswith("segments") else -1)).all())


@pytest.mark.parametrize("name,seed,modality", CASES)
def test_fixture_carries_the_cases_and_the_misstatements_are_rejected(name, seed, modality):
    g, tb = load(name), make_tables(seed, modality)
    ws = tb["windows"]
    assert 7 <= len(ws) <= 9 and 2 <= len({w["video_id"] for w in ws}) <= 3
    assert (tb["max_visual_actions"], tb["max_audio_actions"], tb["num_feats"]) == (MAX_V, MAX_A, NF) == (3, 2, 6)
    assert {0, 1, MAX_V} <= {w["v_labels"].shape[0] for w in ws} and {0, 1, MAX_A} <= {w["a_labels"].shape[0] for w in ws}
    assert sum(w["start_sec"] >= 1000.0 for w in ws) >= 3
    ft = tb["v_feat_times"] if "visual" in modality else tb["a_feat_times"]
    d = np.concatenate([(ft[w["video_id"]][w["feat_indices"], :2] - np.float32(w["start_sec"])).reshape(-1) for w in ws]).astype(np.float32)
    assert (d < 0).any()                                              # a feature time before its window's start: the clamp
    seg = np.concatenate([w["v_gt_segments"].reshape(-1) - np.float32(w["start_sec"]) for w in ws])
    assert (seg < 0).any()
    # exact ties of d * 1000 with an even and an odd neighbour below: half-to-even goes down once and up once
    assert np.float32(0.0625) in d and np.float32(0.1875) in d
    assert round3_f32(np.float32(0.0625)) == np.float32(0.062) and round3_f32(np.float32(0.1875)) == np.float32(0.188)
    ties = d[(d * np.float32(1000.0)) % 1 == 0.5]
    assert ties.size >= 8 and {0.0, 1.0} <= set((np.floor(ties * np.float32(1000.0)) % 2).tolist())
    # the restatement matches; the float64 one and the 0.001f one each miss at least 8 elements of this very file
    assert windows_match(tb, g, round3_f32) == 0
    n64, nmul = windows_match(tb, g, round3_f64), windows_match(tb, g, round3_mul)
    print("%s: float64 restatement differs in %d elements, 0.001f restatement in %d" % (name, n64, nmul))
    assert n64 >= 8 and nmul >= 8
