"""The restatement of the detection meter (tests/det_meter_ref.py) against fixtures recorded from the reference's own TrainMeter /
InferenceMeter and loss functions (tests/golden/make_golden_det_meter.py), on the CPU; and the host side of tim_amd's detection meter
(the layout mirror in tim_amd/_lib.py, tim_amd.meters.decode_det_state) against the header and the restatement."""
import os
import re

import numpy as np
import pytest
import torch

from tests import det_meter_ref as DR
from tests import losses_ref as R
from tests.helpers import GOLDEN

NAMES = ("visual_vn", "visual_single", "audio", "av")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGGED = ("verb", "noun", "action", "positive", "negative")


def load(name):
    return np.load(os.path.join(GOLDEN, "det_meter_%s.npz" % name))


def sides_of(fx):
    return [str(s) for s in fx["sides"]]


def replay(fx, accidents=False):
    """the restatement over the fixture's recorded per-iteration float32 values -> per-batch (sum, count, avg) arrays"""
    m = DR.DetMeter(accidents=accidents)
    present = sides_of(fx)
    nb = fx["stats"].shape[0]
    out = {k: np.zeros((nb, len(DR.SLOTS)), np.int64 if k == "count" else np.float64) for k in ("sum", "count", "avg")}
    for b in range(nb):
        m.update(fx["stats"][b, 0] if "visual" in present else None, fx["stats"][b, 1] if "audio" in present else None,
                 3 if bool(fx["include_verb_noun"]) else 1, fx["total"][b], fx["drloc"][b])
        out["sum"][b], out["count"][b] = m.sum, m.count
        out["avg"][b] = [m.avg(k) for k in DR.SLOTS]
    return out, m


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_reference_meters(name):
    """sums, counts and averages after every batch, bit for bit: every slot in the one-modality fixtures, the slots pinned to the
    reference in `av` (the flagged ones hold the restatement's own numbers there and are checked as a regression)"""
    fx = load(name)
    got, _ = replay(fx)
    pinned = fx["pinned_to_reference"]
    assert pinned.all() == (name != "av")
    assert [DR.SLOTS[s] for s in np.nonzero(~pinned)[0]] == ([] if name != "av" else list(FLAGGED))
    for k in ("sum", "count", "avg"):
        assert same_bits(got[k][:, pinned], fx["ref_slot_" + k][:, pinned]), k
        assert same_bits(got[k], fx["slot_" + k]), k
    assert fx["slot_count"][-1, DR.SLOTS.index("total")] > 0
    assert bool(fx["mask_restricted"].any()) and not bool(fx["mask_restricted"][0].any())


@pytest.mark.parametrize("name", NAMES)
def test_accidents_are_the_whole_difference(name):
    """the restatement with the two audio_visual accidents of the reference's loop put back (per-head sums over the normaliser the
    audio side advanced; the audio side's positive / negative loss for both sides) equals the reference's meter on EVERY slot, in
    every fixture; in `av` the fixture's flagged slots reject it, with one modality it changes nothing"""
    fx = load(name)
    got, _ = replay(fx, accidents=True)
    for k in ("sum", "count", "avg"):
        assert same_bits(got[k], fx["ref_slot_" + k]), k
    if name != "av":
        for k in ("sum", "count", "avg"):
            assert same_bits(got[k], fx["slot_" + k])
        return
    for slot in FLAGGED:
        s = DR.SLOTS.index(slot)
        assert not same_bits(got["sum"][:, s], fx["slot_sum"][:, s]), "%s: the accident must show in the av fixture" % slot
        assert same_bits(got["count"][:, s], fx["slot_count"][:, s])          # (the accidents move values, never counts)
    for slot in ("total", "drloc", "visual", "visual_reg", "audio", "audio_reg"):
        s = DR.SLOTS.index(slot)
        assert same_bits(got["sum"][:, s], fx["slot_sum"][:, s])


@pytest.mark.parametrize("name", NAMES)
def test_side_statistics_within_derived_bound(name):
    """the float64 side statistics against the reference's float32 values: every per-head sum and both parts within the first-order
    bound `_side_check` applies to the focal sum (per-element focal_bound terms plus the summation term), the counts exact, the
    divided values within that bound over the normaliser plus the roundings of the normaliser and the division (8u relative)"""
    fx = load(name)
    U = R.EPS32
    hy = {k: float(fx[k]) for k in ("iou_threshold", "lambda_reg", "momentum", "norm0")}
    norm, worst = hy["norm0"], 0.0
    T = torch.from_numpy
    for b in range(fx["stats"].shape[0]):
        for side in sides_of(fx):
            s = DR.SIDES.index(side)
            K = len(fx["heads_" + side])
            xs = [T(fx["b%d_%s_logits%d" % (b, side, k)]) for k in range(K)]
            ts = [T(fx["b%d_%s_targets%d" % (b, side, k)]) for k in range(K)]
            iou, off, reg = (T(fx["b%d_%s_%s" % (b, side, k)]) for k in ("iou", "offsets", "reg"))
            w, bound, mag = DR.side_stats(xs, ts, iou, off, reg, hy["iou_threshold"], 0.25, 2.0, 1e-8, hy["lambda_reg"], hy["momentum"], norm)
            ref = fx["stats"][b, s].astype(np.float64)
            norm_in, norm = norm, w[DR.NORMALISER]
            assert ref[DR.VALID] == w[DR.VALID] and ref[DR.POSITIVES] == w[DR.POSITIVES]
            assert abs(ref[DR.NORMALISER] - norm) <= 4 * U * norm, (norm_in, norm)      # (one step of the running value at a time)
            sums = [DR.HEAD_SUM + k for k in range(K)] + [DR.POS_SUM, DR.NEG_SUM]
            vals = [DR.HEAD + k for k in range(K)] + [DR.POS, DR.NEG]
            for i, j in zip(sums, vals):
                assert abs(ref[i] - w[i]) <= bound[i], (b, side, i, ref[i], w[i], bound[i])
                worst = max(worst, abs(ref[i] - w[i]) / bound[i])
                assert abs(ref[j] - w[j]) <= bound[i] / norm + 8 * U * abs(w[j]) + R.TINY32, (b, side, j)
            b_cls = sum(bound[DR.HEAD_SUM + k] for k in range(K)) / (K * norm) + 8 * U * abs(w[DR.CLS]) + R.TINY32
            assert abs(ref[DR.CLS] - w[DR.CLS]) <= b_cls
            assert abs(ref[DR.DIOU_SUM] - w[DR.DIOU_SUM]) <= bound[DR.DIOU_SUM]
            assert abs(ref[DR.REG] - w[DR.REG]) <= hy["lambda_reg"] * bound[DR.DIOU_SUM] / norm + 8 * U * abs(w[DR.REG]) + R.TINY32
            assert (w[DR.POSITIVES] > 0) or ref[DR.REG] == 0.0
            # the two parts make up the last head's sum: the same products, so within the summation term of that sum
            last = DR.HEAD_SUM + K - 1
            assert abs((ref[DR.POS_SUM] + ref[DR.NEG_SUM]) - ref[last]) <= DR.summation_term(xs[-1].numel(), mag[last])
            norm = ref[DR.NORMALISER]          # the next step starts from the reference's own float32 value
    print("%s: worst |reference fp32 - float64| / bound over the sums: %.3g" % (name, worst))
    assert float(fx["final_normaliser"]) == norm


@pytest.mark.parametrize("name", NAMES)
def test_update_epoch_strings_and_best_losses(name):
    """three epochs of two batches, the meter reset after each: the best losses handed back and the reference's strings"""
    fx = load(name)
    m, best = DR.DetMeter(), [float("inf"), float("inf")]
    present = sides_of(fx)
    strings = []
    for b in range(fx["stats"].shape[0]):
        m.update(fx["stats"][b, 0] if "visual" in present else None, fx["stats"][b, 1] if "audio" in present else None,
                 3 if bool(fx["include_verb_noun"]) else 1, fx["total"][b], None)
        if b % 2 == 1:
            before, is_best = DR.update_epoch(best, m.avg("visual"), m.avg("audio"))
            assert same_bits(np.array([before["visual"], before["audio"]]), fx["best_before"][b // 2])
            strings.append(is_best)
            m.reset()
    assert strings == [str(s) for s in fx["is_best"]]
    assert strings[0] == "audio_visual"        # (an absent modality's average is 0.0: a best loss once, as in the reference)


# ================================================================================================ the host side of tim_amd's meter
def header_enum():
    txt = open(os.path.join(ROOT, "include", "timhip.h")).read()
    out = {k: int(v) for k, v in re.findall(r"\b(TIMHIP_DET_(?:METER|STAT)_[A-Z_0-9]+) = (\d+)", txt)}
    out.update({k: int(v) for k, v in re.findall(r"#define (TIMHIP_DET_(?:METER|SIDE)_[A-Z_]+) (\d+)", txt)})
    return out


def test_layout_mirrors_agree():
    """include/timhip.h, tim_amd/_lib.py and the restatement name the same words; 64-bit fields start on even words"""
    from tim_amd import _lib as L
    H = header_enum()
    for slot, name in enumerate(DR.SLOTS):
        assert H["TIMHIP_DET_METER_" + name.upper()] == slot == getattr(L, "DET_METER_" + name.upper())
    for k in ("UPDATES", "SUM", "COUNT", "RUN", "VAL", "LAST", "NORM", "STATE_WORDS", "SLOTS"):
        want = H["TIMHIP_DET_METER_" + k]
        assert getattr(L, "DET_METER_" + k) == want
        assert k == "SLOTS" or getattr(DR, k) == want
    for k in ("HEAD_SUM", "POS_SUM", "NEG_SUM", "VALID", "POSITIVES", "DIOU_SUM", "NORMALISER", "LOSS", "CLS", "REG", "HEAD", "POS", "NEG",
              "RESERVED"):
        assert H["TIMHIP_DET_STAT_" + k] == getattr(L, "DET_STAT_" + k) == getattr(DR, k)
    assert H["TIMHIP_DET_SIDE_STATS_WORDS"] == L.DET_SIDE_STATS_WORDS == DR.STATS_WORDS
    assert H["TIMHIP_DET_SIDE_STATS_PARTIALS"] == L.DET_SIDE_STATS_PARTIALS and H["TIMHIP_DET_SIDE_PARTIALS"] == L.DET_SIDE_PARTIALS == 4096
    assert all(w % 2 == 0 for w in (L.DET_METER_UPDATES, L.DET_METER_SUM, L.DET_METER_COUNT, L.DET_METER_RUN, L.DET_METER_STATE_WORDS))
    assert L.DET_METER_COUNT + 4 * (L.DET_METER_SLOTS - 1) + 2 == L.DET_METER_RUN and L.DET_METER_RUN + 8 == L.DET_METER_VAL
    assert L.DET_METER_VAL + L.DET_METER_SLOTS == L.DET_METER_LAST and L.DET_METER_LAST + 4 == L.DET_METER_NORM
    assert L.DET_METER_NORM + 2 <= L.DET_METER_STATE_WORDS
    assert "timhip_det_meter_update" in L.exported_symbols() and "timhip_det_side_loss_fwd_stats" in L.exported_symbols()


@pytest.mark.parametrize("name", NAMES)
def test_decode_det_state_reads_the_block(name):
    """tim_amd.meters.decode_det_state on the restatement's block after the whole stream: the fixture's averages to the bit,
    counts, last values, the sides' counters and normalisers"""
    from tim_amd.meters import DET_SLOTS, decode_det_state
    assert DET_SLOTS == DR.SLOTS
    fx = load(name)
    _, m = replay(fx)
    d = decode_det_state(m.words())
    assert d["updates"] == fx["stats"].shape[0]
    for s, k in enumerate(DR.SLOTS):
        got = d["losses"][k]
        assert np.float64(got["avg"]).tobytes() == np.float64(fx["slot_avg"][-1, s]).tobytes(), k
        assert got["count"] == int(fx["slot_count"][-1, s]) and np.float64(got["sum"]).tobytes() == fx["slot_sum"][-1, s].tobytes()
        assert np.float32(got["val"]) == m.val[s]
    for s, side in enumerate(DR.SIDES):
        got = d["sides"][side]
        assert got["valid"] == int(fx["stats"][:, s, DR.VALID].sum()) and got["positives"] == int(fx["stats"][:, s, DR.POSITIVES].sum())
        assert got["batch_valid"] == int(fx["stats"][-1, s, DR.VALID]) and got["batch_positives"] == int(fx["stats"][-1, s, DR.POSITIVES])
        assert np.float32(got["normaliser"]) == fx["stats"][-1, s, DR.NORMALISER]
    with pytest.raises(ValueError):
        decode_det_state(np.zeros(10, np.int32))
