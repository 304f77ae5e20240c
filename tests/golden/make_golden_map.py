"""Golden vectors for the detection scoring from the reference's own scoring script (build container only).

    python tests/golden/make_golden_map.py

Imports detection/eval_detection/evaluate_detection_json.py of the reference from its own directory (the module only builds
its argparse parser when imported) and runs ANETdetection(...).evaluate() on seeded synthetic inputs: 6 videos with ground
truth and one without, 7 ground-truth classes of which one gets no predictions, 2 further prediction labels the ground truth
does not have, about 400 ground-truth segments and about 3000 predictions, half of them jittered copies of ground truth;
one (class, video) group of more than 128 segments, one of exactly 1.  Ground-truth times are "HH:MM:SS.ss" strings, as the
annotation files carry them; prediction segments have three decimals and fp32-origin scores, as a submission file does.

The maker leaves out the few predictions that break them and then asserts the conditions under which the reference itself is well defined (its numpy sorts leave ties undefined): no
two predictions of one class have equal scores, no prediction sees two segments of its group at an equal nonzero tIoU, every
tIoU is at least 1e-12 away from every threshold.

tests/golden/detmap_small.npz holds the inputs and the reference's outputs - numbers and names only, nothing of the
reference: ap, mAP, average_mAP and the score / matched_gt / iou columns of correct_predictions (matched_gt -1: None).
tests/golden/detmap_ties.npz is made without the reference: equal scores, duplicated ground-truth segments, predictions
that sit at equal tIoU to two segments; expected tp / lock / ap from tests/detmap_ref.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import detmap_ref as R  # noqa: E402

SEED = 20267
THRESHOLDS = np.linspace(0.1, 0.5, 5)
GT_VIDEOS = ["P01_11", "P02_03", "P04_101", "P07_08", "P22_16", "P30_05"]
NO_GT_VIDEO = "P35_109"
GT_LABELS = [3, 8, 15, 21, 40, 77, 120]                   # 120 gets no predictions
FOREIGN_LABELS = [5, 99]


def stamp(sec):
    cs = int(round(sec * 100))
    return "%02d:%02d:%02d.%02d" % (cs // 360000, cs // 6000 % 60, cs // 100 % 60, cs % 100)


def make_small():
    rng = np.random.default_rng(SEED)
    gt = []                                                # (video, start, stop, label)

    def segments(n, video, label, span):
        start = np.sort(rng.uniform(0.0, span, size=n))
        length = rng.uniform(0.4, 6.0, size=n)
        for s, w in zip(start, length):
            a = R.timestamp_to_seconds(stamp(s))
            b = R.timestamp_to_seconds(stamp(s + w))
            assert b > a
            gt.append((video, stamp(s), stamp(s + w), label))

    segments(140, "P01_11", 3, 4000.0)                     # more than 128 segments in one group: the workspace path
    segments(1, "P02_03", 3, 600.0)                        # exactly one
    segments(64, "P04_101", 8, 2500.0)
    segments(65, "P07_08", 8, 2500.0)
    for label in (15, 21, 40, 77, 120):
        for video in GT_VIDEOS:
            n = int(rng.integers(0, 9))
            if n:
                segments(n, video, label, 1200.0)
    order = rng.permutation(len(gt))                       # groups are not contiguous in the annotation table
    gt = [gt[i] for i in order]
    g_video = np.asarray([g[0] for g in gt])
    g_start = np.asarray([g[1] for g in gt])
    g_stop = np.asarray([g[2] for g in gt])
    g_label = np.asarray([g[3] for g in gt], np.int64)
    g_sec = np.asarray([[R.timestamp_to_seconds(a), R.timestamp_to_seconds(b)] for a, b in zip(g_start, g_stop)], np.float64)
    narration = 5000 + 3 * np.arange(len(gt))

    n_pred = 3000
    pred = []
    usable = np.nonzero(g_label != 120)[0]
    for _ in range(n_pred // 2):                           # jittered copies of ground truth, sometimes in another video
        i = int(rng.choice(usable))
        s = g_sec[i, 0] + rng.normal(0, 0.8)
        e = g_sec[i, 1] + rng.normal(0, 0.8)
        v = g_video[i] if rng.random() < 0.9 else str(rng.choice(GT_VIDEOS + [NO_GT_VIDEO]))
        lab = int(g_label[i]) if rng.random() < 0.9 else int(rng.choice(GT_LABELS[:-1] + FOREIGN_LABELS))
        pred.append((v, s, e, lab))
    for _ in range(n_pred - n_pred // 2):
        s = rng.uniform(0.0, 4000.0)
        pred.append((str(rng.choice(GT_VIDEOS + [NO_GT_VIDEO])), s, s + rng.uniform(0.3, 8.0),
                     int(rng.choice(GT_LABELS[:-1] + FOREIGN_LABELS))))
    p_seg32 = np.asarray([[max(p[1], 0.0), p[2]] for p in pred], np.float32)
    p_seg = np.asarray([[round(float(a), 3), round(float(b), 3)] for a, b in p_seg32], np.float64)
    ok = p_seg[:, 1] > p_seg[:, 0]
    p_video = np.asarray([p[0] for p in pred])[ok]
    p_label = np.asarray([p[3] for p in pred], np.int64)[ok]
    p_seg = p_seg[ok]
    p_score = rng.uniform(0.01, 1.0, size=p_seg.shape[0]).astype(np.float32).astype(np.float64)
    # a submission lists its detections video by video, by descending score
    vids = GT_VIDEOS[3:] + [NO_GT_VIDEO] + GT_VIDEOS[:3]
    o = np.concatenate([np.nonzero(p_video == v)[0][np.argsort(-p_score[p_video == v], kind="stable")] for v in vids])
    p_video, p_label, p_seg, p_score = p_video[o], p_label[o], p_seg[o], p_score[o]
    return (g_video, g_start, g_stop, g_sec, g_label, narration), (vids, p_video, p_seg, p_score, p_label)


def ill_defined(gt, pred):
    """rows of predictions that sit on a threshold or at an equal nonzero tIoU to two segments (millisecond predictions
    against centisecond ground truth reach 1/5 or 1/2 exactly now and then): main() leaves them out"""
    g_video, _, _, g_sec, g_label, _ = gt
    _, p_video, p_seg, p_score, p_label = pred
    bad = []
    for i, (v, (ps, pe), lab) in enumerate(zip(p_video, p_seg, p_label)):
        g = g_sec[(g_label == lab) & (g_video == v)]
        if len(g):
            t = R.tiou(ps, pe, g[:, 0], g[:, 1])
            nz = t[t > 0]
            if len(np.unique(nz)) != len(nz) or np.abs(t[:, None] - THRESHOLDS[None, :]).min() < 1e-12:
                bad.append(i)
    return bad


def assert_well_defined(gt, pred):
    g_video, _, _, g_sec, g_label, _ = gt
    _, p_video, p_seg, p_score, p_label = pred
    for lab in np.unique(g_label):
        sc = p_score[p_label == lab]
        assert len(np.unique(sc)) == len(sc), "equal scores in class %d" % lab
    n_big = n_one = 0
    for lab in np.unique(g_label):
        for v in np.unique(g_video):
            g = g_sec[(g_label == lab) & (g_video == v)]
            n_big += len(g) > 128
            n_one += len(g) == 1
            if not len(g):
                continue
            for ps, pe in p_seg[(p_label == lab) & (p_video == v)]:
                t = R.tiou(ps, pe, g[:, 0], g[:, 1])
                nz = t[t > 0]
                assert len(np.unique(nz)) == len(nz), "a prediction sees two segments at an equal tIoU"
                assert np.abs(t[:, None] - THRESHOLDS[None, :]).min() >= 1e-12, "a tIoU on a threshold"
    assert n_big >= 1 and n_one >= 1


def run_reference(gt, pred):
    import pandas as pd
    sys.path.insert(0, "/root/reference/detection/eval_detection")
    import evaluate_detection_json as E
    g_video, g_start, g_stop, g_sec, g_label, narration = gt
    vids, p_video, p_seg, p_score, p_label = pred
    ann = pd.DataFrame({"video_id": g_video, "start_timestamp": g_start, "stop_timestamp": g_stop, "action_class": g_label},
                       index=narration)
    results = {v: [] for v in vids}
    for v, s, c, lab in zip(p_video, p_seg, p_score, p_label):
        results[str(v)].append({"action": int(lab), "score": float(c), "segment": [float(s[0]), float(s[1])]})
    det = E.ANETdetection(ann, {"results": results}, tiou_thresholds=THRESHOLDS)
    assert np.array_equal(det.ground_truth["t-start"].values, g_sec[:, 0])
    assert np.array_equal(det.ground_truth["t-end"].values, g_sec[:, 1])
    mAP, avg = det.evaluate()
    cp = det.correct_predictions
    matched = np.asarray([-1 if m is None or m != m else int(m) for m in cp["matched_gt"]], np.int64)
    return (det.ap, np.asarray(mAP), float(avg), cp["score"].values.astype(np.float64), cp["action"].values.astype(np.int64),
            matched, cp["iou"].values.astype(np.float64))


def make_ties():
    """equal scores, duplicated segments, equal nonzero tIoU: only the project's tie rules decide"""
    rng = np.random.default_rng(SEED + 1)
    g_video, g_seg, g_label = [], [], []
    for lab in (2, 4, 9):
        for v in ("a", "b", "c"):
            n = int(rng.integers(1, 7))
            base = np.round(rng.uniform(0, 50, size=n) * 4) / 4
            for s in base:
                for _ in range(int(rng.integers(1, 4))):                 # duplicates
                    g_video.append(v)
                    g_seg.append((s, s + 2.0))
                    g_label.append(lab)
    g_seg = np.asarray(g_seg, np.float64)
    o = rng.permutation(len(g_label))
    g_video, g_seg, g_label = np.asarray(g_video)[o], g_seg[o], np.asarray(g_label, np.int64)[o]
    n = 400
    i = rng.integers(0, len(g_label), size=n)
    shift = rng.choice([-1.0, -0.5, 0.0, 0.5, 1.0], size=n)              # symmetric shifts: equal tIoU to neighbours
    p_seg = g_seg[i] + shift[:, None]
    p_seg[:, 0] = np.maximum(p_seg[:, 0], 0.0)
    p_video = np.where(rng.random(n) < 0.85, g_video[i], rng.choice(["a", "b", "c", "d"], size=n))
    p_label = np.where(rng.random(n) < 0.85, g_label[i], rng.choice([2, 4, 9, 11], size=n)).astype(np.int64)
    p_score = (rng.integers(1, 12, size=n) / 16.0).astype(np.float64)    # many equal scores
    return (g_video, g_seg, g_label), (p_video, p_seg, p_score, p_label)


def main():
    gt, pred = make_small()
    bad = ill_defined(gt, pred)
    keep = np.setdiff1d(np.arange(len(pred[4])), bad)
    pred = (pred[0],) + tuple(a[keep] for a in pred[1:])
    print("left out %d predictions on a threshold or at an equal tIoU to two segments" % len(bad))
    assert_well_defined(gt, pred)
    ap, mAP, avg, cp_score, cp_action, cp_matched, cp_iou = run_reference(gt, pred)
    g_video, g_start, g_stop, g_sec, g_label, narration = gt
    vids, p_video, p_seg, p_score, p_label = pred
    out = os.path.join(HERE, "detmap_small.npz")
    np.savez_compressed(out, seed=SEED, thresholds=THRESHOLDS, gt_video=g_video, gt_start=g_start, gt_stop=g_stop,
                        gt_seconds=g_sec, gt_label=g_label, gt_narration=narration, video_ids=np.asarray(vids),
                        pred_video=p_video, pred_seg=p_seg, pred_score=p_score, pred_label=p_label, ap=ap, mAP=mAP,
                        average_mAP=avg, cp_score=cp_score, cp_action=cp_action, cp_matched_gt=cp_matched, cp_iou=cp_iou)
    print("small: %d gt, %d predictions, mAP %s -> %s, %d bytes" % (len(g_label), len(p_label), mAP, out, os.path.getsize(out)))

    (tv, ts, tl), (qv, qs, qc, ql) = make_ties()
    thr = np.asarray([0.1, 1.0 / 3.0, 0.5, 0.5, 1.0])                    # 1/3 and 1 are tIoUs the shifted copies reach exactly
    tp, lock, tap, tab = R.evaluate(tv, ts, tl, qv, qs, qc, ql, thr)
    assert len(np.unique(qc)) < len(qc) // 4
    out = os.path.join(HERE, "detmap_ties.npz")
    np.savez_compressed(out, seed=SEED + 1, thresholds=thr, gt_video=tv, gt_seg=ts, gt_label=tl, pred_video=qv, pred_seg=qs,
                        pred_score=qc, pred_label=ql, tp=tp, lock=lock, ap=tap)
    print("ties: %d gt, %d predictions, %d true positives at thr[0], mean ap %s -> %s, %d bytes"
          % (len(tl), len(ql), int(tp[0].sum()), tap.mean(axis=1), out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
