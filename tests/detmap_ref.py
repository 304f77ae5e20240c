"""float64 numpy restatement of the detection scoring (tim_amd/csrc/detmap.hip + tim_amd/detmap.py), written
from the description of the metric: ActivityNet-style interpolated average precision per class and tIoU threshold.

    tab = prepare(gt_video, gt_seg, gt_label, p_video, p_seg, p_score, p_label)    the sorted / grouped tables
    tp, lock = match(tab, thresholds)                                              [T, N] uint8, [T, G] int32
    ap = average_precision(tp, tab, T)                                             [T, C'] float64
    tp, lock, ap, tab = evaluate(...)                                              the three in one call

Rules (the project's, where numpy's default sort leaves the reference's undefined):
  * classes are the sorted unique ground-truth labels; predictions of other labels are dropped;
  * predictions are ordered by class ascending, then score descending, equal scores in reverse input order; a prediction's
    position is its row in that order, its rank the position minus its class's first position;
  * ground-truth segments keep their input order inside a (class, video) group; `lock` is indexed by the INPUT row;
  * a prediction takes, at threshold t, the segment of its (class, video) group with the largest tIoU among those with
    tIoU >= thr[t] not yet taken at t; among exactly equal tIoU the segment with the higher index inside the group;
  * tIoU = inter / union, inter = max(min(pe, ge) - max(ps, gs), 0), union = (ge - gs) + (pe - ps) - inter.
"""
import numpy as np


def timestamp_to_seconds(ts):
    h, m, s = (float(x) for x in ts.split(":"))
    return h * 3600 + m * 60 + s


def round_segments(x):
    """three decimals, as the submission file carries them"""
    return np.rint(np.asarray(x, np.float64) * 1000) / 1000


def order_predictions(cls, score):
    """class ascending, score descending, equal scores in reverse input order"""
    rev = np.arange(len(score))[::-1]
    o = rev[np.argsort(-score[rev], kind="stable")]
    return o[np.argsort(cls[o], kind="stable")]


def prepare(gt_video, gt_seg, gt_label, p_video, p_seg, p_score, p_label):
    gt_label = np.asarray(gt_label, np.int64)
    gt_seg = np.asarray(gt_seg, np.float64).reshape(-1, 2)
    classes = np.unique(gt_label)
    C = len(classes)
    names = sorted(set(str(v) for v in gt_video))
    vidx = {v: i for i, v in enumerate(names)}
    V = len(names) + 1                                          # slot V - 1: a video without ground truth
    g_cls = np.searchsorted(classes, gt_label)
    g_vid = np.asarray([vidx[str(v)] for v in gt_video], np.int64)
    g_key = g_cls * V + g_vid
    g_order = np.argsort(g_key, kind="stable")
    keys, start = np.unique(g_key[g_order], return_index=True)
    gt_off = np.concatenate([start, [len(g_key)]]).astype(np.int32)

    p_label = np.asarray(p_label, np.int64)
    keep = np.nonzero(np.isin(p_label, classes))[0]             # input rows that survive, in input order
    p_cls = np.searchsorted(classes, p_label[keep])
    p_score = np.asarray(p_score, np.float64)[keep]
    p_seg = np.asarray(p_seg, np.float64).reshape(-1, 2)[keep]
    p_vid = np.asarray([vidx.get(str(v), V - 1) for v in np.asarray(p_video)[keep]], np.int64)
    o = order_predictions(p_cls, p_score)
    cls_s = p_cls[o]
    class_off = np.searchsorted(cls_s, np.arange(C + 1)).astype(np.int32)
    p_key = cls_s * V + p_vid[o]
    group_pred = np.argsort(p_key, kind="stable").astype(np.int32)
    ks = p_key[group_pred]
    return {
        "classes": classes, "pred_seg": np.ascontiguousarray(p_seg[o]), "pred_score": p_score[o],
        "pred_cls": cls_s, "pred_input_row": keep[o], "class_off": class_off,
        "npos": np.bincount(g_cls, minlength=C).astype(np.int32),
        "gt_seg": np.ascontiguousarray(gt_seg[g_order]), "gt_order": g_order, "gt_off": gt_off,
        "group_cls": (keys // V).astype(np.int64), "group_pred": group_pred,
        "group_pred_lo": np.searchsorted(ks, keys, side="left").astype(np.int32),
        "group_pred_hi": np.searchsorted(ks, keys, side="right").astype(np.int32),
        "group_pos0": class_off[keys // V].astype(np.int32),
    }


def tiou(ps, pe, gs, ge):
    inter = np.maximum(np.minimum(pe, ge) - np.maximum(ps, gs), 0.0)
    union = (ge - gs) + (pe - ps) - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / union


def match_tables(tab, thresholds):
    """-> tp [T, N] uint8, lock [T, G] int32 indexed by the GROUPED ground-truth row (what the kernel writes)"""
    thr = np.asarray(thresholds, np.float64).reshape(-1)
    T, N, G = len(thr), tab["pred_seg"].shape[0], tab["gt_seg"].shape[0]
    tp = np.zeros((T, N), np.uint8)
    lock = np.full((T, G), -1, np.int32)
    for g in range(len(tab["gt_off"]) - 1):
        g0, g1 = int(tab["gt_off"][g]), int(tab["gt_off"][g + 1])
        gs, ge = tab["gt_seg"][g0:g1, 0], tab["gt_seg"][g0:g1, 1]
        idx = np.arange(g1 - g0)
        for i in range(int(tab["group_pred_lo"][g]), int(tab["group_pred_hi"][g])):
            pos = int(tab["group_pred"][i])
            v = tiou(tab["pred_seg"][pos, 0], tab["pred_seg"][pos, 1], gs, ge)
            for t in range(T):
                ok = (v >= thr[t]) & (lock[t, g0:g1] < 0)
                if not ok.any():
                    continue
                best = v[ok].max()
                j = int(idx[ok & (v == best)].max())
                lock[t, g0 + j] = pos - int(tab["group_pos0"][g])
                tp[t, pos] = 1
    return tp, lock


def match(tab, thresholds):
    """-> tp [T, N] uint8 by position, lock [T, G] int32 by the ground truth's INPUT row"""
    tp, lock_g = match_tables(tab, thresholds)
    lock = np.empty_like(lock_g)
    lock[:, tab["gt_order"]] = lock_g
    return tp, lock


def average_precision(tp, tab, T=None):
    T = tp.shape[0] if T is None else T
    C = len(tab["classes"])
    ap = np.zeros((T, C), np.float64)
    for c in range(C):
        lo, hi = int(tab["class_off"][c]), int(tab["class_off"][c + 1])
        npos = float(tab["npos"][c])
        if hi <= lo:
            continue
        for t in range(T):
            f = tp[t, lo:hi].astype(np.float64)
            tpc = np.cumsum(f)
            prec = tpc / np.arange(1, hi - lo + 1, dtype=np.float64)
            mx = np.maximum.accumulate(prec[::-1])[::-1]
            k = np.nonzero(f)[0]
            ap[t, c] = np.sum((tpc[k] / npos - (tpc[k] - 1.0) / npos) * mx[k])
    return ap


def evaluate(gt_video, gt_seg, gt_label, p_video, p_seg, p_score, p_label, thresholds):
    tab = prepare(gt_video, gt_seg, gt_label, p_video, p_seg, p_score, p_label)
    tp, lock = match(tab, thresholds)
    return tp, lock, average_precision(tp, tab), tab
