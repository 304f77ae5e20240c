#!/usr/bin/env python3
"""Timing of the detection scoring on one MI355X at an EPIC-sized synthetic problem: 3,806 action classes,
about 10^4 ground-truth segments in 138 videos, 2 * 10^6 detections (a tenth of them jittered copies of ground truth, the
rest anywhere, with a skewed class distribution as detections have).

  hip    DetectionScorer.evaluate: device sorts and table building (torch), timhip_det_match, timhip_det_ap and the read of
         the five mAPs; eager, warm, device events around each call; the two library calls also on their own
  host   tests/detmap_ref.py (numpy, one process) on a 1/100 subsample of the detections, host clock

Method: the evaluate is warmed up, then timed --reps times; the median and the spread (min - max) are printed.  The
subsample's host time is NOT a hundredth of the full problem's (its true positives are as many, its false positives fewer):
it is printed as what it is.

    python tools/detmap_bench.py [--reps 10] [--detections 2000000] [--segments 10000]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import detmap_ref as R  # noqa: E402
from tim_amd import DetectionScorer  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tools._timing import timed  # noqa: E402

CLASSES, VIDEOS = 3806, 138


def make_problem(n_gt, n_det, seed=0):
    rng = np.random.default_rng(seed)
    weight = 1.0 / np.arange(1, CLASSES + 1) ** 0.8                       # a long tail of classes
    weight /= weight.sum()
    g_label = rng.choice(CLASSES, size=n_gt, p=weight)
    g_video = rng.integers(0, VIDEOS, size=n_gt)
    start = rng.uniform(0.0, 1800.0, size=n_gt)
    g_seg = np.round(np.stack([start, start + rng.uniform(0.5, 8.0, size=n_gt)], axis=1), 2)
    i = rng.integers(0, n_gt, size=n_det)
    copy = rng.random(n_det) < 0.1
    a = rng.uniform(0.0, 1800.0, size=n_det)
    seg = np.where(copy[:, None], g_seg[i] + rng.normal(0, 0.5, size=(n_det, 2)), np.stack([a, a + rng.uniform(0.5, 8.0, size=n_det)], axis=1))
    seg[:, 0] = np.maximum(seg[:, 0], 0.0)
    seg[:, 1] = np.maximum(seg[:, 1], seg[:, 0] + 0.01)
    label = np.where(copy, g_label[i], rng.choice(CLASSES, size=n_det, p=weight))
    video = np.where(copy, g_video[i], rng.integers(0, VIDEOS, size=n_det))
    score = rng.uniform(0.01, 1.0, size=n_det).astype(np.float32)
    names = ["P%02d_%03d" % (v // 10, v % 10) for v in range(VIDEOS)]
    return ([names[v] for v in g_video], g_seg, g_label), (seg.astype(np.float32), score, label.astype(np.int64), video.astype(np.int64)), names


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--detections", type=int, default=2000000)
    ap.add_argument("--segments", type=int, default=10000)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    (gv, gs, gl), (seg, score, label, video), names = make_problem(args.segments, args.detections)
    sc = DetectionScorer(gv, gs, gl)
    d = [torch.from_numpy(x).to(dev) for x in (seg, score, label, video)]
    mAP, avg = sc.evaluate(*d, names)                                     # warm-up (library load, allocator, sort temporaries)
    sc.evaluate(*d, names)
    ms = lambda fn: tuple(t / 1e3 for t in timed(fn, args.reps, 1))       # one call per window, milliseconds
    med, lo, hi = ms(lambda: sc.evaluate(*d, names))
    groups = sc._host["gt_off"].shape[0] - 1
    print("%d detections, %d ground-truth segments in %d (class, video) groups of up to %d, %d classes; mAP %s avg %.4f"
          % (args.detections, args.segments, groups, int(np.diff(sc._host["gt_off"]).max()), sc.classes.shape[0],
             np.round(mAP, 4).tolist(), avg))
    print("hip   evaluate (sorts + tables + match + ap + read): median %.2f ms (%.2f - %.2f) over %d calls" % (med, lo, hi, args.reps))

    # the two library calls on their own, on the tables of the last evaluate (rebuilt here as evaluate builds them)
    st = sc._state(dev)
    T, C, G, V, M = 5, sc.classes.shape[0], args.segments, sc._V, args.detections
    order = sc.order
    lab = d[2]
    cls = torch.searchsorted(st["classes"], lab).clamp_(max=C - 1)
    cls = torch.where(st["classes"][cls] == lab, cls, C)
    lut = torch.from_numpy(np.asarray([sc._video_index.get(v, V - 1) for v in names], np.int64)).to(dev)
    cls_s = cls[order]
    class_off = torch.searchsorted(cls_s, torch.arange(C + 1, device=dev)).to(torch.int32)
    pseg = (torch.round(d[0].to(torch.float64) * 1000) / 1000)[order].contiguous()
    ks, gp = torch.sort(cls_s * V + lut[d[3]][order], stable=True)
    gp = gp.to(torch.int32)
    plo = torch.searchsorted(ks, st["group_key"]).to(torch.int32)
    phi = torch.searchsorted(ks, st["group_key"], right=True).to(torch.int32)
    pos0 = class_off[st["group_cls"]].contiguous()
    tp = torch.zeros((T, M), dtype=torch.uint8, device=dev)
    lock = torch.full((T, G), -1, dtype=torch.int32, device=dev)
    apd = torch.zeros((T, C), dtype=torch.float64, device=dev)

    def match():
        tp.zero_()
        lock.fill_(-1)
        L.call("timhip_det_match", L.ptr(pseg), M, L.ptr(gp), L.ptr(plo), L.ptr(phi), L.ptr(pos0), L.ptr(st["gt_seg"]), G,
               L.ptr(st["gt_off"]), groups, L.ptr(st["thr"]), T, L.ptr(tp), L.ptr(lock), L.ptr(st["work"]), None)

    def avp():
        L.call("timhip_det_ap", L.ptr(tp), M, L.ptr(class_off), L.ptr(st["npos"]), C, T, L.ptr(apd), None)
    match()
    avp()
    assert torch.equal(apd, sc.ap)
    print("hip   timhip_det_match (+ the two fills): median %.3f ms (%.3f - %.3f)" % ms(match))
    print("hip   timhip_det_ap: median %.3f ms (%.3f - %.3f)" % ms(avp))

    if not args.no_host:
        sub = np.arange(0, args.detections, 100)
        t0 = time.perf_counter()
        _, _, ap_h, _ = R.evaluate(gv, gs, gl, [names[v] for v in video[sub]], R.round_segments(seg[sub]), score[sub].astype(np.float64),
                                   label[sub], sc.tiou_thresholds)
        t1 = time.perf_counter()
        print("host  tests/detmap_ref.py on every 100th detection (%d): %.2f s, avg mAP %.4f" % (sub.shape[0], t1 - t0, ap_h.mean()))


if __name__ == "__main__":
    main()
