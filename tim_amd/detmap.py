"""Detection scoring on the MI355X: per-video detections in, per-class AP and mAP out.

`DetectionScorer` takes the place of the reference's `eval_detection/evaluate_detection_json.py` (`ANETdetection`): the
ActivityNet-style interpolated average precision per ground-truth class at tIoU 0.1 ... 0.5 and its means.  Sorting and
grouping are torch device sorts, matching and AP are the two library calls of tim_amd/csrc/detmap.hip; what comes back to
the host is the `T` mean values.  There is no CPU path: the kernels run or the call raises.

        sc = DetectionScorer(gt_video_ids, gt_segments, gt_labels)            # strings, float64 seconds [G, 2], integer labels
        mAP, avg = sc.score(collector, sigma=0.1)                             # a DetectionCollector and its NMS arguments
        mAP, avg = sc.evaluate(segs, scores, labels, video, video_ids)        # what collector.detections() returns
        mAP, avg = sc.evaluate_results(results)                               # a submission's `results` dict (host)
        sc.ap, sc.classes                                                     # [T, C'] float64 on the device; the labels

Semantics are the reference's: classes are the sorted unique ground-truth labels, predictions of other labels are dropped,
a prediction in a video without ground truth of its class is a false positive at every threshold.  Predictions are ordered
by class, then by descending score; equal scores go in REVERSE input order (`argsort()[::-1]` under a stable sort - numpy's
default sort, which the reference uses, does not define the order of ties, so this rule is the project's).  Among segments
at exactly equal tIoU the one later in the ground truth wins (same remark).
"""
import numpy as np
import torch

from . import _lib as L
from ._collect import require_gpu
from ._lib import call, ptr
from .functional import _stream

MAX_THRESHOLDS = 16   # include/timhip.h: TIMHIP_DET_MAX_THRESHOLDS


def timestamp_to_seconds(timestamp):
    """"HH:MM:SS.ss" -> seconds, h * 3600 + m * 60 + s evaluated in that order in float64 (as the reference does)"""
    h, m, s = (float(x) for x in timestamp.split(":"))
    return h * 3600 + m * 60 + s


_WHO = ("DetectionScorer.evaluate", "detection scoring runs")


class DetectionScorer:
    def __init__(self, gt_video_ids, gt_segments, gt_labels, tiou_thresholds=np.linspace(0.1, 0.5, 5), round_segments=True):
        thr = np.asarray(tiou_thresholds, dtype=np.float64).reshape(-1)
        if not 1 <= thr.shape[0] <= MAX_THRESHOLDS:
            raise ValueError("1 to %d tIoU thresholds, got %d" % (MAX_THRESHOLDS, thr.shape[0]))
        seg = np.asarray(gt_segments, dtype=np.float64)
        labels = np.asarray(gt_labels).astype(np.int64).reshape(-1)
        vids = [str(v) for v in gt_video_ids]
        if seg.ndim != 2 or seg.shape[1] != 2 or not (seg.shape[0] == labels.shape[0] == len(vids)):
            raise ValueError("ground truth: %d video ids, segments of shape %s, %d labels"
                             % (len(vids), seg.shape, labels.shape[0]))
        if labels.shape[0] == 0:
            raise ValueError("the ground truth is empty")
        self.tiou_thresholds = thr
        self.round_segments = bool(round_segments)
        self.classes = np.unique(labels)
        names = sorted(set(vids))
        self._video_index = {v: i for i, v in enumerate(names)}
        self._V = len(names) + 1                                 # slot V - 1: a video without ground truth
        cls = np.searchsorted(self.classes, labels)
        key = cls * self._V + np.asarray([self._video_index[v] for v in vids], dtype=np.int64)
        self.gt_order = np.argsort(key, kind="stable")           # (class, video) groups; input order inside a group
        keys, start = np.unique(key[self.gt_order], return_index=True)
        self._host = {
            "gt_seg": np.ascontiguousarray(seg[self.gt_order]), "gt_order": self.gt_order.astype(np.int64),
            "gt_off": np.concatenate([start, [key.shape[0]]]).astype(np.int32), "group_key": keys.astype(np.int64),
            "group_cls": (keys // self._V).astype(np.int64),
            "npos": np.bincount(cls, minlength=self.classes.shape[0]).astype(np.int32),
            "thr": thr, "classes": self.classes.astype(np.int64),
        }
        self._dev = {}
        self.ap = self.tp = self.lock = self.order = None

    def _state(self, dev):
        st = self._dev.get(dev)
        if st is None:
            st = self._dev[dev] = {k: torch.from_numpy(v).to(dev) for k, v in self._host.items()}
            st["work"] = torch.empty((self._host["gt_seg"].shape[0],), dtype=torch.int32, device=dev)
        return st

    def evaluate(self, segs, scores, labels, video, video_ids, round_segments=None):
        """segs [M, 2], scores [M], labels [M], video [M] (index into `video_ids`), device tensors -> (mAP [T] numpy float64,
        their mean).  Leaves `ap` [T, C'], `tp` [T, M] (by position: class, then descending score; columns of dropped labels
        at the end, all 0), `order` [M] (position -> input row) and `lock` [T, G] (ground-truth input row -> the rank inside
        its class of the prediction that took it, -1: none) on the device."""
        for t, what in ((segs, "segs"), (scores, "scores"), (labels, "labels"), (video, "video")):
            require_gpu(t, _WHO, what)
        M = scores.shape[0]
        if scores.dim() != 1 or tuple(segs.shape) != (M, 2) or tuple(labels.shape) != (M,) or tuple(video.shape) != (M,):
            raise ValueError("segs %s, scores %s, labels %s, video %s do not describe one list of detections"
                             % (tuple(segs.shape), tuple(scores.shape), tuple(labels.shape), tuple(video.shape)))
        L.load()
        dev = scores.device
        st = self._state(dev)
        T, C, G, V = self.tiou_thresholds.shape[0], self.classes.shape[0], self._host["gt_seg"].shape[0], self._V
        ap = torch.zeros((T, C), dtype=torch.float64, device=dev)
        tp = torch.zeros((T, M), dtype=torch.uint8, device=dev)
        lock = torch.full((T, G), -1, dtype=torch.int32, device=dev)
        order = torch.zeros((M,), dtype=torch.int64, device=dev)
        if M > 0:
            nv = len(video_ids)
            lut = torch.from_numpy(np.asarray([self._video_index.get(str(v), V - 1) for v in video_ids] + [V - 1],
                                              dtype=np.int64)).to(dev)
            video = video.to(torch.int64)
            vid = lut[torch.where((video >= 0) & (video < nv), video, nv)]
            lab = labels.to(torch.int64)
            cls = torch.searchsorted(st["classes"], lab).clamp_(max=C - 1)
            cls = torch.where(st["classes"][cls] == lab, cls, C)                 # C: a label the ground truth does not have
            rev = torch.arange(M - 1, -1, -1, device=dev)
            order = rev[torch.sort(-scores.to(torch.float64)[rev], stable=True).indices]
            order = order[torch.sort(cls[order], stable=True).indices]
            cls_s = cls[order]
            class_off = torch.searchsorted(cls_s, torch.arange(C + 1, device=dev)).to(torch.int32)
            seg = segs.to(torch.float64)
            if self.round_segments if round_segments is None else round_segments:
                seg = torch.round(seg * 1000) / 1000
            pseg = seg[order].contiguous()
            ks, gp = torch.sort(cls_s * V + vid[order], stable=True)
            gp = gp.to(torch.int32)
            lo = torch.searchsorted(ks, st["group_key"]).to(torch.int32)
            hi = torch.searchsorted(ks, st["group_key"], right=True).to(torch.int32)
            pos0 = class_off[st["group_cls"]].contiguous()
            s = _stream()
            call("timhip_det_match", ptr(pseg), M, ptr(gp), ptr(lo), ptr(hi), ptr(pos0), ptr(st["gt_seg"]), G,
                 ptr(st["gt_off"]), st["group_key"].shape[0], ptr(st["thr"]), T, ptr(tp), ptr(lock), ptr(st["work"]), s)
            call("timhip_det_ap", ptr(tp), M, ptr(class_off), ptr(st["npos"]), C, T, ptr(ap), s)
        self.ap, self.tp, self.order = ap, tp, order
        self.lock = torch.empty_like(lock)
        self.lock[:, st["gt_order"]] = lock
        mAP = ap.mean(dim=1).cpu().numpy()                                       # the one device-to-host read
        return mAP, float(mAP.mean())

    def score(self, collector, **nms_args):
        """the detections of a `DetectionCollector` (its grouped NMS runs with `nms_args`)"""
        return self.evaluate(*collector.detections(**nms_args), collector.video_ids)

    def evaluate_results(self, results, device=None):
        """a submission's `results` dict {video_id: [{"action", "score", "segment"}]}, read video by video as the reference
        reads the file; the segments are taken as they stand"""
        if not torch.cuda.is_available():
            raise L.TimHipError("DetectionScorer runs on the MI355X HIP kernels only (no CPU fallback)")
        dev = torch.device("cuda") if device is None else torch.device(device)
        video_ids = list(results)
        rows = [(i, int(d["action"]), float(d["score"]), float(d["segment"][0]), float(d["segment"][1]))
                for i, v in enumerate(video_ids) for d in results[v]]
        a = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
        return self.evaluate(torch.from_numpy(np.ascontiguousarray(a[:, 3:5])).to(dev), torch.from_numpy(a[:, 2].copy()).to(dev),
                             torch.from_numpy(a[:, 1].astype(np.int64)).to(dev), torch.from_numpy(a[:, 0].astype(np.int64)).to(dev),
                             video_ids, round_segments=False)
