"""TEST INFRASTRUCTURE ONLY: numpy restatement of the detection inference tail - what the reference's
FeatureMeter.update (detection/time_interval_machine/utils/meters.py) and eval_detection/format_predictions.py compute
between the heads' outputs and the submission, written from their contract.  tests/test_detect_ref.py pins it to a
fixture recorded from the reference itself; tests/test_gpu_detect.py then checks the HIP kernels and
tim_amd.DetectionCollector against it.  The NMS goes through oracle.nms_oracle.  Never imported by tim_amd."""
import numpy as np

from oracle import nms_oracle


def sigmoid32(x):
    """the float64 sigmoid rounded once to fp32 (the device evaluates exactly this expression)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


def proposals(reg, window_start, window_size, max_time, num_queries):
    """-> [R, 2] float64: the decoded proposals, NOT rounded (what the reference saves as v_proposals)"""
    reg = np.asarray(reg, dtype=np.float32)
    p = np.minimum(np.maximum(reg, np.float32(0.0)), np.float32(max_time))              # fp32 clamp (NaN propagates)
    p = (p * np.float32(window_size)).astype(np.float32)                                # fp32 product, rounded once
    start = np.repeat(np.asarray(window_start, dtype=np.float64), num_queries)
    return p.astype(np.float64) + start[:, None]                                        # the sum is float64


def decode(reg, window_start, window_size, max_time, num_queries):
    """-> (seg64 [R, 2] float64 rounded to three decimals, ok [R] bool)"""
    p = proposals(reg, window_start, window_size, max_time, num_queries)
    p = np.rint(p * 1000.0) / 1000.0                                                    # numpy.round(p, 3)
    return p, (p[:, 1] - p[:, 0]) > 0.0


def batch_candidates(logits, reg, window_start, window_size, max_time, video_index, score_threshold):
    """one batch -> dict(seg [N, 2] fp32, score [N] fp32, key [N] int64, row [N] int32, cls [N], video [N]): proposal by
    proposal, ascending class inside a proposal"""
    logits = np.asarray(logits, dtype=np.float32)
    R, C = logits.shape
    B = len(window_start)
    nq = R // B
    seg64, ok = decode(reg, window_start, window_size, max_time, nq)
    score = sigmoid32(logits)
    passed = (score > np.float32(score_threshold)) & ok[:, None]
    rows, cls = np.nonzero(passed)                      # row-major: rows ascending, classes ascending inside a row
    video = np.asarray(video_index, dtype=np.int64)[rows // nq]
    return dict(seg=seg64[rows].astype(np.float32), score=score[rows, cls], key=video * C + cls,
                row=rows.astype(np.int32), cls=cls.astype(np.int64), video=video, seg32=seg64.astype(np.float32), ok=ok)


class CollectorBase:
    """what the numpy mirrors of the two collectors share: the video index and the per-video NMS loop"""

    def __init__(self):
        self.video_ids, self._index, self.chunks = [], {}, []

    def _video_index(self, video_ids):
        idx = []
        for v in video_ids:
            v = str(v)
            if v not in self._index:
                self._index[v] = len(self.video_ids)
                self.video_ids.append(v)
            idx.append(self._index[v])
        return idx

    def _nms_per_video(self, c, labels, iou_threshold, min_score, sigma, method, nms):
        """candidates `c` with `labels` -> (segs, scores, labels, video) ordered by video, then descending score (stable)"""
        out = [[], [], [], []]
        for v in range(len(self.video_ids)):
            m = c["video"] == v
            if not m.any():
                continue
            s, sc, lb = nms_oracle.batched_nms(c["seg"][m], c["score"][m], labels[m], iou_threshold, min_score, sigma, method, nms)
            out[0].append(s); out[1].append(sc); out[2].append(lb); out[3].append(np.full(len(sc), v, np.int64))
        if not out[1]:
            return np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
        return tuple(np.concatenate(o) for o in out)


class Collector(CollectorBase):
    """numpy mirror of tim_amd.DetectionCollector"""

    def __init__(self, num_classes, score_threshold=0.01):
        super().__init__()
        self.C, self.thr = int(num_classes), score_threshold

    def update(self, logits, reg, query_times, video_ids, window_start, window_size):
        idx = self._video_index(video_ids)
        max_time = np.asarray(query_times, dtype=np.float32).max()
        self.chunks.append(batch_candidates(logits, reg, window_start, window_size, max_time, idx, self.thr))

    def candidates(self):
        if not self.chunks:
            return dict(seg=np.zeros((0, 2), np.float32), score=np.zeros(0, np.float32), key=np.zeros(0, np.int64),
                        cls=np.zeros(0, np.int64), video=np.zeros(0, np.int64))
        return {k: np.concatenate([c[k] for c in self.chunks]) for k in ("seg", "score", "key", "cls", "video")}

    def detections(self, sigma=0.1, iou_threshold=0.1, min_score=0.001, method=2, nms="soft"):
        """-> (segs, scores, labels, video) ordered by video, then descending score (stable)"""
        c = self.candidates()
        return self._nms_per_video(c, c["cls"], iou_threshold, min_score, sigma, method, nms)

    def results(self, **nms_args):
        s, sc, lb, vd = self.detections(**nms_args)
        res = {v: [] for v in self.video_ids}
        for i in range(len(sc)):
            res[self.video_ids[int(vd[i])]].append({"action": int(lb[i]), "score": float(sc[i]),
                                                    "segment": [round(float(s[i, 0]), 3), round(float(s[i, 1]), 3)]})
        return res
