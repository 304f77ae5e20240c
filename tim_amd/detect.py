"""Detection inference tail on the MI355X: class logits and regressed segments in, per-video detections out.

`DetectionCollector` takes the place of the reference's `FeatureMeter` (detection/time_interval_machine/utils/meters.py)
plus `eval_detection/format_predictions.py`: `update()` has `FeatureMeter.update`'s signature and runs the two library
calls of tim_amd/csrc/detect.hip on each batch (decode / round / threshold -> the candidate list, in the reference's
order); `detections()` runs the grouped soft-NMS of tim_amd/nms.py once over everything collected; `results()` is the
`results` dict of the reference's submission file.  The dense score matrix never exists and nothing but a 4-byte
candidate count is read back per batch.  There is no CPU path: the kernels run or the call raises.
"""
import numpy as np
import torch

from . import _lib as L
from ._collect import CandidateCollector, candidate_buffers, fp32_rows, require_gpu
from ._lib import call, ptr
from .functional import _stream

# head -> (slot of the classification outputs, slot of the regressions / query times)
HEADS = {"verb": (0, 0), "noun": (1, 0), "action": (2, 0), "audio": (3, 1)}


def head_classes(num_class, head):
    """number of classes of `head` for a model's `num_class` ([[verb, noun, action], audio] or [action, audio])"""
    if isinstance(num_class, (int, np.integer)):
        return int(num_class)
    if head == "audio":
        return int(num_class[1])
    vis = num_class[0]
    if isinstance(vis, (list, tuple)):
        return int(vis[HEADS[head][0]])
    if head != "action":
        raise ValueError("num_class %r has no %s head" % (num_class, head))
    return int(vis)


_WHO = ("DetectionCollector.update", "the detection tail runs")


def candidates(logits, reg, window_start, window_size, max_time, video_index, num_queries, score_threshold, out=None):
    """One batch through timhip_det_candidates_count / _emit.  logits [R, C] fp32 (rows may be strided), reg [R, 2],
    window_start [B] float64, max_time a 0-dim device tensor, video_index [B] int32, all on the device.
    -> (seg [N, 2], score [N], key [N] int64 = video_index * C + class, row [N] int32), N read back from the device.
    `out` = (seg, score, key, row) buffers to fill instead (their length is the capacity; nothing is read back and the
    returned tensors are the buffers, valid up to row_offsets[R] which is returned as a fifth, device, value)."""
    L.load()
    logits = fp32_rows(logits)
    R, C = logits.shape
    reg = reg.to(torch.float32).contiguous()
    dev = logits.device
    seg32 = torch.empty((R, 2), dtype=torch.float32, device=dev)
    ok = torch.empty((R,), dtype=torch.uint8, device=dev)
    off = torch.empty((R + 1,), dtype=torch.int32, device=dev)
    thr = float(np.float32(score_threshold))
    st = _stream()
    call("timhip_det_candidates_count", ptr(logits), logits.stride(0), ptr(reg), ptr(window_start),
         float(np.float32(window_size)), ptr(max_time), R, C, int(num_queries), thr, ptr(seg32), ptr(ok), ptr(off), st)
    (seg, score, key, row), n = candidate_buffers(off, R, out)
    call("timhip_det_candidates_emit", ptr(logits), logits.stride(0), ptr(seg32), ptr(ok), ptr(off), ptr(video_index),
         R, C, int(num_queries), thr, n, ptr(seg), ptr(score), ptr(key), ptr(row), st)
    if out is None:
        return seg, score, key, row
    return seg, score, key, row, off[R]


class DetectionCollector(CandidateCollector):
    """Collects the detection candidates of one head over an evaluation and turns them into detections.

        col = DetectionCollector(num_class, head="action", score_threshold=0.01)
        for batch: col.update(output[0], output[1], query_times, metadata)      # FeatureMeter.update's arguments
        segs, scores, labels, video = col.detections(sigma=0.1)                 # device tensors
        results = col.results(sigma=0.1)                                        # {video_id: [{"action", "score", "segment"}]}
    """

    def __init__(self, num_class, head="action", score_threshold=0.01):
        if head not in HEADS:
            raise ValueError("head must be one of %s" % sorted(HEADS))
        self.head = head
        self.num_classes = head_classes(num_class, head)
        self.score_threshold = float(score_threshold)
        self.reset()

    def update(self, features, regressions, query_times, metadata):
        cls_slot, reg_slot = HEADS[self.head]
        logits, reg, qt = features[cls_slot], regressions[reg_slot], query_times[reg_slot]
        require_gpu(logits, _WHO, "features[%d]" % cls_slot)
        require_gpu(reg, _WHO, "regressions[%d]" % reg_slot)
        require_gpu(qt, _WHO, "query_times[%d]" % reg_slot)
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError("the %s head has %d classes, got logits of shape %s"
                             % (self.head, self.num_classes, tuple(logits.shape)))
        vids = list(metadata["video_id"])
        B, R = len(vids), logits.shape[0]
        if B == 0 or R % B != 0 or reg.shape[0] != R:
            raise ValueError("%d proposal rows do not divide into %d windows" % (R, B))
        idx = self._video_index(vids)
        starts, window_size = self._windows(metadata, B)
        dev = logits.device
        seg, score, key, _ = candidates(logits.detach(), reg.detach(), starts.to(dev), window_size, self._max_time(qt),
                                        torch.from_numpy(idx).to(dev), R // B, self.score_threshold)
        self._keep(seg, score, key)

    def detections(self, sigma=0.1, iou_threshold=0.1, min_score=0.001, method=2, nms="soft"):
        """-> (segs [M, 2] fp32, scores [M] fp32, labels [M] int64, video [M] int64 index into `video_ids`), ordered by
        video and, inside a video, by descending score (stable: equal scores keep class, then selection order)"""
        return self._detections(iou_threshold, min_score, sigma, method, nms)

    def results(self, **nms_args):
        """the `results` dict of the reference's submission (format_predictions.py): every video seen, its detections by
        descending score, start / stop rounded to three decimals"""
        s, c, l, v = (t.cpu().numpy() for t in self.detections(**nms_args))
        out = {vid: [] for vid in self.video_ids}
        for i in range(c.shape[0]):
            out[self.video_ids[int(v[i])]].append({"action": int(l[i]), "score": float(c[i]),
                                                   "segment": [round(float(s[i, 0]), 3), round(float(s[i, 1]), 3)]})
        return out
