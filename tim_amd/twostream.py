"""Two-stream detection fusion on the MI355X: the outputs of a verb model and a noun model over the same windows in,
per-video (verb, noun) action detections out.

`TwoStreamCollector` takes the place of the reference's `eval_detection/format_two_stream_predictions_epic.py` (on top of
`FeatureMeter`): `update()` runs the two library calls of tim_amd/csrc/twostream.hip on each batch (scores, the top k classes
of each stream, the fused score and the score-weighted blend of the two segments -> the candidate list, in the reference's
order); `detections()` runs the grouped soft-NMS of tim_amd/nms.py once over everything collected, one group per (video,
verb, noun); `results()` is the `results` dict of the reference's submission file.  Neither dense score matrix ever exists
and nothing but a 4-byte candidate count is read back per batch.  `detections()` / `video_ids` keep `DetectionCollector`'s
contract, so `DetectionScorer.score(col)` works unchanged.  There is no CPU path: the kernels run or the call raises.
"""
import numpy as np
import torch

from . import _lib as L
from ._collect import CandidateCollector, candidate_buffers, fp32_rows, require_gpu
from ._lib import call, ptr
from .detect import HEADS
from .functional import _stream

MAX_TOP_K = 8         # csrc/twostream.hip: k * k pairs, one lane each
TASKS = ("action", "verb", "noun")


_WHO = ("TwoStreamCollector.update", "the two-stream fusion runs")


def exponents(verb_alpha):
    """(alpha32, beta32) as the library takes them: the subtraction in double, each rounded to fp32"""
    return float(np.float32(verb_alpha)), float(np.float32(1.0 - float(verb_alpha)))


def candidates(verb_logits, noun_logits, verb_reg, noun_reg, window_start, window_size, max_time, video_index, num_queries,
               score_threshold, verb_alpha, top_k, out=None, records=False):
    """One batch through timhip_ts_candidates_count / _emit.  verb_logits [R, Cv] / noun_logits [R, Cn] fp32 (rows may be
    strided), verb_reg / noun_reg [R, 2], window_start [B] float64, max_time a 0-dim device tensor, video_index [B] int32, all
    on the device.
    -> (seg [N, 2], score [N], key [N] int64 = video_index * (Cv * Cn) + verb * Cn + noun, row [N] int32), N read back from
    the device.  `out` = (seg, score, key, row) buffers to fill instead (their length is the capacity; nothing is read back
    and the returned tensors are the buffers, valid up to row_offsets[R] which is returned as a fifth, device, value).
    `records=True` appends the per-row records (sel_idx [R, 2, k], sel_score [R, 2, k], pair_score [R, k * k],
    pair_seg [R, k * k, 2], pair_mask [R] int64, row_offsets [R + 1])."""
    L.load()
    verb_logits, noun_logits = fp32_rows(verb_logits), fp32_rows(noun_logits)
    R, Cv = verb_logits.shape
    Cn = noun_logits.shape[1]
    k = int(top_k)
    kk = max(k, 0) ** 2
    verb_reg, noun_reg = verb_reg.to(torch.float32).contiguous(), noun_reg.to(torch.float32).contiguous()
    dev = verb_logits.device
    sel_idx = torch.empty((R, 2, max(k, 0)), dtype=torch.int32, device=dev)
    sel_score = torch.empty((R, 2, max(k, 0)), dtype=torch.float32, device=dev)
    pair_score = torch.empty((R, kk), dtype=torch.float32, device=dev)
    pair_seg = torch.empty((R, kk, 2), dtype=torch.float32, device=dev)
    pair_mask = torch.empty((R,), dtype=torch.int64, device=dev)
    off = torch.empty((R + 1,), dtype=torch.int32, device=dev)
    a32, b32 = exponents(verb_alpha)
    st = _stream()
    call("timhip_ts_candidates_count", ptr(verb_logits), verb_logits.stride(0), ptr(noun_logits), noun_logits.stride(0),
         ptr(verb_reg), ptr(noun_reg), ptr(window_start), float(np.float32(window_size)), ptr(max_time), R, Cv, Cn,
         int(num_queries), k, float(np.float32(score_threshold)), a32, b32, ptr(sel_idx), ptr(sel_score), ptr(pair_score),
         ptr(pair_seg), ptr(pair_mask), ptr(off), st)
    (seg, score, key, row), n = candidate_buffers(off, R, out)
    call("timhip_ts_candidates_emit", ptr(sel_idx), ptr(pair_score), ptr(pair_seg), ptr(pair_mask), ptr(off), ptr(video_index),
         R, Cv, Cn, int(num_queries), k, n, ptr(seg), ptr(score), ptr(key), ptr(row), st)
    res = (seg, score, key, row) if out is None else (seg, score, key, row, off[R])
    if records:
        res = res + ((sel_idx, sel_score, pair_score, pair_seg, pair_mask, off),)
    return res


class TwoStreamCollector(CandidateCollector):
    """Collects the fused (verb, noun) detection candidates of two streams over an evaluation and turns them into detections.

        col = TwoStreamCollector(num_verbs=97, num_nouns=300, score_threshold=0.03, verb_alpha=0.65, top_k=1)
        for batch: col.update(verb_output, noun_output, query_times, metadata)   # *_output = (features, regressions) of a model
        segs, scores, labels, video = col.detections(sigma=0.25, task="action")  # device tensors; label = verb * num_nouns + noun
        results = col.results(sigma=0.25)          # {video_id: [{"verb", "noun", "action": "v,n", "score", "segment"}]}

    `verb_head` / `noun_head` name the slot of `detect.HEADS` each stream's scores are read from: the default, each model's
    "action" head, is the reference's recipe of two single-head models; "verb" and "noun" with the same output passed twice
    fuse one model that has both heads."""

    def __init__(self, num_verbs=97, num_nouns=300, score_threshold=0.03, verb_alpha=0.65, top_k=1, verb_head="action",
                 noun_head="action"):
        for h in (verb_head, noun_head):
            if h not in HEADS:
                raise ValueError("head must be one of %s" % sorted(HEADS))
        self.num_verbs, self.num_nouns = int(num_verbs), int(num_nouns)
        self.top_k = int(top_k)
        if self.num_verbs < 1 or self.num_nouns < 1:
            raise ValueError("num_verbs and num_nouns must be positive")
        if not 1 <= self.top_k <= min(self.num_verbs, self.num_nouns, MAX_TOP_K):
            raise ValueError("top_k must be between 1 and min(num_verbs, num_nouns, %d), got %d" % (MAX_TOP_K, self.top_k))
        self.verb_head, self.noun_head = verb_head, noun_head
        self.score_threshold, self.verb_alpha = float(score_threshold), float(verb_alpha)
        self.num_classes = self.num_verbs * self.num_nouns          # of the fused label verb * num_nouns + noun
        self.reset()

    def update(self, verb_output, noun_output, query_times, metadata):
        streams = []
        for name, output, head, ncls in (("verb", verb_output, self.verb_head, self.num_verbs),
                                         ("noun", noun_output, self.noun_head, self.num_nouns)):
            cls_slot, reg_slot = HEADS[head]
            logits, reg = output[0][cls_slot], output[1][reg_slot]
            require_gpu(logits, _WHO, "%s_output[0][%d]" % (name, cls_slot))
            require_gpu(reg, _WHO, "%s_output[1][%d]" % (name, reg_slot))
            if logits.dim() != 2 or logits.shape[1] != ncls:
                raise ValueError("the %s stream has %d classes, got logits of shape %s" % (name, ncls, tuple(logits.shape)))
            streams.append((logits, reg, reg_slot))
        (vl, vr, slot_v), (nl, nr, slot_n) = streams
        if slot_v != slot_n:
            raise ValueError("the %s and %s heads regress different queries" % (self.verb_head, self.noun_head))
        qt = query_times[slot_v]
        require_gpu(qt, _WHO, "query_times[%d]" % slot_v)
        vids = list(metadata["video_id"])
        B, R = len(vids), vl.shape[0]
        if nl.shape[0] != R:
            raise ValueError("the verb stream has %d proposal rows, the noun stream %d" % (R, nl.shape[0]))
        if B == 0 or R % B != 0 or vr.shape[0] != R or nr.shape[0] != R:
            raise ValueError("%d proposal rows do not divide into %d windows" % (R, B))
        idx = self._video_index(vids)
        starts, window_size = self._windows(metadata, B)
        dev = vl.device
        seg, score, key, _ = candidates(vl.detach(), nl.detach(), vr.detach(), nr.detach(), starts.to(dev), window_size,
                                        self._max_time(qt), torch.from_numpy(idx).to(dev), R // B, self.score_threshold,
                                        self.verb_alpha, self.top_k)
        self._keep(seg, score, key)

    def detections(self, sigma=0.25, iou_threshold=0.1, min_score=0.001, method=2, nms="soft", task="action"):
        """-> (segs [M, 2] fp32, scores [M] fp32, labels [M] int64, video [M] int64 index into `video_ids`), ordered by
        video and, inside a video, by descending score (stable: equal scores keep label, then selection order).  The label
        is verb * num_nouns + noun for task "action", the verb for "verb", the noun for "noun" (the same detections)."""
        if task not in TASKS:
            raise ValueError("task must be one of %s" % (TASKS,))
        s, c, labels, video = self._detections(iou_threshold, min_score, sigma, method, nms)
        if task == "verb":
            labels = torch.div(labels, self.num_nouns, rounding_mode="floor")
        elif task == "noun":
            labels = labels % self.num_nouns
        return s, c, labels, video

    def results(self, **nms_args):
        """the `results` dict of the reference's submission (format_two_stream_predictions_epic.py): the videos that had at
        least one candidate, their detections by descending score, start / stop rounded to three decimals"""
        nms_args.pop("task", None)
        s, c, l, v = (t.cpu().numpy() for t in self.detections(**nms_args))
        key = self.candidates()[2]
        seen = torch.unique(torch.div(key, self.num_classes, rounding_mode="floor")).cpu().numpy()
        out = {self.video_ids[int(i)]: [] for i in seen}
        for i in range(c.shape[0]):
            verb, noun = divmod(int(l[i]), self.num_nouns)
            out[self.video_ids[int(v[i])]].append({"verb": verb, "noun": noun, "action": "%d,%d" % (verb, noun),
                                                   "score": float(c[i]),
                                                   "segment": [round(float(s[i, 0]), 3), round(float(s[i, 1]), 3)]})
        return out
