"""TEST INFRASTRUCTURE ONLY: numpy restatement of the two-stream detection fusion - what the reference's
eval_detection/format_two_stream_predictions_epic.py computes between the saved outputs of a verb model and a noun model and
its submission, written from its contract.  tests/test_twostream_ref.py pins it to a fixture recorded from the reference
itself; tests/test_gpu_twostream.py then checks the HIP kernels and tim_amd.TwoStreamCollector against it.  The sigmoid and
the decode of a stream's proposals are tests/detect_ref.py's, the NMS goes through oracle.nms_oracle.  Never imported by tim_amd."""
import numpy as np

from tests.detect_ref import CollectorBase, proposals, sigmoid32  # noqa: F401 (proposals: the shared decode, per stream)


def select_top_k(score, k):
    """score [R, C] fp32 -> idx [R, k]: by descending score, equal scores to the lower class, a NaN above every number"""
    score = np.ascontiguousarray(score, dtype=np.float32)
    rank = score.view(np.uint32).astype(np.int64) + 1                # scores lie in [0, 1]: their bits order as integers
    rank[np.isnan(score)] = 1 << 32
    return np.argsort(-rank, axis=1, kind="stable")[:, :k]


def exponents(alpha):
    """(a32, b32): the subtraction in double, each rounded to fp32"""
    return np.float32(alpha), np.float32(1.0 - float(alpha))


def fuse_rows(vs, ns, prop_v, prop_n, thr, alpha):
    """vs [R, k], ns [R, k] fp32 selected scores, prop_* [R, 2] float64 -> (score [R, k, k] fp32, seg [R, k, k, 2] float64
    rounded to three decimals, ok [R, k, k] bool); pair (i, j) = i-th verb, j-th noun"""
    thr32 = np.float32(thr)
    a32, b32 = exponents(alpha)
    v, n = vs[:, :, None], ns[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        A = np.power(v.astype(np.float64), np.float64(a32)).astype(np.float32)          # float64 pow, rounded once
        B = np.power(n.astype(np.float64), np.float64(b32)).astype(np.float32)
        score = (A * B).astype(np.float32)                                              # fp32 product, one rounding
        w = (v / (v + n)).astype(np.float32)
        w1 = (np.float32(1.0) - w).astype(np.float32)
        seg = w.astype(np.float64)[..., None] * prop_v[:, None, None, :] + w1.astype(np.float64)[..., None] * prop_n[:, None, None, :]
        seg = np.rint(seg * 1000.0) / 1000.0                                            # numpy.round(seg, 3)
        ok = (v > thr32) & (n > thr32) & (score > thr32) & ((seg[..., 1] - seg[..., 0]) > 0.0)
    return score, seg, ok


def batch_candidates(verb_logits, noun_logits, verb_reg, noun_reg, window_start, window_size, max_time, video_index,
                     score_threshold, alpha, top_k):
    """one batch -> dict: the per-row records (sel_idx [R, 2, k], sel_score [R, 2, k], pair_score [R, k * k],
    pair_seg [R, k * k, 2] fp32, pair_ok [R, k * k]) and the candidate list (seg [N, 2] fp32, score [N] fp32, key [N] int64,
    row [N] int32, verb [N], noun [N], video [N]): rows ascending, verbs by descending score, nouns by descending score"""
    verb_logits, noun_logits = np.asarray(verb_logits, np.float32), np.asarray(noun_logits, np.float32)
    R, Cv = verb_logits.shape
    Cn = noun_logits.shape[1]
    k, nq = int(top_k), R // len(window_start)
    sv, sn = sigmoid32(verb_logits), sigmoid32(noun_logits)
    iv, jn = select_top_k(sv, k), select_top_k(sn, k)
    vs, ns = np.take_along_axis(sv, iv, 1), np.take_along_axis(sn, jn, 1)
    pv = proposals(verb_reg, window_start, window_size, max_time, nq)
    pn = proposals(noun_reg, window_start, window_size, max_time, nq)
    score, seg, ok = fuse_rows(vs, ns, pv, pn, score_threshold, alpha)
    rows, i, j = np.nonzero(ok)                            # row-major: rows, then the verb rank, then the noun rank
    verb, noun = iv[rows, i].astype(np.int64), jn[rows, j].astype(np.int64)
    video = np.asarray(video_index, dtype=np.int64)[rows // nq]
    return dict(sel_idx=np.stack([iv, jn], 1).astype(np.int32), sel_score=np.stack([vs, ns], 1),
                pair_score=score.reshape(R, k * k), pair_seg=seg.reshape(R, k * k, 2).astype(np.float32),
                pair_ok=ok.reshape(R, k * k),
                seg=seg[rows, i, j].astype(np.float32), seg64=seg[rows, i, j], score=score[rows, i, j],
                key=video * (Cv * Cn) + verb * Cn + noun, row=rows.astype(np.int32), verb=verb, noun=noun, video=video)


class Collector(CollectorBase):
    """numpy mirror of tim_amd.TwoStreamCollector"""

    def __init__(self, num_verbs, num_nouns, score_threshold=0.03, verb_alpha=0.65, top_k=1):
        super().__init__()
        self.V, self.N, self.thr, self.alpha, self.k = int(num_verbs), int(num_nouns), score_threshold, verb_alpha, int(top_k)

    def update(self, verb_logits, noun_logits, verb_reg, noun_reg, query_times, video_ids, window_start, window_size):
        idx = self._video_index(video_ids)
        max_time = np.asarray(query_times, dtype=np.float32).max()
        self.chunks.append(batch_candidates(verb_logits, noun_logits, verb_reg, noun_reg, window_start, window_size, max_time,
                                            idx, self.thr, self.alpha, self.k))

    def candidates(self):
        names = ("seg", "seg64", "score", "key", "verb", "noun", "video")
        if not self.chunks:
            return {k: np.zeros((0, 2) if k.startswith("seg") else 0, np.float32 if k in ("seg", "score") else np.int64)
                    for k in names}
        return {k: np.concatenate([c[k] for c in self.chunks]) for k in names}

    def detections(self, sigma=0.25, iou_threshold=0.1, min_score=0.001, method=2, nms="soft", task="action"):
        """-> (segs, scores, labels, video) ordered by video, then descending score (stable)"""
        c = self.candidates()
        s, sc, lb, vd = self._nms_per_video(c, c["verb"] * self.N + c["noun"], iou_threshold, min_score, sigma, method, nms)
        lb = lb.astype(np.int64)
        return s, sc, {"action": lb, "verb": lb // self.N, "noun": lb % self.N}[task], vd

    def results(self, **nms_args):
        """only the videos that had a candidate, as the reference's dict"""
        s, sc, lb, vd = self.detections(**nms_args)
        seen = set(int(v) for v in self.candidates()["video"])
        res = {vid: [] for i, vid in enumerate(self.video_ids) if i in seen}
        for i in range(len(sc)):
            verb, noun = int(lb[i]) // self.N, int(lb[i]) % self.N
            res[self.video_ids[int(vd[i])]].append({"verb": verb, "noun": noun, "action": "%d,%d" % (verb, noun),
                                                    "score": float(sc[i]),
                                                    "segment": [round(float(s[i, 0]), 3), round(float(s[i, 1]), 3)]})
        return res
