"""What the collectors of the evaluation tails share on the host: the device-only check, the operand helpers of the candidate
calls and `CandidateCollector`, the base of `DetectionCollector` (detect.py) and `TwoStreamCollector` (twostream.py)."""
import numpy as np
import torch

from . import _lib as L
from .nms import grouped_nms


def require_gpu(t, who, what):
    """`who` = ("DetectionCollector.update", "the detection tail runs"): the caller and what it does, for the message"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.TimHipError("%s: %s must be a device tensor; %s on the MI355X HIP kernels only (there is no CPU fallback)"
                            % (who[0], what, who[1]))


def fp32_rows(t):
    """[R, C] -> fp32 rows of unit stride, as the kernels read them (the rows themselves may be strided)"""
    if t.dtype != torch.float32 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.to(torch.float32).contiguous()
    return t


def candidate_buffers(off, R, out):
    """the (seg, score, key, row) buffers an emit fills and their capacity: `out` itself, or exact-size ones after the one
    device-to-host read of a batch (row_offsets[R], 4 bytes)"""
    if out is not None:
        return tuple(out), out[1].shape[0]
    n, dev = int(off[R].item()), off.device
    return (torch.empty((n, 2), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev),
            torch.empty((n,), dtype=torch.int64, device=dev), torch.empty((n,), dtype=torch.int32, device=dev)), n


class CandidateCollector:
    """Candidates (seg, score, key = video * num_classes + label) per batch, one grouped NMS over all of them at the end.
    A subclass sets `num_classes` and appends to `_chunks` in its `update()`."""

    def reset(self):
        self.video_ids = []          # dense index -> video id, in first-seen order
        self._index = {}
        self._chunks = []            # per batch (seg, score, key) on the device

    def _video_index(self, video_ids):
        """-> int32 [B]: the dense index of each window's video (new ids are appended to `video_ids`)"""
        idx = np.empty(len(video_ids), dtype=np.int32)
        for i, v in enumerate(video_ids):
            v = str(v)
            j = self._index.get(v)
            if j is None:
                j = self._index[v] = len(self.video_ids)
                self.video_ids.append(v)
            idx[i] = j
        return idx

    @staticmethod
    def _windows(metadata, B):
        """-> (window_start float64 [B] on the host, window_size)"""
        starts = torch.as_tensor(metadata["window_start"]).detach().to(torch.float64).reshape(-1)
        if starts.numel() != B:
            raise ValueError("metadata['window_start'] holds %d values for %d windows" % (starts.numel(), B))
        return starts, float(torch.as_tensor(metadata["window_size"]).reshape(-1)[0])

    @staticmethod
    def _max_time(query_times):
        return query_times.detach().to(torch.float32).max()       # stays on the device

    def _keep(self, seg, score, key):
        if score.shape[0]:
            self._chunks.append((seg, score, key))

    def candidates(self):
        """everything collected so far: (seg [N, 2], score [N], key [N]) in collection order"""
        if not self._chunks:
            if not torch.cuda.is_available():
                raise L.TimHipError("%s runs on the MI355X HIP kernels only (no CPU fallback)" % type(self).__name__)
            dev = torch.device("cuda")
            return (torch.zeros((0, 2), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.float32, device=dev),
                    torch.zeros((0,), dtype=torch.int64, device=dev))
        if len(self._chunks) > 1:                            # concatenate once, and keep the result as the one chunk
            self._chunks = [tuple(torch.cat([c[i] for c in self._chunks]) for i in range(3))]
        return self._chunks[0]

    def _detections(self, iou_threshold, min_score, sigma, method, nms):
        """the grouped NMS over `candidates()` -> (segs, scores, labels = key % num_classes, video), ordered by video and,
        inside a video, by descending score (stable)"""
        seg, score, key = self.candidates()
        s, c, k = grouped_nms(seg, score, key, iou_threshold, min_score, sigma, method, nms)
        video = torch.div(k, self.num_classes, rounding_mode="floor")
        labels = k - video * self.num_classes
        o = torch.argsort(-c, stable=True)
        o = o[torch.argsort(video[o], stable=True)]
        return s[o], c[o], labels[o], video[o]
