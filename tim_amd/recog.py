"""Recognition inference tail on the MI355X: head logits in, per-action scores and top-1 / top-5 accuracies out.

`RecognitionCollector` takes the place of the reference's `InferenceMeter` and recognition `FeatureMeter`
(recognition/time_interval_machine/utils/meters.py), of the boolean indexing and dense device-to-host copies in front of
them (recognition/scripts/test.py:122-211) and of utils/metrics.py: `update()` takes the UNFILTERED head outputs and the
flattened, -1-padded ids and labels of a batch and runs `timhip_rec_accumulate` once per modality (tim_amd/csrc/recog.hip:
the serial-order fp32 ensemble sum, bit-identical to the reference's CPU `index_add_` and independent of the batch split);
`accuracies()` and `predictions()` run `timhip_rec_finalize` / `timhip_rec_counts` and read back a handful of integers,
respectively the touched actions' probabilities.  There is no CPU path: the kernels run or the call raises.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from ._collect import require_gpu
from ._lib import call, ptr
from .detect import HEADS, head_classes
from .functional import _stream

VISUAL_HEADS = ("verb", "noun", "action")
NO_RANK = 0x7fffffff            # rank of an action without a usable label (csrc/recog.hip)


_WHO = ("RecognitionCollector.update", "the recognition tail runs")


def accuracy_floats(count1, count5, size):
    """utils/metrics.py accuracy(): float(correct_k.to(float32).sum().mul_(100.0 / size)) - the Python double 100.0 / size
    becomes an fp32 scalar, the product is fp32"""
    if size == 0:
        return (0.0, 0.0)
    scale = np.float32(100.0 / size)
    return tuple(float(np.float32(c) * scale) for c in (count1, count5))


def multitask_floats(count1, count5, size):
    """utils/metrics.py multitask_accuracy(): float(count.float() * 100.0 / size), both steps in fp32"""
    if size == 0:
        return (0.0, 0.0)
    return tuple(float(np.float32(np.float32(c) * np.float32(100.0)) / np.float32(size)) for c in (count1, count5))


class _Group:
    """the state of one modality: its heads' accumulators, labels and touched bytes"""

    def __init__(self, heads, classes, n_labels, valid_col, num_actions, dev):
        self.heads, self.classes, self.n_labels, self.valid_col = heads, classes, n_labels, valid_col
        self.pitch = [(c + 63) // 64 * 64 for c in classes]                        # aligned 256-byte wave stores
        self.sum = [torch.zeros((num_actions, p), dtype=torch.float32, device=dev) for p in self.pitch]
        self.labels = torch.full((num_actions, n_labels), -1, dtype=torch.int32, device=dev)
        self.touched = torch.zeros((num_actions,), dtype=torch.uint8, device=dev)
        self.rank = [torch.empty((num_actions,), dtype=torch.int32, device=dev) for _ in heads]
        self.table = (L.TimRecHead * len(heads))()

    def reset(self):
        for s in self.sum:
            s.zero_()
        self.labels.fill_(-1)
        self.touched.zero_()


class RecognitionCollector:
    """Ensembles the recognition heads' logits per action over an evaluation and scores them.

        col = RecognitionCollector(num_class, num_actions, modality="audio_visual", include_verb_noun=True)
        for batch: col.update(output[0], v_action_ids, a_action_ids, v_labels, a_labels)
        acc = col.accuracies()       # {"verb": (top1, top5), "noun", "action", "mt_action", "audio"}
        preds = col.predictions()    # {head: (probs [n, C] fp32, action_ids [n] int64)}, device tensors
        col.reset()

    `num_class` is the model's ([[verb, noun, action], audio]); `num_actions` the number of action ids of the dataset (the
    visual and the audio ids share one range and one seen count, as in the reference).
    """

    def __init__(self, num_class, num_actions, modality="audio_visual", include_verb_noun=True, device="cuda"):
        if not torch.cuda.is_available():
            raise L.TimHipError("RecognitionCollector needs the MI355X (no CPU fallback)")
        L.load()
        self.num_actions = int(num_actions)
        if self.num_actions < 1:
            raise ValueError("num_actions must be positive")
        self.device = torch.device(device)
        self.include_verb_noun = bool(include_verb_noun)
        self.groups = {}
        if "visual" in modality:
            heads = VISUAL_HEADS if self.include_verb_noun else ("action",)
            self.groups["visual"] = _Group(heads, [head_classes(num_class, h) for h in heads], 3, 2, self.num_actions, self.device)
        if "audio" in modality:
            self.groups["audio"] = _Group(("audio",), [head_classes(num_class, "audio")], 1, 0, self.num_actions, self.device)
        if not self.groups:
            raise ValueError("modality %r names neither visual nor audio" % (modality,))
        self.seen = torch.zeros((self.num_actions,), dtype=torch.float32, device=self.device)
        self.err = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self._counts = torch.zeros((8, 3), dtype=torch.int32, device=self.device)
        self._work = None
        self._combined = None            # (action probabilities, audio probabilities, rank) of accuracies(combined=True)

    def reset(self):
        for g in self.groups.values():
            g.reset()
        self.seen.zero_()
        self.err.zero_()

    # ---- update ------------------------------------------------------------------------------------------------------------
    def _labels(self, g, labels, R, what):
        """-> int64 [R, >= n_labels] view (or one small stack) and its row stride"""
        if isinstance(labels, dict):
            labels = [labels[k] for k in (VISUAL_HEADS if g.n_labels == 3 else ("class_id",))]
        if isinstance(labels, (list, tuple)):
            for t in labels:
                require_gpu(t, _WHO, what)
            if len(labels) != g.n_labels:
                raise ValueError("%s: %d label vectors for %d label columns" % (what, len(labels), g.n_labels))
            labels = torch.stack([t.reshape(-1) for t in labels], dim=1) if g.n_labels > 1 else labels[0]
        require_gpu(labels, _WHO, what)
        if labels.dtype != torch.int64:
            labels = labels.to(torch.int64)
        if labels.numel() != R * g.n_labels:
            raise ValueError("%s holds %d values for %d rows of %d labels" % (what, labels.numel(), R, g.n_labels))
        if g.n_labels == 1:
            labels = labels.reshape(-1)                                            # a view wherever the strides allow one
            return labels, max(int(labels.stride(0)), 1)
        return labels.reshape(R, g.n_labels).contiguous(), g.n_labels

    def _prepare_group(self, g, features, ids, labels, valid, name):
        """checks one modality's arguments and fills its head table; nothing is launched before every group has passed"""
        table, R = g.table, None
        keep = []
        for i, h in enumerate(g.heads):
            slot = HEADS[h][0]
            x = features[slot]
            require_gpu(x, _WHO, "features[%d]" % slot)
            if x.dim() != 2 or x.shape[1] != g.classes[i]:
                raise ValueError("the %s head has %d classes, got logits of shape %s" % (h, g.classes[i], tuple(x.shape)))
            x = x.detach()
            if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) < x.shape[1]:
                x = x.to(torch.float32).contiguous()
            if R is None:
                R = x.shape[0]
            elif x.shape[0] != R:
                raise ValueError("the %s heads disagree on the number of rows" % name)
            keep.append(x)
            table[i].logits, table[i].sum, table[i].ld = ptr(x), ptr(g.sum[i]), max(int(x.stride(0)), g.classes[i])
            table[i].C, table[i].pitch = g.classes[i], g.pitch[i]
        require_gpu(ids, _WHO, "%s_action_ids" % name[0])
        ids = ids.detach().reshape(-1)
        if ids.dtype != torch.int64 or ids.stride(0) != 1:
            ids = ids.to(torch.int64).contiguous()
        if ids.numel() != R:
            raise ValueError("%d %s action ids for %d rows" % (ids.numel(), name, R))
        ld_labels = 0
        if labels is not None:
            labels, ld_labels = self._labels(g, labels, R, "%s_labels" % name[0])
        if valid is not None:
            require_gpu(valid, _WHO, "%s_valid" % name[0])
            valid = valid.detach().reshape(-1)
            if valid.numel() != R:
                raise ValueError("%s_valid holds %d values for %d rows" % (name[0], valid.numel(), R))
            valid = (valid != 0).to(torch.uint8) if valid.dtype not in (torch.uint8, torch.bool) or valid.stride(0) != 1 else valid
        elif labels is None:
            raise ValueError("%s rows need labels or a valid mask" % name)
        return (keep, ids, valid, labels, ld_labels, R)

    def _launch_group(self, g, prepared):
        keep, ids, valid, labels, ld_labels, R = prepared
        if R == 0:
            return
        if self._work is None or self._work.numel() < 3 * R:
            self._work = torch.empty((3 * R,), dtype=torch.int32, device=self.device)
        call("timhip_rec_accumulate", ctypes.addressof(g.table), len(g.heads), ptr(ids), ptr(valid), ptr(labels), ld_labels,
             g.n_labels, g.valid_col, R, self.num_actions, ptr(self.seen), ptr(g.labels), ptr(g.touched), ptr(self.err),
             ptr(self._work), _stream())

    def update(self, features, v_action_ids=None, a_action_ids=None, v_labels=None, a_labels=None, v_valid=None, a_valid=None):
        """features = output[0] of the model, unfiltered: (verb, noun, action, audio) logits [rows, C].  Ids and labels are the
        flattened (or [B, queries]) -1-padded tensors of the batch; v_labels holds (verb, noun, action) per row - a [rows, 3]
        tensor, three vectors or the batch's label dict - and a row counts iff its action label is not -1 (audio: its class
        id).  v_valid / a_valid device masks replace that test (feature extraction: no labels)."""
        args = {"visual": (v_action_ids, v_labels, v_valid), "audio": (a_action_ids, a_labels, a_valid)}
        prepared = [(g, self._prepare_group(g, features, *args[name], name)) for name, g in self.groups.items()]
        for g, p in prepared:
            self._launch_group(g, p)

    # ---- results -----------------------------------------------------------------------------------------------------------
    def _finalize(self, g, i, prob=None):
        call("timhip_rec_finalize", ptr(g.sum[i]), g.pitch[i], g.classes[i], ptr(self.seen), ptr(g.labels), g.n_labels,
             HEADS[g.heads[i]][0] if g.n_labels == 3 else 0, ptr(g.touched), self.num_actions, ptr(prob), ptr(g.rank[i]),
             _stream())

    def _check(self, err):
        if err:
            raise L.TimHipError("RecognitionCollector: a valid row carried an action id outside [0, %d) (the reference's "
                                "index_add_ raises an IndexError there); that row was skipped" % self.num_actions)

    def _launch_accuracies(self):
        """finalize (ranks only) + counts of every head into self._counts, nothing read back -> the row names"""
        rows, st = [], _stream()
        for g in self.groups.values():
            for i, h in enumerate(g.heads):
                self._finalize(g, i)
                call("timhip_rec_counts", ptr(g.rank[i]), None, ptr(g.touched), self.num_actions, ptr(self._counts[len(rows)]), st)
                rows.append(h)
            if g.heads == VISUAL_HEADS:
                call("timhip_rec_counts", ptr(g.rank[0]), ptr(g.rank[1]), ptr(g.touched), self.num_actions,
                     ptr(self._counts[len(rows)]), st)
                rows.append("mt_action")
        return rows

    def _launch_combined(self, row):
        """the AVE-only "combined" accuracy (the reference's meters.py:283-285): the action and the audio probabilities of
        the labelled actions, paired by position, averaged and ranked -> self._counts[row]"""
        v, a = self.groups.get("visual"), self.groups.get("audio")
        if v is None or a is None:
            raise ValueError("the combined accuracy needs both modalities")
        i = v.heads.index("action")
        if v.classes[i] != a.classes[0]:
            raise ValueError("the combined accuracy adds the action and the audio probabilities: %d and %d classes do not "
                             "broadcast" % (v.classes[i], a.classes[0]))
        if self._combined is None:
            self._combined = (torch.zeros_like(v.sum[i]), torch.zeros_like(a.sum[0]),
                              torch.empty((self.num_actions,), dtype=torch.int32, device=self.device))
        pv, pa, rank = self._combined
        self._finalize(v, i, pv)
        self._finalize(a, 0, pa)
        st = _stream()
        call("timhip_rec_combined", ptr(pv), v.pitch[i], ptr(pa), a.pitch[0], v.classes[i], ptr(v.labels), v.n_labels,
             HEADS["action"][0], ptr(v.touched), ptr(a.touched), self.num_actions, ptr(rank), st)
        call("timhip_rec_counts", ptr(rank), None, ptr(v.touched), self.num_actions, ptr(self._counts[row]), st)

    def accuracies(self, combined=False):
        """{"verb" / "noun" / "action" / "audio": (top1, top5), "mt_action": (top1, top5)} in per cent, the floats the
        reference's accuracy() / multitask_accuracy() return.  One read of a few integers; raises if an id was out of range.
        combined=True (AVE, both modalities) adds "combined": the k-th labelled visual action's probabilities and the k-th
        labelled audio action's, in ascending id order, averaged in fp32 and ranked against the visual action label - the
        reference's positional add; unequal numbers of labelled actions or of classes raise ValueError (the reference fails
        to broadcast there)."""
        rows = self._launch_accuracies()
        if combined:
            self._launch_combined(len(rows))
            rows.append("combined")
        back = torch.cat([self._counts[:len(rows)].reshape(-1), self.err]).cpu().numpy()
        self._check(int(back[-1]))
        out = {}
        for k, h in enumerate(rows):
            c1, c5, n = (int(v) for v in back[3 * k:3 * k + 3])
            out[h] = multitask_floats(c1, c5, n) if h == "mt_action" else accuracy_floats(c1, c5, n)
        if combined:
            n_v, n_a = (int(back[3 * rows.index(h) + 2]) for h in ("action", "audio"))
            if n_v != n_a:
                raise ValueError("the combined accuracy pairs the labelled actions by position: %d visual and %d audio "
                                 "actions do not broadcast" % (n_v, n_a))
        return out

    def ranks(self):
        """{head: (rank [n] int32, action_ids [n] int64)} of the touched actions' labels (device tensors)"""
        out = {}
        for g in self.groups.values():
            ids = torch.nonzero(g.touched).reshape(-1)
            for i, h in enumerate(g.heads):
                self._finalize(g, i)
                out[h] = (g.rank[i][ids], ids)
        return out

    def predictions(self):
        """{head: (probs [n, C] fp32, action_ids [n] int64)} over the actions seen in the head's modality, ascending ids"""
        self._check(int(self.err.item()))
        out = {}
        for g in self.groups.values():
            ids = torch.nonzero(g.touched).reshape(-1)
            for i, h in enumerate(g.heads):
                prob = torch.zeros_like(g.sum[i])
                self._finalize(g, i, prob)
                out[h] = (prob[ids, :g.classes[i]], ids)
        return out
