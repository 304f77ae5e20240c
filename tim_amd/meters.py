"""Training meter on the MI355X: loss averages and top-1 / top-5 accuracies that never leave the device until they are read.

`TrainMeter` takes the place of the reference's recognition `TrainMeter` (recognition/time_interval_machine/utils/meters.py:30-395)
and of what recognition/scripts/train.py:391-410 does in front of it every iteration: a device-to-host copy of all four heads'
logits, a CPU `index_add_` and seven `.item()` calls.  Here the state is one block of `_lib.METER_STATE_WORDS` 32-bit words in
device memory (include/timhip.h: TIMHIP_METER_*).  `update()` launches kernels only (`timhip_meter_update`, tim_amd/csrc/meter.hip:
at most two launches, besides the three per modality of the owned `RecognitionCollector` with `ensemble=True`), so it runs
inside `torch.cuda.graph` and never synchronises; `read()` is one copy of the block (336 bytes).  There is no CPU path: the
kernels run or the call raises.

Beyond the reference: with `batch_accuracy=True` the block also counts, per head, the valid rows whose label ranks first /
among the first five over the row's raw logits - of the last batch and since the reset - so an accuracy is there at every
`print_freq`, not only after `update_epoch()`.

Two recorded deviations:
  1. the ensemble's accumulators are fp32: the reference run with `enable_amp=False`.  Its fp16 accumulators under AMP are not
     reproduced.
  2. the reference's train.py hands `AverageMeter` 0-dim int tensors as counts, which silently turns its sums into float32
     tensors.  Here the sums are doubles and the counts int64: what the class computes from the Python numbers its signature
     suggests.

Out of scope: the timers, the RAM / GPU probes and a cross-rank reduction of the state.

`DetectionMeter` is the detection counterpart: the eleven loss averages of the reference's detection `TrainMeter`
and `InferenceMeter`, fed by the side statistics `detection_side_loss(..., stats=)` leaves on the device.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from ._collect import fp32_rows, require_gpu
from ._lib import call, ptr
from .detect import HEADS, head_classes
from .functional import _stream
from .recog import VISUAL_HEADS, RecognitionCollector, accuracy_floats, multitask_floats

SLOTS = ("total", "drloc", "visual", "verb", "noun", "action", "audio")      # _lib.METER_TOTAL .. METER_AUDIO
COUNTER_ROWS = ("verb", "noun", "action", "mt_action", "audio")              # _lib.METER_HEAD_VERB .. METER_HEAD_AUDIO
_HEAD_SLOT = {"verb": L.METER_HEAD_VERB, "noun": L.METER_HEAD_NOUN, "action": L.METER_HEAD_ACTION, "audio": L.METER_HEAD_AUDIO}
_WHO = ("TrainMeter.update", "the training meter runs")

# the reference's get_train_stats() names of the loss averages (meters.py:169-209); "Train/loss" is ours: the reference prints
# the total only in its message line
_STAT_KEYS = {"total": "Train/loss", "drloc": "Train/drloc_loss", "visual": "Train/visual_loss", "verb": "Train/verb/visual_loss",
              "noun": "Train/noun/visual_loss", "action": "Train/visual_action_loss", "audio": "Train/audio_loss"}
_BATCH_KEYS = {"verb": "Train_batch/visual/verb", "noun": "Train_batch/visual/noun", "action": "Train_batch/visual/act",
               "mt_action": "Train_batch/visual/", "audio": "Train_batch/audio/"}


def decode_state(words):
    """the state block (int32 view, `_lib.METER_STATE_WORDS` words, on the host) -> the dict `TrainMeter.read()` returns"""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1)).view(np.int32)
    if w.size != L.METER_STATE_WORDS:
        raise ValueError("a meter state block holds %d words, got %d" % (L.METER_STATE_WORDS, w.size))
    q64, f64, f32 = w[:L.METER_VAL].view(np.int64), w[:L.METER_VAL].view(np.float64), w.view(np.float32)
    out = {"updates": int(q64[L.METER_UPDATES // 2]), "nv": int(w[L.METER_NV]), "na": int(w[L.METER_NA]), "losses": {}, "acc": {}}
    for s, name in enumerate(SLOTS):
        total, count = float(f64[(L.METER_SUM + 4 * s) // 2]), int(q64[(L.METER_COUNT + 4 * s) // 2])
        out["losses"][name] = {"avg": total / count if count else 0.0, "val": float(f32[L.METER_VAL + s]), "count": count,
                               "sum": total}
    for h, name in enumerate(COUNTER_ROWS):
        rows, c1, c5 = (int(q64[(L.METER_RUN + 6 * h + 2 * k) // 2]) for k in range(3))
        brows, b1, b5 = (int(w[L.METER_LAST + 3 * h + k]) for k in range(3))
        floats = multitask_floats if name == "mt_action" else accuracy_floats
        (t1, t5), (bt1, bt5) = floats(c1, c5, rows), floats(b1, b5, brows)
        out["acc"][name] = {"top1": t1, "top5": t5, "rows": rows, "hits1": c1, "hits5": c5,
                            "batch_top1": bt1, "batch_top5": bt5, "batch_rows": brows, "batch_hits1": b1, "batch_hits5": b5}
    return out


class TrainMeter:
    """Loss averages, batch accuracies and the per-action ensemble of a recognition training run, on the device.

        meter = TrainMeter(num_class, num_actions, modality="audio_visual", include_verb_noun=True,
                           dataset="epic", ensemble=True, batch_accuracy=True)
        # inside the (captured) iteration:
        meter.update(output[0], v_action_ids, a_action_ids, v_labels, a_labels,
                     losses={"total": loss, "visual": ..., "verb": ..., "noun": ..., "action": ..., "audio": ..., "drloc": ...})
        # at print_freq, outside:
        s = meter.read()            # one copy: averages, counts, running and last-batch top-1 / top-5
        acc = meter.update_epoch()  # the ensemble's accuracies (+ "combined" for AVE); then meter.reset()

    The arguments of `update()` are `RecognitionCollector.update`'s: the UNFILTERED head outputs and the flattened, -1-padded
    ids and labels of the batch (under mixup: target_a).  A visual row counts iff its action label is not -1, an audio row
    iff its class id is not -1; the two counts nv / na are taken on the device and weight the losses as the reference's
    `update()` does (meters.py:140-167).  `losses` maps slot names to 1-element device tensors; a missing one counts as 0.
    The scratch of a call is allocated when a batch is larger than every batch before it: run one update of the largest shape
    (the warm-up steps of a captured iteration do) before capturing.
    """

    def __init__(self, num_class, num_actions, modality="audio_visual", include_verb_noun=True, dataset="epic", ensemble=True,
                 batch_accuracy=True, device="cuda"):
        if not torch.cuda.is_available():
            raise L.TimHipError("TrainMeter needs the MI355X (no CPU fallback)")
        L.load()
        self.device = torch.device(device)
        self.modality, self.dataset = modality, dataset
        self.include_verb_noun, self.batch_accuracy = bool(include_verb_noun), bool(batch_accuracy)
        self.num_actions = int(num_actions)
        self.groups = {}
        if "visual" in modality:
            heads = VISUAL_HEADS if self.include_verb_noun else ("action",)
            self.groups["visual"] = (heads, [head_classes(num_class, h) for h in heads], 3)
        if "audio" in modality:
            self.groups["audio"] = (("audio",), [head_classes(num_class, "audio")], 1)
        if not self.groups:
            raise ValueError("modality %r names neither visual nor audio" % (modality,))
        self._tables = {name: (L.TimMeterHead * len(g[0]))() for name, g in self.groups.items()}
        self._losses = (ctypes.c_void_p * L.METER_SLOTS)()
        self._flags = (L.METER_VERB_NOUN if self.include_verb_noun else 0) | (L.METER_BATCH_ACCURACY if self.batch_accuracy else 0)
        self.state = torch.zeros((L.METER_STATE_WORDS // 2,), dtype=torch.int64, device=self.device)     # 8-byte aligned words
        self._work = None
        self.collector = RecognitionCollector(num_class, num_actions, modality, include_verb_noun, device) if ensemble else None

    # ---- update ------------------------------------------------------------------------------------------------------------
    def _prepare_group(self, name, features, labels):
        """checks one modality's arguments and fills its head table -> (tensors to keep alive, labels, ld_labels, R)"""
        heads, classes, n_labels = self.groups[name]
        table, keep, R = self._tables[name], [], None
        for i, h in enumerate(heads):
            slot = HEADS[h][0]
            x = features[slot]
            require_gpu(x, _WHO, "features[%d]" % slot)
            if x.dim() != 2 or x.shape[1] != classes[i]:
                raise ValueError("the %s head has %d classes, got logits of shape %s" % (h, classes[i], tuple(x.shape)))
            x = fp32_rows(x.detach())
            if R is None:
                R = x.shape[0]
            elif x.shape[0] != R:
                raise ValueError("the %s heads disagree on the number of rows" % name)
            keep.append(x)
            table[i].logits, table[i].ld, table[i].C = ptr(x), max(int(x.stride(0)), classes[i]), classes[i]
            table[i].label_col, table[i].slot, table[i].reserved = (slot if n_labels == 3 else 0), _HEAD_SLOT[h], 0
        what = "%s_labels" % name[0]
        if labels is None:
            raise ValueError("%s rows need their labels" % name)
        if isinstance(labels, dict):
            labels = [labels[k] for k in (VISUAL_HEADS if n_labels == 3 else ("class_id",))]
        if isinstance(labels, (list, tuple)):
            for t in labels:
                require_gpu(t, _WHO, what)
            if len(labels) != n_labels:
                raise ValueError("%s: %d label vectors for %d label columns" % (what, len(labels), n_labels))
            labels = torch.stack([t.reshape(-1) for t in labels], dim=1) if n_labels > 1 else labels[0]
        require_gpu(labels, _WHO, what)
        labels = labels.detach()
        if labels.dtype != torch.int64:
            labels = labels.to(torch.int64)
        if labels.numel() != R * n_labels:
            raise ValueError("%s holds %d values for %d rows of %d labels" % (what, labels.numel(), R, n_labels))
        labels = labels.reshape(R, n_labels).contiguous()
        return keep, labels, n_labels, R

    def _loss_pointers(self, losses):
        keep = []
        losses = losses or {}
        unknown = set(losses) - set(SLOTS)
        if unknown:
            raise ValueError("unknown loss names %s (known: %s)" % (sorted(unknown), ", ".join(SLOTS)))
        for s, name in enumerate(SLOTS):
            t = losses.get(name)
            if t is None:
                self._losses[s] = None
                continue
            require_gpu(t, _WHO, "losses[%r]" % name)
            if t.numel() != 1:
                raise ValueError("losses[%r] holds %d values, not one" % (name, t.numel()))
            t = t.detach().reshape(1)
            if t.dtype != torch.float32:
                t = t.to(torch.float32)
            keep.append(t)
            self._losses[s] = ptr(t)
        return keep

    def update(self, features, v_action_ids=None, a_action_ids=None, v_labels=None, a_labels=None, losses=None):
        """one batch: kernels only, nothing is read back.  Every argument is checked before the first launch."""
        args = {"visual": v_labels, "audio": a_labels}
        prep = {name: self._prepare_group(name, features, args[name]) for name in self.groups}
        keep = self._loss_pointers(losses)                  # (held until the launches are queued)
        empty = (None, None, 0, 0)
        (_, vl, vld, Rv), (_, al, ald, Ra) = prep.get("visual", empty), prep.get("audio", empty)
        vt, at = self._tables.get("visual"), self._tables.get("audio")
        nv_heads, na_heads = (len(vt) if vt is not None else 0), (len(at) if at is not None else 0)
        vtp = ctypes.addressof(vt) if vt is not None else None
        atp = ctypes.addressof(at) if at is not None else None
        if self.batch_accuracy:
            words = int(L.load().timhip_meter_work_words(vtp, nv_heads, Rv, atp, na_heads, Ra))
            if words and (self._work is None or self._work.numel() < words):
                self._work = torch.empty((words,), dtype=torch.int32, device=self.device)
        call("timhip_meter_update", vtp, nv_heads, ptr(vl), vld, Rv, atp, na_heads, ptr(al), ald, Ra,
             ctypes.addressof(self._losses), self._flags, ptr(self.state), ptr(self._work), _stream())
        if self.collector is not None:
            feats = list(features)
            for name, (tensors, _, _, _) in prep.items():                     # the fp32 rows made above: no second conversion
                for h, x in zip(self.groups[name][0], tensors):
                    feats[HEADS[h][0]] = x
            self.collector.update(feats, v_action_ids, a_action_ids, vl, al)

    # ---- results -----------------------------------------------------------------------------------------------------------
    def read(self):
        """the block, through ONE device-to-host copy, as plain Python numbers:
            {"updates", "nv", "na" (valid rows of the last batch),
             "losses": {slot: {"avg", "val", "count", "sum"}}            slot in total / drloc / visual / verb / noun / action / audio
             "acc": {head: {"top1", "top5", "rows", "hits1", "hits5", "batch_top1", "batch_top5", "batch_rows", ...}}}
        head in verb / noun / action / mt_action / audio; the per cent figures are the floats the reference's accuracy() /
        multitask_accuracy() would return for those counts.  A slot or head that never counted reports 0."""
        return decode_state(self.state.cpu().numpy())

    def stats(self, lr=None, training_iterations=None, include_dr_loc=True):
        """`read()` under the reference's get_train_stats() key names for the loss averages (meters.py:169-209); the batch
        accuracies - which the reference does not have - under "Train_batch/..." keys"""
        s = self.read()
        out = {}
        if lr is not None:
            out["Train/lr"] = lr
        if training_iterations is not None:
            out["train_step"] = training_iterations
        use = ["total"] + (["drloc"] if include_dr_loc else [])
        if "visual" in self.groups:
            use += (["verb", "noun"] if self.include_verb_noun else []) + ["visual", "action"]
        if "audio" in self.groups:
            use += ["audio"]
        for name in use:
            out[_STAT_KEYS[name]] = s["losses"][name]["avg"]
        if self.batch_accuracy:
            rows = []
            if "visual" in self.groups:
                rows += ["verb", "noun", "action", "mt_action"] if self.include_verb_noun else ["action"]
            if "audio" in self.groups:
                rows += ["audio"]
            for h in rows:
                a = s["acc"][h]
                out[_BATCH_KEYS[h] + "Top1_acc"], out[_BATCH_KEYS[h] + "Top5_acc"] = a["batch_top1"], a["batch_top5"]
                out[_BATCH_KEYS[h] + "running_Top1_acc"], out[_BATCH_KEYS[h] + "running_Top5_acc"] = a["top1"], a["top5"]
        return out

    def update_epoch(self):
        """the ensemble's accuracies, as the reference's update_epoch() computes them (meters.py:253-285): the collector's
        `accuracies()`, with "combined" for dataset == "ave" on both modalities"""
        if self.collector is None:
            raise L.TimHipError("TrainMeter.update_epoch: this meter was built with ensemble=False")
        return self.collector.accuracies(combined=self.dataset == "ave" and len(self.groups) == 2)

    def reset(self):
        self.state.zero_()
        if self.collector is not None:
            self.collector.reset()

    # ---- checkpoint --------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """host copies of the block and of the ensemble's buffers (the reference checkpoints its meter: train.py:149)"""
        out = {"state": self.state.cpu()}
        if self.collector is not None:
            c = self.collector
            out["seen"], out["err"] = c.seen.cpu(), c.err.cpu()
            for name, g in c.groups.items():
                out[name] = {"sum": [s.cpu() for s in g.sum], "labels": g.labels.cpu(), "touched": g.touched.cpu()}
        return out

    def load_state_dict(self, sd):
        if tuple(sd["state"].shape) != tuple(self.state.shape):
            raise ValueError("the checkpoint's state block has shape %s, this meter's %s" % (tuple(sd["state"].shape), tuple(self.state.shape)))
        if ("seen" in sd) != (self.collector is not None):
            raise ValueError("the checkpoint and this meter disagree on ensemble=")
        self.state.copy_(sd["state"])
        if self.collector is not None:
            c = self.collector
            c.seen.copy_(sd["seen"])
            c.err.copy_(sd["err"])
            for name, g in c.groups.items():
                for dst, src in zip(g.sum, sd[name]["sum"]):
                    dst.copy_(src)
                g.labels.copy_(sd[name]["labels"])
                g.touched.copy_(sd[name]["touched"])


# ================================================================================================ detection
DET_SLOTS = ("total", "drloc", "visual", "verb", "noun", "action", "visual_reg", "audio", "audio_reg", "positive", "negative")
DET_SIDES = ("visual", "audio")
# the reference's get_train_stats() / get_val_epoch_stats() names (detection utils/meters.py:139-179, :492-524); "Train/loss" and
# "Val/loss" are ours: the reference prints the total only in its message lines.  The positive / negative averages are ONE pair of
# meters that both modalities feed; the reference reports it under both modalities' names
_DET_KEYS = {
    "train": {"total": ("Train/loss",), "drloc": ("Train/drloc_loss",), "visual": ("Train/visual_loss",), "verb": ("Train/verb/visual_loss",),
              "noun": ("Train/noun/visual_loss",), "action": ("Train/visual_action_loss",), "visual_reg": ("Train/visual_reg_loss",),
              "audio": ("Train/audio_loss",), "audio_reg": ("Train/audio_reg_loss",),
              "positive": ("Train/visual_positive_loss", "Train/audio_positive_loss"),
              "negative": ("Train/visual_negative_loss", "Train/audio_negative_loss")},
    "val": {"total": ("Val/loss",), "visual": ("Val/visual/loss",), "verb": ("Val/visual/verb_loss",), "noun": ("Val/visual/noun_loss",),
            "action": ("Val/visual/action_loss",), "visual_reg": ("Val/visual/reg_loss",), "audio": ("Val/audio/loss",),
            "audio_reg": ("Val/audio/reg_loss",), "positive": ("Val/visual/positive_loss", "Val/audio/positive_loss"),
            "negative": ("Val/visual/negative_loss", "Val/audio/negative_loss")},
}


def decode_det_state(words):
    """the detection state block (int32 view, `_lib.DET_METER_STATE_WORDS` words, on the host) -> the dict `DetectionMeter.read()`
    returns"""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1)).view(np.int32)
    if w.size != L.DET_METER_STATE_WORDS:
        raise ValueError("a detection meter state block holds %d words, got %d" % (L.DET_METER_STATE_WORDS, w.size))
    q64, f64, f32 = w[:L.DET_METER_VAL].view(np.int64), w[:L.DET_METER_VAL].view(np.float64), w.view(np.float32)
    out = {"updates": int(q64[L.DET_METER_UPDATES // 2]), "losses": {}, "sides": {}}
    for s, name in enumerate(DET_SLOTS):
        total, count = float(f64[(L.DET_METER_SUM + 4 * s) // 2]), int(q64[(L.DET_METER_COUNT + 4 * s) // 2])
        out["losses"][name] = {"avg": total / count if count else 0.0, "val": float(f32[L.DET_METER_VAL + s]), "count": count,
                               "sum": total}
    for s, name in enumerate(DET_SIDES):
        valid, pos = (int(q64[(L.DET_METER_RUN + 4 * s + 2 * k) // 2]) for k in range(2))
        out["sides"][name] = {"valid": valid, "positives": pos, "batch_valid": int(w[L.DET_METER_LAST + 2 * s]),
                              "batch_positives": int(w[L.DET_METER_LAST + 2 * s + 1]), "normaliser": float(f32[L.DET_METER_NORM + s])}
    return out


class DetectionMeter:
    """The loss averages of a detection training or validation run, on the device: the reference's detection `TrainMeter`
    (mode="train") and `InferenceMeter` (mode="val"), detection/time_interval_machine/utils/meters.py:29-315, :317-572.

        meter = DetectionMeter("audio_visual", include_verb_noun=True)
        # inside the (captured) iteration:
        lv = detection_side_loss(..., stats=meter.side_stats("visual"))
        la = detection_side_loss(..., stats=meter.side_stats("audio"))
        loss = lv + lambda_audio * la + lambda_drloc * drloc
        meter.update(loss, drloc)
        # at print_freq, outside:
        s = meter.stats(lr, iters)      # one copy of the block

    The side losses leave their statistics in the meter's two fixed tensors (timhip_det_side_loss_fwd_stats: no second pass over
    the logits); `update()` is ONE launch of one block (timhip_det_meter_update) that folds them and the two loss scalars into
    the state block in the reference's order, sums in double, counts in int64.  Nothing synchronises; `read()` is one copy of
    `_lib.DET_METER_STATE_WORDS` words.  A side whose loss did not run since the last update is read again as it stands: run every
    side of `modality` before every update.

    Every value is its own side's, divided by that side's normaliser.  With one modality these are the reference's numbers; with
    two, the reference divides the visual per-head sums by the normaliser the audio side has advanced and hands the audio side's
    positive / negative loss to the meter twice (det scripts/train.py:416-418, :325-326): accidents of variable reuse that are not
    reproduced.  Positive and negative are taken among the rows with iou >= 0 (the reference's mask indexing raises when a row has
    iou < 0).  Out of scope: timers, RAM / GPU probes, message strings, a cross-rank reduction."""

    def __init__(self, modality="audio_visual", include_verb_noun=True, include_dr_loc=True, mode="train", device="cuda"):
        if not torch.cuda.is_available():
            raise L.TimHipError("DetectionMeter needs the MI355X (no CPU fallback)")
        if mode not in ("train", "val"):
            raise ValueError('mode is "train" or "val", not %r' % (mode,))
        L.load()
        self.device = torch.device(device)
        self.modality, self.mode = modality, mode
        self.sides = tuple(s for s in DET_SIDES if s in modality)
        if not self.sides:
            raise ValueError("modality %r names neither visual nor audio" % (modality,))
        self.include_verb_noun = bool(include_verb_noun)
        self.include_dr_loc = bool(include_dr_loc) and mode == "train"
        self.state = torch.zeros((L.DET_METER_STATE_WORDS // 2,), dtype=torch.int64, device=self.device)     # 8-byte aligned words
        self._stats = {s: torch.zeros((L.DET_SIDE_STATS_WORDS,), dtype=torch.float32, device=self.device) for s in self.sides}
        self._sides = (ctypes.c_void_p * 2)(*[ptr(self._stats.get(s)) for s in DET_SIDES])
        self.best_vis_loss = self.best_aud_loss = float("inf")
        self.last_best_epoch = None

    def side_stats(self, side):
        """the fixed tensor to hand to `detection_side_loss(..., stats=)` for "visual" / "audio" """
        if side not in self._stats:
            raise ValueError("this meter (modality %r) has no %r side" % (self.modality, side))
        return self._stats[side]

    @staticmethod
    def _scalar(t, what):
        if t is None:
            return None
        require_gpu(t, ("DetectionMeter.update", "the detection meter runs"), what)
        if t.numel() != 1:
            raise ValueError("%s holds %d values, not one" % (what, t.numel()))
        t = t.detach().reshape(1)
        return t if t.dtype == torch.float32 else t.to(torch.float32)

    def update(self, loss, drloc_loss=None):
        """one iteration: one launch, nothing is read back.  loss / drloc_loss: 1-element device tensors (None counts as 0)"""
        total, drloc = self._scalar(loss, "loss"), self._scalar(drloc_loss, "drloc_loss")
        call("timhip_det_meter_update", ptr(self.state), ctypes.addressof(self._sides), 3 if self.include_verb_noun else 1, ptr(total),
             ptr(drloc), _stream())

    # ---- results -----------------------------------------------------------------------------------------------------------
    def read(self):
        """the block, through ONE device-to-host copy, as plain Python numbers:
            {"updates", "losses": {slot: {"avg", "val", "count", "sum"}}, "sides": {side: {"valid", "positives", "batch_valid",
             "batch_positives", "normaliser"}}};  slot in DET_SLOTS.  A slot that never counted reports 0."""
        return decode_det_state(self.state.cpu().numpy())

    def _slots(self):
        use = ["total"] + (["drloc"] if self.include_dr_loc else [])
        if "visual" in self.sides:
            use += (["verb", "noun"] if self.include_verb_noun else []) + ["visual", "action", "visual_reg"]
        if "audio" in self.sides:
            use += ["audio", "audio_reg"]
        return use + ["positive", "negative"]

    def stats(self, lr=None, training_iterations=None):
        """`read()` under the reference's key names: get_train_stats() (meters.py:139-179) in train mode, get_val_epoch_stats()
        (:492-524) in val mode.  In train mode also "Train/normaliser" (the last side's), "Train/positives", "Train/negatives"
        and "Train/positive_ratio" of the last batch, from the block's counters, summed over the sides."""
        s = self.read()
        out, keys = {}, _DET_KEYS[self.mode]
        if lr is not None and self.mode == "train":
            out["Train/lr"] = lr
        if training_iterations is not None:
            out["train_step" if self.mode == "train" else "val_step"] = training_iterations
        for name in self._slots():
            for i, key in enumerate(keys[name]):
                if len(keys[name]) == 1 or DET_SIDES[i] in self.sides:
                    out[key] = s["losses"][name]["avg"]
        if self.mode == "train":
            pos = sum(s["sides"][k]["batch_positives"] for k in self.sides)
            neg = sum(s["sides"][k]["batch_valid"] for k in self.sides) - pos
            out["Train/normaliser"] = s["sides"][self.sides[-1]]["normaliser"]
            out["Train/positives"], out["Train/negatives"] = pos, neg
            out["Train/positive_ratio"] = pos / (pos + neg) if pos + neg else 0.0
        return out

    def update_epoch(self, epoch):
        """the InferenceMeter's best-loss bookkeeping (meters.py:425-444) on the host after one `read()`: (best_loss, is_best)
        with best_loss the two best losses BEFORE this epoch and is_best "none" / "visual" / "audio" / "audio_visual".  As in
        the reference an absent modality's average is 0.0, which is a best loss once."""
        s = self.read()["losses"]
        vis, aud = s["visual"]["avg"], s["audio"]["avg"]
        is_best_visual, is_best_audio = vis < self.best_vis_loss, aud < self.best_aud_loss
        best_loss = {"visual": self.best_vis_loss, "audio": self.best_aud_loss}
        is_best = "none"
        if is_best_visual:
            is_best = "visual"
            self.best_vis_loss = min(vis, self.best_vis_loss)
            self.last_best_epoch = epoch
        if is_best_audio:
            is_best = "audio_" + is_best if "visual" in is_best else "audio"
            self.best_aud_loss = min(aud, self.best_aud_loss)
            self.last_best_epoch = epoch
        return best_loss, is_best

    def reset(self):
        """zeroes the block; the best losses stay"""
        self.state.zero_()

    # ---- checkpoint --------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"state": self.state.cpu(), "best_vis_loss": self.best_vis_loss, "best_aud_loss": self.best_aud_loss,
                "last_best_epoch": self.last_best_epoch}

    def load_state_dict(self, sd):
        if tuple(sd["state"].shape) != tuple(self.state.shape):
            raise ValueError("the checkpoint's state block has shape %s, this meter's %s" % (tuple(sd["state"].shape), tuple(self.state.shape)))
        self.state.copy_(sd["state"])
        self.best_vis_loss, self.best_aud_loss = float(sd["best_vis_loss"]), float(sd["best_aud_loss"])
        self.last_best_epoch = sd["last_best_epoch"]
