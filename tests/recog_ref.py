"""TEST INFRASTRUCTURE ONLY: numpy restatement of the recognition inference tail - what the reference's
InferenceMeter / FeatureMeter (recognition/time_interval_machine/utils/meters.py) and utils/metrics.py compute between the
heads' outputs and the accuracies, written from their contract.  tests/test_recog_ref.py pins it to a fixture recorded from
the reference itself; tests/test_gpu_recog.py then checks the HIP kernels and tim_amd.RecognitionCollector against it.
Never imported by tim_amd."""
import numpy as np

NO_RANK = 0x7fffffff


def accumulate(acc, seen, labels_state, touched, logits, ids, valid, labels=None):
    """one batch of one head group, in place: acc = list of [num_actions, C] fp32 (one per head), logits the matching list
    of [R, C]; the serial fp32 accumulation in row order.  -> True if a valid row carried an id out of range (skipped)"""
    num_actions = seen.shape[0]
    err = False
    for r in range(len(ids)):
        if not valid[r]:
            continue
        a = int(ids[r])
        if a < 0 or a >= num_actions:
            err = True
            continue
        for s, x in zip(acc, logits):
            s[a] = s[a] + np.asarray(x[r], dtype=np.float32)            # fp32 add, one row at a time
        seen[a] = seen[a] + np.float32(1.0)
        touched[a] = 1
        if labels is not None:
            labels_state[a] = np.asarray(labels[r]).astype(np.int32)
    return err


def mean_logits(acc, seen):
    """fp32 sum / fp32 seen count (rows never seen: left at zero)"""
    seen = np.asarray(seen, dtype=np.float32)
    out = np.zeros_like(acc, dtype=np.float32)
    m = seen > 0
    out[m] = (acc[m] / seen[m, None]).astype(np.float32)
    return out


def softmax32(mean):
    """the float64 softmax of fp32 rows (row maximum subtracted), rounded once to fp32"""
    x = np.asarray(mean, dtype=np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def ranks(mean, labels):
    """rank = #{c : mean_c > mean_label} + #{c < label : mean_c == mean_label}; NO_RANK for a label outside [0, C)"""
    mean = np.asarray(mean, dtype=np.float32)
    n, C = mean.shape
    out = np.full(n, NO_RANK, dtype=np.int64)
    for i in range(n):
        l = int(labels[i])
        if 0 <= l < C:
            ml = mean[i, l]
            out[i] = int((mean[i] > ml).sum()) + int((mean[i, :l] == ml).sum())
    return out


def accuracy(rank, size=None):
    """utils/metrics.py accuracy(): float32(count) * float32(100.0 / size) for k = 1, 5"""
    size = len(rank) if size is None else size
    if size == 0:
        return (0.0, 0.0)
    scale = np.float32(100.0 / size)
    return tuple(float(np.float32((np.asarray(rank) < k).sum()) * scale) for k in (1, 5))


def multitask_accuracy(rank_a, rank_b):
    """utils/metrics.py multitask_accuracy(): float32(count) * 100 / size in fp32, every task inside the top k"""
    size = len(rank_a)
    if size == 0:
        return (0.0, 0.0)
    r = np.maximum(np.asarray(rank_a), np.asarray(rank_b))
    return tuple(float(np.float32(np.float32((r < k).sum()) * np.float32(100.0)) / np.float32(size)) for k in (1, 5))


class Collector:
    """numpy mirror of tim_amd.RecognitionCollector (class counts given per head)"""

    VISUAL = ("verb", "noun", "action")

    def __init__(self, classes, num_actions, modality="audio_visual", include_verb_noun=True):
        self.num_actions = num_actions
        self.seen = np.zeros(num_actions, np.float32)
        self.err = False
        self.groups = {}
        if "visual" in modality:
            heads = self.VISUAL if include_verb_noun else ("action",)
            self.groups["visual"] = self._group(heads, classes, 3)
        if "audio" in modality:
            self.groups["audio"] = self._group(("audio",), classes, 1)

    def _group(self, heads, classes, n_labels):
        return dict(heads=heads, acc=[np.zeros((self.num_actions, classes[h]), np.float32) for h in heads],
                    labels=np.full((self.num_actions, n_labels), -1, np.int32), touched=np.zeros(self.num_actions, np.uint8))

    def update(self, logits, v_ids=None, a_ids=None, v_labels=None, a_labels=None, v_valid=None, a_valid=None):
        """logits: {head: [R, C]}; labels [R, 3] (verb, noun, action) / [R]; a row counts iff its last label column != -1"""
        for name, ids, labels, valid in (("visual", v_ids, v_labels, v_valid), ("audio", a_ids, a_labels, a_valid)):
            if name not in self.groups:
                continue
            g = self.groups[name]
            if labels is not None:
                labels = np.asarray(labels).reshape(len(ids), -1)
            if valid is None:
                valid = labels[:, -1] != -1
            self.err |= accumulate(g["acc"], self.seen, g["labels"], g["touched"], [logits[h] for h in g["heads"]],
                                   np.asarray(ids).reshape(-1), np.asarray(valid).reshape(-1), labels)

    def _per_head(self):
        for g in self.groups.values():
            ids = np.nonzero(g["touched"])[0]
            for i, h in enumerate(g["heads"]):
                col = self.VISUAL.index(h) if h != "audio" else 0
                yield h, ids, mean_logits(g["acc"][i][ids], self.seen[ids]), g["labels"][ids, col]

    def ranks(self):
        return {h: (ranks(mean, lab), ids) for h, ids, mean, lab in self._per_head()}

    def predictions(self):
        return {h: (softmax32(mean), ids) for h, ids, mean, lab in self._per_head()}

    def accuracies(self):
        r = self.ranks()
        out = {h: accuracy(v[0]) for h, v in r.items()}
        if "verb" in r and "noun" in r:
            out["mt_action"] = multitask_accuracy(r["verb"][0], r["noun"][0])
        return out
