"""TEST INFRASTRUCTURE ONLY: numpy restatement of the training meter (tim_amd/csrc/meter.hip), written from its
contract in include/timhip.h: float64 loss slots weighted by the valid counts (the reference's AverageMeter.update under the
conditions of TrainMeter.update, recognition/time_interval_machine/utils/meters.py:13-29, :140-167), the rank rule on raw
logits, the running and last-batch counters, and the positional pairing of the AVE "combined" accuracy (meters.py:283-285).
tests/test_meter_ref.py pins it to fixtures recorded from the reference itself; tests/test_gpu_meter.py then checks the HIP
kernels and tim_amd.TrainMeter against it, bit for bit.  Never imported by tim_amd."""
import numpy as np

NO_RANK = 0x7fffffff
SLOTS = ("total", "drloc", "visual", "verb", "noun", "action", "audio")
HEADS = ("verb", "noun", "action", "mt_action", "audio")
LABEL_COL = {"verb": 0, "noun": 1, "action": 2, "audio": 0}
# word offsets of the state block (include/timhip.h: TIMHIP_METER_*)
UPDATES, SUM, COUNT, RUN, VAL, LAST, NV, NA, STATE_WORDS = 0, 2, 4, 30, 60, 67, 82, 83, 84


def row_rank(x, y):
    """rank of label y over one row of raw logits: #{c : x_c > x_y} + #{c < y : x_c == x_y}; NO_RANK when y is outside
    [0, C) or x_y is NaN (comparisons with a NaN elsewhere in the row are false: it never counts)"""
    x = np.asarray(x, dtype=np.float32)
    y = int(y)
    if y < 0 or y >= x.shape[0] or np.isnan(x[y]):
        return NO_RANK
    with np.errstate(invalid="ignore"):
        return int((x > x[y]).sum()) + int((x[:y] == x[y]).sum())


def ranks(logits, labels):
    return np.array([row_rank(x, y) for x, y in zip(logits, labels)], dtype=np.int64)


class Meter:
    """the state block as named numbers; `words()` lays it out as the device does"""

    def __init__(self, include_verb_noun=True, batch_accuracy=True):
        self.include_verb_noun, self.batch_accuracy = include_verb_noun, batch_accuracy
        self.reset()

    def reset(self):
        self.updates = 0
        self.val = np.zeros(len(SLOTS), np.float32)
        self.sum = np.zeros(len(SLOTS), np.float64)
        self.count = np.zeros(len(SLOTS), np.int64)
        self.run = np.zeros((len(HEADS), 3), np.int64)       # rows, top-1 hits, top-5 hits
        self.last = np.zeros((len(HEADS), 3), np.int32)
        self.nv = self.na = 0

    def _slot(self, name, val, n):
        s = SLOTS.index(name)
        self.val[s] = val
        self.sum[s] = self.sum[s] + np.float64(val) * np.float64(n)          # the product rounded, then the add
        self.count[s] += n

    def update(self, logits, v_labels=None, a_labels=None, losses=None):
        """logits: {head: [R, C] fp32} (the heads this meter ranks); v_labels [Rv, 3] / a_labels [Ra] or None; losses:
        {slot: fp32 value}, a missing one counts as 0"""
        Rv = 0 if v_labels is None else len(v_labels)
        Ra = 0 if a_labels is None else len(a_labels)
        if Rv == 0 and Ra == 0:
            return
        losses = {k: np.float32(v) for k, v in (losses or {}).items()}
        val = lambda k: losses.get(k, np.float32(0.0))   # noqa: E731
        v_labels = np.zeros((0, 3), np.int64) if v_labels is None else np.asarray(v_labels).reshape(Rv, 3)
        a_labels = np.zeros((0,), np.int64) if a_labels is None else np.asarray(a_labels).reshape(Ra)
        vv, va = v_labels[:, 2] != -1, a_labels != -1
        nv, na = int(vv.sum()), int(va.sum())
        self.updates += 1
        self.nv, self.na = nv, na
        self.last[:] = 0
        if self.batch_accuracy:
            got = {}
            for h in ("verb", "noun", "action", "audio"):
                if h not in logits:
                    continue
                rows, lab = (np.nonzero(va)[0], a_labels) if h == "audio" else (np.nonzero(vv)[0], v_labels[:, LABEL_COL[h]])
                got[h] = ranks(np.asarray(logits[h])[rows], lab[rows])
            if "verb" in got and "noun" in got:
                got["mt_action"] = np.maximum(got["verb"], got["noun"])
            for h, r in got.items():
                self.last[HEADS.index(h)] = (len(r), int((r < 1).sum()), int((r < 5).sum()))
        self.run += self.last
        self._slot("total", val("total"), nv + na)
        self._slot("drloc", val("drloc"), nv + na)
        if nv > 0:
            self._slot("visual", val("visual"), nv)
            if self.include_verb_noun:
                self._slot("verb", val("verb"), nv)
                self._slot("noun", val("noun"), nv)
            self._slot("action", val("action"), nv)
        if na > 0:
            self._slot("audio", val("audio"), na)

    def avg(self, name):
        s = SLOTS.index(name)
        return float(self.sum[s] / self.count[s]) if self.count[s] else 0.0

    def words(self):
        """the block: STATE_WORDS int32"""
        w = np.zeros(STATE_WORDS, np.int32)
        q = w[:VAL].view(np.int64)
        q[UPDATES // 2] = self.updates
        for s in range(len(SLOTS)):
            q[(SUM + 4 * s) // 2] = self.sum[s:s + 1].view(np.int64)[0]
            q[(COUNT + 4 * s) // 2] = self.count[s]
        for h in range(len(HEADS)):
            for k in range(3):
                q[(RUN + 6 * h + 2 * k) // 2] = self.run[h, k]
                w[LAST + 3 * h + k] = self.last[h, k]
        w[VAL:VAL + len(SLOTS)] = self.val.view(np.int32)
        w[NV], w[NA] = self.nv, self.na
        return w


def combined_ranks(prob_action, ids_v, prob_audio, ids_a, action_labels):
    """the positional pairing of meters.py:283-285: the k-th labelled visual action (ascending id) with the k-th labelled
    audio action; (p_action + p_audio) * 0.5 in fp32, ranked against the visual action label with the tie rule above.
    prob_*: [n, C] fp32 over ascending ids_*; unequal n or C do not broadcast in the reference: ValueError"""
    prob_action, prob_audio = np.asarray(prob_action, np.float32), np.asarray(prob_audio, np.float32)
    assert np.all(np.diff(ids_v) > 0) and np.all(np.diff(ids_a) > 0)
    if prob_action.shape != prob_audio.shape:
        raise ValueError("%s and %s do not broadcast" % (prob_action.shape, prob_audio.shape))
    score = ((prob_action + prob_audio).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    return ranks(score, action_labels)
