"""TEST INFRASTRUCTURE ONLY: restatement of the detection meter, written from its contract in include/timhip.h.

Two parts:
  * `side_stats`: the words timhip_det_side_loss_fwd_stats writes, in float64 (per-head focal sums, the last head's positive /
    negative parts among the rows with iou >= 0, the counts, the divisions), on top of tests/losses_ref.py; `focal_part` gives a
    part's float64 sum with the first-order fp32 bound `_side_check` of tests/test_gpu_loss_kernels.py applies to the focal sum
    (the per-element `focal_bound` terms plus the summation term);
  * `DetMeter`: the slot rules of timhip_det_meter_update in double / int64, in the kernel's order (the reference's
    TrainMeter.update, detection/time_interval_machine/utils/meters.py:94-137); `words()` lays the block out as the device does.
    `accidents=True` puts the two audio_visual accidents of the reference's loop back (det scripts/train.py:416-418, :325-326).
tests/test_det_meter_ref.py pins it to fixtures recorded from the reference; tests/test_gpu_det_meter.py checks the kernels and
tim_amd.DetectionMeter against it.  Never imported by tim_amd."""
import numpy as np
import torch

from tests import losses_ref as R

F64 = torch.float64
SLOTS = ("total", "drloc", "visual", "verb", "noun", "action", "visual_reg", "audio", "audio_reg", "positive", "negative")
SIDES = ("visual", "audio")
# words of a side stats block (include/timhip.h: TIMHIP_DET_STAT_*)
(HEAD_SUM, POS_SUM, NEG_SUM, VALID, POSITIVES, DIOU_SUM, NORMALISER, LOSS, CLS, REG, HEAD, POS, NEG, RESERVED, STATS_WORDS) = \
    0, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 17, 18, 19, 20
# word offsets of the state block (include/timhip.h: TIMHIP_DET_METER_*)
UPDATES, SUM, COUNT, RUN, VAL, LAST, NORM, STATE_WORDS = 0, 2, 4, 46, 54, 65, 69, 72


# ================================================================================================ side statistics
def focal_part(x, t, iou, rows_mask, thr, alpha, gamma):
    """the focal sum of one head over the rows of `rows_mask` that have iou >= 0, in float64 -> (sum, bound, magnitude).
    bound: sum of the per-element bounds of `_side_check` (f * focal_bound + 8 * the float32-CPU error + 2u |term| + tiny) plus its
    summation term ((terms per thread) + 8 + blocks) u sum|terms| for the head's launch of min(ceil(n / 256), 512) blocks."""
    x64, t64 = x.to(F64), t.to(F64)
    valid = (iou >= 0) & rows_mask
    w = torch.where(iou < thr, torch.ones_like(iou), iou).to(F64)
    re, s, _ = R.focal(x64, t64, w, valid, alpha, gamma)
    fe, _, _ = R.focal(x.float(), t.float(), w.float(), valid, alpha, gamma)
    bl, _ = R.focal_bound(x64, t64, alpha, gamma)
    f = R._row_factor(x64.shape[0], w, valid, F64)[:, None]
    b_e = f * bl + 8 * (fe.to(F64) - re).abs() + 2 * R.EPS32 * re.abs() + R.TINY32
    n = x.numel()
    blocks = max(min((n + 255) // 256, 512), 1)
    mag = re.abs().sum().item()
    bound = b_e.sum().item() + ((n + blocks * 256 - 1) // (blocks * 256) + 8 + blocks) * R.EPS32 * mag + R.TINY32
    return s.item(), bound, mag


def summation_term(n, mag):
    """the summation term of the same bound alone, for n elements of total magnitude mag"""
    blocks = max(min((n + 255) // 256, 512), 1)
    return ((n + blocks * 256 - 1) // (blocks * 256) + 8 + blocks) * R.EPS32 * mag + R.TINY32


def side_stats(logits, targets, iou, off, reg, thr, alpha, gamma, eps, lambda_reg, momentum, norm_in):
    """float64 restatement of the stats block -> (words [STATS_WORDS] float64, bounds [STATS_WORDS] float64 for the sum words
    HEAD_SUM .. NEG_SUM and DIOU_SUM, 0 elsewhere, mags: the same words' sum of |terms|)"""
    K, rows = len(logits), iou.numel()
    w, b, m = np.zeros(STATS_WORDS), np.zeros(STATS_WORDS), np.zeros(STATS_WORDS)
    pos = off[:, 0] != float("inf") if rows else torch.zeros(0, dtype=torch.bool)
    every = torch.ones(rows, dtype=torch.bool)
    for k in range(K):
        w[HEAD_SUM + k], b[HEAD_SUM + k], m[HEAD_SUM + k] = focal_part(logits[k], targets[k], iou, every, thr, alpha, gamma)
    w[POS_SUM], b[POS_SUM], m[POS_SUM] = focal_part(logits[-1], targets[-1], iou, pos, thr, alpha, gamma)
    w[NEG_SUM], b[NEG_SUM], m[NEG_SUM] = focal_part(logits[-1], targets[-1], iou, ~pos, thr, alpha, gamma)
    dl = R.diou_1d(reg.to(F64), off.to(F64), pos, eps)[0] if rows else torch.zeros(0, dtype=F64)
    npos = float(pos.sum())
    # (the DIoU sum's bound of `_side_check`: 16u per positive row plus the rows launch's summation term)
    blocks = max(min((rows + 255) // 256, 256), 1)
    m[DIOU_SUM] = dl.abs().sum().item()
    b[DIOU_SUM] = 16 * R.EPS32 * npos + ((rows + blocks * 256 - 1) // (blocks * 256) + 6 + 4 * blocks) * R.EPS32 * m[DIOU_SUM] + R.TINY32
    nm = momentum * norm_in + (1.0 - momentum) * max(npos, 1.0)
    w[VALID], w[POSITIVES], w[DIOU_SUM], w[NORMALISER] = float((iou >= 0).sum()), npos, dl.sum().item(), nm
    focal = w[HEAD_SUM:HEAD_SUM + 4].sum()
    w[CLS] = focal / (K * nm)
    w[REG] = lambda_reg * w[DIOU_SUM] / nm if npos > 0 else 0.0
    w[LOSS] = w[CLS] + w[REG]
    w[HEAD:HEAD + 4] = w[HEAD_SUM:HEAD_SUM + 4] / nm
    w[POS], w[NEG] = w[POS_SUM] / nm, w[NEG_SUM] / nm
    return w, b, m


# ================================================================================================ the slot rules
class DetMeter:
    """the state block as named numbers.  update(): `visual` / `audio` are side stats blocks (STATS_WORDS fp32 values, None: the
    side is absent), total / drloc fp32 values (None counts as 0)"""

    def __init__(self, accidents=False):
        self.accidents = accidents
        self.reset()

    def reset(self):
        self.updates = 0
        self.val = np.zeros(len(SLOTS), np.float32)
        self.sum = np.zeros(len(SLOTS), np.float64)
        self.count = np.zeros(len(SLOTS), np.int64)
        self.run = np.zeros((2, 2), np.int64)        # (side, valid / positives)
        self.last = np.zeros((2, 2), np.int32)
        self.norm = np.zeros(2, np.float32)

    def _slot(self, name, val, n):
        s = SLOTS.index(name)
        self.val[s] = np.float32(val)
        self.sum[s] = self.sum[s] + np.float64(np.float32(val)) * np.float64(n)          # the product rounded, then the add
        self.count[s] += n

    def update(self, visual, audio, nheads, total=None, drloc=None):
        zero = np.zeros(STATS_WORDS, np.float32)
        v = zero if visual is None else np.asarray(visual, np.float32).reshape(STATS_WORDS)
        a = zero if audio is None else np.asarray(audio, np.float32).reshape(STATS_WORDS)
        self.updates += 1
        for s, side in enumerate((v, a)):
            self.last[s] = (int(side[VALID]), int(side[POSITIVES]))
            self.run[s] += self.last[s]
            self.norm[s] = side[NORMALISER]
        (v_cls, v_pos), (a_cls, a_pos) = (int(c) for c in self.last[0]), (int(c) for c in self.last[1])
        head = [v[HEAD + k] for k in range(4)]
        v_posl, v_negl = v[POS], v[NEG]
        if self.accidents and audio is not None and visual is not None:
            # train.py:416-418: the per-head sums over the normaliser the audio side has advanced; :325-326: positive_loss and
            # negative_loss hold the audio side's values by the time the meter sees them
            head = [np.float32(v[HEAD_SUM + k]) / np.float32(a[NORMALISER]) for k in range(4)]
            v_posl, v_negl = a[POS], a[NEG]
        if v_cls > 0:
            self._slot("visual", v[CLS], v_cls)
            if nheads == 3:
                self._slot("verb", head[0], v_cls)
                self._slot("noun", head[1], v_cls)
            self._slot("action", head[nheads - 1], v_cls)
            self._slot("visual_reg", v[REG], v_pos)
            self._slot("positive", v_posl, v_pos)
            self._slot("negative", v_negl, v_cls - v_pos)
        if a_cls > 0:
            self._slot("audio", a[CLS], a_cls)
            self._slot("audio_reg", a[REG], a_pos)
            self._slot("positive", a[POS], a_pos)
            self._slot("negative", a[NEG], a_cls - a_pos)
        self._slot("total", np.float32(0.0) if total is None else total, v_cls + a_cls)
        self._slot("drloc", np.float32(0.0) if drloc is None else drloc, v_cls + a_cls)

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
        for s in range(2):
            for k in range(2):
                q[(RUN + 4 * s + 2 * k) // 2] = self.run[s, k]
                w[LAST + 2 * s + k] = self.last[s, k]
        w[VAL:VAL + len(SLOTS)] = self.val.view(np.int32)
        w[NORM:NORM + 2] = self.norm.view(np.int32)
        return w


def update_epoch(best, vis_avg, aud_avg):
    """InferenceMeter.update_epoch (meters.py:425-444) on plain numbers: best = [best_vis, best_aud], updated in place ->
    (best_loss before, is_best)"""
    is_v, is_a = vis_avg < best[0], aud_avg < best[1]
    before = {"visual": best[0], "audio": best[1]}
    is_best = "none"
    if is_v:
        is_best = "visual"
        best[0] = min(vis_avg, best[0])
    if is_a:
        is_best = "audio_" + is_best if "visual" in is_best else "audio"
        best[1] = min(aud_avg, best[1])
    return before, is_best
