"""Golden vectors for the detection meter from the reference's own code (build container only).

    python tests/golden/make_golden_det_meter.py

Drives, on the CPU and in float32, the reference's sigmoid_focal_loss, ctr_diou_loss_1d and get_loss through the arithmetic of
one iteration of detection/scripts/train.py:222-349 (per side: flags from the IoU / offset targets, the running normaliser, the
heads' focal sums, the second reduction="none" pass split into a positive and a negative part, the DIoU term), then hands the
reference's TrainMeter and InferenceMeter (detection/time_interval_machine/utils/meters.py:29-315, :317-572) what train.py:413-430
hands them, as Python floats and ints.  fvcore, simplejson (and psutil where missing) are stubbed: only a timer and a logger are
asked of them.

    det_meter_visual_vn.npz       visual, verb / noun / action heads of 5 / 7 / 23 classes
    det_meter_visual_single.npz   visual, one 11-class head
    det_meter_audio.npz           audio, one 11-class head
    det_meter_av.npz              audio_visual, 5 / 7 / 23 visual heads and an 11-class audio head

Each is a seeded stream of 6 batches of at most 40 query rows; batch 3 has no positive row, batch 5 no valid row (iou < 0
everywhere, three of its rows positive).  The reference indexes the loss of the valid rows with a mask over ALL rows (train.py:272-273), which raises as soon
as one row has iou < 0: on such a (batch, side) the recorder restricts the mask to the valid rows - the third deviation of 7q - and
says so in `mask_restricted`.  In the one-modality fixtures some batches carry such rows; in `av` only the no-valid batch's sides
and the visual side of batch 1 do.

Recorded: the inputs; per (batch, side) a stats block of the reference's float32 values laid out as TIMHIP_DET_STAT_* (raw sums,
counts, the side's normaliser, each value divided by ITS OWN side's normaliser); total and DRLoc loss; every AverageMeter's sum /
count / avg after every batch (`ref_slot_*`: the reference's TrainMeter; the InferenceMeter is asserted equal on the slots it has);
update_epoch() over three epochs of two batches.  `slot_*` is what the tests pin: the reference's numbers where
`pinned_to_reference` is set, and for `av` - where the reference's loop divides the visual per-head sums by the normaliser the
audio side has advanced (train.py:416-418) and overwrites the visual positive / negative loss with the audio side's (:325-326) -
the restatement's numbers (tests/det_meter_ref.py) on VERB, NOUN, ACTION, POSITIVE, NEGATIVE.  Numbers only, nothing of the reference.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/detection"

# ---- stubs for what is not installed
sj = types.ModuleType("simplejson")
sj.dumps = lambda *a, **k: ""
sys.modules["simplejson"] = sj
for name in ("fvcore", "fvcore.common", "fvcore.common.file_io", "fvcore.common.timer"):
    sys.modules[name] = types.ModuleType(name)
try:
    import psutil  # noqa: F401
except ImportError:
    sys.modules["psutil"] = types.ModuleType("psutil")


class _PM:
    open = staticmethod(open)


class _Timer:
    def seconds(self):
        return 0.0

    def reset(self):
        pass

    def pause(self):
        pass


sys.modules["fvcore.common.file_io"].PathManager = _PM
sys.modules["fvcore.common.timer"].Timer = _Timer
sys.path.insert(0, REF)
import time_interval_machine.utils.meters as ref_meters  # noqa: E402
from time_interval_machine.models.helpers.losses.iou import ctr_diou_loss_1d  # noqa: E402
from time_interval_machine.models.helpers.losses.loss import get_loss  # noqa: E402
from time_interval_machine.models.helpers.losses.sigmoid import sigmoid_focal_loss  # noqa: E402

from tests import det_meter_ref as DR  # noqa: E402

NB, MAX_ROWS = 6, 40
NO_POSITIVE, NO_VALID = 3, 5     # (never the first batch after a reset: AverageMeter divides by its count, 0 / 0 raises on Python numbers)
HYPER = dict(iou_threshold=0.6, lambda_reg=0.5, momentum=0.9, norm0=250.0, lambda_audio=0.7, lambda_drloc=0.3)
RUNS = {
    "visual_vn": dict(seed=41003, modality="visual", vn=True, heads={"visual": (5, 7, 23)}),
    "visual_single": dict(seed=41017, modality="visual", vn=False, heads={"visual": (11,)}),
    "audio": dict(seed=41029, modality="audio", vn=False, heads={"audio": (11,)}),
    "av": dict(seed=41041, modality="audio_visual", vn=True, heads={"visual": (5, 7, 23), "audio": (11,)}),
}
ATTR = {"total": "losses", "drloc": "drloc_losses", "visual": "visual_losses", "verb": "visual_verb_losses", "noun": "visual_noun_losses",
        "action": "visual_action_losses", "visual_reg": "visual_reg_losses", "audio": "audio_losses", "audio_reg": "audio_reg_losses",
        "positive": "positive_losses", "negative": "negative_losses"}
AV_FROM_RESTATEMENT = ("verb", "noun", "action", "positive", "negative")


def make_side(rng, b, Cs, outside):
    """one side of one batch: logits / soft targets per head, iou (-1: outside), offsets (inf: not positive), regression output"""
    rows = int(rng.integers(12, MAX_ROWS + 1)) if b != 4 else MAX_ROWS
    xs = [(rng.normal(0.0, 3.0, size=(rows, c))).astype(np.float32) for c in Cs]
    ts = [np.where(rng.uniform(size=(rows, c)) < 0.2, rng.uniform(size=(rows, c)), 0.0).astype(np.float32) for c in Cs]
    iou = rng.uniform(0.0, 1.0, size=rows).astype(np.float32)
    if b == NO_VALID:
        iou[:] = -1.0
    elif outside:
        iou[rng.choice(rows, size=max(rows // 6, 1), replace=False)] = -1.0
    off = np.full((rows, 2), np.inf, np.float32)
    if b == NO_VALID:
        pos = np.arange(min(3, rows))          # positive rows outside: the regression term runs, the classification section does not
    elif b == NO_POSITIVE:
        pos = np.arange(0)
    else:
        cand = np.nonzero(iou >= 0.5)[0]
        pos = cand[:max(len(cand) // 2, 1)]
    off[pos] = rng.uniform(0.05, 3.0, size=(len(pos), 2)).astype(np.float32)
    reg = rng.uniform(0.05, 3.0, size=(rows, 2)).astype(np.float32)
    return xs, ts, iou, off, reg


def reference_side(xs, ts, iou, off, reg, normaliser):
    """the arithmetic of one side of train.py:222-349 on the reference's functions -> (stats block of float32 values, new
    normaliser, whether the split's mask had to be restricted to the valid rows)"""
    T = torch.from_numpy
    K = len(xs)
    iou_t, off_t, reg_t = T(iou.copy()), T(off), T(reg)
    is_pos = off_t[:, 0] != float("inf")
    is_valid = iou_t >= 0.0
    num_pos = is_pos.sum()
    w = iou_t[is_valid]
    w.masked_fill_(w < HYPER["iou_threshold"], 1.0)
    normaliser = (HYPER["momentum"] * normaliser) + ((1.0 - HYPER["momentum"]) * max(num_pos, 1))
    sums = [get_loss(sigmoid_focal_loss, T(x)[is_valid], T(t)[is_valid], weights=w, reduction="sum") for x, t in zip(xs, ts)]
    split = get_loss(sigmoid_focal_loss, T(xs[-1])[is_valid], T(ts[-1])[is_valid], weights=w, reduction="none")
    restricted = not bool(is_valid.all())
    mask = is_pos[is_valid] if restricted else is_pos
    pos_sum, neg_sum = split[mask].sum(), split[~mask].sum()
    cls = (sums[0] + sums[1] + sums[2]) / (3.0 * normaliser) if K == 3 else sums[0] / normaliser
    diou = torch.zeros(())
    regl = torch.zeros(())
    if num_pos > 0:
        diou = get_loss(ctr_diou_loss_1d, reg_t[is_pos], off_t[is_pos], reduction="sum")
        regl = (diou * HYPER["lambda_reg"]) / normaliser
    w32 = np.zeros(DR.STATS_WORDS, np.float32)
    for k in range(K):
        w32[DR.HEAD_SUM + k] = sums[k].item()
        w32[DR.HEAD + k] = (sums[k] / normaliser).item()
    w32[DR.POS_SUM], w32[DR.NEG_SUM] = pos_sum.item(), neg_sum.item()
    w32[DR.POS], w32[DR.NEG] = (pos_sum / normaliser).item(), (neg_sum / normaliser).item()
    w32[DR.VALID], w32[DR.POSITIVES] = int(is_valid.sum()), int(num_pos)
    w32[DR.DIOU_SUM], w32[DR.NORMALISER] = diou.item(), float(normaliser)
    w32[DR.CLS], w32[DR.REG] = cls.item(), regl.item()
    w32[DR.LOSS] = (cls + regl).item()
    tensors = dict(sums=sums, cls=cls, reg=regl, pos=pos_sum / normaliser, neg=neg_sum / normaliser, n_cls=is_valid.sum(), n_pos=num_pos)
    return w32, normaliser, restricted, tensors


def record(name, run):
    rng = np.random.default_rng(run["seed"])
    sides = [s for s in DR.SIDES if s in run["modality"]]
    args = argparse.Namespace(data_modality=run["modality"], include_verb_noun=run["vn"], lambda_drloc=HYPER["lambda_drloc"])
    train, val = ref_meters.TrainMeter(args), ref_meters.InferenceMeter(args)
    val_run = ref_meters.InferenceMeter(args)      # never reset: compared with the TrainMeter; `val` is reset after every epoch
    restate = DR.DetMeter()
    out = {"ref_slot_" + k: np.zeros((NB, len(DR.SLOTS)), np.int64 if k == "count" else np.float64) for k in ("sum", "count", "avg")}
    out.update({"slot_" + k: np.zeros_like(out["ref_slot_" + k]) for k in ("sum", "count", "avg")})
    stats = np.zeros((NB, 2, DR.STATS_WORDS), np.float32)
    restricted = np.zeros((NB, 2), bool)
    total, drloc = np.zeros(NB, np.float32), np.zeros(NB, np.float32)
    inputs = {}
    normaliser = HYPER["norm0"]
    best_before, best_str = np.zeros((3, 2)), []
    zero = torch.zeros(())
    for b in range(NB):
        got = {}
        for side in sides:
            s = DR.SIDES.index(side)
            outside = (b in (1, 3)) if name != "av" else (b == 1 and side == "visual")
            xs, ts, iou, off, reg = make_side(rng, b, run["heads"][side], outside)
            for k, (x, t) in enumerate(zip(xs, ts)):
                inputs["b%d_%s_logits%d" % (b, side, k)], inputs["b%d_%s_targets%d" % (b, side, k)] = x, t
            inputs["b%d_%s_iou" % (b, side)], inputs["b%d_%s_offsets" % (b, side)], inputs["b%d_%s_reg" % (b, side)] = iou, off, reg
            stats[b, s], normaliser, restricted[b, s], got[side] = reference_side(xs, ts, iou, off, reg, normaliser)
        v, a = got.get("visual"), got.get("audio")
        if run["modality"] == "visual":
            loss = v["cls"] + v["reg"]
        elif run["modality"] == "audio":
            loss = a["cls"] + a["reg"]
        else:
            loss = (v["cls"] + v["reg"]) + HYPER["lambda_audio"] * (a["cls"] + a["reg"])
        dr = torch.tensor(float(np.float32(rng.uniform(0.1, 2.0))))
        loss = loss + HYPER["lambda_drloc"] * dr
        total[b], drloc[b] = loss.item(), dr.item()
        # what train.py:413-430 hands over: the per-head sums over the FINAL normaliser, the LAST side's positive / negative loss
        last = a if a is not None else v
        vs = v["sums"] if v is not None else [zero, zero, zero]
        verb, noun, action = (vs[0], vs[1], vs[2]) if len(vs) == 3 else (zero, zero, vs[0])
        num = lambda t: int(t) if t is not None else 0   # noqa: E731
        handed = [(v["cls"] if v else zero).item(), (verb / normaliser).item(), (noun / normaliser).item(), (action / normaliser).item(),
                  (v["reg"] if v else zero).item(), (a["cls"] if a else zero).item(), (a["reg"] if a else zero).item(), loss.item()]
        counts = [num(v and v["n_cls"]), num(a and a["n_cls"]), num(v and v["n_pos"]), num(a and a["n_pos"])]
        train.update(*handed, dr.item(), last["pos"].item(), last["neg"].item(), *counts)
        val.update(*handed, last["pos"].item(), last["neg"].item(), *counts)
        val_run.update(*handed, last["pos"].item(), last["neg"].item(), *counts)
        restate.update(stats[b, 0] if v else None, stats[b, 1] if a else None, 3 if run["vn"] else 1, total[b], drloc[b])
        for s, k in enumerate(DR.SLOTS):
            if not hasattr(train, ATTR[k]):
                continue
            m = getattr(train, ATTR[k])
            out["ref_slot_sum"][b, s], out["ref_slot_count"][b, s], out["ref_slot_avg"][b, s] = m.sum, m.count, m.avg
            if k != "drloc":
                mv = getattr(val_run, ATTR[k])
                assert (mv.sum, mv.count, mv.avg) == (m.sum, m.count, m.avg), "the InferenceMeter runs the same averages"
        for s, k in enumerate(DR.SLOTS):
            out["slot_sum"][b, s], out["slot_count"][b, s], out["slot_avg"][b, s] = restate.sum[s], restate.count[s], restate.avg(k)
        if b % 2 == 1:     # an epoch of two batches ends: the InferenceMeter's bookkeeping, then its reset
            e = b // 2
            before, is_best = val.update_epoch(e)
            best_before[e] = (before["visual"], before["audio"])
            best_str.append(is_best)
            val.reset()
    pinned = np.array([not (name == "av" and k in AV_FROM_RESTATEMENT) for k in DR.SLOTS])
    for s in np.nonzero(pinned)[0]:
        for k in ("sum", "count", "avg"):
            assert np.array_equal(out["slot_" + k][:, s], out["ref_slot_" + k][:, s]), (name, DR.SLOTS[s], k)
            out["slot_" + k][:, s] = out["ref_slot_" + k][:, s]
    assert restricted[NO_VALID].any() and (stats[NO_POSITIVE, :, DR.POSITIVES] == 0).all()
    path = os.path.join(HERE, "det_meter_%s.npz" % name)
    np.savez_compressed(path, seed=run["seed"], modality=run["modality"], include_verb_noun=run["vn"], sides=np.asarray(sides),
                        heads_visual=np.asarray(run["heads"].get("visual", ()), np.int64),
                        heads_audio=np.asarray(run["heads"].get("audio", ()), np.int64), stats=stats, mask_restricted=restricted,
                        total=total, drloc=drloc, pinned_to_reference=pinned, best_before=best_before, is_best=np.asarray(best_str),
                        final_normaliser=np.float32(float(normaliser)), **{k: np.float64(v) for k, v in HYPER.items()}, **inputs, **out)
    print("%-14s total avg %.6f, positives %d, restricted masks %d -> %s (%d bytes)"
          % (name, out["slot_avg"][-1, 0], int(stats[:, :, DR.POSITIVES].sum()), int(restricted.sum()), path, os.path.getsize(path)))


if __name__ == "__main__":
    for name, run in RUNS.items():
        record(name, run)
