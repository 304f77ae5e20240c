"""Golden vectors for the training meter from the reference's own code (build container only).

    python tests/golden/make_golden_meter.py

Drives the reference's recognition TrainMeter (recognition/time_interval_machine/utils/meters.py:30-395: update, update_epoch)
and utils/metrics.py (accuracy, multitask_accuracy) with a seeded synthetic stream of 7 batches of 18 visual and 16 audio
query rows, -1-padded rows in every batch, one batch without a valid visual row and one without a valid audio row.  The
rows are filtered as recognition/scripts/train.py:220-330 filters them (boolean index on the action label / the class id),
and the meter is handed Python floats and ints - the numbers its signature suggests (train.py itself hands it 0-dim tensors as
counts: DESIGN.md 7p, deviation 2).  fvcore and simplejson are stubbed exactly as tests/golden/make_golden_recog.py stubs
them (that module is imported for it).

    meter_small.npz   dataset "epic", include_verb_noun, head widths 5 / 7 / 23 / 11, 40 action ids (0 .. 27 visual, 26 .. 39
                      audio: two ids are seen by both modalities)
    meter_ave.npz     dataset "ave", no verb / noun heads, 11 classes on both heads, 20 visual ids (0 .. 19) and 20 audio ids
                      (20 .. 39): equal counts, disjoint ranges, so update_epoch() forms the "combined" accuracy

Recorded: the inputs, the seven loss values per batch (fp32-representable), every AverageMeter's sum / count / avg after every
batch, the epoch accuracies (with combined_acc for AVE), the ensemble's probabilities, and - the batch accuracies the device
meter adds - what the reference's accuracy() / multitask_accuracy() return on each batch's valid raw logits.  Numbers only,
nothing of the reference.

The recorder asserts the fixtures' condition: for every action, in float64, the label's probability differs from every other
class's by more than 1e-5 relative, for the single heads and for the combined scores alike, so that no reference topk tie or
last-ulp softmax difference decides a count; and no label of a valid row ties another class of its raw logits.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_recog as G  # noqa: E402  (stubs fvcore / simplejson and imports the reference's meters module)

from time_interval_machine.utils.metrics import accuracy, multitask_accuracy  # noqa: E402

from tests import meter_ref as MR  # noqa: E402
from tests import recog_ref as RR  # noqa: E402

ref_meters = G.ref_meters
NB, RV, RA, NUM_ACTIONS = 7, 18, 16, 40
MARGIN = 1e-5
RUNS = {
    "small": dict(seed=31007, dataset="epic", include_verb_noun=True, classes={"verb": 5, "noun": 7, "action": 23, "audio": 11},
                  v_actions=np.arange(0, 28), a_actions=np.arange(26, 40), empty_v=5, empty_a=3),
    "ave": dict(seed=31011, dataset="ave", include_verb_noun=False, classes={"action": 11, "audio": 11},
                v_actions=np.arange(0, 20), a_actions=np.arange(20, 40), empty_v=2, empty_a=4),
}
ATTR = {"total": "losses", "drloc": "drloc_losses", "visual": "visual_losses", "verb": "visual_verb_losses",
        "noun": "visual_noun_losses", "action": "visual_action_losses", "audio": "audio_losses"}


def make_inputs(run):
    rng = np.random.default_rng(run["seed"])
    classes = run["classes"]

    def stream(action_ids, rows, skip_batch):
        """ids [NB, rows] (-1 padded): action k of the list is seen 1 + k % 5 times, at random slots in stream order"""
        occ = np.concatenate([np.full(1 + k % 5, a) for k, a in enumerate(action_ids)])
        rng.shuffle(occ)
        usable = np.array([b * rows + r for b in range(NB) if b != skip_batch for r in range(rows)])
        assert len(occ) < len(usable)
        slots = np.sort(rng.choice(usable, size=len(occ), replace=False))
        ids = np.full(NB * rows, -1, np.int64)
        ids[slots] = occ
        return ids.reshape(NB, rows)

    v_ids = stream(run["v_actions"], RV, run["empty_v"])
    a_ids = stream(run["a_actions"], RA, run["empty_a"])
    widths = [classes.get("verb", classes["action"]), classes.get("noun", classes["action"]), classes["action"]]
    act_labels = np.stack([rng.integers(0, w, size=NUM_ACTIONS) for w in widths], axis=1)
    aud_labels = rng.integers(0, classes["audio"], size=NUM_ACTIONS)
    v_labels = np.where(v_ids[..., None] >= 0, act_labels[np.maximum(v_ids, 0)], -1).astype(np.int64)     # [NB, RV, 3]
    a_labels = np.where(a_ids >= 0, aud_labels[np.maximum(a_ids, 0)], -1).astype(np.int64)               # [NB, RA]
    logits = {}
    for h in classes:
        rows, lab = (RA, a_labels) if h == "audio" else (RV, v_labels[..., MR.LABEL_COL[h]])
        x = rng.normal(0.0, 2.0, size=(NB, rows, classes[h]))
        b, r = np.nonzero(lab >= 0)
        x[b, r, lab[b, r]] += 2.5 * rng.uniform(0, 1, size=len(b))          # about half of the labels end up on top
        logits[h] = x.astype(np.float32)
    losses = rng.uniform(0.05, 6.0, size=(NB, len(MR.SLOTS))).astype(np.float32)
    return v_ids, a_ids, v_labels, a_labels, logits, losses


def margin_ok(prob64, labels):
    """every other class's probability is more than MARGIN (relative) away from the label's"""
    for p, l in zip(prob64, labels):
        d = np.abs(p - p[l]) / np.maximum(p, p[l])
        d[l] = 1.0
        if d.min() <= MARGIN:
            return False
    return True


def softmax64(mean32):
    x = np.asarray(mean32, np.float32).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def record(name, run):
    v_ids, a_ids, v_labels, a_labels, logits, losses = make_inputs(run)
    classes, vn = run["classes"], run["include_verb_noun"]
    assert (v_ids[run["empty_v"]] == -1).all() and (a_ids[run["empty_a"]] == -1).all()
    assert (v_ids == -1).any(axis=1).all() and (a_ids == -1).any(axis=1).all()
    num_class = [[classes["verb"], classes["noun"], classes["action"]] if vn else classes["action"], classes["audio"]]
    args = argparse.Namespace(dataset=run["dataset"], data_modality="audio_visual", include_verb_noun=vn, lambda_drloc=0.1,
                              enable_amp=False, num_class=num_class)
    meter = ref_meters.TrainMeter(args, NUM_ACTIONS)
    T = torch.from_numpy
    heads = [h for h in ("verb", "noun", "action", "audio") if h in classes]
    out = {"slot_" + k: np.zeros((NB, len(MR.SLOTS)), np.float64 if k != "count" else np.int64) for k in ("sum", "count", "avg")}
    for h in heads + (["mt_action"] if vn else []):
        out["batch_acc_" + h] = np.zeros((NB, 2), np.float64)
    for b in range(NB):
        vv, va = v_labels[b, :, 2] != -1, a_labels[b] != -1
        nv, na = int(vv.sum()), int(va.sum())
        assert nv + na > 0
        x = {h: T(logits[h][b])[T(va if h == "audio" else vv)] for h in heads}
        zeros = torch.zeros((RV, 3))
        loss = {k: float(losses[b, s]) for s, k in enumerate(MR.SLOTS)}                    # Python floats, fp32-representable
        meter.update(x.get("verb", zeros), x.get("noun", zeros), x["action"], x["audio"], T(v_ids[b])[T(vv)], T(a_ids[b])[T(va)],
                     T(v_labels[b])[T(vv)], T(a_labels[b])[T(va)], loss["visual"], loss["verb"], loss["noun"], loss["action"],
                     loss["audio"], loss["total"], loss["drloc"], nv, na)
        for s, k in enumerate(MR.SLOTS):
            m = getattr(meter, ATTR[k])
            out["slot_sum"][b, s], out["slot_count"][b, s], out["slot_avg"][b, s] = m.sum, m.count, m.avg
        # ---- the batch accuracies: the reference's own accuracy functions on the valid rows' raw logits
        for h in heads:
            lab = T(a_labels[b])[T(va)] if h == "audio" else T(v_labels[b, :, MR.LABEL_COL[h]])[T(vv)]
            if len(lab):
                assert G.boundary_ties(x[h].numpy(), lab.numpy()) == 0, "a raw-logit tie at a boundary: pick another seed"
                out["batch_acc_" + h][b] = accuracy(x[h], lab)
        if vn and nv:
            out["batch_acc_mt_action"][b] = multitask_accuracy((x["verb"], x["noun"]), (T(v_labels[b, :, 0])[T(vv)], T(v_labels[b, :, 1])[T(vv)]))
    if not vn:
        assert all(getattr(meter, ATTR[k]).count == 0 for k in ("verb", "noun"))

    # ---- update_epoch, with the probabilities it hands to accuracy() recorded
    handed, orig = [], ref_meters.accuracy

    def recording(output, target, topk=(1, 5)):
        handed.append((output.numpy().copy(), target.numpy().copy()))
        return orig(output, target, topk)

    ref_meters.accuracy = recording
    try:
        meter.update_epoch()
    finally:
        ref_meters.accuracy = orig
    names = heads + (["combined"] if run["dataset"] == "ave" else [])
    assert len(handed) == len(names)
    seen, state_v, state_a = meter.seen_count.numpy(), meter.v_labels.numpy(), meter.a_labels.numpy()
    ids_v, ids_a = np.nonzero(state_v[:, 2] != -1)[0], np.nonzero(state_a != -1)[0]
    assert np.array_equal(ids_v, run["v_actions"]) and np.array_equal(ids_a, run["a_actions"])
    p64 = {}
    for h, (prob, lab) in zip(names, handed):
        out["prob_" + h] = prob
        if h == "combined":
            p64[h] = (p64["action"] + p64["audio"]) / 2.0
        else:
            acc = getattr(meter, {"verb": "verb_preds", "noun": "noun_preds", "action": "action_preds", "audio": "aud_preds"}[h]).numpy()
            ids = ids_a if h == "audio" else ids_v
            p64[h] = softmax64(RR.mean_logits(acc[ids], seen[ids]))
            out["sum_" + h] = acc.copy()
        assert np.abs(p64[h] - prob).max() < 1e-6
        assert margin_ok(p64[h], lab), "%s: a label's probability is within %g of another class's: pick another seed" % (h, MARGIN)
        assert G.boundary_ties(prob, lab) == 0
    for h, v in (("verb", meter.verb_acc), ("noun", meter.noun_acc), ("action", meter.action_acc), ("audio", meter.aud_acc),
                 ("mt_action", meter.mt_action_acc), ("combined", meter.combined_acc)):
        if h in names or (h == "mt_action" and vn):
            out["acc_" + h] = np.asarray(v, np.float64)
            print("%-6s %-9s top-1 %.6f  top-5 %.6f" % (name, h, v[0], v[1]))
    path = os.path.join(HERE, "meter_%s.npz" % name)
    np.savez_compressed(path, seed=run["seed"], num_actions=NUM_ACTIONS, include_verb_noun=vn, dataset=run["dataset"],
                        heads=np.asarray(heads), classes=np.asarray([classes[h] for h in heads]), v_ids=v_ids, a_ids=a_ids,
                        v_labels=v_labels, a_labels=a_labels, losses=losses, seen=seen, state_v_labels=state_v, state_a_labels=state_a,
                        **{"logits_" + h: x for h, x in logits.items()}, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for name, run in RUNS.items():
        record(name, run)
