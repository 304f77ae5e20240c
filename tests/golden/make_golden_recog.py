"""Golden vectors for the recognition inference tail from the reference's own code (build container only).

    python tests/golden/make_golden_recog.py

Runs the reference's InferenceMeter.update / update_epoch and FeatureMeter.update / finalize_metrics
(recognition/time_interval_machine/utils/meters.py, with utils/metrics.py behind them) on a seeded synthetic stream: 7
batches of 14 visual and 10 audio query rows, head widths 5 / 7 / 23 (verb / noun / action) and 11 (audio), 40 action ids of
which 0 .. 27 are visual, 26 .. 39 audio (two ids are seen by both modalities: the seen count is shared), every action seen
1 to 5 times, several of them more than once inside one batch, -1-padded rows in every batch and one batch without any valid
audio row.  The rows are filtered as recognition/scripts/test.py:122-176 filters them (boolean index on the action label /
the class id) before InferenceMeter sees them; FeatureMeter gets the unfiltered logits and narration-id strings.  fvcore and
simplejson are stubbed (only a timer and a logger are asked of them) and the memory probes of utils/misc.py are replaced
(they query a GPU).  The probabilities InferenceMeter hands to accuracy() are recorded by a wrapper around that function.

The recorder asserts the fixture's condition: in the reference's own fp32 probabilities no action's label ties another
class at the top-1 or top-5 boundary (the cap is zero; the seed is chosen so that it holds).  It also prints the largest
distance, in fp32 ulps, between those probabilities and the float64 softmax of the same mean logits rounded to fp32 - the
bound tests/test_recog_ref.py allows is twice that figure.

tests/golden/recog_small.npz holds the seed, the inputs, the meters' accumulators, seen counts and labels, the recorded
probabilities and the accuracy floats - numbers only, nothing of the reference.
"""
import argparse
import os
import sys
import types

import numpy as np
import numpy._core.defchararray  # noqa: F401  (numpy 2: the reference's np.core.defchararray resolves only once this is imported)
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/recognition"

# ---- stubs for what is not installed / needs a GPU
sj = types.ModuleType("simplejson")
sj.dumps = lambda *a, **k: ""
sys.modules["simplejson"] = sj
for name in ("fvcore", "fvcore.common", "fvcore.common.file_io", "fvcore.common.timer"):
    sys.modules[name] = types.ModuleType(name)


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
import time_interval_machine.utils.misc as ref_misc  # noqa: E402

ref_misc.gpu_mem_usage = lambda: (0.0, 0.0)
ref_misc.cpu_mem_usage = lambda: (0.0, 0.0)

from tests import recog_ref as RR  # noqa: E402

SEED = 20271
NB, RV, RA = 7, 14, 10
CLASSES = {"verb": 5, "noun": 7, "action": 23, "audio": 11}
NUM_ACTIONS, N_VISUAL, FIRST_AUDIO = 40, 28, 26
EMPTY_AUDIO_BATCH = 3


def make_inputs(seed=SEED):
    rng = np.random.default_rng(seed)

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

    v_ids = stream(np.arange(N_VISUAL), RV, None)
    a_ids = stream(np.arange(FIRST_AUDIO, NUM_ACTIONS), RA, EMPTY_AUDIO_BATCH)
    act_labels = np.stack([rng.integers(0, CLASSES[h], size=NUM_ACTIONS) for h in ("verb", "noun", "action")], axis=1)
    aud_labels = rng.integers(0, CLASSES["audio"], size=NUM_ACTIONS)
    v_labels = np.where(v_ids[..., None] >= 0, act_labels[np.maximum(v_ids, 0)], -1).astype(np.int64)     # [NB, RV, 3]
    a_labels = np.where(a_ids >= 0, aud_labels[np.maximum(a_ids, 0)], -1).astype(np.int64)               # [NB, RA]
    logits = {}
    for col, h in enumerate(("verb", "noun", "action", "audio")):
        rows, lab = (RV, v_labels[..., col]) if h != "audio" else (RA, a_labels)
        x = rng.normal(0.0, 2.0, size=(NB, rows, CLASSES[h]))
        b, r = np.nonzero(lab >= 0)
        x[b, r, lab[b, r]] += 2.5 * rng.uniform(0, 1, size=len(b))          # about half of the labels end up on top
        logits[h] = x.astype(np.float32)
    return v_ids, a_ids, v_labels, a_labels, logits


def boundary_ties(prob, labels):
    """number of rows whose label's membership in the top 1 / top 5 depends on how equal probabilities are ordered"""
    n = 0
    for p, l in zip(prob, labels):
        gt, eq = int((p > p[l]).sum()), int((p == p[l]).sum()) - 1
        n += any(gt < k <= gt + eq for k in (1, 5))
    return n


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def main():
    v_ids, a_ids, v_labels, a_labels, logits = make_inputs()
    assert (v_ids == -1).any(axis=1).all() and (a_ids[EMPTY_AUDIO_BATCH] == -1).all()
    assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in v_ids), "no duplicate inside a batch"
    args = argparse.Namespace(dataset="epic", data_modality="audio_visual", include_verb_noun=True, early_stop_period=0,
                              num_class=[[CLASSES["verb"], CLASSES["noun"], CLASSES["action"]], CLASSES["audio"]])
    meter = ref_meters.InferenceMeter(args, NUM_ACTIONS)
    feat = ref_meters.FeatureMeter(NUM_ACTIONS, args)
    T = torch.from_numpy
    for b in range(NB):
        # ---- recognition/scripts/test.py:122-176, restated: filter the rows, then InferenceMeter.update
        target = {"verb": T(v_labels[b, :, 0]), "noun": T(v_labels[b, :, 1]), "action": T(v_labels[b, :, 2]),
                  "class_id": T(a_labels[b])}
        vv = target["action"] != -1
        va = target["class_id"] != -1
        v_target = torch.stack([v[vv] for k, v in target.items() if k != "class_id"], dim=1)
        meter.update(T(logits["verb"][b])[vv], T(logits["noun"][b])[vv], T(logits["action"][b])[vv],
                     T(logits["audio"][b])[va] if va.sum() > 0 else torch.zeros((RA, CLASSES["audio"])),
                     T(v_ids[b])[vv], T(a_ids[b])[va] if va.sum() > 0 else torch.empty((RA,)),
                     v_target, target["class_id"][va] if va.sum() > 0 else torch.empty((RA,)),
                     0.0, 0.0, 0.0, 0.0, 0.0, int(vv.sum()), int(va.sum()))
        # ---- FeatureMeter.update: validity from the narration-id strings
        metadata = {"v_narration_ids": np.array([("v_%d" % i) if i >= 0 else "-1" for i in v_ids[b]]),
                    "a_narration_ids": np.array([("a_%d" % i) if i >= 0 else "-1" for i in a_ids[b]]),
                    "v_action_ids": T(v_ids[b]), "a_action_ids": T(a_ids[b])}
        feat.update((T(logits["verb"][b]), T(logits["noun"][b]), T(logits["action"][b]), T(logits["audio"][b])), metadata)

    out = {"sum_" + h: getattr(meter, p).numpy().copy() for h, p in
           (("verb", "verb_preds"), ("noun", "noun_preds"), ("action", "action_preds"), ("audio", "aud_preds"))}
    for h, p in (("verb", "verb_preds"), ("noun", "noun_preds"), ("action", "action_preds"), ("audio", "aud_preds")):
        assert np.array_equal(out["sum_" + h], getattr(feat, p).numpy()), h      # both meters accumulate alike
    out["seen"] = meter.seen_count.numpy().copy()
    assert np.array_equal(out["seen"], feat.seen_count.numpy())
    out["state_v_labels"], out["state_a_labels"] = meter.v_labels.numpy().copy(), meter.a_labels.numpy().copy()
    counts = np.concatenate([out["seen"][:FIRST_AUDIO], out["seen"][N_VISUAL:]])
    assert set(counts.astype(int)) == {1, 2, 3, 4, 5}, counts

    # ---- update_epoch, with the probabilities it hands to accuracy() recorded
    handed, orig = [], ref_meters.accuracy

    def recording(output, target, topk=(1, 5)):
        handed.append((output.numpy().copy(), target.numpy().copy()))
        return orig(output, target, topk)

    ref_meters.accuracy = recording
    try:
        meter.update_epoch(0)
    finally:
        ref_meters.accuracy = orig
    assert len(handed) == 4
    worst = 0
    for h, (prob, lab) in zip(("verb", "noun", "action", "audio"), handed):
        assert boundary_ties(prob, lab) == 0, "%s: a label ties another class at the top-1 / top-5 boundary: pick another seed" % h
        out["prob_" + h] = prob
        ids = np.nonzero((out["state_v_labels"][:, 2] if h != "audio" else out["state_a_labels"]) != -1)[0]
        d = int(ulps(RR.softmax32(RR.mean_logits(out["sum_" + h][ids], out["seen"][ids])), prob).max())
        print("%-6s C = %2d: %2d actions, reference fp32 softmax vs rounded float64 softmax: at most %d ulp" % (h, prob.shape[1], len(ids), d))
        worst = max(worst, d)
    print("largest distance over the fixture: %d ulp" % worst)
    for h, v in (("verb", meter.verb_acc), ("noun", meter.noun_acc), ("action", meter.action_acc), ("audio", meter.aud_acc),
                 ("mt_action", meter.mt_action_acc)):
        out["acc_" + h] = np.asarray(v, np.float64)
        print("%-9s top-1 %.6f  top-5 %.6f" % (h, v[0], v[1]))

    # ---- FeatureMeter.finalize_metrics: visual actions [0, last_visual), audio actions behind them
    data = feat.finalize_metrics()
    assert int(feat.last_visual) == N_VISUAL
    for h in ("verb", "noun", "action", "audio"):
        out["feat_prob_" + h] = np.asarray(data[h], np.float32)

    path = os.path.join(HERE, "recog_small.npz")
    np.savez_compressed(path, seed=SEED, num_actions=NUM_ACTIONS, last_visual=N_VISUAL, max_ulp=worst,
                        classes=np.asarray([CLASSES[h] for h in ("verb", "noun", "action", "audio")]),
                        v_ids=v_ids, a_ids=a_ids, v_labels=v_labels, a_labels=a_labels,
                        **{"logits_" + h: x for h, x in logits.items()}, **out)
    print("->", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
