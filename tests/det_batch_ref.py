"""CPU restatement, in numpy, of the reference's DETECTION `SlidingWindowDataset.__getitem__`
(detection/time_interval_machine/datasets/sliding_window.py:324-399) plus `default_collate`, over the tables of
tests/golden/det_batch_inputs.py - what `tim_amd.det_data.DeviceDetectionDataset.batch()` and `timhip_det_window_batch` must
return, bit for bit.  tests/test_det_batch_ref.py holds it against the reference's own outputs (tests/golden/det_batch_*.npz).

Every floating-point step is one fp32 operation, as torch's CPU kernels do them:
    d = t - float32(start_sec)            (the Python scalar is rounded to fp32, then one subtraction)
    r = rint(d * 1000f) / 1000f           (torch.round(decimals=3): product, round half to even, division)
    out = max(r / float32(window_size), 0)
`round3` swaps the middle step for the two restatements that are NOT torch's (float64, a product with 0.001f): the tests
show that the same comparison rejects them.
"""
import numpy as np

from tests.golden.det_batch_inputs import round3_f32

F32 = np.float32


def action_column(dataset_name="epic", include_verb_noun=True, verb_only=True):
    if dataset_name == "epic" and not include_verb_noun:
        return 0 if verb_only else 1
    return 2


def normalise(t, start_sec, window_size, round3=round3_f32):
    d = (np.asarray(t, F32) - F32(start_sec)).astype(F32)
    return np.maximum((round3(d) / F32(window_size)).astype(F32), F32(0.0)).astype(F32)


def getitem(tb, i, v_aug=None, a_aug=None, action_col=2, round3=round3_f32):
    """-> dict of one window's sample: v, a (or empty), times [T, 2], the six label entries, window_start, video_id"""
    w, nf, ws = tb["windows"][i], tb["num_feats"], tb["window_size"]
    fi, vid, start = np.asarray(w["feat_indices"]), w["video_id"], w["start_sec"]
    v, a, times = np.zeros((0,), F32), np.zeros((0,), F32), np.zeros((0, 2), F32)
    if "visual" in tb["model_modality"]:
        v = tb["v_feats"][vid][fi, np.zeros(nf, np.int64) if v_aug is None else np.asarray(v_aug)]
        times = np.concatenate([times, tb["v_feat_times"][vid][fi, :2]])
    if "audio" in tb["model_modality"]:
        a = tb["a_feats"][vid][fi, np.zeros(nf, np.int64) if a_aug is None else np.asarray(a_aug)]
        times = np.concatenate([times, tb["a_feat_times"][vid][fi, :2]])
    out = {"v": v, "a": a, "times": normalise(times, start, ws, round3), "window_start": float(start), "video_id": vid}
    for side, mx in (("v", tb["max_visual_actions"]), ("a", tb["max_audio_actions"])):
        seg, lab = np.asarray(w[side + "_gt_segments"], F32).reshape(-1, 2), np.asarray(w[side + "_labels"], np.int64).reshape(-1, 4)
        n = lab.shape[0]
        assert n <= mx
        ps, pl = np.zeros((mx, 2), F32), np.full((mx, 4), -1, np.int64)
        ps[:n], pl[:n] = normalise(seg, start, ws, round3), lab          # (padded slots: 0.0 after the rounding, 0.0 / ws = 0.0)
        out[side + "_gt_segments"] = ps
        if side == "v":
            out["verb"], out["noun"], out["action"] = pl[:, 0], pl[:, 1], pl[:, action_col]
        else:
            out["class_id"] = pl[:, 3]
    return out


LABEL_KEYS = ("v_gt_segments", "a_gt_segments", "verb", "noun", "action", "class_id")


def batch(tb, windows, v_aug=None, a_aug=None, action_col=2, valid=None, round3=round3_f32):
    """default_collate of getitem over `windows` -> (v, a, times, label, metadata); an absent modality is an empty [B, 0].
    valid (uint8 [B], the sampler's): a row with valid == 0 keeps features, times, window_start and video_index and reads -1 in
    every label, 0.0 in every ground-truth segment."""
    items = [getitem(tb, int(w), None if v_aug is None else v_aug[b], None if a_aug is None else a_aug[b], action_col, round3)
             for b, w in enumerate(windows)]
    stack = lambda k: np.stack([it[k] for it in items])   # noqa: E731
    v, a = stack("v"), stack("a")
    label = {k: stack(k) for k in LABEL_KEYS}
    if valid is not None:
        gone = np.asarray(valid) == 0
        for k in LABEL_KEYS:
            label[k][gone] = 0.0 if k.endswith("segments") else -1
    vids = tb["video_ids"]
    meta = {"window_start": np.array([it["window_start"] for it in items], np.float64),
            "window_size": np.full(len(items), tb["window_size"], np.float64), "video_id": [it["video_id"] for it in items],
            "video_index": np.array([vids.index(it["video_id"]) for it in items], np.int32)}
    return v, a, stack("times"), label, meta
