"""Recognition evaluation end to end on the MI355X path, on synthetic data - the shape of recognition/scripts/test.py
(validate) with every piece served by tim_amd:

    DeviceWindowDataset.batch()      <- DataLoader workers + default_collate + .cuda()      (sliding_window.py:341-421)
    model.eval(); model(times, "time_mlp"), model(inputs, "encoder", ...)                    (models/tim.py)
    RecognitionCollector.update      <- boolean indexing, dense .cpu() copies, InferenceMeter.update (test.py:122-211)
    RecognitionCollector.accuracies  <- InferenceMeter.update_epoch + utils/metrics.py

Sliding windows overlap by half, so most actions are queried by two or three windows: the collector sums their logits per
action (in stream order, like the reference's CPU index_add_), divides by the seen count and ranks the label.

    python examples/eval_synthetic.py [--videos 3] [--actions 6] [--batch 4] [--precision bf16]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import RecognitionCollector, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.data import DeviceWindowDataset  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402


def synthetic_eval_dataset(cfg, n_videos, n_actions, nv, na, dev, seed=0):
    """videos with `n_actions` visual and `n_actions` audio annotations each, cut into windows that advance by half a window:
    a window queries every annotation it overlaps (at most nv / na of them).  -> (dataset, number of action ids)"""
    rs = np.random.RandomState(seed)
    nf, hop = cfg.num_feats, 0.2
    window = nf * 2 * hop                                     # a window takes every second feature
    n_feat = 6 * nf
    st = (np.arange(n_feat) * hop).astype(np.float32)
    ft = np.stack([st, st + 1.0], 1)
    vids = ["vid%02d" % i for i in range(n_videos)]
    vf = {v: synth.normal(seed, "v" + v, (n_feat, 1, cfg.visual_input_dim)).astype(np.float32) for v in vids}
    af = {v: synth.normal(seed, "a" + v, (n_feat, 1, cfg.audio_input_dim)).astype(np.float32) for v in vids}
    vc, ac = cfg.num_class[0], cfg.num_class[1]
    length = n_feat * hop
    n_visual = n_videos * n_actions                           # visual ids first, audio ids behind them, as in the reference
    windows = []
    for k, v in enumerate(vids):
        t0 = np.sort(rs.uniform(0, length - 1.0, size=(2, n_actions)), axis=1)
        seg = np.stack([t0, t0 + rs.uniform(0.3, 1.0, size=(2, n_actions))], axis=-1).astype(np.float32)     # [modality, action, 2]
        vlab = np.stack([rs.randint(0, vc[0], n_actions), rs.randint(0, vc[1], n_actions), rs.randint(0, vc[2], n_actions),
                         np.full(n_actions, -1)], 1)
        alab = np.stack([np.full(n_actions, -1)] * 3 + [rs.randint(0, ac, n_actions)], 1)
        for first in range(0, n_feat - 2 * nf + 1, nf):       # half a window at a time
            start = first * hop
            hit = lambda s, most: np.nonzero((s[:, 1] > start) & (s[:, 0] < start + window))[0][:most]
            iv, ia = hit(seg[0], nv), hit(seg[1], na)
            windows.append({"video_id": v, "start_sec": start, "feat_indices": np.arange(first, first + 2 * nf, 2),
                            "v_queries": seg[0][iv], "v_labels": vlab[iv].astype(np.int64), "v_action_ids": k * n_actions + iv,
                            "v_narration_ids": ["v_%s_%d" % (v, i) for i in iv],
                            "a_queries": seg[1][ia], "a_labels": alab[ia].astype(np.int64),
                            "a_action_ids": n_visual + k * n_actions + ia, "a_narration_ids": ["a_%s_%d" % (v, i) for i in ia]})
    ds = DeviceWindowDataset(windows, nf, window, nv, na, "audio_visual", vf, {v: ft for v in vids}, af, {v: ft for v in vids}, dev)
    return ds, 2 * n_visual


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--actions", type=int, default=6, help="annotations per video and modality")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    cfg = named_config("tiny")
    nv, na = 4, 2
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    model = model.to(dev).eval()
    ds, num_actions = synthetic_eval_dataset(cfg, args.videos, args.actions, nv, na, dev)
    col = RecognitionCollector(cfg.num_class, num_actions, modality="audio_visual", include_verb_noun=True)
    with torch.no_grad():
        for i in range(0, len(ds), args.batch):
            visual, audio, times, label, metadata = ds.batch(torch.arange(i, min(i + args.batch, len(ds))))
            output = model([visual, audio], "encoder", model(times, "time_mlp"), nv, na)
            # unfiltered head outputs, -1-padded ids and labels: validity is decided on the device
            col.update(output[0], metadata["v_action_ids"], metadata["a_action_ids"], label, label)
    acc = col.accuracies()
    seen = col.seen.cpu().numpy()
    print("%d windows of %d videos, %d of %d actions seen, up to %d times each (untrained weights: chance-level accuracies)"
          % (len(ds), args.videos, int((seen > 0).sum()), num_actions, int(seen.max())))
    for h in ("verb", "noun", "action", "mt_action", "audio"):
        print("  %-9s top-1 %6.2f %%   top-5 %6.2f %%" % (h, acc[h][0], acc[h][1]))
    probs, ids = col.predictions()["action"]
    print("  action probabilities: %s for action ids %d .. %d" % (tuple(probs.shape), int(ids.min()), int(ids.max())))
    return {"accuracies": acc, "seen": seen, "num_actions": num_actions}


if __name__ == "__main__":
    main()
