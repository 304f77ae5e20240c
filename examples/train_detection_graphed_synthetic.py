"""The detection training iteration captured whole, the data side included: nothing reaches a replay from the host but the
replay call.  The detection counterpart of examples/train_graphed_device_data_synthetic.py.

train_detection_synthetic.py trains on one frozen batch of random tensors.  Here a small synthetic detection dataset lives on
the device (`tim_amd.det_data.DeviceDetectionDataset`: the tables of the reference's detection `SlidingWindowDataset`) and the
captured step is

    smp.next_batch()         two launches: iteration t of a seeded, epoch-shuffled, rank-sharded order (a device counter), and
                             its batch - features, rounded feature times, ground-truth segments and labels - assembled into
                             tensors of fixed address
    model(..., label_queries=True)     the query draw, IoU labelling against the batch's own ground truth, the encoder
    detection_side_loss per side       focal + DIoU with the side's EMA normaliser, a device scalar advanced in place
                                       (ordered=True: sums in a fixed order, so the printed loss of one state is one number)
    backward, FusedAdamW

    python examples/train_detection_graphed_synthetic.py [--steps 20] [--batch 4] [--precision fp16]

prints window numbers and loss per replay: the windows change every step, and a second run with the same --seed prints the same
windows.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import functional as F  # noqa: E402
from tim_amd import losses, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.det_data import DeviceDetectionDataset  # noqa: E402
from tim_amd.detection import TIM  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tim_amd.optim import FusedAdamW  # noqa: E402


def synthetic_detection_dataset(cfg, n_videos, n_windows, max_v, max_a, dev, seed=0):
    """in-memory tables in the format of the reference's detection dataset (see tests/golden/det_batch_inputs.py)"""
    rs = np.random.RandomState(seed)
    nf = cfg.num_feats
    vids = ["vid%02d" % i for i in range(n_videos)]
    n_feat = 4 * nf
    st = (np.arange(n_feat) * 0.2).astype(np.float32)
    ft = np.stack([st, st + 1.0], 1)
    vf = {v: synth.normal(seed, "dv" + v, (n_feat, 2, cfg.visual_input_dim)).astype(np.float32) for v in vids}
    af = {v: synth.normal(seed, "da" + v, (n_feat, 2, cfg.audio_input_dim)).astype(np.float32) for v in vids}
    vc, ac = cfg.num_class[0], cfg.num_class[1]
    windows = []
    for i in range(n_windows):
        first = int(rs.randint(0, n_feat - 2 * nf))
        start = first * 0.2
        seg = lambda m: (start + np.sort(rs.rand(m, 2) * nf * 0.4, axis=1)).astype(np.float32)   # noqa: E731
        kv, ka = int(rs.randint(1, max_v + 1)), int(rs.randint(1, max_a + 1))
        vl = np.stack([rs.randint(0, vc[0], kv), rs.randint(0, vc[1], kv), rs.randint(0, vc[2], kv), np.full(kv, -1)], 1)
        al = np.stack([np.full(ka, -1)] * 3 + [rs.randint(0, ac, ka)], 1)
        windows.append({"video_id": vids[i % n_videos], "start_sec": start, "feat_indices": np.arange(first, first + 2 * nf, 2),
                        "v_gt_segments": seg(kv), "v_labels": vl.astype(np.int64), "a_gt_segments": seg(ka), "a_labels": al.astype(np.int64)})
    return DeviceDetectionDataset(windows, nf, nf * 0.4, max_v, max_a, "audio_visual", vf, {v: ft for v in vids}, af, {v: ft for v in vids},
                                  dataset_name="epic", include_verb_noun=True, verb_only=True, device=dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0, help="seed of the batch order")
    ap.add_argument("--rank", type=int, default=0, help="data parallel: this rank's shard of every epoch's order")
    ap.add_argument("--world", type=int, default=1)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(args.seed)              # the model draws its training queries with torch.randperm (host in the warm-up, device in the replays)
    cfg = named_config("tiny")
    cfg.variant = "detection"
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, feat_drop=0.1, seq_drop=0.1, enc_dropout=0.1,
                precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    model = model.to(dev).train()
    opt = FusedAdamW.for_model(model, lr=args.lr, weight_decay=1e-4, max_grad_norm=1.0)
    ds = synthetic_detection_dataset(cfg, 4, 48, 3, 2, dev, seed=0)
    # last="drop": a short last batch would bring rows without ground truth, whose queries all count as negatives
    smp = ds.sampler(args.batch, seed=args.seed, shuffle=True, rank=args.rank, world=args.world, last="drop")
    # the loop's EMA normalisers (det train.py:230), one device scalar per side, advanced in place by every replay
    normaliser = [torch.full((), 100.0, dtype=torch.float32, device=dev) for _ in range(2)]

    def step():
        for p in model.parameters():
            p.grad = None
        visual, audio, times, target, _ = smp.next_batch()
        output, offsets, labels, _, ious = model([visual, audio], "encoder", times, target, label_queries=True)
        loss = None
        for m, (cls_ids, lab) in enumerate((((0, 1, 2), labels[0]), ((3,), [labels[1]]))):   # visual, audio
            side = losses.detection_side_loss([output[0][c] for c in cls_ids], lab, output[1][m], offsets[m], ious[m], normaliser[m],
                                              model.iou_threshold, lambda_reg=1.0, momentum=0.9, ordered=True)
            loss = side if loss is None else loss + side
        loss.backward()
        opt.step()
        return loss.detach()

    graphed = GraphedStep(model, step, optimizer=opt)     # (its warm-up steps are real steps: they draw and update too)
    hist = []
    for it in range(args.steps):
        loss = graphed()                                   # the whole iteration: no copy into static inputs
        hist.append((loss.item(), smp.window.tolist(), int(smp.epoch.item()), [n.item() for n in normaliser]))
        print("replay %3d  epoch %d  windows %s  loss %.4f" % (it, hist[-1][2], hist[-1][1], hist[-1][0]), flush=True)
    graphed.reset()
    F.graph_safe_dropout(dev, enable=False)   # the salt word GraphedStep registered is process-wide: hand eager code its plain seeds back
    return hist


if __name__ == "__main__":
    main()
