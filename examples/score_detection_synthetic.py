"""Detection scoring end to end on the MI355X path, on synthetic data: windows of a few videos through
`tim_amd.detection.TIM` in eval(), `tim_amd.DetectionCollector` (logits to per-video detections) and
`tim_amd.DetectionScorer` (detections to per-class AP and mAP at tIoU 0.1 ... 0.5) - what eval_detection/
format_predictions.py and eval_detection/evaluate_detection_json.py do on the host in the reference, through a JSON file.
The synthetic ground truth is a jittered subset of the model's own detections plus segments nothing detects, so the
numbers are neither 0 nor 1.

    python examples/score_detection_synthetic.py [--videos 3] [--windows 5] [--batch 4] [--head action]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import DetectionCollector, DetectionScorer, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.detection import TIM  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5, help="windows per video")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--head", default="action", choices=["verb", "noun", "action", "audio"])
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--score-threshold", type=float, default=0.01)
    ap.add_argument("--sigma", type=float, default=0.1)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    cfg = named_config("tiny")
    cfg.variant = "detection"
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    with torch.no_grad():                                    # forward segments, as in examples/detect_synthetic.py
        for name, p in model.named_parameters():
            if name.startswith("reg_head.") and name.endswith(".4.bias"):
                p.copy_(torch.tensor([-1.0, 1.0]))
    model = model.to(dev).eval()
    window_size, stride = 30.0, 7.5
    windows = [("video_%02d" % v, stride * w + 0.1234 * v) for v in range(args.videos) for w in range(args.windows)]
    col = DetectionCollector(cfg.num_class, head=args.head, score_threshold=args.score_threshold)
    for i in range(0, len(windows), args.batch):
        chunk = windows[i:i + args.batch]
        inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, len(chunk), 0, 0, seed=100 + i).items()}
        metadata = {"video_id": [c[0] for c in chunk], "window_start": torch.tensor([c[1] for c in chunk], dtype=torch.float64),
                    "window_size": torch.tensor([window_size] * len(chunk), dtype=torch.float64)}
        with torch.no_grad():
            output, _, _, query_times, _ = model([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)
        col.update(output[0], output[1], query_times, metadata)

    # ---- synthetic ground truth: every third detection of a video, jittered, and as many segments that overlap nothing
    segs, scores, labels, video = (t.cpu().numpy() for t in col.detections(sigma=args.sigma))
    rng = np.random.default_rng(0)
    pick = np.arange(0, segs.shape[0], 3)
    gt_seg = segs[pick].astype(np.float64) + rng.normal(0.0, 0.3, size=(pick.shape[0], 2))
    gt_seg[:, 1] = np.maximum(gt_seg[:, 1], gt_seg[:, 0] + 0.05)
    far = gt_seg + 10000.0
    gt_video = [col.video_ids[int(v)] for v in video[pick]] * 2
    scorer = DetectionScorer(gt_video, np.concatenate([gt_seg, far]), np.concatenate([labels[pick], labels[pick]]))
    mAP, avg = scorer.score(col, sigma=args.sigma)
    print("%d windows of %d videos, head %s: %d detections against %d ground-truth segments of %d classes"
          % (len(windows), args.videos, args.head, segs.shape[0], 2 * pick.shape[0], scorer.classes.shape[0]))
    for thr, m in zip(scorer.tiou_thresholds, mAP):
        print("  mAP @ tIoU %.1f: %.4f" % (thr, m))
    print("  average mAP: %.4f" % avg)
    return mAP, avg


if __name__ == "__main__":
    main()
