"""Detection inference end to end on the MI355X path, on synthetic data: windows of a few videos through
`tim_amd.detection.TIM` in eval() (the evaluation route) and `tim_amd.DetectionCollector`, which keeps everything between
the heads' outputs and the per-video detections on the device - what detection/scripts/extract_feats.py (FeatureMeter) and
eval_detection/format_predictions.py do on the host in the reference.

    python examples/detect_synthetic.py [--videos 3] [--windows 5] [--batch 4] [--head action]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import DetectionCollector, synth  # noqa: E402
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
    ap.add_argument("--top", type=int, default=3, help="detections printed per video")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    cfg = named_config("tiny")
    cfg.variant = "detection"
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    # synthetic weights leave the sign of (end - start) to chance; a trained regression head emits forward segments, so bias
    # the last layer of each regression branch towards start < end
    with torch.no_grad():
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
        col.update(output[0], output[1], query_times, metadata)          # FeatureMeter.update's arguments
    n_cand = int(col.candidates()[1].numel())
    results = col.results(sigma=args.sigma)
    print("%d windows of %d videos, head %s: %d candidates over %.2f -> %d detections"
          % (len(windows), args.videos, args.head, n_cand, args.score_threshold, sum(len(v) for v in results.values())))
    for vid, dets in results.items():
        print("  %s: %d detections" % (vid, len(dets)))
        for d in dets[:args.top]:
            print("      class %4d  score %.4f  %9.3f - %9.3f s" % (d["action"], d["score"], d["segment"][0], d["segment"][1]))
    return results


if __name__ == "__main__":
    main()
