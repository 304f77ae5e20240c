"""Two-stream detection end to end on the MI355X path, on synthetic data: the same windows of a few videos through a verb
model and a noun model (`tim_amd.detection.TIM` in eval(), one "action" head each), `tim_amd.TwoStreamCollector` (the two
models' outputs to per-video (verb, noun) detections) and `tim_amd.DetectionScorer` (detections to mAP at tIoU 0.1 ... 0.5,
for the action, verb and noun tasks) - what eval_detection/format_two_stream_predictions_epic.py and
evaluate_detection_json_ek100.py do on the host in the reference, through two saved score matrices and a JSON file.  The
synthetic ground truth is a jittered subset of the models' own detections plus segments nothing detects, so the numbers are
neither 0 nor 1.

    python examples/twostream_synthetic.py [--videos 3] [--windows 5] [--batch 4] [--top-k 2]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import DetectionScorer, TwoStreamCollector, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.detection import TIM  # noqa: E402


def make_model(num_classes, seed, precision, dev):
    cfg = named_config("tiny")
    cfg.variant = "detection"
    cfg.include_verb_noun = False
    cfg.num_class = (num_classes, cfg.num_class[1])         # a tuple: the detection model reads a list as [verb, noun, action]
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, include_verb_noun=False,
                precision=precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=seed).items()})
    with torch.no_grad():                                    # forward segments, as in examples/detect_synthetic.py
        for name, p in model.named_parameters():
            if name.startswith("reg_head.") and name.endswith(".4.bias"):
                p.copy_(torch.tensor([-1.0, 1.0]))
    return cfg, model.to(dev).eval()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5, help="windows per video")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--verbs", type=int, default=7)
    ap.add_argument("--nouns", type=int, default=11)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--score-threshold", type=float, default=0.03)
    ap.add_argument("--verb-alpha", type=float, default=0.65)
    ap.add_argument("--sigma", type=float, default=0.25)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    cfg, verb_model = make_model(args.verbs, 0, args.precision, dev)
    _, noun_model = make_model(args.nouns, 1, args.precision, dev)
    window_size, stride = 30.0, 7.5
    windows = [("video_%02d" % v, stride * w + 0.1234 * v) for v in range(args.videos) for w in range(args.windows)]
    col = TwoStreamCollector(num_verbs=args.verbs, num_nouns=args.nouns, score_threshold=args.score_threshold,
                             verb_alpha=args.verb_alpha, top_k=args.top_k)
    for i in range(0, len(windows), args.batch):
        chunk = windows[i:i + args.batch]
        inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, len(chunk), 0, 0, seed=100 + i).items()}
        metadata = {"video_id": [c[0] for c in chunk], "window_start": torch.tensor([c[1] for c in chunk], dtype=torch.float64),
                    "window_size": torch.tensor([window_size] * len(chunk), dtype=torch.float64)}
        with torch.no_grad():
            v_out, _, _, query_times, _ = verb_model([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)
            n_out, _, _, _, _ = noun_model([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)
        col.update(v_out, n_out, query_times, metadata)

    # ---- synthetic ground truth: every third detection of a video, jittered, and as many segments that overlap nothing
    segs, scores, labels, video = (t.cpu().numpy() for t in col.detections(sigma=args.sigma))
    rng = np.random.default_rng(0)
    pick = np.arange(0, segs.shape[0], 3)
    gt_seg = segs[pick].astype(np.float64) + rng.normal(0.0, 0.3, size=(pick.shape[0], 2))
    gt_seg[:, 1] = np.maximum(gt_seg[:, 1], gt_seg[:, 0] + 0.05)
    far = gt_seg + 10000.0
    gt_video = [col.video_ids[int(v)] for v in video[pick]] * 2
    gt_action = np.concatenate([labels[pick], labels[pick]])
    print("%d windows of %d videos, top_k %d: %d (verb, noun) detections against %d ground-truth segments"
          % (len(windows), args.videos, args.top_k, segs.shape[0], 2 * pick.shape[0]))
    out = {}
    for task, gt_labels in (("action", gt_action), ("verb", gt_action // args.nouns), ("noun", gt_action % args.nouns)):
        scorer = DetectionScorer(gt_video, np.concatenate([gt_seg, far]), gt_labels)
        mAP, avg = scorer.score(col, sigma=args.sigma, task=task)
        print("  %-6s mAP @ tIoU %s: %s   average %.4f" % (task, " ".join("%.1f" % t for t in scorer.tiou_thresholds),
                                                          " ".join("%.4f" % m for m in mAP), avg))
        out[task] = (mAP, avg)
    return out, col.results(sigma=args.sigma)


if __name__ == "__main__":
    main()
