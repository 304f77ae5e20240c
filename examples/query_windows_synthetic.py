"""Encode a batch of detection windows once, query it twice, on synthetic data: `encode_windows` keeps every layer's keys and
values of the windows' feature tokens; `query_windows` then scores the model's own query pyramid and, from the same cache, a
second set of hand-made intervals (proposals refined around a few centres) - without embedding or encoding the features again.
Both sets of scores go to one `tim_amd.DetectionCollector` as `forward_inference`'s would.

    python examples/query_windows_synthetic.py [--videos 2] [--windows 3] [--proposals 24] [--head action]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import DetectionCollector, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.detection import TIM  # noqa: E402


def proposals(n_windows, n, dev):
    """n hand-made segments per window, in window coordinates [0, 1]: three widths around evenly spaced centres"""
    centres = torch.linspace(0.1, 0.9, n, device=dev)
    half = torch.tensor([0.02, 0.05, 0.11], device=dev)[torch.arange(n, device=dev) % 3]
    seg = torch.stack([(centres - half).clamp(min=0.0), (centres + half).clamp(max=1.0)], -1)
    return seg.unsqueeze(0).expand(n_windows, -1, -1).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=2)
    ap.add_argument("--windows", type=int, default=3, help="windows per video")
    ap.add_argument("--proposals", type=int, default=24, help="hand-made intervals per window in the second query set")
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
    with torch.no_grad():   # (synthetic weights: bias the regression heads towards start < end, as a trained head emits)
        for name, p in model.named_parameters():
            if name.startswith("reg_head.") and name.endswith(".4.bias"):
                p.copy_(torch.tensor([-1.0, 1.0]))
    model = model.to(dev).eval()
    window_size, stride = 30.0, 7.5
    windows = [("video_%02d" % v, stride * w + 0.1234 * v) for v in range(args.videos) for w in range(args.windows)]
    W = len(windows)
    inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, W, 0, 0, seed=100).items()}
    metadata = {"video_id": [c[0] for c in windows], "window_start": torch.tensor([c[1] for c in windows], dtype=torch.float64),
                "window_size": torch.tensor([window_size] * W, dtype=torch.float64)}
    col = DetectionCollector(cfg.num_class, head=args.head, score_threshold=args.score_threshold)

    cache = model.encode_windows([inp["visual"], inp["audio"]], inp["times"])          # the feature tokens, once
    # 1. the model's own pyramid
    cls, reg = model.query_windows(cache)
    pyramid = model.inference_queries.to(dev).expand(W, -1, -1).flatten(0, 1)
    col.update(cls, reg, (pyramid if "visual" in model.data_modality else None, pyramid if "audio" in model.data_modality else None),
               metadata)
    n_first = int(col.candidates()[1].numel())
    # 2. a second set of intervals against the same cache
    seg = proposals(W, args.proposals, dev)
    v = seg if "visual" in model.data_modality else None
    a = seg if "audio" in model.data_modality else None
    cls2, reg2 = model.query_windows(cache, v, a)
    flat = seg.flatten(0, 1)
    col.update(cls2, reg2, (flat if v is not None else None, flat if a is not None else None), metadata)
    n_both = int(col.candidates()[1].numel())
    results = col.results(sigma=args.sigma)
    print("%d windows encoded once (%d bytes of keys and values): %d pyramid queries + %d proposals per window, head %s: "
          "%d + %d candidates over %.2f -> %d detections"
          % (W, cache.nbytes, model.num_queries, args.proposals, args.head, n_first, n_both - n_first, args.score_threshold,
             sum(len(d) for d in results.values())))
    for vid, dets in results.items():
        print("  %s: %d detections" % (vid, len(dets)))
    return {"results": results, "candidates": (n_first, n_both), "cache_bytes": cache.nbytes}


if __name__ == "__main__":
    main()
