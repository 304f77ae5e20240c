"""Which feature tokens, at which times, does each interval read - asked of a window cache.  W windows of synthetic EPIC
audio-visual features (C2a: 50 visual + 50 audio feature tokens) are encoded once with `encode_windows`; then several interval
sets are asked of the cache with `query_attention_maps`, each a handful of hand-made intervals per group with its own
window_index (more groups than windows, windows repeated).  Every call returns `query_windows`' scores and the last layer's
attention map of the query rows alone; for each printed interval the time span covered by its most attended feature tokens is
shown next to the interval itself.  Neither the feature embedding nor the windows' encoder pass runs again.

    python examples/query_maps_synthetic.py [--windows 4] [--sets 3] [--intervals 4] [--top 5] [--precision fp16]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402


def interval_set(k, groups, n, dev):
    """set k: n intervals per group, in window coordinates [0, 1] - evenly spaced centres shifted with k, widths growing with k"""
    centres = (torch.linspace(0.15, 0.85, n, device=dev) + 0.03 * k).clamp(max=0.95)
    half = 0.03 + 0.03 * k
    seg = torch.stack([(centres - half).clamp(min=0.0), (centres + half).clamp(max=1.0)], -1)
    return seg.unsqueeze(0).expand(groups, -1, -1).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--sets", type=int, default=3, help="interval sets asked of the one cache")
    ap.add_argument("--intervals", type=int, default=4, help="visual intervals per group")
    ap.add_argument("--top", type=int, default=5, help="most attended feature tokens whose time span is printed")
    ap.add_argument("--precision", default="fp16")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    cfg = named_config("C2a")
    nf, W = cfg.num_feats, args.windows
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    model = model.to(dev).eval()
    inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, W, 0, 0, seed=0).items()}
    feat_times = inp["times"][:, :cfg.F]                        # [W, 2 nf, 2]: the visual, then the audio feature tokens' times
    with torch.no_grad():
        cache = model.encode_windows([inp["visual"], inp["audio"]], model(feat_times, "time_mlp"))      # the windows, once
    print("%d windows encoded once: %d bytes of keys and values" % (W, cache.nbytes))
    nv, na = args.intervals, 0
    rows = []
    for k in range(args.sets):
        # set k asks W + k groups: every window once, then the first k windows again
        widx = list(range(W)) + [g % W for g in range(k)]
        seg = interval_set(k, len(widx), nv, dev)
        with torch.no_grad():
            te_q = model(seg, "time_mlp")
        scores, maps = model.query_attention_maps(cache, te_q, nv, na, window_index=widx)      # layers="last"
        w = maps.for_head("action")                             # [G, nv, F + 1]: column j < F = feature token j of window widx[g]
        torch.cuda.synchronize()
        print("set %d: %d groups x %d intervals against %d cached windows, map %s of layer %d"
              % (k, len(widx), nv, W, tuple(maps.weights[maps.layers[-1]].shape), maps.layers[-1]))
        g = len(widx) - 1                                       # print the last group of the set
        for j in range(nv):
            top = torch.topk(w[g, j, :maps.F], min(args.top, maps.F))
            t = feat_times[widx[g], top.indices]                # the times of those tokens, of the group's own window
            span = (float(t[:, 0].min()), float(t[:, 1].max()))
            share = (float(w[g, j, :nf].sum()), float(w[g, j, nf:maps.F].sum()), float(w[g, j, maps.F]))
            q = seg[g, j].tolist()
            print("  group %d (window %d) interval [%.3f, %.3f]: top-%d tokens span [%.3f, %.3f] with weight %.3f; "
                  "visual %.3f  audio %.3f  self %.3f" % ((g, widx[g], q[0], q[1], top.indices.numel()) + span + (float(top.values.sum()),) + share))
            rows.append({"set": k, "group": g, "window": widx[g], "interval": q, "span": span, "top": top.indices.tolist(), "share": share})
        last = {"scores": scores, "maps": maps, "window_index": widx}
    return {"cache": cache, "intervals": rows, "last": last}


if __name__ == "__main__":
    main()
