"""Which feature tokens, at which times, does an interval query read?  `model.attention_maps` on synthetic features: the
EPIC audio-visual model (C2a: 50 visual + 50 audio feature tokens, 15 visual and 10 audio queries per window) runs one
evaluation forward that also returns the encoder's attention weights - what the reference's `TransformerEncoder.forward`
returns as `attn_weights` and `TIM.forward_encoder` drops - and prints, for a few action queries, the query's interval, the
five feature tokens it weighs most with their times, and how its weight splits between the visual tokens, the audio tokens
and the query itself.

    python examples/attention_maps_synthetic.py [--windows 4] [--queries 3] [--layer -1] [--precision fp16]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--queries", type=int, default=3, help="action queries of window 0 to print")
    ap.add_argument("--layer", type=int, default=-1)
    ap.add_argument("--precision", default="fp16")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    cfg = named_config("C2a")
    nv, na, nf = 15, 10, cfg.num_feats
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    model = model.to(dev).eval()
    inp = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_inputs(cfg, args.windows, nv, na, seed=0).items()}
    times = inp["times"]                                       # [B, 2 nf + nv + na, 2]: visual, audio feature times, then the queries
    with torch.no_grad():
        te = model(times, "time_mlp")
    (cls, feats), maps = model.attention_maps([inp["visual"], inp["audio"]], te, nv, na, layers=[args.layer], rows="queries")
    layer = maps.layers[0]
    w = maps.for_head("action", layer)                         # [B, nv, F + 1]
    vis, aud = w[..., :nf], w[..., nf:maps.F]                  # the modality halves of the feature columns
    torch.cuda.synchronize()
    print("layer %d of %d, %d windows: maps %s for %d query tokens and %d feature tokens (+ the query itself)"
          % (layer, cfg.num_layers, args.windows, tuple(maps.weights[layer].shape), maps.S - maps.F, maps.F))
    rows = []
    for j in range(min(args.queries, nv)):
        q = times[0, 2 * nf + j].tolist()
        top = torch.topk(w[0, j, :maps.F], 5)
        share = (float(vis[0, j].sum()), float(aud[0, j].sum()), float(w[0, j, maps.F]))
        print("  action query %d, interval [%.3f, %.3f]: visual %.3f  audio %.3f  self %.3f" % ((j, q[0], q[1]) + share))
        for p, tok in zip(top.values.tolist(), top.indices.tolist()):
            t = times[0, tok].tolist()
            print("      %-6s token %2d  [%.3f, %.3f]  weight %.4f" % ("visual" if tok < nf else "audio", tok % nf, t[0], t[1], p))
        rows.append({"interval": q, "top": top.indices.tolist(), "share": share})
    return {"maps": maps, "outputs": (cls, feats), "queries": rows}


if __name__ == "__main__":
    main()
