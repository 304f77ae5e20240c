"""An AVE-shaped TIM training loop on the MI355X path, on synthetic data: the recipe the reference runs with
`--apply_feature_pooling True` (recognition/time_interval_machine/models/tim.py:137-144,155-156) - every window brings ten 7 x 7
maps of 512-d VGG cells and ten 128-d audio vectors, the audio-guided visual attention pooling (AVGA, helpers/pool.py) collapses
each map to one 512-d visual token in front of the encoder, and 28 event classes are predicted per modality.

    TIM(pool_features=True)            the pooling runs as one fused kernel with a recomputing parameter backward
                                       (tim_amd/avga.py; TIM_AMD_AVGA=0 runs the stock torch ops instead)
    model.pool.attention_map(a, v)     the [B, T, 49] attention map, for a look at what the audio points to
    losses.CrossEntropyLoss            the per-head criterion (train.py:48)
    torch.optim.AdamW                  (train.py:66-70); the pool.* parameters get their .grad from autograd like any other

    python examples/train_ave_synthetic.py [--steps 20] [--batch 16] [--precision fp16] [--tiny]

Synthetic task: the event class of a window brightens one class-specific cell of every map and shifts the audio by a
class-specific vector, so both heads can learn it and the attention has something to find.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import losses  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402


def synthetic_windows(n, T, cv, ca, classes, nq, dev, seed=0):
    """n windows: video [n, T, 7, 7, cv] (non-negative, like post-ReLU VGG maps), audio [n, T, ca], times [n, 2 T + 2 nq, 2]
    (T visual + T audio feature intervals, nq visual + nq audio query intervals, window-relative), labels [n]"""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, classes, (n,), generator=g)
    video = torch.randn(n, T, 7, 7, cv, generator=g).abs()
    cell = label % 49
    video[torch.arange(n), :, cell // 7, cell % 7] += 2.0
    proto = torch.randn(classes, ca, generator=g)
    audio = torch.randn(n, T, ca, generator=g) * 0.5 + proto[label][:, None]
    st = torch.arange(T, dtype=torch.float32) / T
    feat_t = torch.stack([st, st + 1.0 / T], 1)
    qs = torch.arange(nq, dtype=torch.float32) / nq
    query_t = torch.stack([qs, qs + 1.0 / nq], 1)
    times = torch.cat([feat_t, feat_t, query_t, query_t], 0)[None].repeat(n, 1, 1)
    return video.to(dev), audio.to(dev), times.to(dev), label.to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--tiny", action="store_true", help="64-d cells, d_model 32, 6 + 6 feature tokens, 5 classes: the test's shape")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if args.tiny:
        cv, ca, d, heads, layers, T, classes, nq = 64, 40, 32, 2, 2, 6, 5, 2
    else:
        cv, ca, d, heads, layers, T, classes, nq = 512, 128, 256, 8, 4, 10, 28, 10
    model = TIM([classes, classes], visual_input_dim=cv, audio_input_dim=ca, d_model=d, nhead=heads, num_layers=layers,
                num_feats=T, include_verb_noun=False, pool_features=True, feat_drop=0.0, seq_drop=0.0, enc_dropout=0.0,
                precision=args.precision).to(dev).train()
    opt = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=1e-4)
    video, audio, times, label = synthetic_windows(args.windows, T, cv, ca, classes, nq, dev)
    crit = losses.CrossEntropyLoss()
    g = torch.Generator().manual_seed(1)
    hist = []
    for step in range(args.steps):
        idx = (torch.arange(args.batch) if args.batch >= args.windows else torch.randint(0, args.windows, (args.batch,), generator=g)).to(dev)
        idx = idx % args.windows
        te = model(times[idx], "time_mlp")
        (_, _, action, aud), _ = model([video[idx], audio[idx]], "encoder", te, nq, nq)
        target = label[idx][:, None].expand(-1, nq).reshape(-1)          # every query of a window carries the window's event
        loss = crit(action, target) + crit(aud, target)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        gnorm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        if torch.isfinite(gnorm) and model.rt.grads_finite():
            opt.step()
        hist.append(loss.item())
        if step % 5 == 0 or step == args.steps - 1:
            print("step %3d  loss %.4f" % (step, hist[-1]), flush=True)
    with torch.no_grad():
        amap = model.pool.attention_map(audio[:2], video[:2])
    print("attention map %s: the brightened cell of window 0 gets %.3f (uniform would be %.3f)"
          % (tuple(amap.shape), amap[0, :, int(label[0]) % 49].mean().item(), 1.0 / 49))
    return hist


if __name__ == "__main__":
    main()
