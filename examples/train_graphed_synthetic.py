"""The training loop of examples/train_synthetic.py as ONE captured HIP graph per iteration, mixup included.

A captured step freezes everything the host draws: with `lam = np.random.beta(...)` and `torch.randperm(...)` in the loop, every
replay would train on the lam and the permutation of the capture.  Here the mixup state lives on the device
(`tim_amd.mixup.Mixup`) and the captured step redraws it:

    mix.draw()                                   one launch: lam ~ Beta(0.2, 0.2), a permutation, its inverse
    mix.mix([visual, audio, time encodings])     one launch for the three tensors (and one in the backward, for the encodings)
    mix.targets(labels)                          device gathers
    encoder, four cross entropies reading lam from device memory, DRLoc, backward, FusedAdamW (clip + AdamW + skip)

    python examples/train_graphed_synthetic.py [--steps 20] [--batch 8] [--precision fp16]

prints lam per replay: it changes every step, and a second run with the same --seed prints the same sequence.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from train_synthetic import synthetic_dataset  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd import losses, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tim_amd.mixup import Mixup  # noqa: E402
from tim_amd.optim import FusedAdamW  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0, help="mixup seed (data parallel: the rank, so that the ranks draw different sets)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = named_config("tiny")
    nv, na, nf, m = 4, 2, cfg.num_feats, 8
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=nf, feat_drop=0.1, seq_drop=0.1, enc_dropout=0.1,
                precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    model = model.to(dev).train()
    opt = FusedAdamW.for_model(model, lr=args.lr, weight_decay=1e-4, max_grad_norm=1.0)
    ds = synthetic_dataset(cfg, 4, 64, nv, na, dev, seed=0)
    g = torch.Generator().manual_seed(0)
    mix = Mixup(args.batch, alpha=0.2, device=dev, seed=args.seed)

    # static inputs of the captured step: every iteration copies its batch into them
    visual, audio, times, label, _ = ds.batch(torch.randint(0, len(ds), (args.batch,), generator=g))
    static = {"visual": visual.clone(), "audio": audio.clone(), "times": times.clone()}
    labels = {k: v.clone() for k, v in label.items()}
    pos = (torch.zeros((args.batch, m), dtype=torch.int64, device=dev), torch.zeros((args.batch, m), dtype=torch.int64, device=dev))

    def step():
        for p in model.parameters():
            p.grad = None
        mix.draw()
        te = model(static["times"], "time_mlp")
        vis, aud, te = mix.mix([static["visual"], static["audio"], te])
        y_a, y_b = mix.targets(labels)
        (verb, noun, action, aud_logits), feats = model([vis, aud], "encoder", te, nv, na)
        ce = lambda x, k: losses.mixup_cross_entropy(x, y_a[k].reshape(-1), y_b[k].reshape(-1), mix.lam, 0.2)   # noqa: E731
        loss = (ce(verb, "verb") + ce(noun, "noun") + ce(action, "action")) / 3.0 + ce(aud_logits, "class_id")
        loss = loss + 0.3 * losses.dense_relative_localization_loss_crossmodal(feats[:, :nf], feats[:, nf:], model, m, positions=pos)
        loss.backward()
        opt.step()
        return loss.detach()

    graphed = GraphedStep(model, step, optimizer=opt)     # (its warm-up steps are real steps: they draw and update too)
    hist = []
    for it in range(args.steps):
        visual, audio, times, label, _ = ds.batch(torch.randint(0, len(ds), (args.batch,), generator=g))
        for k, v in (("visual", visual), ("audio", audio), ("times", times)):
            static[k].copy_(v)
        for k in labels:
            labels[k].copy_(label[k])
        for p in pos:                                          # the DRLoc sample positions are host draws: through static tensors
            p.copy_(torch.randint(nf, (args.batch, m), generator=g))
        loss = graphed()
        hist.append((loss.item(), mix.lam.item(), mix.index.tolist()))
        print("replay %3d  lam %.6f  index %s  loss %.4f" % (it, hist[-1][1], hist[-1][2], hist[-1][0]), flush=True)
    graphed.reset()
    F.graph_safe_dropout(dev, enable=False)   # the salt word GraphedStep registered is process-wide: hand eager code its plain seeds back
    return hist


if __name__ == "__main__":
    main()
