"""The captured training iteration of examples/train_graphed_synthetic.py with the data side on the device as well: nothing
reaches a replay from the host but the replay call.

train_graphed_synthetic.py assembles every batch eagerly (`ds.batch(host indices)`), copies it into the static inputs of the
captured step and draws the DRLoc sample positions with the host RNG - a second pass over the inputs and a dozen launches in
front of every replay.  Here both live inside the captured step:

    smp.next_batch()         two launches: iteration t of a seeded, epoch-shuffled, rank-sharded order (a device counter), and
                             its batch assembled into tensors of fixed address
    drloc_pos.draw()         one launch: the DRLoc sample positions and their normalised distance
    mix.draw(), mix.mix(...), encoder, cross entropies, DRLoc, backward, FusedAdamW      as before

    python examples/train_graphed_device_data_synthetic.py [--steps 20] [--batch 8] [--precision fp16] [--store-dtype fp32]

--store-dtype fp16 | bf16 holds the feature stores in that type (half the bytes; batches stay fp32, every element the exact
widening of the stored one).  With the type the model's --precision rounds its inputs to, the forward sees the same operands.

prints window numbers, lam and loss per replay: they change every step, and a second run with the same --seed prints the same
windows and lam.
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
from tim_amd.losses import DrlocPositions  # noqa: E402
from tim_amd.mixup import Mixup  # noqa: E402
from tim_amd.optim import FusedAdamW  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402

STORE_DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0, help="seed of the batch order, mixup and DRLoc draws")
    ap.add_argument("--rank", type=int, default=0, help="data parallel: this rank's shard of every epoch's order")
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--store-dtype", choices=sorted(STORE_DTYPES), default="fp32", help="element type of the feature stores in device memory")
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
    ds = synthetic_dataset(cfg, 4, 64, nv, na, dev, seed=0, store_dtype=STORE_DTYPES[args.store_dtype])
    # every rank walks the SAME shuffled order (one seed) and takes its own share; mixup and DRLoc draw per rank
    smp = ds.sampler(args.batch, seed=args.seed, shuffle=True, rank=args.rank, world=args.world)
    mix = Mixup(args.batch, alpha=0.2, device=dev, seed=args.seed + args.rank)
    drloc_pos = DrlocPositions(args.batch, m, nf, dev, seed=args.seed + args.rank)

    def step():
        for p in model.parameters():
            p.grad = None
        visual, audio, times, labels, _ = smp.next_batch()      # (rows beyond the rank's share of a short last batch carry -1 labels)
        drloc_pos.draw()
        mix.draw()
        te = model(times, "time_mlp")
        vis, aud, te = mix.mix([visual, audio, te])
        y_a, y_b = mix.targets(labels)
        (verb, noun, action, aud_logits), feats = model([vis, aud], "encoder", te, nv, na)
        ce = lambda x, k: losses.mixup_cross_entropy(x, y_a[k].reshape(-1), y_b[k].reshape(-1), mix.lam, 0.2)   # noqa: E731
        loss = (ce(verb, "verb") + ce(noun, "noun") + ce(action, "action")) / 3.0 + ce(aud_logits, "class_id")
        loss = loss + 0.3 * losses.dense_relative_localization_loss_crossmodal(feats[:, :nf], feats[:, nf:], model, m, positions=drloc_pos)
        loss.backward()
        opt.step()
        return loss.detach()

    graphed = GraphedStep(model, step, optimizer=opt)     # (its warm-up steps are real steps: they draw and update too)
    hist = []
    for it in range(args.steps):
        loss = graphed()                                   # the whole iteration: no copy into static inputs, no host RNG
        hist.append((loss.item(), mix.lam.item(), smp.window.tolist(), int(smp.epoch.item()), drloc_pos.pos_1[0].tolist()))
        print("replay %3d  epoch %d  windows %s  lam %.6f  loss %.4f" % (it, hist[-1][3], hist[-1][2], hist[-1][1], hist[-1][0]), flush=True)
    graphed.reset()
    F.graph_safe_dropout(dev, enable=False)   # the salt word GraphedStep registered is process-wide: hand eager code its plain seeds back
    return hist


if __name__ == "__main__":
    main()
