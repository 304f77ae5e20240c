"""The captured training iteration of examples/train_graphed_device_data_synthetic.py with the reference's learning-rate schedule
attached: cosine annealing under a linear warm-up, counted by the optimizer's steps.

The reference's iteration ends with `with warmup_scheduler.dampening(): lr_scheduler.step()`.  `tim_amd.CosineWarmupSchedule`
is both schedulers as one closed form, attached to the optimizer: `GraphedStep` writes the rate of the coming replay into the
optimizer's state block before every replay (one word, only when it changed), so the loop has no scheduler line:

    opt = FusedAdamW.for_model(model, lr=..., max_grad_norm=1.0)
    sched = CosineWarmupSchedule(opt, T_max=steps, eta_min=1e-6, warmup_period=warmup)
    ... opt.step() inside the captured step; no sched.step() anywhere ...

    python examples/train_graphed_scheduled_synthetic.py [--steps 20] [--warmup-steps 5] [--batch 8] [--precision fp16]

GraphedStep's warm-up runs are real steps: they train, and they advance the schedule.  This example accepts their updates as a
head start and calls `sched.set_step(0)` after the capture, so replay 0 trains at iteration 0 of the curve.  Leaving the call out
keeps the offset: replay 0 then trains at iteration 3.

prints the rate the replay read from device memory next to the definition evaluated on the host, lam and loss per replay.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from train_synthetic import synthetic_dataset  # noqa: E402
from tim_amd import CosineWarmupSchedule  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd import losses, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tim_amd.losses import DrlocPositions  # noqa: E402
from tim_amd.mixup import Mixup  # noqa: E402
from tim_amd.optim import FusedAdamW  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="replays; also the schedule's T_max")
    ap.add_argument("--warmup-steps", type=int, default=5, help="the schedule's warmup_period (0: none)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--eta-min", type=float, default=1e-6)
    ap.add_argument("--seed", type=int, default=0, help="seed of the batch order, mixup and DRLoc draws")
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
    sched = CosineWarmupSchedule(opt, T_max=args.steps, eta_min=args.eta_min, warmup_period=args.warmup_steps)
    ds = synthetic_dataset(cfg, 4, 64, nv, na, dev, seed=0)
    smp = ds.sampler(args.batch, seed=args.seed, shuffle=True)
    mix = Mixup(args.batch, alpha=0.2, device=dev, seed=args.seed)
    drloc_pos = DrlocPositions(args.batch, m, nf, dev, seed=args.seed)

    def step():
        for p in model.parameters():
            p.grad = None
        visual, audio, times, labels, _ = smp.next_batch()
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
        opt.step()                                         # norm, finish, update: the rate is a word of the state block
        return loss.detach()

    graphed = GraphedStep(model, step, optimizer=opt)     # (its warm-up steps are real steps: they advanced the schedule to 3)
    sched.set_step(0)                                      # the curve starts at the first replay
    hist = []
    for it in range(args.steps):
        loss = graphed()                                   # the schedule's rate of this replay was written just before it
        rate = opt.device_lr[0].item()                     # one small device read (this loop's synchronisation)
        hist.append((loss.item(), rate, sched.lr_at(it), mix.lam.item()))
        print("replay %3d  lr %.9g  (definition %.9g)  lam %.6f  loss %.4f" % (it, rate, hist[-1][2], hist[-1][3], hist[-1][0]), flush=True)
    graphed.reset()
    F.graph_safe_dropout(dev, enable=False)   # the salt word GraphedStep registered is process-wide: hand eager code its plain seeds back
    return hist


if __name__ == "__main__":
    main()
