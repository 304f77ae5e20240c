"""The captured device-data iteration of examples/train_graphed_device_data_synthetic.py with the numbers a person watches kept
on the device as well: `tim_amd.TrainMeter.update` runs inside the captured step, and the loop reads the meter every
--print-freq replays with one small copy.  There is no `.item()` in the loop: the loss averages, the valid counts and the
top-1 / top-5 accuracies of the last batch and of the run so far come out of `meter.read()`.

    python examples/train_metered_synthetic.py [--steps 20] [--print-freq 5] [--batch 8] [--precision fp16]

The reference's loop copies all four heads' logits to the host every iteration, runs a CPU `index_add_` and calls `.item()` on
seven losses (recognition/scripts/train.py:391-410); here an iteration adds two small launches (and three per modality for
the per-action ensemble `update_epoch()` scores at the end).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from train_synthetic import synthetic_dataset  # noqa: E402
from tim_amd import TrainMeter  # noqa: E402
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--print-freq", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=1e-3)
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
    ds = synthetic_dataset(cfg, 4, 64, nv, na, dev, seed=0)
    smp = ds.sampler(args.batch, seed=args.seed, shuffle=True)
    mix = Mixup(args.batch, alpha=0.2, device=dev, seed=args.seed)
    drloc_pos = DrlocPositions(args.batch, m, nf, dev, seed=args.seed)
    meter = TrainMeter(cfg.num_class, max(nv, na), modality="audio_visual", include_verb_noun=True, device=dev)   # (the synthetic ids: 0 .. queries - 1)
    last = {}      # what the last step handed to the meter, for a reader that wants to check it (tests): device tensors only

    def step():
        for p in model.parameters():
            p.grad = None
        visual, audio, times, labels, meta = smp.next_batch()
        drloc_pos.draw()
        mix.draw()
        te = model(times, "time_mlp")
        vis, aud, te = mix.mix([visual, audio, te])
        y_a, y_b = mix.targets(labels)
        (verb, noun, action, aud_logits), feats = model([vis, aud], "encoder", te, nv, na)
        ce = lambda x, k: losses.mixup_cross_entropy(x, y_a[k].reshape(-1), y_b[k].reshape(-1), mix.lam, 0.2)   # noqa: E731
        l_verb, l_noun, l_action, l_audio = ce(verb, "verb"), ce(noun, "noun"), ce(action, "action"), ce(aud_logits, "class_id")
        l_visual = (l_verb + l_noun + l_action) / 3.0
        l_drloc = losses.dense_relative_localization_loss_crossmodal(feats[:, :nf], feats[:, nf:], model, m, positions=drloc_pos)
        loss = l_visual + l_audio + 0.3 * l_drloc
        loss.backward()
        opt.step()
        # the meter: the unfiltered logits, the -1-padded ids and target_a, the losses as device scalars - launches only
        meter.update((verb, noun, action, aud_logits), meta["v_action_ids"], meta["a_action_ids"],
                     [y_a["verb"], y_a["noun"], y_a["action"]], y_a["class_id"],
                     losses={"total": loss, "visual": l_visual, "verb": l_verb, "noun": l_noun, "action": l_action,
                             "audio": l_audio, "drloc": l_drloc})
        last["loss"], last["v_action"], last["a_class"] = loss.detach(), y_a["action"], y_a["class_id"]
        return loss.detach()

    graphed = GraphedStep(model, step, optimizer=opt)     # (its warm-up steps are real steps: they update the meter too)
    meter.reset()
    hist = []
    for it in range(args.steps):
        graphed()                                          # the whole iteration, meter included: nothing is read back
        hist.append((last["loss"].clone(), (last["v_action"] != -1).sum() + (last["a_class"] != -1).sum()))   # device-side copies
        if (it + 1) % args.print_freq == 0 or it + 1 == args.steps:
            s = meter.read()                               # one copy of the meter's block
            a = s["acc"]
            print("replay %3d  loss %.4f (avg %.4f over %d rows)  visual %.4f  audio %.4f  drloc %.4f  batch top-1: verb %.1f "
                  "noun %.1f action %.1f audio %.1f  running top-5 action %.1f"
                  % (it, s["losses"]["total"]["val"], s["losses"]["total"]["avg"], s["losses"]["total"]["count"],
                     s["losses"]["visual"]["avg"], s["losses"]["audio"]["avg"], s["losses"]["drloc"]["avg"], a["verb"]["batch_top1"],
                     a["noun"]["batch_top1"], a["action"]["batch_top1"], a["audio"]["batch_top1"], a["action"]["top5"]), flush=True)
    final = meter.read()
    epoch = meter.update_epoch()
    print("epoch: " + "  ".join("%s %.1f / %.1f" % (h, v[0], v[1]) for h, v in sorted(epoch.items())), flush=True)
    per_replay = [(float(l.item()), int(n.item())) for l, n in hist]      # read back afterwards, outside the loop
    graphed.reset()
    F.graph_safe_dropout(dev, enable=False)   # the salt word GraphedStep registered is process-wide: hand eager code its plain seeds back
    return {"read": final, "epoch": epoch, "per_replay": per_replay}


if __name__ == "__main__":
    main()
