"""The captured detection iteration of train_detection_graphed_synthetic.py with its meter inside the graph: the loop reads no
scalar back per replay.

The reference's detection loop ends every iteration with thirteen device-to-host reads for its TrainMeter, and computes the
action head's focal loss a second time to split it into a positive and a negative part (detection/scripts/train.py:262-273,
:413-430).  Here the side losses leave those statistics behind from the pass they make anyway
(`detection_side_loss(..., stats=meter.side_stats(side))`) and `tim_amd.DetectionMeter.update()` folds them into a state block
in device memory with one launch, both inside the captured step.  Every --print-freq replays the block is read with one copy:

    python examples/train_detection_metered_synthetic.py [--steps 20] [--batch 4] [--print-freq 5] [--precision fp16]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import DetectionMeter  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd import losses, synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.detection import TIM  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tim_amd.optim import FusedAdamW  # noqa: E402
from train_detection_graphed_synthetic import synthetic_detection_dataset  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--print-freq", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--seed", type=int, default=0, help="seed of the batch order")
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(args.seed)
    cfg = named_config("tiny")
    cfg.variant = "detection"
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, feat_drop=0.1, seq_drop=0.1, enc_dropout=0.1,
                precision=args.precision)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    model = model.to(dev).train()
    opt = FusedAdamW.for_model(model, lr=args.lr, weight_decay=1e-4, max_grad_norm=1.0)
    ds = synthetic_detection_dataset(cfg, 4, 48, 3, 2, dev, seed=0)
    smp = ds.sampler(args.batch, seed=args.seed, shuffle=True, last="drop")
    normaliser = [torch.full((), 100.0, dtype=torch.float32, device=dev) for _ in range(2)]
    meter = DetectionMeter("audio_visual", include_verb_noun=True, include_dr_loc=False, device=dev)

    def step():
        for p in model.parameters():
            p.grad = None
        visual, audio, times, target, _ = smp.next_batch()
        output, offsets, labels, _, ious = model([visual, audio], "encoder", times, target, label_queries=True)
        loss = None
        for m, (name, cls_ids, lab) in enumerate((("visual", (0, 1, 2), labels[0]), ("audio", (3,), [labels[1]]))):
            side = losses.detection_side_loss([output[0][c] for c in cls_ids], lab, output[1][m], offsets[m], ious[m], normaliser[m],
                                              model.iou_threshold, lambda_reg=1.0, momentum=0.9, stats=meter.side_stats(name))
            loss = side if loss is None else loss + side
        meter.update(loss)                                 # one launch: the block advances with the replay
        loss.backward()
        opt.step()
        return loss.detach()

    graphed = GraphedStep(model, step, optimizer=opt)     # (its warm-up steps are real steps: the meter counts them too)
    meter.reset()
    hist = []
    for it in range(args.steps):
        graphed()
        if (it + 1) % args.print_freq == 0 or it + 1 == args.steps:
            s = meter.stats(lr=args.lr, training_iterations=it + 1)          # ONE copy of the block
            hist.append(s)
            print("replay %3d  windows %s  " % (it, smp.window.tolist()) + "  ".join(
                "%s %.4f" % (k.replace("Train/", ""), s[k]) for k in ("Train/loss", "Train/visual_loss", "Train/visual_action_loss",
                                                                        "Train/visual_positive_loss", "Train/visual_negative_loss",
                                                                        "Train/visual_reg_loss", "Train/audio_loss", "Train/audio_reg_loss",
                                                                        "Train/normaliser", "Train/positive_ratio")), flush=True)
    graphed.reset()
    F.graph_safe_dropout(dev, enable=False)   # the salt word GraphedStep registered is process-wide: hand eager code its plain seeds back
    return hist, meter.read()


if __name__ == "__main__":
    main()
