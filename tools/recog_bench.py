#!/usr/bin/env python3
"""Timing of the recognition inference tail on one MI355X at the C2a head widths (verb 97, noun 300, action
3,806, audio 44; 15 visual and 10 audio queries per window) over 20,000 action ids:

  hip      RecognitionCollector.update of one batch (visual group + audio group = 2 library calls, 6 launches), eager and as a
           captured graph replayed; accuracies() (finalize without probabilities + counts, then the read of 16 integers) and
           the finalize of all four heads with probabilities, eager and replayed
  torch    the stock-torch device form of the same update: boolean index of the valid rows (one host sync per modality) +
           index_add_ (floating-point atomics: its sums differ from run to run in the last bits) and, for the finalize,
           (sum / seen).softmax(1).topk(5)
  host     the reference's form, restated: boolean index on the device, dense .cpu() copies, CPU index_add_

Method: every timed callable is warmed up, then timed --reps times with device events around --inner back-to-back calls
(host clock around a synchronise for the host form); the median and the spread (min - max) are printed.  The update's
operands (16 MB of logits, the accumulator rows it touches) stay resident in the 256 MiB Infinity Cache between calls, as
they are right behind the heads' GEMMs in an evaluation.  The achievable stream rate is measured in the same run: a torch
copy of 512 MiB (read + write), which no cache holds.  Algorithmic bytes of an update: the logits of the valid rows read
once, the accumulator chunk of every distinct id read once and written once.

    python tools/recog_bench.py [--reps 20] [--inner 10] [--actions 20000]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import RecognitionCollector  # noqa: E402
from tools._timing import captured, host_timed, timed  # noqa: E402

CLASSES = {"verb": 97, "noun": 300, "action": 3806, "audio": 44}
NUM_CLASS = [[97, 300, 3806], 44]
NV, NA = 15, 10
HEADS = ("verb", "noun", "action", "audio")


def make_batch(windows, n_act, seed, dev):
    """a batch of consecutive, half-overlapping windows: an action is queried by about three windows; a fifth of the query
    slots is padding"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, per, first in (("v", NV, 0), ("a", NA, n_act // 2)):
        R = windows * per
        ids = first + rng.integers(0, max(1, R // 3), size=R)
        pad = rng.uniform(size=R) < 0.2
        ids[pad] = -1
        out[name + "_ids"] = torch.from_numpy(ids.astype(np.int64)).to(dev)
        k = 3 if name == "v" else 1
        lab = np.stack([np.where(pad, -1, ids % c) for c in ((97, 300, 3806) if name == "v" else (44,))], axis=1)
        out[name + "_labels"] = torch.from_numpy(lab.astype(np.int64).reshape(R, k)).to(dev)
    g = torch.Generator(device="cpu").manual_seed(seed)
    out["logits"] = tuple((torch.randn(windows * (NV if h != "audio" else NA), CLASSES[h], generator=g) * 3.0).to(dev) for h in HEADS)
    return out


class TorchState:
    """the stock-torch device form / the reference's host form of the meters"""

    def __init__(self, n_act, dev):
        self.acc = {h: torch.zeros((n_act, c), device=dev) for h, c in CLASSES.items()}
        self.seen = torch.zeros(n_act, device=dev)
        self.v_labels = torch.full((n_act, 3), -1, dtype=torch.int32, device=dev)
        self.a_labels = torch.full((n_act,), -1, dtype=torch.int32, device=dev)

    def update(self, b, to=lambda t: t):
        """to = identity: everything stays on the device; to = .cpu(): the reference's copies (state on the host)"""
        vv = b["v_labels"][:, 2] != -1
        if vv.any():                                          # the host sync of test.py's `valid_visual > 0`
            ids = to(b["v_ids"][vv])
            for h, x in zip(HEADS[:3], b["logits"]):
                self.acc[h].index_add_(0, ids, to(x[vv]))
            self.seen.index_add_(0, ids, torch.ones_like(ids).float())
            self.v_labels[ids] = to(b["v_labels"][vv]).int()
        va = b["a_labels"][:, 0] != -1
        if va.any():
            ids = to(b["a_ids"][va])
            self.acc["audio"].index_add_(0, ids, to(b["logits"][3][va]))
            self.seen.index_add_(0, ids, torch.ones_like(ids).float())
            self.a_labels[ids] = to(b["a_labels"][va][:, 0]).int()

    def finalize(self):
        out = []
        for h in HEADS:
            p = (self.acc[h] / self.seen.clamp(min=1.0)[:, None]).softmax(dim=1)
            out.append(p.topk(5, dim=1)[1])
        return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--actions", type=int, default=20000)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "tools/recog_bench.py measures on the MI355X; there is nothing to time without it"
    dev = torch.device("cuda", 0)
    n_act = args.actions
    print("recognition tail at the C2a head widths %s, %d action ids; microseconds, median (min - max) of %d windows of %d calls"
          % (CLASSES, n_act, args.reps, args.inner))
    src = torch.empty(128 << 20, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    med, lo, hi = timed(lambda: dst.copy_(src), args.reps, args.inner)
    rate = 2 * src.numel() * 4 / med / 1e6                                         # TB/s
    print("achievable stream rate: torch copy of 512 MiB (read + write) %.1f us (%.1f - %.1f) = %.2f TB/s" % (med, lo, hi, rate))
    del src, dst

    col = RecognitionCollector(NUM_CLASS, n_act)
    for windows in (64, 8):
        b = make_batch(windows, n_act, 1 + windows, dev)
        vv, va = (b["v_ids"] >= 0), (b["a_ids"] >= 0)
        rows_v, rows_a = int(vv.sum()), int(va.sum())
        dist_v, dist_a = int(torch.unique(b["v_ids"][vv]).numel()), int(torch.unique(b["a_ids"][va]).numel())
        read = (rows_v * 4203 + rows_a * 44) * 4
        rmw = 2 * (dist_v * 4203 + dist_a * 44) * 4
        print("\nupdate, %d windows: %d visual rows (%d valid, %d distinct ids), %d audio rows (%d valid, %d distinct); dense logits "
              "%.1f MB; bytes the update must move: %.1f MB of valid logits read + %.1f MB of accumulators read and written"
              % (windows, windows * NV, rows_v, dist_v, windows * NA, rows_a, dist_a, (windows * NV * 4203 + windows * NA * 44) * 4 / 1e6,
                 read / 1e6, rmw / 1e6))
        run = lambda: col.update(b["logits"], b["v_ids"], b["a_ids"], b["v_labels"], b["a_labels"])
        ts = TorchState(n_act, dev)
        th = TorchState(n_act, "cpu")
        rows = [("hip  RecognitionCollector.update, eager", run)]
        graph = captured(run)
        rows.append(("hip  the same, captured and replayed", graph.replay))
        rows.append(("torch boolean index + index_add_ (device)", lambda: ts.update(b)))
        for name, fn in rows:
            med, lo, hi = timed(fn, args.reps, args.inner)
            extra = ""
            if name.startswith("hip"):
                extra = "   %.2f TB/s of %.1f MB = %.0f %% of the stream rate" % ((read + rmw) / med / 1e6, (read + rmw) / 1e6,
                                                                                100.0 * (read + rmw) / med / 1e6 / rate)
            print("  %-44s %10.1f (%.1f - %.1f)%s" % (name, med, lo, hi, extra))
        med, lo, hi = host_timed(lambda: th.update(b, to=lambda t: t.cpu()))
        print("  %-44s %10.1f (%.1f - %.1f)   host clock, 5 runs" % ("host  boolean index + .cpu() + CPU index_add_", med, lo, hi))
        del graph

    # ---- finalize over every action id
    col.reset()
    ts = TorchState(n_act, dev)
    g = torch.Generator(device="cpu").manual_seed(5)
    for grp in col.groups.values():
        for i, h in enumerate(grp.heads):
            x = (torch.randn(n_act, grp.classes[i], generator=g) * 6.0).to(dev)
            grp.sum[i][:, :grp.classes[i]] = x
            ts.acc[h].copy_(x)
        grp.touched.fill_(1)
        grp.labels.copy_(torch.stack([torch.randint(0, CLASSES[h], (n_act,), generator=g) for h in
                                      (HEADS[:3] if grp.n_labels == 3 else HEADS[3:])], 1).to(dev))
    col.seen.fill_(3.0)
    ts.seen.fill_(3.0)
    sum_bytes = n_act * 4247 * 4
    print("\nfinalize, %d touched actions: %.1f MB of accumulators; the probabilities add as many bytes written" % (n_act, sum_bytes / 1e6))
    probs = {h: torch.zeros_like(grp.sum[i]) for grp in col.groups.values() for i, h in enumerate(grp.heads)}

    def with_probs():
        for grp in col.groups.values():
            for i, h in enumerate(grp.heads):
                col._finalize(grp, i, probs[h])

    rows = [("hip  accuracies() (ranks + counts + the read)", col.accuracies, sum_bytes),
            ("hip  ranks + counts, captured and replayed", captured(col._launch_accuracies).replay, sum_bytes),
            ("hip  finalize with probabilities, 4 heads", with_probs, 2 * sum_bytes),
            ("hip  the same, captured and replayed", captured(with_probs).replay, 2 * sum_bytes),
            ("torch (sum / seen).softmax(1).topk(5), 4 heads", ts.finalize, 0)]
    for name, fn, nbytes in rows:
        med, lo, hi = timed(fn, args.reps, max(1, args.inner // 2))
        extra = "   %.2f TB/s of %.0f MB = %.0f %% of the stream rate" % (nbytes / med / 1e6, nbytes / 1e6, 100.0 * nbytes / med / 1e6 / rate) if nbytes else ""
        print("  %-44s %10.1f (%.1f - %.1f)%s" % (name, med, lo, hi, extra))


if __name__ == "__main__":
    main()
