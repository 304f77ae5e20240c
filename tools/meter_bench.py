"""What the training meter costs per iteration at the C2a shapes (heads 97 / 300 / 3,806 / 44 classes; 25 visual and 10 audio
queries per window), at 64 and at 8 windows:

    (a) tim_amd.TrainMeter.update, statistics only (ensemble=False)            graph replay
    (b) the same with the per-action ensemble (ensemble=True)                  graph replay
    (c) the same statistics written with torch ops on the device               graph replay
        (topk(5), eq, masked sums, seven multiply-adds into double accumulators)
    (d) the reference's host form, eagerly: .cpu() of the four heads' logits (pageable memory), a CPU index_add_ into
        per-action accumulators and seven .item() calls (recognition/scripts/train.py:391-410)

    python tools/meter_bench.py [--windows 64 8] [--sets 12] [--replays 50] [--trials 5] [--num-actions 20000]

(a) - (c) are timed with device events around `--replays` replays of a graph that holds one update for each of `--sets`
distinct input sets (12 sets of 27 MB are more than the 256 MB of last-level cache: "cold"), and again with one set ("warm":
the logits of the previous replay are still in cache, as a head GEMM's output partly is in a real step); the figure is the
median over `--trials` of the time per update, the three variants alternating inside a trial.  The byte floor of (a) is its
read of the logits.  Prints one JSON line.
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import TrainMeter  # noqa: E402

CLASSES = (97, 300, 3806, 44)
NV, NA = 25, 10
SLOTS = ("total", "drloc", "visual", "verb", "noun", "action", "audio")
HBM_GBS = 8000.0     # MI355X peak HBM bandwidth, for the byte floor


def make_set(seed, W, num_actions, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    Rv, Ra = W * NV, W * NA
    logits = [torch.randn((Rv if i < 3 else Ra, C), generator=g).to(dev) for i, C in enumerate(CLASSES)]
    v_labels = torch.stack([torch.randint(0, C, (Rv,), generator=g) for C in CLASSES[:3]], dim=1)
    a_labels = torch.randint(0, CLASSES[3], (Ra,), generator=g)
    v_pad, a_pad = torch.rand((Rv,), generator=g) < 0.2, torch.rand((Ra,), generator=g) < 0.2
    v_labels[v_pad], a_labels[a_pad] = -1, -1
    v_ids = torch.where(v_pad, -1, torch.randint(0, num_actions, (Rv,), generator=g))
    a_ids = torch.where(a_pad, -1, torch.randint(0, num_actions, (Ra,), generator=g))
    losses = {k: torch.rand((1,), generator=g).to(dev) for k in SLOTS}
    return logits, v_ids.to(dev), a_ids.to(dev), v_labels.to(dev), a_labels.to(dev), losses


class TorchMeter:
    """variant (c): the same statistics with torch ops on the device, capturable (no boolean indexing: masks and sums)"""

    def __init__(self, dev):
        self.sum = torch.zeros(7, dtype=torch.float64, device=dev)
        self.count = torch.zeros(7, dtype=torch.int64, device=dev)
        self.val = torch.zeros(7, dtype=torch.float32, device=dev)
        self.run = torch.zeros((5, 3), dtype=torch.int64, device=dev)
        self.last = torch.zeros((5, 3), dtype=torch.int64, device=dev)

    def update(self, logits, v_labels, a_labels, losses):
        vv, va = v_labels[:, 2] != -1, a_labels != -1
        nv, na = vv.sum(), va.sum()
        hits = []
        for i, x in enumerate(logits):
            lab, ok = (v_labels[:, i], vv) if i < 3 else (a_labels, va)
            top = x.topk(5, dim=1).indices
            eq = (top == lab[:, None]) & ok[:, None]
            hits.append(eq)
        for row, i in ((0, 0), (1, 1), (2, 2), (4, 3)):
            self.last[row, 0] = nv if i < 3 else na
            self.last[row, 1] = hits[i][:, 0].sum()
            self.last[row, 2] = hits[i].any(dim=1).sum()
        self.last[3, 0] = nv
        self.last[3, 1] = (hits[0][:, 0] & hits[1][:, 0]).sum()
        self.last[3, 2] = (hits[0].any(dim=1) & hits[1].any(dim=1)).sum()
        self.run += self.last
        for s, k in enumerate(SLOTS):
            n = nv + na if s < 2 else (na if k == "audio" else nv)
            on = (n > 0) if s >= 2 else torch.ones_like(n, dtype=torch.bool)
            v = losses[k].reshape(())
            self.val[s] = torch.where(on, v, self.val[s])
            self.sum[s] += torch.where(on, v.double() * n.double(), torch.zeros_like(self.sum[s]))
            self.count[s] += torch.where(on, n, torch.zeros_like(n))


def host_form(sets, num_actions, iters):
    """variant (d), eagerly -> ms per iteration"""
    acc = [torch.zeros((num_actions, C), dtype=torch.float32) for C in CLASSES]
    seen = torch.zeros((num_actions,), dtype=torch.float32)
    t = []
    for it in range(iters + 2):
        logits, v_ids, a_ids, v_labels, a_labels, losses = sets[it % len(sets)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [x.detach().cpu() for x in logits]
        vi, ai, vl, al = v_ids.cpu(), a_ids.cpu(), v_labels.cpu(), a_labels.cpu()
        vv, va = vl[:, 2] != -1, al != -1
        for i in range(3):
            acc[i].index_add_(0, vi[vv], host[i][vv])
        acc[3].index_add_(0, ai[va], host[3][va])
        seen.index_add_(0, vi[vv], torch.ones(int(vv.sum())))
        seen.index_add_(0, ai[va], torch.ones(int(va.sum())))
        vals = [losses[k].item() for k in SLOTS]   # noqa: F841
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t[2:])


def graph_of(fn, sets):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in sets:
            fn(s)                                           # warm-up: sizes the scratch, loads the code objects
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for s in sets:
            fn(s)
    return g


def time_graphs(graphs, n_updates, replays, trials):
    """{name: graph} alternating inside every trial -> {name: median microseconds per update}"""
    out = {k: [] for k in graphs}
    for _ in range(trials):
        for k, g in graphs.items():
            g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * 1e3 / (replays * n_updates))
    return {k: statistics.median(v) for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--sets", type=int, default=12)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--num-actions", type=int, default=20000)
    ap.add_argument("--host-iters", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/meter_bench.py measures on the MI355X: no device here, no number")
    dev = torch.device("cuda", 0)
    num_class = [list(CLASSES[:3]), CLASSES[3]]
    result = {"tool": "meter_bench", "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "num_actions": args.num_actions,
              "sets": args.sets, "replays": args.replays, "trials": args.trials, "unit": "microseconds per update", "shapes": {}}
    for W in args.windows:
        sets = [make_set(100 * W + i, W, args.num_actions, dev) for i in range(args.sets)]
        stats_only = TrainMeter(num_class, args.num_actions, ensemble=False)
        with_ens = TrainMeter(num_class, args.num_actions, ensemble=True)
        torch_meter = TorchMeter(dev)
        fns = {"a_update_statistics": lambda s: stats_only.update(s[0], s[1], s[2], s[3], s[4], losses=s[5]),
               "b_update_with_ensemble": lambda s: with_ens.update(s[0], s[1], s[2], s[3], s[4], losses=s[5]),
               "c_torch_ops_on_device": lambda s: torch_meter.update(s[0], s[3], s[4], s[5])}
        row = {}
        for label, use in (("cold", sets), ("warm", sets[:1])):
            graphs = {k: graph_of(fn, use) for k, fn in fns.items()}
            row[label] = {k: round(v, 2) for k, v in time_graphs(graphs, len(use), args.replays, args.trials).items()}
            del graphs
        row["d_reference_host_form_ms"] = round(host_form(sets, args.num_actions, args.host_iters), 3)
        nbytes = 4 * (W * NV * sum(CLASSES[:3]) + W * NA * CLASSES[3])
        row["logit_bytes"] = nbytes
        row["byte_floor_us"] = round(nbytes / (HBM_GBS * 1e3), 2)
        # the two ways of counting agree before anything is reported: the torch variant's counters are the meter's
        s = stats_only.read()
        torch.cuda.synchronize()
        mine = np.array([[s["acc"][h][k] for k in ("rows", "hits1", "hits5")] for h in ("verb", "noun", "action", "mt_action", "audio")])
        row["counters_agree_with_torch_ops"] = bool(np.array_equal(mine, torch_meter.run.cpu().numpy()))
        result["shapes"]["%d_windows" % W] = row
        del sets, stats_only, with_ens, torch_meter
        torch.cuda.empty_cache()
    print(json.dumps(result), flush=True)
    return result


if __name__ == "__main__":
    main()
