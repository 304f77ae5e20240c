"""What the detection meter costs per iteration at the C4 training shape (16 windows: 6,384 query rows, visual heads of 97 / 300 /
3,806 classes), one modality side:

    (a) timhip_det_side_loss_fwd_ordered                                        graph replay
    (b) timhip_det_side_loss_fwd_stats: (a) plus the side statistics            graph replay
    (c) (b) plus timhip_det_meter_update                                        graph replay
    (d) (a) plus the reference's form of the same numbers in torch ops on the device: a second focal pass with
        reduction="none" over the action head, masked positive / negative sums, the counts and the divisions
        (detection/scripts/train.py:262-273; masks instead of boolean indexing, so that it captures)   graph replay
    (e) (d) eagerly with the reference's thirteen host reads (train.py:413-430)  wall clock per iteration

    python tools/det_meter_bench.py [--sets 2] [--replays 30] [--trials 5]

(a) - (d) are timed with device events around `--replays` replays of a graph that holds one call for each of `--sets` distinct
input sets (a set is 215 MB of logits and targets: two sets are more than the 256 MB of last-level cache, "cold"), and again with
one set ("warm"); the figure is the median over `--trials` of the time per call, the variants alternating inside a trial.  Before
anything is reported the counts of (d) are asserted equal to those of (b).  Also printed: the bytes of a SEPARATE second pass over
the action head, against whose time at the streaming rate (b) - (a) is to be held: 97 MB for the logits alone, 194 MB with the
targets such a pass reads too.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import _lib as L  # noqa: E402
from tim_amd.functional import _stream  # noqa: E402

ROWS, CLASSES = 6384, (97, 300, 3806)
THR, ALPHA, GAMMA, EPS, LAM, MOM = 0.6, 0.25, 2.0, 1e-8, 0.5, 0.9


class Set:
    def __init__(self, seed, dev):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.x = [torch.randn((ROWS, C), generator=g, device=dev) * 3.0 for C in CLASSES]
        self.t = [torch.rand((ROWS, C), generator=g, device=dev).pow(8.0) for C in CLASSES]
        self.iou = torch.rand((ROWS,), generator=g, device=dev)
        self.iou[torch.rand((ROWS,), generator=g, device=dev) < 0.1] = -1.0
        self.off = torch.full((ROWS, 2), float("inf"), device=dev)
        pos = (self.iou >= 0.6) & (torch.rand((ROWS,), generator=g, device=dev) < 0.25)
        self.off[pos] = torch.rand((int(pos.sum()), 2), generator=g, device=dev) * 3.0
        self.reg = torch.rand((ROWS, 2), generator=g, device=dev) * 3.0
        self.px = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in self.x])
        self.pt = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in self.t])
        self.C = (ctypes.c_int * 3)(*CLASSES)


class Buffers:
    def __init__(self, dev):
        self.block = torch.zeros(8, device=dev)
        self.norm = torch.full((), 250.0, device=dev)
        self.partials = torch.zeros(L.DET_SIDE_STATS_PARTIALS, device=dev)
        self.stats = torch.zeros(L.DET_SIDE_STATS_WORDS, device=dev)
        self.state = torch.zeros(L.DET_METER_STATE_WORDS // 2, dtype=torch.int64, device=dev)
        self.sides = (ctypes.c_void_p * 2)(self.stats.data_ptr(), None)
        self.torch_out = torch.zeros(8, device=dev)      # (d): positive, negative, per-head x3 are not free there, counts
        self.torch_counts = torch.zeros(2, dtype=torch.int64, device=dev)


def side_args(s, b):
    return (s.px, s.pt, s.C, 3, ROWS, L.ptr(s.iou), L.ptr(s.off), L.ptr(s.reg), THR, ALPHA, GAMMA, EPS, LAM, MOM, L.ptr(b.norm), L.ptr(b.block))


def ordered(s, b):
    L.call("timhip_det_side_loss_fwd_ordered", *side_args(s, b), L.ptr(b.partials), _stream())


def with_stats(s, b):
    L.call("timhip_det_side_loss_fwd_stats", *side_args(s, b), L.ptr(b.partials), L.ptr(b.stats), _stream())


def with_meter(s, b):
    with_stats(s, b)
    L.call("timhip_det_meter_update", L.ptr(b.state), ctypes.addressof(b.sides), 3, L.ptr(b.block), None, _stream())


def reference_form(s, b):
    """the second pass of train.py:262-273 with masks: elementwise focal over the action head, weighted, summed over the positive
    and over the other valid rows, divided by the normaliser the side loss left; the two counts"""
    ordered(s, b)
    x, t = s.x[2], s.t[2]
    valid, pos = s.iou >= 0, s.off[:, 0] != float("inf")
    w = torch.where(s.iou < THR, torch.ones_like(s.iou), s.iou)
    p = torch.sigmoid(x)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** GAMMA) * (ALPHA * t + (1 - ALPHA) * (1 - t)) * w[:, None]
    rows = loss.sum(dim=1)
    zero = torch.zeros_like(rows)
    b.torch_out[0] = torch.where(valid & pos, rows, zero).sum() / b.norm
    b.torch_out[1] = torch.where(valid & ~pos, rows, zero).sum() / b.norm
    b.torch_counts[0], b.torch_counts[1] = valid.sum(), pos.sum()


def host_reads(sets, b, iters):
    """variant (e), eagerly -> ms per iteration: (d), then the thirteen reads"""
    t = []
    for it in range(iters + 2):
        s = sets[it % len(sets)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_form(s, b)
        vals = [b.block[0].cpu().item() for _ in range(7)] + [b.torch_out[0].cpu().item(), b.torch_out[1].cpu().item()]   # noqa: F841
        vals += [b.block[0].cpu().item(), b.block[0].cpu().item()]                                                      # loss, drloc
        counts = [b.torch_counts[0].cpu(), b.torch_counts[1].cpu()]                                                     # noqa: F841
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t[2:])


def graph_of(fn, sets, b):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in sets:
            fn(s, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for s in sets:
            fn(s, b)
    return g


def time_graphs(graphs, n_calls, replays, trials):
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
            out[k].append(e0.elapsed_time(e1) * 1e3 / (replays * n_calls))
    return {k: (statistics.median(v), v) for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/det_meter_bench.py measures on the MI355X: no device here, no number")
    dev = torch.device("cuda", 0)
    L.load()
    sets = [Set(900 + i, dev) for i in range(args.sets)]
    b = Buffers(dev)
    fns = {"a_fwd_ordered": ordered, "b_fwd_stats": with_stats, "c_fwd_stats_and_meter": with_meter, "d_ordered_and_torch_ops": reference_form}
    result = {"tool": "det_meter_bench", "box": socket.gethostname(), "device": torch.cuda.get_device_name(0), "rows": ROWS,
              "classes": list(CLASSES), "sets": args.sets, "replays": args.replays, "trials": args.trials, "unit": "microseconds per call"}
    # the two ways of counting agree before anything is reported
    with_stats(sets[0], b)
    b.norm.fill_(250.0)                                   # (the running normaliser: both forms start from the same value)
    reference_form(sets[0], b)
    torch.cuda.synchronize()
    b.norm.fill_(250.0)
    stats, counts = b.stats.cpu(), b.torch_counts.cpu()
    assert int(stats[L.DET_STAT_VALID]) == int(counts[0]) and int(stats[L.DET_STAT_POSITIVES]) == int(counts[1]), (stats, counts)
    result["valid_rows"], result["positives"] = int(counts[0]), int(counts[1])
    result["split_rel_diff_vs_torch_ops"] = [abs(float(stats[k]) - float(v)) / max(abs(float(v)), 1e-30)
                                             for k, v in ((L.DET_STAT_POS, b.torch_out[0]), (L.DET_STAT_NEG, b.torch_out[1]))]
    for label, use in (("cold", sets), ("warm", sets[:1])):
        graphs = {k: graph_of(fn, use, b) for k, fn in fns.items()}
        timed = time_graphs(graphs, len(use), args.replays, args.trials)
        result[label] = {k: round(v[0], 2) for k, v in timed.items()}
        result[label + "_raw"] = {k: [round(x, 2) for x in v[1]] for k, v in timed.items()}
        del graphs
    result["e_reference_host_reads_ms"] = round(host_reads(sets, b, args.host_iters), 3)
    result["side_bytes"] = 8 * ROWS * sum(CLASSES)
    result["second_pass_logit_bytes"], result["second_pass_bytes_with_targets"] = 4 * ROWS * CLASSES[2], 8 * ROWS * CLASSES[2]
    print(json.dumps(result), flush=True)
    return result


if __name__ == "__main__":
    main()
