#!/usr/bin/env python3
"""Timing of the two-stream detection fusion on one MI355X, per batch at the C4 inference shape
(16 windows x 399 queries = 6,384 proposals), Cv = 97 verbs and Cn = 300 nouns, for top_k = 1 and top_k = 5:

  hip      timhip_ts_candidates_count + _emit into a worst-case-sized output (no host read), eager and replayed from a
           captured graph (the `out=` form), and TwoStreamCollector.update (the calls + the 4-byte read of the total + the
           exact-size allocation)
  torch    the same candidate list from stock torch ops on the device (sigmoid, topk, broadcasting, boolean index; fp32
           arithmetic, so its scores are torch's, not the reproducible ones)
  host     the reference's form, restated: sigmoid on the device, dense copies of both [R, C] score matrices to the host,
           then the per-proposal Python loop (argpartition per row, the k x k inner loop, one dict per pair)

and a stream of --stream batches through TwoStreamCollector.update, then detections().

Method: every timed callable is warmed up, then timed --reps times with device events around --inner back-to-back calls
(host clock around a synchronise for the host form); the median and the spread (min - max) are printed.  All rows are
"warm": the same logits every call (10 MB for both streams, resident in the Infinity Cache).

    python tools/twostream_bench.py [--reps 20] [--inner 10] [--stream 200] [--host-rows 6384]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import TwoStreamCollector  # noqa: E402
from tim_amd import twostream as ts  # noqa: E402
from tools._timing import captured, host_timed, synthetic_windows, timed  # noqa: E402

B, NQ, CV, CN = 16, 399, 97, 300
R = B * NQ
WS, THR, ALPHA = 30.0, 0.03, 0.65


def make(seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    vl = torch.randn(R, CV, generator=g) * 1.5 - 7.0                    # the best verb of a row passes 0.03 about half the time
    nl = torch.randn(R, CN, generator=g) * 1.5 - 7.6
    q, (vr, nr), starts, vidx = synthetic_windows(g, B, NQ, streams=2)
    return dict(vl=vl.to(dev), nl=nl.to(dev), vr=vr.to(dev), nr=nr.to(dev), q=q.to(dev), starts=starts.to(dev), vidx=vidx.to(dev))


def torch_form(d, mt, k):
    start = d["starts"].repeat_interleave(NQ)[:, None]
    pv = (d["vr"].clamp(min=0.0).minimum(mt) * WS).double() + start
    pn = (d["nr"].clamp(min=0.0).minimum(mt) * WS).double() + start
    vs, vi = torch.sigmoid(d["vl"]).topk(k, dim=1)
    ns, ni = torch.sigmoid(d["nl"]).topk(k, dim=1)
    v, n = vs[:, :, None], ns[:, None, :]
    score = v.pow(ALPHA) * n.pow(1.0 - ALPHA)
    w = v / (v + n)
    seg = w.double()[..., None] * pv[:, None, None, :] + (1 - w).double()[..., None] * pn[:, None, None, :]
    seg = torch.round(seg * 1000.0) / 1000.0
    ok = (v > THR) & (n > THR) & (score > THR) & ((seg[..., 1] - seg[..., 0]) > 0)
    idx = ok.nonzero()
    r, i, j = idx[:, 0], idx[:, 1], idx[:, 2]
    key = d["vidx"].long()[r // NQ] * (CV * CN) + vi[r, i] * CN + ni[r, j]
    return seg[r, i, j].float(), score[r, i, j], key, r


def host_form(d, mt, k, rows):
    """FeatureMeter.update per stream + the loop of format_two_stream_predictions_epic.main, restated, on the first `rows`
    proposals"""
    verb, noun = torch.sigmoid(d["vl"][:rows]).cpu().numpy(), torch.sigmoid(d["nl"][:rows]).cpu().numpy()
    start = d["starts"].cpu().repeat_interleave(NQ)[:rows, None]
    pv = ((torch.clamp(d["vr"][:rows].cpu(), min=0.0, max=float(mt)) * WS) + start).numpy()
    pn = ((torch.clamp(d["nr"][:rows].cpu(), min=0.0, max=float(mt)) * WS) + start).numpy()
    entries = []
    for i in range(rows):
        vi = np.argpartition(verb[i], -k)[-k:]
        ni = np.argpartition(noun[i], -k)[-k:]
        for v, vs in zip(vi, verb[i][vi]):
            if vs > THR:
                for n, ns in zip(ni, noun[i][ni]):
                    if ns > THR:
                        score = (vs ** ALPHA) * (ns ** (1.0 - ALPHA))
                        if score > THR:
                            w = vs / (vs + ns)
                            p = np.round(w * pv[i] + (1 - w) * pn[i], 3)
                            if p[1] - p[0] > 0.0:
                                entries.append({"verb": v, "noun": n, "action": "%d,%d" % (v, n), "score": score,
                                                "segment": [p[0], p[1]]})
    return entries


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--stream", type=int, default=200)
    ap.add_argument("--host-rows", type=int, default=R)
    ap.add_argument("--top-k", type=int, nargs="+", default=[1, 5])
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "tools/twostream_bench.py measures on the MI355X; there is nothing to time without it"
    dev = torch.device("cuda", 0)
    print("two-stream fusion, one batch = %d windows x %d queries = %d proposals, Cv = %d, Cn = %d, threshold %.2f, alpha %.2f; "
          "microseconds, median (min - max) of %d windows of %d calls" % (B, NQ, R, CV, CN, THR, ALPHA, args.reps, args.inner))
    d = make(1, dev)
    mt = d["q"].max().reshape(1)
    logit_bytes = R * (CV + CN) * 4
    for k in args.top_k:
        seg, score, key, row = ts.candidates(d["vl"], d["nl"], d["vr"], d["nr"], d["starts"], WS, mt, d["vidx"], NQ, THR, ALPHA, k)
        n = int(score.numel())
        t = torch_form(d, mt, k)
        same = bool(torch.equal(t[2], key) and torch.equal(t[3].int(), row) and torch.equal(t[0], seg))
        cap = R * k * k
        out = (torch.empty((cap, 2), device=dev), torch.empty(cap, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
               torch.empty(cap, dtype=torch.int32, device=dev))
        print("\ntop_k = %d: logits %.1f MB, %d candidates of %d pairs, %d rows with candidates; torch-op list bit-identical in "
              "order, keys and segments (its arithmetic is torch's fp32, so not expected): %s" % (k, logit_bytes / 1e6, n, R * k * k, int(torch.unique(row).numel()), same))

        def hip_pair():
            ts.candidates(d["vl"], d["nl"], d["vr"], d["nr"], d["starts"], WS, mt, d["vidx"], NQ, THR, ALPHA, k, out=out)

        graph = captured(hip_pair)

        col = TwoStreamCollector(CV, CN, THR, ALPHA, k)
        meta = {"video_id": ["v%d" % (i // 4) for i in range(B)], "window_start": d["starts"].cpu(),
                "window_size": torch.tensor([WS] * B, dtype=torch.float64)}

        def hip_update():
            col.reset()
            col.update(((None, None, d["vl"], None), (d["vr"], None)), ((None, None, d["nl"], None), (d["nr"], None)),
                       (d["q"], None), meta)

        rows = [("hip  select + scan + emit, eager", hip_pair), ("hip  select + scan + emit, graph replay", graph.replay),
                ("hip  TwoStreamCollector.update", hip_update), ("torch ops on the device", lambda: torch_form(d, mt, k))]
        for name, fn in rows:
            med, lo, hi = timed(fn, args.reps, args.inner)
            extra = "   %.0f GB/s of the %.1f MB read once" % (logit_bytes / med / 1e3, logit_bytes / 1e6) if "graph" in name else ""
            print("  %-42s %10.1f (%.1f - %.1f)%s" % (name, med, lo, hi, extra))
        hr = min(args.host_rows, R)
        entries = []
        med, lo, hi = host_timed(lambda: entries.append(len(host_form(d, mt, k, hr))), runs=3)
        print("  %-42s %10.1f (%.1f - %.1f)   host clock, %d of %d proposals, %d entries, 3 runs"
              % ("host form (dense copies + Python loop)", med, lo, hi, hr, R, entries[-1]))
        del graph, out

    # ---- a stream of batches, then detections()
    batches = [make(50 + i, dev) for i in range(8)]
    col = TwoStreamCollector(CV, CN, THR, ALPHA, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.stream):
        s = batches[i % 8]
        meta = {"video_id": ["v%03d" % ((i * B + j) // 40) for j in range(B)], "window_start": s["starts"].cpu() + 120.0 * i,
                "window_size": torch.tensor([WS] * B, dtype=torch.float64)}
        col.update(((None, None, s["vl"], None), (s["vr"], None)), ((None, None, s["nl"], None), (s["nr"], None)), (s["q"], None), meta)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ncand = int(col.candidates()[1].numel())
    dets = []
    med, lo, hi = (t / 1e3 for t in host_timed(lambda: dets.append(col.detections(sigma=0.25)), runs=3))
    print("\nstream of %d batches (top_k 1, %d videos): update %.1f us per batch = %.0f windows/s (host clock, synchronised at the "
          "end); %d candidates; detections() %.1f ms (min %.1f, max %.1f; host clock, 3 runs, the first includes the one "
          "concatenation) -> %d detections"
          % (args.stream, len(col.video_ids), (t1 - t0) * 1e6 / args.stream, B * args.stream / (t1 - t0), ncand,
             med, lo, hi, int(dets[-1][1].numel())))


if __name__ == "__main__":
    main()
