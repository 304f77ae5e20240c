#!/usr/bin/env python3
"""Timing of the detection inference tail on one MI355X, per batch at the C4 inference shape
(16 windows x 399 queries = 6,384 proposals) for C = 97 and C = 3,806 classes:

  hip      timhip_det_candidates_count + _emit into a worst-case-sized output (no host read): the two library calls alone,
           and DetectionCollector.update (the calls + the 4-byte read of the total + the exact-size allocation)
  torch    the same candidate list from stock torch ops on the device (sigmoid, compare, nonzero, gathers; fp32 arithmetic,
           so its scores are torch's, not the reproducible ones)
  host     the reference's form, restated: sigmoid on the device, dense copy of the [R, C] scores to the host, then the
           per-proposal Python loop (round, width test, numpy.where, one dict per candidate)

and DetectionCollector.detections() end to end on a stream of --stream batches (C = 97).

Method: every timed callable is warmed up, then timed --reps times with device events around --inner back-to-back
calls (host clock around a synchronise for the host form); the median and the spread (min - max) are printed.  "warm":
the same logits every call (2.5 MB at C = 97 and 97 MB at C = 3,806 both fit the 256 MiB Infinity Cache; 97 MB does not
fit one XCD's 4 MiB L2).  "cold": the calls rotate through enough distinct logits buffers to exceed 256 MiB, so each
call's first read comes from HBM.  Bytes are what each launch must move by the algorithm: count reads the logits of the
valid rows once and writes 13 bytes per row; emit reads them again and writes 24 bytes per candidate.

    python tools/detect_bench.py [--reps 20] [--inner 10] [--stream 200] [--host-rows 6384]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import DetectionCollector  # noqa: E402
from tim_amd import detect as hd  # noqa: E402
from tools._timing import host_timed, synthetic_windows, timed  # noqa: E402

B, NQ = 16, 399
R = B * NQ
WS, THR = 30.0, 0.01


def make(C, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = torch.randn(R, C, generator=g) * 1.5 - 7.0                 # ~ 5 % of the scores above 0.01
    q, (reg,), starts, vidx = synthetic_windows(g, B, NQ)
    return dict(logits=logits.to(dev), reg=reg.to(dev), q=q.to(dev), starts=starts.to(dev), vidx=vidx.to(dev))


def torch_form(d, mt, C):
    p = (d["reg"].clamp(min=0.0).minimum(mt) * WS).double() + d["starts"].repeat_interleave(NQ)[:, None]
    p = torch.round(p * 1000.0) / 1000.0
    ok = (p[:, 1] - p[:, 0]) > 0
    s = torch.sigmoid(d["logits"])
    idx = ((s > THR) & ok[:, None]).nonzero()
    r, c = idx[:, 0], idx[:, 1]
    return p[r].float(), s[r, c], d["vidx"].long()[r // NQ] * C + c, r


def host_form(d, mt, rows):
    """FeatureMeter.update + the loop of format_predictions.main, restated, on the first `rows` proposals"""
    scores = torch.sigmoid(d["logits"][:rows]).cpu().numpy()
    props = torch.clamp(d["reg"][:rows].cpu(), min=0.0, max=float(mt))
    props = ((props * WS) + d["starts"].cpu().repeat_interleave(NQ)[:rows, None]).numpy()
    entries = []
    for i in range(rows):
        p = np.round(props[i], 3)
        if p[1] - p[0] > 0.0:
            sc = scores[i]
            for c in np.where(sc > THR)[0]:
                entries.append({"action": c, "score": sc[c], "segment": [p[0], p[1]]})
    return entries


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--stream", type=int, default=200)
    ap.add_argument("--host-rows", type=int, default=R)
    ap.add_argument("--classes", type=int, nargs="+", default=[97, 3806])
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "tools/detect_bench.py measures on the MI355X; there is nothing to time without it"
    dev = torch.device("cuda", 0)
    print("detection tail, one batch = %d windows x %d queries = %d proposals, threshold %.2f; microseconds, median (min - max) of "
          "%d windows of %d calls" % (B, NQ, R, THR, args.reps, args.inner))
    for C in args.classes:
        nbuf = max(2, int(np.ceil((320 << 20) / (R * C * 4.0))))        # > 256 MiB of logits in rotation for the cold rows
        nbuf = min(nbuf, 8) if C < 1000 else nbuf                      # (C = 97: 2.5 MB a batch; 8 buffers stay cache-resident - said below)
        sets = [make(C, 1 + i, dev) for i in range(nbuf)]
        d = sets[0]
        mt = d["q"].max()
        seg, score, key, row = hd.candidates(d["logits"], d["reg"], d["starts"], WS, mt, d["vidx"], NQ, THR)
        n = int(score.numel())
        valid = int(torch.unique(row).numel())                         # rows that emit; the count reads every valid row
        t = torch_form(d, mt, C)
        same = bool(torch.equal(t[2], key) and torch.equal(t[3].int(), row) and torch.equal(t[0], seg))
        cap = R * C
        out = (torch.empty((cap, 2), device=dev), torch.empty(cap, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
               torch.empty(cap, dtype=torch.int32, device=dev))
        logit_bytes = R * C * 4
        print("\nC = %d: logits %.1f MB, %d candidates (%.1f %% of %d scores), %d rows with candidates; torch-op list identical in "
              "order, keys and segments: %s" % (C, logit_bytes / 1e6, n, 100.0 * n / (R * C), R * C, valid, same))
        print("  bytes a call must move: count %.1f MB read + %.2f MB written; emit %.1f MB read + %.2f MB written"
              % (logit_bytes / 1e6, R * 13 / 1e6, logit_bytes / 1e6, n * 24 / 1e6))

        def hip_pair(i=0):
            s = sets[i]
            hd.candidates(s["logits"], s["reg"], s["starts"], WS, mt, s["vidx"], NQ, THR, out=out)

        col = DetectionCollector(C, "action", THR)
        meta = {"video_id": ["v%d" % (i // 4) for i in range(B)], "window_start": d["starts"].cpu(),
                "window_size": torch.tensor([WS] * B, dtype=torch.float64)}

        def hip_update(i=0):
            s = sets[i]
            col.reset()
            col.update((None, None, s["logits"], None), (s["reg"], None), (s["q"], None), meta)

        rows = [("hip  count + emit (3 launches), warm", hip_pair, 1), ("hip  count + emit (3 launches), cold", hip_pair, nbuf),
                ("hip  DetectionCollector.update, warm", hip_update, 1),
                ("torch ops on the device, warm", lambda i=0: torch_form(sets[i], mt, C), 1),
                ("torch ops on the device, cold", lambda i: torch_form(sets[i], mt, C), nbuf)]
        for name, fn, rot in rows:
            med, lo, hi = timed(fn, args.reps, args.inner, rot)
            extra = ""
            if name.startswith("hip  count"):
                extra = "   %.0f GB/s of the %.1f MB both passes read" % (2 * logit_bytes / med / 1e3, 2 * logit_bytes / 1e6)
            note = " (rotation of %d buffers = %.0f MB%s)" % (rot, rot * logit_bytes / 1e6,
                                                              ", still cache-resident" if rot * logit_bytes < (256 << 20) else "") if rot > 1 else ""
            print("  %-40s %10.1f (%.1f - %.1f)%s%s" % (name, med, lo, hi, extra, note))
        hr = min(args.host_rows, R)
        entries = []
        med, lo, hi = host_timed(lambda: entries.append(len(host_form(d, mt, hr))), runs=3)
        print("  %-40s %10.1f (%.1f - %.1f)   host clock, %d of %d proposals, %d entries, 3 runs"
              % ("host form (dense copy + Python loop)", med, lo, hi, hr, R, entries[-1]))
        del sets, out
        torch.cuda.empty_cache()

    # ---- detections() end to end on a stream
    C = 97
    batches = [make(C, 50 + i, dev) for i in range(8)]
    col = DetectionCollector(C, "action", THR)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.stream):
        s = batches[i % 8]
        meta = {"video_id": ["v%03d" % ((i * B + j) // 40) for j in range(B)], "window_start": s["starts"].cpu() + 120.0 * i,
                "window_size": torch.tensor([WS] * B, dtype=torch.float64)}
        col.update((None, None, s["logits"], None), (s["reg"], None), (s["q"], None), meta)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ncand = int(col.candidates()[1].numel())
    dets = []
    med, lo, hi = (t / 1e3 for t in host_timed(lambda: dets.append(col.detections(sigma=0.1)), runs=3))
    print("\nstream of %d batches (C = %d, %d videos): update %.1f us per batch (host clock, synchronised at the end); %d candidates; "
          "detections() %.1f ms (min %.1f, max %.1f; host clock, 3 runs, the first includes the one concatenation) -> %d detections"
          % (args.stream, C, len(col.video_ids), (t1 - t0) * 1e6 / args.stream, ncand, med, lo, hi,
             int(dets[-1][1].numel())))


if __name__ == "__main__":
    main()
