"""Timing helpers of the evaluation-tail benches (detect, twostream, recog, detmap) and the synthetic proposals the
detect and two-stream benches share."""
import statistics
import time

import torch


def timed(fn, reps, inner, rotate=1):
    """median / min / max microseconds per call over `reps` windows of `inner` calls (device events), after three warm-up
    calls.  rotate > 1: `fn` takes the index of the operand set to use, and the calls go round `rotate` of them."""
    run = (lambda k: fn()) if rotate == 1 else (lambda k: fn(k % rotate))
    for i in range(3):
        run(i)
    torch.cuda.synchronize()
    out, k = [], 0
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            run(k)
            k += 1
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def host_timed(fn, runs=5):
    """median / min / max microseconds of `runs` calls, host clock around a synchronise on either side"""
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts), min(ts), max(ts)


def captured(fn):
    """`fn` captured into a graph (after one run on a side stream, as capture asks for)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph


def synthetic_windows(g, B, NQ, streams=1):
    """the proposal side of a synthetic detection batch, drawn from `g`: -> (q [NQ, 2] query times, `streams` regressions
    [B * NQ, 2] = the queries + noise, window starts [B] float64, video index [B] int32: four windows a video)"""
    centre, half = torch.rand(NQ, generator=g) * 0.85 + 0.05, torch.rand(NQ, generator=g) * 0.07 + 0.01
    q = torch.stack([centre - half, centre + half], 1).clamp(0, 0.98)
    regs = [q.repeat(B, 1) + 0.01 * torch.randn(B * NQ, 2, generator=g) for _ in range(streams)]
    starts = torch.arange(B, dtype=torch.float64) * 7.5 + 0.000123
    return q, regs, starts, torch.arange(B, dtype=torch.int32) // 4
