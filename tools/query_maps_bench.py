#!/usr/bin/env python3
"""What a map from a window cache costs, against the only other way to the same map - one process, one MI355X.

    python tools/query_maps_bench.py [--rounds 7] [--inner 20] [--cold 10] [--precision fp16] [--workloads c2a_b64,c2a_b8,c4_b16]

Workloads: C2a at 64 and at 8 windows (15 visual + 10 audio interval queries per window: 55 query rows); C4 in the detection
model's inference form at 16 windows (the model's own pyramid).  The windows are encoded once, outside every timed region.
Variants, all replays of one torch.cuda.graph capture each, on ONE model per workload, the same windows and the same queries:
  (a) the cache route:  `query`      query_windows
                        `qmap_last`  query_attention_maps(layers="last")
                        `qmap_all`   query_attention_maps(layers="all")
  (b) the full forward: `fmap_last`  attention_maps(..., layers="last", rows="queries")   - before this entry the only way to
                        `fmap_all`   attention_maps(..., layers="all",  rows="queries")     the maps of (a)
  and the weights kernel alone at the workload's query shape against layer 0 of the cache (`kernel`).
Method: after warm-up replays of every variant, `--rounds` rounds; a round times every variant once, (a) and (b) alternating
(drift hits both alike).  WARM: a window of `--inner` back-to-back replays between two device events, per call.  COLD: `--cold`
single replays, each between its own two events and each behind a 512 MB fill that evicts L2 and the Infinity Cache - what a
caller sees who does other work between two calls.  Reported: median and [min, max] over the rounds, in ms (kernel: us).  The map
buffers are `out=` buffers made before the capture.  Prints a table and ONE JSON line.  No GPU: the tool fails, it does not fall
back."""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tim_amd import _lib as L  # noqa: E402
from tim_amd import synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tools._timing import captured  # noqa: E402
from tools.infer_bench import DEV, WORKLOADS, build  # noqa: E402


def variants(m, inp, nv, na):
    """-> ({name: callable}, things to keep alive, (G, Q)): every callable leaves its maps in buffers made here"""
    cfg = m.cfg
    Fk = cfg.F
    x = [inp["visual"], inp["audio"]]
    m.eval_feats = False                                          # (the forward of (b) without the `feats` store nobody reads here)
    if cfg.variant == "detection":
        cache = m.encode_windows(x, inp["times"][:, :Fk].contiguous())

        def query():
            return m.query_windows(cache, validate=False)

        def qmap(layers, out=None):
            return m.query_attention_maps(cache, layers=layers, out=out, validate=False)[1]

        def fmap(layers, out=None):
            return m.attention_maps(x, inp["times"], None, layers=layers, rows="queries", out=out)[1]
    else:
        te = m(inp["times"], "time_mlp")
        te_q = te[:, Fk:].contiguous()
        cache = m.encode_windows(x, te)

        def query():
            return m.query_windows(cache, te_q, nv, na, validate=False)

        def qmap(layers, out=None):
            return m.query_attention_maps(cache, te_q, nv, na, layers=layers, out=out, validate=False)[1]

        def fmap(layers, out=None):
            return m.attention_maps(x, te, nv, na, layers=layers, rows="queries", out=out)[1]
    held = {(r, k): f(k) for r, f in (("q", qmap), ("f", fmap)) for k in ("last", "all")}
    fns = {"query": query,
           "qmap_last": lambda: qmap("last", held["q", "last"]), "fmap_last": lambda: fmap("last", held["f", "last"]),
           "qmap_all": lambda: qmap("all", held["q", "all"]), "fmap_all": lambda: fmap("all", held["f", "all"])}
    w = held["q", "last"].weights[cfg.num_layers - 1]
    return fns, (held, cache), (w.shape[0], w.shape[1])


def kernel_alone(m, cache, G, Q):
    cfg, rt = m.cfg, m.rt
    E, Fk = cfg.E, cfg.F
    qkv_q = torch.randn((G * Q, 3 * E), device=DEV).to(rt.op_dtype)
    w = torch.empty((G, Q, Fk + 1), dtype=torch.float32, device=DEV)
    desc = L.TimDesc(G, Q, Fk, cfg.d_model, E, cfg.nhead, cfg.FF, rt.prec, 0.0, 0, 0, 0, None)
    lib = L.load()

    def run():
        L.check(lib.timhip_attention_query_weights(C.byref(desc), L.ptr(qkv_q), L.ptr(cache.kv), 2 * E, Fk, cache.W, None, 0, L.ptr(w),
                                                   Fk + 1, torch.cuda.current_stream().cuda_stream), "timhip_attention_query_weights")
    # bytes the kernel needs: the q | own k columns of the query rows, the K columns of every window once, the map
    nbytes = G * Q * 2 * E * qkv_q.element_size() + cache.W * Fk * E * cache.kv.element_size() + w.numel() * 4
    return run, nbytes, (qkv_q, w)


def warm_window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def cold_calls(fn, n, flush):
    out = []
    for _ in range(n):
        flush.fill_(1.0)                                          # 512 MB written: nothing of the last call is left in a cache
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def run_workload(name, args, flush):
    cname, B, nv, na = WORKLOADS[name]
    cfg = named_config(cname)
    m = build(cfg, args.precision)
    inp = {k: torch.from_numpy(v).float().to(DEV) for k, v in synth.make_inputs(cfg, B, nv, na, seed=2).items()}
    with torch.no_grad():
        fns, keep, (G, Q) = variants(m, inp, nv, na)
        kfn, kbytes, kkeep = kernel_alone(m, keep[1], G, Q)
        fns["kernel"] = kfn
        graphs = {k: captured(fn) for k, fn in fns.items()}
        for _ in range(3):
            for g in graphs.values():
                g.replay()
        torch.cuda.synchronize()
        warm, cold = {k: [] for k in graphs}, {k: [] for k in graphs}
        for _ in range(args.rounds):                              # one window of every variant per round, (a) and (b) alternating
            for k, g in graphs.items():
                warm[k].append(warm_window(g.replay, args.inner))
            for k, g in graphs.items():
                cold[k].append(cold_calls(g.replay, args.cold, flush))
    stat = lambda v: [round(statistics.median(v), 4), [round(min(v), 4), round(max(v), 4)]]
    res = {"config": cname, "windows": B, "groups": G, "query_rows_per_group": Q, "layers": cfg.num_layers,
           "map_bytes_per_layer": G * Q * (cfg.F + 1) * 4, "kernel_bytes": kbytes,
           "warm_ms": {k: stat(v) for k, v in warm.items()}, "cold_ms": {k: stat(v) for k, v in cold.items()}}
    wm = {k: statistics.median(v) for k, v in warm.items()}
    res["warm_ratios"] = {"one_map_over_query": round((wm["qmap_last"] - wm["query"]) / wm["query"], 4),
                          "per_map_of_all_over_query": round((wm["qmap_all"] - wm["query"]) / cfg.num_layers / wm["query"], 4),
                          "qmap_last_over_fmap_last": round(wm["qmap_last"] / wm["fmap_last"], 4),
                          "qmap_all_over_fmap_all": round(wm["qmap_all"] / wm["fmap_all"], 4)}
    res["kernel_warm_us"] = round(wm["kernel"] * 1e3, 2)
    res["kernel_warm_GBps"] = round(kbytes / (wm["kernel"] * 1e-3) / 1e9, 1)
    print("%s at %d windows (G = %d, Q = %d)" % (cname, B, G, Q))
    for k in graphs:
        w_, c_ = res["warm_ms"][k], res["cold_ms"][k]
        print("  %-10s warm %8.4f ms [%8.4f, %8.4f]   cold %8.4f ms [%8.4f, %8.4f]" % (k, w_[0], w_[1][0], w_[1][1], c_[0], c_[1][0], c_[1][1]))
    del graphs, fns, keep, kkeep, m, inp
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cold", type=int, default=10)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("query_maps_bench: no GPU - the route is only timed on the MI355X")
    flush = torch.empty(128 * 1024 * 1024, dtype=torch.float32, device=DEV)
    out = {"tool": "query_maps_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "rounds": args.rounds,
           "inner": args.inner, "cold": args.cold, "workloads": {}}
    for name in args.workloads.split(","):
        out["workloads"][name] = run_workload(name, args, flush)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
