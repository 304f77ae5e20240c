#!/usr/bin/env python3
"""Encode once / query many against the plain evaluation forward, timed on one MI355X.

    python tools/query_bench.py [--calls 20] [--repeats 5] [--warmup 3] [--precision fp16] [--workloads c2a_b64,c2a_b8,c4_b16]

Workloads: C2a at 64 and at 8 windows (15 visual + 10 audio interval queries per window, 55 query rows); C4 in the detection
model's inference form at 16 windows (399 queries per window).
Variants, all on ONE model per workload: the plain evaluation forward with and without `feats` (`forward_feats`,
`forward_no_feats`: the parent's routes, measured in the same run), `encode` (encode_windows), `query_identity` (query_windows,
G = W), `query_4w` (G = 4 W groups on repeated windows through a CUDA window index), `query_one` (G = W, one query per group);
beside them the attention-query kernel alone at each of the three query shapes (`attn_*`) and the cache-store step of one layer
alone (`cache_store`: the pitched device copy of the K | V columns timhip_stack_encode issues per layer).

Method (docs/measurement_log.md, tools/infer_bench.py): one process; after `--warmup` untimed calls of every variant, `--repeats`
rounds; in a round every variant is timed once, one after the other (interleaved: drift hits all of them alike), as a window of
`--calls` calls between two device events.  Reported per variant: the median window in ms per call and the [min, max] of the
windows, eagerly and as replays of one torch.cuda.graph capture.  Time encodings are computed outside the timed region for
every variant but the detection ones, whose calls run the time MLP themselves (both the forward and the query).  Prints ONE
JSON line.  There is no CPU fallback: without a GPU the tool fails."""
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
from tools.infer_bench import DEV, WORKLOADS, build  # noqa: E402


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def interleaved(fns, calls, repeats, warmup):
    """{name: fn} -> {name: (median, min, max) ms per call}; every round times every variant once"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(window(fn, calls))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def variants(m, inp, nv, na):
    """the Python-level variants of one workload -> ({name: fn}, what the kernel-level variants need)"""
    cfg = m.cfg
    W, Fk = inp["times"].shape[0], cfg.F
    det = cfg.variant == "detection"
    x = [inp["visual"], inp["audio"]]
    idx4 = (torch.arange(4 * W, device=DEV, dtype=torch.int32) % W).contiguous()
    if det:
        ft = inp["times"][:, :Fk].contiguous()
        cache = m.encode_windows(x, ft)
        one = torch.tensor([[[0.4, 0.5]]], device=DEV).expand(W, 1, 2).contiguous()
        v1 = one if "visual" in cfg.data_modality else None
        a1 = one if "audio" in cfg.data_modality else None
        pyr = m.inference_queries.to(DEV)
        v4 = pyr.expand(4 * W, -1, -1).contiguous() if "visual" in cfg.data_modality else None
        a4 = pyr.expand(4 * W, -1, -1).contiguous() if "audio" in cfg.data_modality else None

        def fwd(feats):
            m.eval_feats = feats
            return m(x, "encoder", inp["times"], None, label_queries=False)[0]
        fns = {"forward_feats": lambda: fwd(True), "forward_no_feats": lambda: fwd(False),
               "encode": lambda: m.encode_windows(x, ft),
               "query_identity": lambda: m.query_windows(cache, validate=False),
               "query_4w": lambda: m.query_windows(cache, v4, a4, window_index=idx4, validate=False),
               "query_one": lambda: m.query_windows(cache, v1, a1, validate=False)}
        Q = m.num_queries * (("visual" in cfg.data_modality) + ("audio" in cfg.data_modality))
        Q1 = ("visual" in cfg.data_modality) + ("audio" in cfg.data_modality)
    else:
        te = m(inp["times"], "time_mlp")
        te_q = te[:, Fk:].contiguous()
        te_q4 = te_q.repeat(4, 1, 1).contiguous()
        te_q1 = te_q[:, :1].contiguous()
        cache = m.encode_windows(x, te)

        def fwd(feats):
            m.eval_feats = feats
            return m(x, "encoder", te, nv, na)
        fns = {"forward_feats": lambda: fwd(True), "forward_no_feats": lambda: fwd(False),
               "encode": lambda: m.encode_windows(x, te),
               "query_identity": lambda: m.query_windows(cache, te_q, nv, na, validate=False),
               "query_4w": lambda: m.query_windows(cache, te_q4, nv, na, window_index=idx4, validate=False),
               "query_one": lambda: m.query_windows(cache, te_q1, 1, 0, validate=False)}
        Q = m._plan(Fk + nv + na, nv, na).S - Fk
        Q1 = m._plan(Fk + 1, 1, 0).S - Fk
    return fns, dict(cache=cache, W=W, Q=Q, Q1=Q1, idx4=idx4)


def kernel_variants(m, k):
    """the attention-query kernel alone on layer 0 of the cache at the three query shapes, and one layer's cache store alone"""
    cfg, rt, cache = m.cfg, m.rt, k["cache"]
    W, Fk, E, H = k["W"], cfg.F, cfg.E, cfg.nhead
    st = lambda: torch.cuda.current_stream().cuda_stream   # (at call time: a capture runs on a stream of its own)
    lib = L.load()
    fns = {}
    for name, G, Q, widx in (("attn_identity", W, k["Q"], None), ("attn_4w", 4 * W, k["Q"], k["idx4"]), ("attn_one", W, k["Q1"], None)):
        qkv_q = torch.randn((G * Q, 3 * E), device=DEV).to(rt.op_dtype)
        o = torch.empty((G * Q, E), dtype=rt.op_dtype, device=DEV)
        desc = L.TimDesc(G, Q, Fk, cfg.d_model, E, H, cfg.FF, rt.prec, 0.0, 0, 0, 0)

        def run(desc=desc, qkv_q=qkv_q, o=o, widx=widx):
            L.check(lib.timhip_attention_query_fwd(C.byref(desc), L.ptr(qkv_q), L.ptr(cache.kv), 2 * E, Fk, W, L.ptr(widx), L.ptr(o), st()),
                    "timhip_attention_query_fwd")
        fns[name] = run
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    ts = cache.kv.element_size()
    qkv = torch.randn((W * Fk, 3 * E), device=DEV).to(rt.op_dtype)
    dst = torch.empty((W * Fk, 2 * E), dtype=rt.op_dtype, device=DEV)

    def store():
        rc = hip.hipMemcpy2DAsync(dst.data_ptr(), 2 * E * ts, qkv.data_ptr() + E * ts, 3 * E * ts, 2 * E * ts, W * Fk, 3, st())   # 3: device to device
        assert rc == 0, rc
    fns["cache_store"] = store
    return fns, (qkv, dst)


def run_workload(name, args):
    cname, B, nv, na = WORKLOADS[name]
    cfg = named_config(cname)
    m = build(cfg, args.precision)
    inp = {k: torch.from_numpy(v).float().to(DEV) for k, v in synth.make_inputs(cfg, B, nv, na, seed=2).items()}
    res = {"config": cname, "windows": B}
    with torch.no_grad():
        fns, k = variants(m, inp, nv, na)
        kfns, keep = kernel_variants(m, k)
        fns.update(kfns)
        res["query_rows_per_group"], res["cache_bytes"] = k["Q"], k["cache"].nbytes
        eager = interleaved(fns, args.calls, args.repeats, args.warmup)
        graphs = {}
        for key, fn in fns.items():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[key] = g
        replay = interleaved({key: g.replay for key, g in graphs.items()}, args.calls, args.repeats, args.warmup)
        del graphs
    r4 = lambda t: [round(t[0], 4), [round(t[1], 4), round(t[2], 4)]]
    res["eager_ms"] = {key: r4(v) for key, v in eager.items()}
    res["graph_ms"] = {key: r4(v) for key, v in replay.items()}
    g = replay
    res["graph_ratios"] = {"encode_plus_query_over_forward_feats": round((g["encode"][0] + g["query_identity"][0]) / g["forward_feats"][0], 3),
                           "query_over_forward_no_feats": round(g["query_identity"][0] / g["forward_no_feats"][0], 3),
                           "query_4w_over_4_forwards_no_feats": round(g["query_4w"][0] / (4 * g["forward_no_feats"][0]), 3)}
    del m, inp, fns, kfns, keep, k
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20 calls per timed window")
    if not torch.cuda.is_available():
        raise SystemExit("query_bench: no GPU - the route is only timed on the MI355X")
    out = {"tool": "query_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "calls": args.calls,
           "repeats": args.repeats, "workloads": {}}
    for name in args.workloads.split(","):
        out["workloads"][name] = run_workload(name, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
