#!/usr/bin/env python3
"""Forward-only timing of the evaluation forward (model.eval() under torch.no_grad()) on one MI355X.

    python tools/infer_bench.py [--calls 20] [--repeats 5] [--warmup 5] [--precision fp16] [--workloads c2a_b64,c2a_b8,c4_b16]

Workloads: C2a at 64 and at 8 windows (time MLP + encoder, 15 visual + 10 audio interval queries per window); C4 in the
detection model's inference form at 16 windows (forward_inference: 100 feature tokens + 399 dense queries per window).
Arms: `training_route` (TIM_AMD_INFER=0: the autograd Function with dropout off - what an evaluation ran before),
`infer` (the evaluation route), `infer_no_feats` (the same with model.eval_feats = False).  Every arm is timed eagerly and as
a replay of one torch.cuda.graph capture.

Method: one process; per arm a fresh model, `--warmup` untimed calls, then `--repeats` windows of `--calls` forwards between two
device events; the median window is reported as ms per forward.  The arms of a workload run one after the other, each after
the previous one's model is freed.  Peak allocated bytes: torch.cuda.max_memory_allocated over one eager forward after the
warm-up (the model's parameters, operand copies and cached arena included).  Prints ONE JSON line.  There is no CPU fallback:
without a GPU the tool fails."""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tim_amd import synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402

DEV = "cuda:0"
WORKLOADS = {"c2a_b64": ("C2a", 64, 15, 10), "c2a_b8": ("C2a", 8, 15, 10), "c4_b16": ("C4", 16, 0, 0)}
ARMS = (("training_route", "0", True), ("infer", "1", True), ("infer_no_feats", "1", False))


def build(cfg, precision):
    kw = dict(visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model, nhead=cfg.nhead,
              num_layers=cfg.num_layers, input_modality=cfg.input_modality, data_modality=cfg.data_modality,
              num_feats=cfg.num_feats, include_verb_noun=cfg.include_verb_noun, precision=precision)
    if cfg.variant == "detection":
        from tim_amd.detection import TIM
        m = TIM(cfg.num_class, feedfoward_scale=cfg.feedforward_scale, **kw)
    else:
        from tim_amd.tim import TIM
        m = TIM(cfg.num_class, feedforward_scale=cfg.feedforward_scale, **kw)
    sd = {k: torch.from_numpy(v).float() for k, v in synth.make_state_dict(cfg, seed=2).items()}
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def forward(m, inp, nv, na):
    if m.cfg.variant == "detection":
        return m([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)[0]
    return m([inp["visual"], inp["audio"]], "encoder", m(inp["times"], "time_mlp"), nv, na)


def timed(fn, calls, repeats):
    """median over `repeats` windows of `calls` calls between two device events -> ms per call"""
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return statistics.median(ms), min(ms), max(ms)


def run_arm(cfg, B, nv, na, precision, infer, eval_feats, args):
    os.environ["TIM_AMD_INFER"] = infer
    m = build(cfg, precision)
    m.eval_feats = eval_feats
    inp = {k: torch.from_numpy(v).float().to(DEV) for k, v in synth.make_inputs(cfg, B, nv, na, seed=2).items()}
    res = {}
    with torch.no_grad():
        def eager():
            return forward(m, inp, nv, na)
        for _ in range(args.warmup):
            eager()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        eager()
        torch.cuda.synchronize()
        res["peak_allocated_bytes"] = torch.cuda.max_memory_allocated()
        med, lo, hi = timed(eager, args.calls, args.repeats)
        res["eager_ms"], res["eager_ms_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager()
        for _ in range(args.warmup):
            graph.replay()
        torch.cuda.synchronize()
        med, lo, hi = timed(graph.replay, args.calls, args.repeats)
        res["graph_ms"], res["graph_ms_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        del graph
    queries = B * (m.num_queries * (("visual" in cfg.data_modality) + ("audio" in cfg.data_modality))
                   if cfg.variant == "detection" else nv + na)
    res["interval_queries_per_s_eager"] = round(queries / res["eager_ms"] * 1e3)
    res["interval_queries_per_s_graph"] = round(queries / res["graph_ms"] * 1e3)
    del m, inp
    gc.collect()   # (a model is a reference cycle: without this the next arm's peak would include it)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls: at least 20 forwards per timed window")
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench: no GPU - a forward is only timed on the MI355X")
    keep = os.environ.get("TIM_AMD_INFER")
    out = {"tool": "infer_bench", "device": torch.cuda.get_device_name(0), "precision": args.precision, "calls": args.calls,
           "repeats": args.repeats, "workloads": {}}
    try:
        for name in args.workloads.split(","):
            cname, B, nv, na = WORKLOADS[name]
            cfg = named_config(cname)
            out["workloads"][name] = {"config": cname, "windows": B,
                                      "arms": {arm: run_arm(cfg, B, nv, na, args.precision, infer, feats, args)
                                               for arm, infer, feats in ARMS}}
    finally:
        if keep is None:
            os.environ.pop("TIM_AMD_INFER", None)
        else:
            os.environ["TIM_AMD_INFER"] = keep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
