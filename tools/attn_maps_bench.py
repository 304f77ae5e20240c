#!/usr/bin/env python3
"""What the attention maps cost: the evaluation forward with and without `model.attention_maps` (layers="last" and "all"), eager and
as a replayed graph, and the weights kernel alone - C2a at 64 and 8 windows, the C4 inference form at 16.  All variants of a
config run interleaved in one process, window after window, and the medians of the windows are reported (device events,
tools/_timing.py).  Kernel alone: microseconds and GB/s of the qkv it reads plus the map it writes.  One JSON line at the end.

    python tools/attn_maps_bench.py [--rounds 9] [--inner 10] [--precision fp16]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import captured, timed  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402

DEV = "cuda:0"


def build(cfg, precision):
    if cfg.variant == "detection":
        from tim_amd.detection import TIM
    else:
        from tim_amd.tim import TIM
    m = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
            nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, input_modality=cfg.input_modality,
            data_modality=cfg.data_modality, include_verb_noun=cfg.include_verb_noun, precision=precision)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=0).items()})
    return m.to(DEV).eval()


def variants(m, inp, nv, na):
    """name -> callable: the plain evaluation forward and the two map requests, eager and replayed"""
    det = m.cfg.variant == "detection"
    feats = [inp["visual"], inp["audio"]]

    def plain():
        with torch.no_grad():
            if det:
                return m(feats, "encoder", inp["times"], None, label_queries=False)
            return m(feats, "encoder", m(inp["times"], "time_mlp"), nv, na)

    def with_maps(layers, out=None):
        if det:
            return m.attention_maps(feats, inp["times"], None, layers=layers, out=out)[1]
        with torch.no_grad():
            te = m(inp["times"], "time_mlp")
        return m.attention_maps(feats, te, nv, na, layers=layers, out=out)[1]
    fns = {"plain": plain, "last": lambda: with_maps("last"), "all": lambda: with_maps("all")}
    held = {k: with_maps(k) for k in ("last", "all")}           # the replayed forms write into buffers made before the capture
    graphs = {"plain": captured(plain), "last": captured(lambda: with_maps("last", held["last"])),
              "all": captured(lambda: with_maps("all", held["all"]))}
    for k, g in graphs.items():
        fns[k + "_replay"] = g.replay
    return fns, held


def kernel_alone(cfg, B, S, precision):
    F, E, Hh = cfg.F, cfg.E, cfg.nhead
    dt = torch.float16 if precision == "fp16" else (torch.bfloat16 if precision == "bf16" else torch.float32)
    qkv = torch.randn((B * S, 3 * E), device=DEV).to(dt)
    w = torch.empty((B, S - F, F + 1), dtype=torch.float32, device=DEV)
    desc = L.TimDesc(B, S, F, cfg.d_model, E, Hh, cfg.FF, L.PRECISIONS[precision], 0.0, 0, 0, 0, None)
    lib = L.load()

    def run():
        L.check(lib.timhip_attention_weights(C.byref(desc), L.ptr(qkv), F, 0, L.ptr(w), F + 1, torch.cuda.current_stream().cuda_stream))
    return run, qkv.numel() * qkv.element_size() + w.numel() * 4


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--precision", default="fp16")
    args = ap.parse_args(argv)
    res = {"precision": args.precision, "rounds": args.rounds, "inner": args.inner, "configs": {}}
    for cname, B, nv, na in (("C2a", 64, 15, 10), ("C2a", 8, 15, 10), ("C4", 16, 0, 0)):
        cfg = named_config(cname)
        m = build(cfg, args.precision)
        inp = {k: torch.from_numpy(v).to(DEV) for k, v in synth.make_inputs(cfg, B, nv, na, seed=0).items()}
        fns, held = variants(m, inp, nv, na)
        S = held["last"].S
        fns["kernel"], nbytes = kernel_alone(cfg, B, S, args.precision)
        times = {k: [] for k in fns}
        for _ in range(args.rounds):                            # interleaved: one window of every variant per round
            for k, fn in fns.items():
                times[k].append(timed(fn, 1, args.inner)[0])
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {k + "_ms": round(med[k] / 1e3, 4) for k in med if k != "kernel"}
        row.update(kernel_us=round(med["kernel"], 2), kernel_GBps=round(nbytes / med["kernel"] / 1e3, 1), kernel_bytes=nbytes,
                   S=S, F=cfg.F, layers=cfg.num_layers)
        res["configs"]["%s/%d" % (cname, B)] = row
        print("%s at %d windows (S = %d): forward %.3f ms, +last %.3f, +all %.3f | replayed %.3f, +last %.3f, +all %.3f | "
              "kernel alone %.1f us, %.0f GB/s" % (cname, B, S, row["plain_ms"], row["last_ms"], row["all_ms"], row["plain_replay_ms"],
                                                   row["last_replay_ms"], row["all_replay_ms"], row["kernel_us"], row["kernel_GBps"]))
        del m, fns, held
        torch.cuda.empty_cache()
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
