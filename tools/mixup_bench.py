#!/usr/bin/env python3
"""Mixup of the inputs at C2a: the torch-op form against tim_amd.mixup (needs the MI355X; prints one JSON line per batch size).

    python tools/mixup_bench.py [--windows 64 8] [--rounds 7] [--iters 200]

Both sides mix the three input tensors of a C2a training iteration (visual [B, 50, 1024], audio [B, 50, 2304], time encodings
[B, 125, 512], fp32) and permute the four target tensors:

    torch   three torch.lerp(t[perm], t, lam) (a gather pass and a lerp pass per tensor) + four target gathers, lam a Python
            float and perm a device tensor drawn ONCE - the form bench.py's rec_train_step times, and all a captured step can do
    device  Mixup.draw() + Mixup.mix([...]) + Mixup.targets(...): one draw launch, one apply launch, the gathers; redrawn per call

Each side is timed as replays of a captured graph and as back-to-back eager launches (device events around `iters` calls,
after a warm-up of the same calls), the two sides alternating for `rounds` rounds; the median and the spread of the rounds are
reported.  "apply" is the apply launch alone under replay, with its bytes/s against the three-pass count (two reads and one
write of every element).  The inputs of 64 windows (59 MB) fit the chip's 256 MB last-level cache, so that figure is a rate
through the cache hierarchy of a hot working set, not an HBM rate.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd.config import named_config  # noqa: E402
from tim_amd.mixup import Mixup  # noqa: E402


def timed(fn, iters):
    """microseconds per call: device events around `iters` calls, after `iters // 4` warm-up calls"""
    for _ in range(max(3, iters // 4)):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/mixup_bench.py needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    cfg = named_config("C2a")
    nv, na, nf = 15, 10, cfg.num_feats
    for B in args.windows:
        g = torch.Generator().manual_seed(B)
        x = [torch.randn((B, nf, cfg.visual_input_dim), generator=g).to(dev), torch.randn((B, nf, cfg.audio_input_dim), generator=g).to(dev),
             torch.randn((B, 2 * nf + nv + na, cfg.d_model), generator=g).to(dev)]
        tgt = {k: torch.randint(0, 40, (B, n), generator=g).to(dev) for k, n in (("verb", nv), ("noun", nv), ("action", nv), ("class_id", na))}
        perm, lam = torch.randperm(B, generator=g).to(dev), 0.37
        mix = Mixup(B, alpha=0.2, device=dev, seed=0)

        def torch_form():
            return [torch.lerp(t[perm], t, lam) for t in x], {k: v[perm] for k, v in tgt.items()}

        def device_form():
            mix.draw()
            return mix.mix(x), mix.targets(tgt)[1]

        def apply_only():
            return mix.mix(x)

        # same numbers first (section 6 of the measuring rules): the device form at the torch form's lam and permutation
        mix.set(lam, perm.cpu())
        for a, b in zip(torch_form()[0], mix.mix(x)):
            err = (a - b).abs().max().item()
            assert err <= 4 * 2.0 ** -24 * 2 * a.abs().max().item(), err
        graphs = {n: graphed(f) for n, f in (("torch", torch_form), ("device", device_form), ("apply", apply_only))}
        res = {n: {"replay": [], "eager": []} for n in graphs}
        for _ in range(args.rounds):
            for n, f in (("torch", torch_form), ("device", device_form), ("apply", apply_only)):
                res[n]["replay"].append(timed(graphs[n][0].replay, args.iters))
                res[n]["eager"].append(timed(f, args.iters))
        nbytes = 3 * sum(t.numel() * t.element_size() for t in x)
        out = {"config": "C2a", "windows": B, "input_MB": round(nbytes / 3e6, 2), "rounds": args.rounds, "iters": args.iters}
        for n in res:
            for mode in ("replay", "eager"):
                v = res[n][mode]
                out["%s_%s_us" % (n, mode)] = round(statistics.median(v), 2)
                out["%s_%s_us_min_max" % (n, mode)] = [round(min(v), 2), round(max(v), 2)]
        out["replay_speedup"] = round(out["torch_replay_us"] / out["device_replay_us"], 3)
        out["eager_speedup"] = round(out["torch_eager_us"] / out["device_eager_us"], 3)
        out["apply_three_pass_bytes"] = nbytes
        out["apply_GBps_replay"] = round(nbytes / (out["apply_replay_us"] * 1e-6) / 1e9, 1)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
