#!/usr/bin/env python3
"""Batch assembly at C2a shapes: the device-side sampler against the host-fed form (needs the MI355X; one JSON line per batch size).

    python tools/sampler_bench.py [--windows 64 8] [--rounds 7] [--iters 200] [--store-gb 4] [--store-dtype fp32|fp16|bf16]

The batch of a C2a training iteration: visual [B, 50, 1024] and audio [B, 50, 2304] fp32 gathered from a feature store, times
[B, 125, 2], 15 + 10 queries with their labels and ids.  Forms, alternating for `rounds` rounds of `iters` calls each (device
events around the calls, after a warm-up of the same calls); the median and the spread (min, max) of the rounds are reported:

    device    WindowSampler.next_batch(): timhip_sampler_draw + timhip_window_batch, as replays of a captured graph and as
              back-to-back eager calls
    parent    ds.batch(host indices) and the copy_ into static tensors that examples/train_graphed_synthetic.py does in front of
              every replay; eager only (host indices and fresh outputs cannot be captured)
    kernels   timhip_sampler_draw + the three kernels batch() runs (timhip_window_gather x 2, timhip_window_times) reading the
              sampler's device words: the like-for-like floor of the fused launch, which moves the same bytes plus the labels
    draw      timhip_sampler_draw alone; "batch" = device - draw and "three" = kernels - draw are the assembly launches alone
    device16  (--store-dtype fp16 | bf16) `device` over the same tables with the feature stores held in that type
              (timhip_window_batch_st: half the bytes read, the same fp32 bytes written), in the same rounds as `device`, whose
              fp32 path is unchanged and is what the 16-bit figure is compared against; "batch16" = device16 - draw.  The size
              --store-gb names is that of the fp32 stores.  No pass mark on the ratio.

Every call of every form draws NEW windows, so with a store much larger than the 256 MB last-level cache (--store-gb, default 4)
the gathered rows come from HBM; --store-gb 0 runs the 64-window toy of the examples, whose 11 MB store stays in that cache.  The
outputs (43 MB at 64 windows) are rewritten by every call and stay cache-resident either way: the bytes/s figure counts one read
and one write of every gathered element and is a rate through that hierarchy, not an HBM stream rate.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd import _lib as L  # noqa: E402
from tim_amd._lib import ptr  # noqa: E402
from tim_amd.data import DeviceWindowDataset  # noqa: E402

NF, CV, CA, NV, NA = 50, 1024, 2304, 15, 10
STORE_DTYPES = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}


def narrow_store(ds, dtype):
    """the same dataset with its feature stores held in `dtype`, rounded once (every other table is shared)"""
    out = copy.copy(ds)
    out.v = dict(ds.v, feats=ds.v["feats"].to(dtype), dtype=dtype) if ds.v is not None else None
    out.a = dict(ds.a, feats=ds.a["feats"].to(dtype), dtype=dtype) if ds.a is not None else None
    return out


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
        fn()
    return g


def synthetic_store(dev, store_gb, seed=0):
    """a DeviceWindowDataset whose tables are made on the device: one long "video" of `rows` feature rows (one augmentation), W
    windows of 50 features at stride 2 starting anywhere in it.  store_gb = 0: 64 windows over 200 rows"""
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = 200 if store_gb <= 0 else int(store_gb * 2 ** 30 / ((CV + CA) * 4))
    W = 64 if store_gb <= 0 else 8192
    ds = DeviceWindowDataset.__new__(DeviceWindowDataset)
    L.load()
    ds.device, ds.num_feats, ds.window_size = dev, NF, NF * 0.4
    ds.max_visual_actions, ds.max_audio_actions, ds.model_modality, ds.has_v, ds.has_a = NV, NA, "audio_visual", True, True
    ft = torch.stack([torch.arange(rows, device=dev) * 0.2, torch.arange(rows, device=dev) * 0.2 + 1.0], 1).float().contiguous()
    ds.v = {"row0": {}, "num_aug": 1, "C": CV, "feats": torch.randn((rows, CV), device=dev, generator=g), "times": ft, "dtype": torch.float32}
    ds.a = {"row0": {}, "num_aug": 1, "C": CA, "feats": torch.randn((rows, CA), device=dev, generator=g), "times": ft.clone(),
            "dtype": torch.float32}
    first = torch.randint(0, rows - 2 * NF, (W,), device=dev, generator=g)
    ds.feat_indices = (first[:, None] + torch.arange(0, 2 * NF, 2, device=dev)[None]).to(torch.int32).contiguous()
    ds.start_sec = (first * 0.2).float()
    ds.v_row0 = torch.zeros(W, dtype=torch.int64, device=dev)
    ds.a_row0 = torch.zeros(W, dtype=torch.int64, device=dev)
    q = lambda n: (ds.start_sec[:, None, None] + torch.sort(torch.rand((W, n, 2), device=dev, generator=g) * NF * 0.4, dim=2).values).contiguous()   # noqa: E731
    ds.v_queries, ds.a_queries = q(NV), q(NA)
    ds.v_labels = torch.randint(0, 97, (W, NV, 4), device=dev, generator=g)
    ds.a_labels = torch.randint(0, 44, (W, NA, 4), device=dev, generator=g)
    ds.v_action_ids = torch.randint(0, 9999, (W, NV), device=dev, generator=g)
    ds.a_action_ids = torch.randint(0, 9999, (W, NA), device=dev, generator=g)
    ds.v_narration_ids, ds.a_narration_ids = [[""] * NV] * W, [[""] * NA] * W
    ds.num_windows = W
    return ds, (rows * (CV + CA) * 4) / 2 ** 30


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--store-gb", type=float, default=4.0)
    ap.add_argument("--store-dtype", choices=sorted(STORE_DTYPES), default="fp32", help="also time the sampler over stores held in this 16-bit type")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/sampler_bench.py needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds, store_gib = synthetic_store(dev, args.store_gb)
    dt16 = STORE_DTYPES[args.store_dtype]
    ds16 = narrow_store(ds, dt16) if dt16 is not None else None
    for B in args.windows:
        smp, ksmp = ds.sampler(B, seed=1), ds.sampler(B, seed=1)
        smp16 = ds16.sampler(B, seed=1) if ds16 is not None else None
        host = torch.Generator().manual_seed(B)
        T = 2 * NF + NV + NA
        static = {"visual": torch.empty((B, NF, CV), device=dev), "audio": torch.empty((B, NF, CA), device=dev), "times": torch.empty((B, T, 2), device=dev)}
        labels = {k: torch.empty((B, n), dtype=torch.int64, device=dev) for k, n in (("verb", NV), ("noun", NV), ("action", NV), ("class_id", NA))}
        kout = {k: torch.empty_like(v) for k, v in static.items()}
        st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

        def draw_only():
            s = ksmp
            L.call("timhip_sampler_draw", s.seed, ptr(s.counter), ds.num_windows, 1, 0, B, 1, L.SAMPLER_WRAP, NF, 1, 1, ptr(s.window), ptr(s.valid),
                   ptr(s.v_aug), ptr(s.a_aug), ptr(s.epoch), ptr(s.iteration), st())

        def parent_kernels():
            draw_only()
            s = ksmp
            L.call("timhip_window_gather", ptr(ds.v["feats"]), CV, 1, ptr(ds.v_row0), ptr(ds.feat_indices), NF, ptr(s.window), B, ptr(s.v_aug), ptr(kout["visual"]), st())
            L.call("timhip_window_gather", ptr(ds.a["feats"]), CA, 1, ptr(ds.a_row0), ptr(ds.feat_indices), NF, ptr(s.window), B, ptr(s.a_aug), ptr(kout["audio"]), st())
            L.call("timhip_window_times", ptr(ds.v["times"]), 2, ptr(ds.v_row0), ptr(ds.a["times"]), 2, ptr(ds.a_row0), ptr(ds.feat_indices), NF, ptr(s.window),
                   B, ptr(ds.v_queries), NV, ptr(ds.a_queries), NA, ptr(ds.start_sec), ds.window_size, ptr(kout["times"]), st())

        def parent_form():
            visual, audio, times, label, _ = ds.batch(torch.randint(0, len(ds), (B,), generator=host))
            for k, v in (("visual", visual), ("audio", audio), ("times", times)):
                static[k].copy_(v)
            for k in labels:
                labels[k].copy_(label[k])

        # same numbers first: the fused launch against the three kernels on one draw
        smp.next_batch()
        parent_kernels()
        torch.cuda.synchronize()
        assert torch.equal(smp.window, ksmp.window) and all(torch.equal(kout[k], getattr(smp, k)) for k in kout)
        forms = {"device": smp.next_batch, "kernels": parent_kernels, "draw": draw_only}
        if smp16 is not None:                           # same numbers: the fp32 batch rounded to the store type, widened
            smp16.next_batch()
            torch.cuda.synchronize()
            assert torch.equal(smp16.window, smp.window) and torch.equal(smp16.times, smp.times)
            assert all(torch.equal(getattr(smp16, k), getattr(smp, k).to(dt16).float()) for k in ("visual", "audio"))
            forms["device16"] = smp16.next_batch
        graphs = {n: graphed(f) for n, f in forms.items()}
        res = {"%s_%s" % (n, m): [] for n in forms for m in ("replay", "eager")}
        res["parent_eager"] = []
        for _ in range(args.rounds):
            for n, f in forms.items():
                res[n + "_replay"].append(timed(graphs[n].replay, args.iters))
                res[n + "_eager"].append(timed(f, args.iters))
            res["parent_eager"].append(timed(parent_form, args.iters))
        moved = 2 * B * NF * (CV + CA) * 4
        out = {"config": "C2a", "windows": B, "store_GiB": round(store_gib, 2), "dataset_windows": ds.num_windows, "gathered_MB": round(moved / 2e6, 2),
               "rounds": args.rounds, "iters": args.iters}
        for n, v in res.items():
            out[n + "_us"] = round(statistics.median(v), 2)
            out[n + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        batch = [d - w for d, w in zip(res["device_replay"], res["draw_replay"])]
        three = [k - w for k, w in zip(res["kernels_replay"], res["draw_replay"])]
        out["batch_replay_us"], out["three_replay_us"] = round(statistics.median(batch), 2), round(statistics.median(three), 2)
        out["batch_replay_us_min_max"], out["three_replay_us_min_max"] = [round(min(batch), 2), round(max(batch), 2)], [round(min(three), 2), round(max(three), 2)]
        out["batch_minus_three_us"] = round(out["batch_replay_us"] - out["three_replay_us"], 2)
        out["three_spread_us"] = round(max(three) - min(three), 2)
        out["fused_within_spread"] = bool(out["batch_minus_three_us"] <= out["three_spread_us"])
        # (a difference of two launch-bound times of a few us is noise: no rate from it)
        out["batch_read_write_GBps"] = round(moved / (out["batch_replay_us"] * 1e-6) / 1e9, 1) if out["batch_replay_us"] >= 5.0 else None
        out["replay_vs_parent_speedup"] = round(out["parent_eager_us"] / out["device_replay_us"], 2)
        if smp16 is not None:
            b16 = [d - w for d, w in zip(res["device16_replay"], res["draw_replay"])]
            out["store_dtype"], out["store16_GiB"] = args.store_dtype, round(ds16.store_bytes() / 2 ** 30, 2)
            out["batch16_replay_us"], out["batch16_replay_us_min_max"] = round(statistics.median(b16), 2), [round(min(b16), 2), round(max(b16), 2)]
            out["batch16_over_batch"] = round(out["batch16_replay_us"] / out["batch_replay_us"], 3) if out["batch_replay_us"] >= 5.0 else None
            out["device16_over_device_replay"] = round(out["device16_replay_us"] / out["device_replay_us"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
