#!/usr/bin/env python3
"""Detection batch assembly at the C4 training shape: the device-side sampler against the host-fed form (needs the MI355X; one
JSON line per batch size).

    python tools/det_sampler_bench.py [--windows 16] [--rounds 7] [--iters 200] [--store-gb 4] [--store-dtype fp32|fp16|bf16]

The batch of bench.py's `c4_train` iteration: 16 windows, visual only, visual [B, 50, 2048] fp32 gathered from a feature store,
times [B, 50, 2], 6 ground-truth segments per window with verb / noun / action, window start and video index.  Forms,
alternating for `rounds` rounds of `iters` calls each (device events around the calls, after a warm-up of the same calls); the
median and the spread (min, max) of the rounds are reported:

    device    DetectionWindowSampler.next_batch(): timhip_sampler_draw + timhip_det_window_batch, as replays of a captured graph
              and as back-to-back eager calls
    host      what a user of this package has without the detection dataset class: host indices and augmentation draws, the
              batch built from the same device tables with torch ops (`host_form` below: index gathers, torch.round(decimals=3),
              clamp, the padding mask), then the copy_ into the static inputs of a captured step; eager only
    draw      timhip_sampler_draw alone; "batch" = device - draw is the assembly launch alone, reported against the bytes it moves
              (one read and one write of every gathered feature element)
    device16  (--store-dtype fp16 | bf16) `device` over the same tables with the feature store held in that type
              (timhip_det_window_batch_st: half the bytes read, the same fp32 bytes written), in the same rounds as `device`,
              whose fp32 path is unchanged and is what the 16-bit figure is compared against; "batch16" = device16 - draw.  The
              size --store-gb names is that of the fp32 store.  No pass mark on the ratio.

Every call of every form draws NEW windows, so with a store much larger than the 256 MB last-level cache (--store-gb, default 4)
the gathered rows come from HBM.  The outputs (6.6 MB at 16 windows) are rewritten by every call and stay cache-resident: the
bytes/s figure is a rate through that hierarchy, not an HBM stream rate.  No pass mark: the numbers go to docs/measurement_log.md.
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
from tim_amd.det_data import DeviceDetectionDataset  # noqa: E402

NF, CV, NGT, NUM_AUG = 50, 2048, 6, 1
STORE_DTYPES = {"fp32": None, "fp16": torch.float16, "bf16": torch.bfloat16}


def narrow_store(ds, dtype):
    """the same dataset with its feature store held in `dtype`, rounded once (every other table is shared)"""
    out = copy.copy(ds)
    out.v = dict(ds.v, feats=ds.v["feats"].to(dtype), dtype=dtype)
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
    """a DeviceDetectionDataset whose tables are made on the device: 4 "videos" sharing `rows` feature rows (one augmentation), W
    windows of 50 features at stride 2 starting anywhere in their video, 1 to 6 actions each.  store_gb = 0: 64 windows over 800 rows"""
    g = torch.Generator(device=dev).manual_seed(seed)
    rows = 800 if store_gb <= 0 else int(store_gb * 2 ** 30 / (CV * 4))
    W, n_vid = (64 if store_gb <= 0 else 8192), 4
    per = rows // n_vid
    ds = DeviceDetectionDataset.__new__(DeviceDetectionDataset)
    L.load()
    ds.device, ds.num_feats, ds.window_size = dev, NF, NF * 0.4
    ds.max_visual_actions, ds.max_audio_actions, ds.model_modality, ds.has_v, ds.has_a = NGT, 0, "visual", True, False
    ds.dataset_name, ds.include_verb_noun, ds.verb_only, ds.action_col = "epic", False, True, 0
    ds.video_ids = ["vid%02d" % i for i in range(n_vid)]
    t = (torch.arange(rows, device=dev) % per) * 0.2
    ds.v = {"row0": {}, "num_aug": NUM_AUG, "C": CV, "feats": torch.randn((rows * NUM_AUG, CV), device=dev, generator=g),
            "times": torch.stack([t, t + 1.0], 1).float().contiguous(), "dtype": torch.float32}
    ds.a = None
    video = torch.randint(0, n_vid, (W,), device=dev, generator=g)
    first = torch.randint(0, per - 2 * NF, (W,), device=dev, generator=g)
    ds.feat_indices = (first[:, None] + torch.arange(0, 2 * NF, 2, device=dev)[None]).to(torch.int32).contiguous()
    ds.window_start_sec = first.double() * 0.2
    ds.start_sec = ds.window_start_sec.float()
    ds.video_of, ds.window_video = video.to(torch.int32), video.tolist()
    ds.v_row0, ds.a_row0 = (video * per).to(torch.int64), None
    count = torch.randint(1, NGT + 1, (W,), device=dev, generator=g)
    pad = torch.arange(NGT, device=dev)[None] >= count[:, None]
    seg = ds.start_sec[:, None, None] + torch.sort(torch.rand((W, NGT, 2), device=dev, generator=g) * NF * 0.4, dim=2).values
    ds.v_segments = seg.masked_fill(pad[..., None], 0.0).contiguous()
    lab = torch.cat([torch.randint(0, 97, (W, NGT, 1), device=dev, generator=g), torch.randint(0, 300, (W, NGT, 1), device=dev, generator=g),
                     torch.randint(0, 3806, (W, NGT, 1), device=dev, generator=g), torch.full((W, NGT, 1), -1, device=dev)], 2)
    ds.v_labels = lab.masked_fill(pad[..., None], -1).contiguous()
    ds.a_segments, ds.a_labels = torch.zeros((W, 0, 2), device=dev), torch.full((W, 0, 4), -1, dtype=torch.int64, device=dev)
    ds.num_windows = W
    return ds, (rows * CV * 4) / 2 ** 30


def host_form(ds, win, aug):
    """The detection batch from window numbers and augmentation indices with torch ops on the device tables: what
    timhip_det_window_batch fuses (visual only).  -> (visual, times, label, window_start, video_index)"""
    ws = ds.window_size
    rows = ds.v_row0[win][:, None] + ds.feat_indices[win].long()                   # [B, nf] rows of the store
    visual = ds.v["feats"].view(-1, ds.v["num_aug"], ds.v["C"])[rows, aug]
    start = ds.start_sec[win][:, None, None]
    norm = lambda x: torch.clamp(torch.round(x - start, decimals=3) / ws, min=0.0)   # noqa: E731
    lab = ds.v_labels[win]
    pad = (lab == -1).all(-1)
    label = {"v_gt_segments": norm(ds.v_segments[win]).masked_fill(pad[..., None], 0.0), "verb": lab[..., 0], "noun": lab[..., 1],
             "action": lab[..., ds.action_col]}
    return visual, norm(ds.v["times"][rows]), label, ds.window_start_sec[win], ds.video_of[win]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--store-gb", type=float, default=4.0)
    ap.add_argument("--store-dtype", choices=sorted(STORE_DTYPES), default="fp32", help="also time the sampler over a store held in this 16-bit type")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("tools/det_sampler_bench.py needs the GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ds, store_gib = synthetic_store(dev, args.store_gb)
    dt16 = STORE_DTYPES[args.store_dtype]
    ds16 = narrow_store(ds, dt16) if dt16 is not None else None
    for B in args.windows:
        smp, ksmp = ds.sampler(B, seed=1), ds.sampler(B, seed=1)
        smp16 = ds16.sampler(B, seed=1) if ds16 is not None else None
        host = torch.Generator().manual_seed(B)
        static = {"visual": torch.empty_like(smp.visual), "times": torch.empty_like(smp.times), "window_start": torch.empty_like(smp.metadata["window_start"]),
                  "video_index": torch.empty_like(smp.metadata["video_index"])}
        static.update({k: torch.empty_like(smp.label[k]) for k in ("v_gt_segments", "verb", "noun", "action")})
        st = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

        def draw_only():
            s = ksmp
            L.call("timhip_sampler_draw", s.seed, ptr(s.counter), ds.num_windows, 1, 0, B, 1, L.SAMPLER_WRAP, NF, NUM_AUG, 0, ptr(s.window), ptr(s.valid),
                   ptr(s.v_aug), None, ptr(s.epoch), ptr(s.iteration), st())

        def host_fed():
            win = torch.randint(0, len(ds), (B,), generator=host).to(dev)           # host indices, host augmentation draw
            aug = torch.randint(0, NUM_AUG, (B, NF), generator=host).to(dev)
            visual, times, label, start, vidx = host_form(ds, win, aug)
            for k, v in (("visual", visual), ("times", times), ("window_start", start), ("video_index", vidx), *label.items()):
                static[k].copy_(v)

        # same numbers first: the fused launch against the torch form on one draw (reported, both are restatements of one contract)
        smp.next_batch()
        visual, times, label, start, vidx = host_form(ds, smp.window.long(), smp.v_aug.long())
        torch.cuda.synchronize()
        pairs = {"visual": (visual, smp.visual), "times": (times, smp.times), "window_start": (start, smp.metadata["window_start"]),
                 "video_index": (vidx, smp.metadata["video_index"]), **{k: (label[k], smp.label[k]) for k in label}}
        # the copies and labels are equal; times and segments need not be: torch divides a tensor by a host scalar ON THE DEVICE as
        # a product with the scalar's reciprocal, the reference's CPU division (and the kernel) is one IEEE division
        same = {k: bool(torch.equal(a, b)) for k, (a, b) in pairs.items()}
        same["times_max_abs_diff"] = float((times - smp.times).abs().max())
        forms = {"device": smp.next_batch, "draw": draw_only}
        if smp16 is not None:                           # same numbers: the fp32 batch rounded to the store type, widened
            smp16.next_batch()
            torch.cuda.synchronize()
            assert torch.equal(smp16.window, smp.window) and torch.equal(smp16.times, smp.times)
            assert torch.equal(smp16.visual, smp.visual.to(dt16).float())
            assert all(torch.equal(smp16.label[k], smp.label[k]) for k in smp.label)
            forms["device16"] = smp16.next_batch
        graphs = {n: graphed(f) for n, f in forms.items()}
        res = {"%s_%s" % (n, m): [] for n in forms for m in ("replay", "eager")}
        res["host_eager"] = []
        for _ in range(args.rounds):
            for n, f in forms.items():
                res[n + "_replay"].append(timed(graphs[n].replay, args.iters))
                res[n + "_eager"].append(timed(f, args.iters))
            res["host_eager"].append(timed(host_fed, args.iters))
        moved = 2 * B * NF * CV * 4
        out = {"config": "C4 train", "windows": B, "store_GiB": round(store_gib, 2), "dataset_windows": ds.num_windows, "gathered_MB": round(moved / 2e6, 2),
               "rounds": args.rounds, "iters": args.iters, "torch_form_equal": same}
        for n, v in res.items():
            out[n + "_us"] = round(statistics.median(v), 2)
            out[n + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
        batch = [d - w for d, w in zip(res["device_replay"], res["draw_replay"])]
        out["batch_replay_us"], out["batch_replay_us_min_max"] = round(statistics.median(batch), 2), [round(min(batch), 2), round(max(batch), 2)]
        # (a difference of two launch-bound times of a few us is noise: no rate from it)
        out["batch_read_write_GBps"] = round(moved / (out["batch_replay_us"] * 1e-6) / 1e9, 1) if out["batch_replay_us"] >= 5.0 else None
        out["replay_vs_host_speedup"] = round(out["host_eager_us"] / out["device_replay_us"], 2)
        if smp16 is not None:
            b16 = [d - w for d, w in zip(res["device16_replay"], res["draw_replay"])]
            out["store_dtype"], out["store16_GiB"] = args.store_dtype, round(ds16.store_bytes() / 2 ** 30, 2)
            out["batch16_replay_us"], out["batch16_replay_us_min_max"] = round(statistics.median(b16), 2), [round(min(b16), 2), round(max(b16), 2)]
            out["batch16_over_batch"] = round(out["batch16_replay_us"] / out["batch_replay_us"], 3) if out["batch_replay_us"] >= 5.0 else None
            out["device16_over_device_replay"] = round(out["device16_replay_us"] / out["device_replay_us"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
