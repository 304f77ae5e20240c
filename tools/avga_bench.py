#!/usr/bin/env python3
"""AVGA pooling at the AVE shape: the device route (tim_amd/csrc/avga.hip) against the stock torch ops (TIM_AMD_AVGA=0) in one
process, interleaved.

    python tools/avga_bench.py [--reps 7] [--inner 10] [--precision fp16] [--batches 64 8]

Per batch size (T = 10 feature steps, 7 x 7 cells of Cv = 512, Ca = 128): forward (no_grad) and forward + backward (the seven
parameter gradients) of `model.pool`, device events around `inner` calls, median (min - max) over `reps` windows in which the
two routes alternate; peak allocated bytes of one forward + backward per route (workspaces included); the forward's share of
the one-read byte floor (the fp32 cells once at the HBM rate this project measures, 4.4 - 5 TB/s); and the outputs of the two
routes compared on the same inputs.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tim_amd.tim import TIM  # noqa: E402

T, S, CV, CA = 10, 49, 512, 128
HBM_LO, HBM_HI = 4.4e12, 5.0e12


def timed(fns, reps, inner):
    """fns: {name: callable}; every window runs each of them `inner` times, in turn -> {name: [us per call, per window]}"""
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / inner)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8])
    args = ap.parse_args(argv)
    assert args.reps >= 5
    assert torch.cuda.is_available(), "tools/avga_bench.py measures on the MI355X; there is nothing to time without it"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = TIM([28, 28], visual_input_dim=CV, audio_input_dim=CA, d_model=256, nhead=8, num_layers=1, num_feats=T,
                include_verb_noun=False, pool_features=True, precision=args.precision).to(dev)
    pool = model.pool
    print("AVGA pooling, T = %d, S = %d, Cv = H = %d, Ca = %d, precision %s; microseconds per call, median (min - max) of %d "
          "windows of %d calls, the two routes alternating inside every window" % (T, S, CV, CA, args.precision, args.reps, args.inner))
    for B in args.batches:
        R = B * T
        g = torch.Generator().manual_seed(B)
        video = torch.randn(B, T, 7, 7, CV, generator=g).abs().to(dev)
        audio = torch.randn(B, T, CA, generator=g).to(dev)
        cot = torch.randn(B, T, CV, generator=g).to(dev)
        in_bytes = video.numel() * 4
        flops = 2.0 * R * S * (CV * CV + S * CV)

        def run(env, grad):
            os.environ["TIM_AMD_AVGA"] = env
            if not grad:
                with torch.no_grad():
                    return pool(audio, video)
            for p in pool.parameters():
                p.grad = None
            out = pool(audio, video)
            out.backward(cot)
            return out

        res = {}
        for env, name in (("1", "device"), ("0", "torch")):
            for _ in range(3):                        # warm-up: code objects, operand copies, workspaces, the BLAS picks
                run(env, False); run(env, True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = run(env, True)
            torch.cuda.synchronize()
            res[name] = (out.detach().clone(), {n: p.grad.detach().clone() for n, p in pool.named_parameters()},
                         torch.cuda.max_memory_allocated() - base)
        od, ot = res["device"][0], res["torch"][0]
        print("\nB = %d (R = %d pooled rows): input %.1f MB fp32, %.2f GFLOP; one-read floor %.1f - %.1f us"
              % (B, R, in_bytes / 1e6, flops / 1e9, in_bytes / HBM_HI * 1e6, in_bytes / HBM_LO * 1e6))
        print("  outputs, device vs torch route: max |diff| / max |out| %.2e; parameter gradients, max |diff| / max |grad|: %s"
              % ((od - ot).abs().max().item() / ot.abs().max().item(),
                 ", ".join("%s %.1e" % (n.replace("affine_", ""), (res["device"][1][n] - res["torch"][1][n]).abs().max().item()
                                        / res["torch"][1][n].abs().max().item()) for n in res["torch"][1])))
        print("  peak allocated bytes above the resident set, one forward + backward: device %.1f MB (its workspaces are resident "
              "after the warm-up: %.1f MB), torch %.1f MB"
              % (res["device"][2] / 1e6, sum(w.numel() for k, w in model._ws.items() if k[1].startswith("avga")) / 1e6,
                 res["torch"][2] / 1e6))
        t = timed({"device fwd": lambda: run("1", False), "torch  fwd": lambda: run("0", False),
                   "device fwd+bwd": lambda: run("1", True), "torch  fwd+bwd": lambda: run("0", True)}, args.reps, args.inner)
        for k, v in t.items():
            med = statistics.median(v)
            extra = ""
            if k == "device fwd":
                extra = "   %.2f TB/s of the input read once = %.0f - %.0f %% of the one-read floor; %.1f TFLOP/s" % (
                    in_bytes / med / 1e6, in_bytes / HBM_HI * 1e6 / med * 100, in_bytes / HBM_LO * 1e6 / med * 100, flops / med / 1e6)
            print("  %-16s %10.1f (%.1f - %.1f)%s" % (k, med, min(v), max(v), extra))
        for kind in ("fwd", "fwd+bwd"):
            print("  %-7s torch / device = %.2f" % (kind, statistics.median(t["torch  " + kind]) / statistics.median(t["device " + kind])))
    os.environ.pop("TIM_AMD_AVGA", None)


if __name__ == "__main__":
    main()
