"""Golden vectors for the detection inference tail from the reference's own code (build container only).

    python tests/golden/make_golden_detect.py

Runs the reference's FeatureMeter.update / finalize_metrics (detection/time_interval_machine/utils/meters.py) and
eval_detection/format_predictions.py main() on seeded synthetic logits / regressions: 3 batches of 2 windows, 3 videos of
which one spans two batches, Nq = 19 queries, C = 23 classes, with proposals that clamp at both ends, that round to zero
width, that are reversed and that sit on a rounding tie, and window starts with more than three decimals.  fvcore and
simplejson are stubbed (only a timer and a logger are asked of them), the memory probes of utils/misc.py are replaced (they
query a GPU), nms_1d_cpu is compiled where it lies into oracle/_ref/ (git-ignored) as make_golden_nms.py does, main() runs
in a temporary directory with n_jobs=1 and its final subprocess.run (the scoring script) patched out.

tests/golden/detect_small.npz holds the seeds, the inputs, the candidate list main() handed to its NMS (recorded by a
wrapper around filter_nms) and the final `results` of its submission file - numbers only, nothing of the reference.
"""
import argparse
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch.utils.cpp_extension import load

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/detection"

# ---- stubs for what is not installed / needs a GPU
sj = types.ModuleType("simplejson")
sj.dumps = lambda *a, **k: ""
sys.modules["simplejson"] = sj
for name in ("fvcore", "fvcore.common", "fvcore.common.file_io", "fvcore.common.timer"):
    sys.modules[name] = types.ModuleType(name)


class _PM:
    open = staticmethod(open)


class _Timer:
    def seconds(self):
        return 0.0

    def reset(self):
        pass

    def pause(self):
        pass


sys.modules["fvcore.common.file_io"].PathManager = _PM
sys.modules["fvcore.common.timer"].Timer = _Timer
sys.path.insert(0, REF)
import time_interval_machine.utils.misc as ref_misc  # noqa: E402
from time_interval_machine.utils.meters import FeatureMeter  # noqa: E402

ref_misc.gpu_mem_usage = lambda: (0.0, 0.0)
ref_misc.cpu_mem_usage = lambda: (0.0, 0.0)

bdir = os.path.join(ROOT, "oracle", "_ref")
os.makedirs(bdir, exist_ok=True)
ext = load(name="nms_1d_cpu", sources=[os.path.join(REF, "eval_detection", "csrc", "nms_cpu.cpp")], build_directory=bdir,
           extra_cflags=["-O2", "-fopenmp"], verbose=False)
sys.modules["nms_1d_cpu"] = ext
sys.path.insert(0, os.path.join(REF, "eval_detection"))
import format_predictions as fp  # noqa: E402

SEED, NB, B, NQ, C = 20261, 3, 2, 19, 23
THRESHOLD, SIGMA = 0.01, 0.1
WINDOW_SIZE = 10.24                                     # not an fp32 number: the product is taken with its fp32 rounding
VIDEOS = [["P03_01", "P03_01"], ["P03_01", "P01_07"], ["P02_05", "P02_05"]]      # first-seen order differs from sorted order
STARTS = [[1.0625, 12.3456789], [17.4657913, 3000.1234567], [0.0004999, 2.7182818]]


def make_inputs():
    rng = np.random.default_rng(SEED)
    ws32 = np.float32(WINDOW_SIZE)
    # query pyramid of one window (the same for every window, as the model's inference queries are); its maximum is below 1
    centre = rng.uniform(0.05, 0.9, size=NQ)
    half = rng.uniform(0.01, 0.07, size=NQ)
    queries = np.stack([centre - half, centre + half], axis=1).clip(0.0, 0.97).astype(np.float32)
    logits = (rng.normal(-6.3, 1.6, size=(NB, B * NQ, C))).astype(np.float32)
    reg = np.tile(queries, (NB, B, 1)).astype(np.float32) + rng.normal(0, 0.02, size=(NB, B * NQ, 2)).astype(np.float32)
    # ---- crafted proposals (batch 0, window 0 starts at 1.0625)
    reg[0, 0] = (-0.3, 1.4)                               # clamps at both ends
    reg[0, 1] = (0.41, 0.41001)                          # rounds to zero width
    reg[0, 2] = (0.6, 0.4)                                # reversed
    # rounding tie: an fp32 product of exactly 2.0 (resp. 3.0) + 1.0625 = x.0625 -> x062.5 after scaling: half-even keeps x062
    def with_product(target):
        r = np.float32(target / float(ws32))
        for _ in range(8):
            for cand in (r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(9))):
                if np.float32(cand * ws32) == np.float32(target):
                    return cand
            r = np.nextafter(r, np.float32(9))
        raise AssertionError("no fp32 factor found")
    reg[0, 3] = (with_product(2.0), with_product(3.0))
    reg[0, 4, 0] = with_product(2.0)
    reg[1, NQ + 5] = (0.1, 1.2)                           # upper clamp in the window that starts at 3000.1234567
    reg[2, 7] = (-0.2, 0.3)                               # lower clamp
    logits[0, 0:5] += 1.5                                 # make sure the crafted rows carry candidates
    logits[1, NQ + 5] += 1.5
    logits[2, NQ:2 * NQ, :] -= 1.0
    logits[2, NQ + 3] = -20.0                             # a proposal with no class over the threshold
    logits[2, NQ + 4] = 3.0 + 0.01 * np.arange(C)         # and one with all of them (no two scores equal)
    # no score within 1e-5 of the threshold
    s = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    near = np.abs(s - THRESHOLD) < 1e-5
    logits[near] += np.float32(0.01)
    s = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    assert not (np.abs(s - THRESHOLD) < 1e-5).any()
    return queries, logits, reg


def main():
    queries, logits, reg = make_inputs()
    args = argparse.Namespace(data_modality="visual", include_verb_noun=False, num_class=[C, 5])
    meter = FeatureMeter(args)
    qt = torch.from_numpy(queries)[None].repeat(B, 1, 1)                 # [B, Nq, 2]
    for b in range(NB):
        metadata = {"video_id": list(VIDEOS[b]),
                    "window_start": torch.tensor(STARTS[b], dtype=torch.float64),          # what default_collate makes of
                    "window_size": torch.tensor([WINDOW_SIZE] * B, dtype=torch.float64)}   # Python floats
        meter.update((None, None, torch.from_numpy(logits[b]), None), (torch.from_numpy(reg[b]), None), (qt, None), metadata)
    data = meter.finalize_metrics()

    recorded = {}
    orig_filter = fp.filter_nms

    def recording_filter(results_in_vid, vid, **kw):
        recorded[vid] = [(int(d["action"]), np.float32(d["score"]), float(d["segment"][0]), float(d["segment"][1]))
                         for d in results_in_vid]
        return orig_filter(results_in_vid=results_in_vid, vid=vid, **kw)

    fp.filter_nms = recording_filter
    fp.subprocess = types.SimpleNamespace(run=lambda *a, **k: None)
    orig_load = torch.load
    fp.torch.load = lambda f, **k: orig_load(f, weights_only=False, **k)   # the file holds numpy arrays (pickled objects)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            torch.save(data, "preds.pt")
            fp.main(argparse.Namespace(path_to_preds="preds.pt", path_to_gt="", score_threshold=THRESHOLD, sigma=SIGMA,
                                       is_audio=False, n_jobs=1))
            results = json.load(open("tim.json"))["results"]
        finally:
            os.chdir(cwd)
            fp.torch.load = orig_load
            fp.filter_nms = orig_filter

    names = sorted(set(v for row in VIDEOS for v in row))
    cand = [(names.index(v),) + e for v in names for e in recorded.get(v, [])]
    res = [(names.index(v), int(e["action"]), float(e["score"]), float(e["segment"][0]), float(e["segment"][1]))
           for v in names for e in results[v]]
    for v in names:                                       # no two final scores of a video tie
        sc = [e["score"] for e in results[v]]
        assert len(set(sc)) == len(sc), v
    out = os.path.join(HERE, "detect_small.npz")
    np.savez_compressed(
        out, seed=SEED, threshold=THRESHOLD, sigma=SIGMA, window_size=WINDOW_SIZE, num_queries=NQ,
        queries=queries, logits=logits, reg=reg, window_start=np.asarray(STARTS, np.float64),
        video_ids=np.asarray(VIDEOS), video_names=np.asarray(names),
        v_proposals=data["v_proposals"].astype(np.float64),
        cand_video=np.asarray([c[0] for c in cand], np.int64), cand_class=np.asarray([c[1] for c in cand], np.int64),
        cand_score=np.asarray([c[2] for c in cand], np.float32),
        cand_seg=np.asarray([[c[3], c[4]] for c in cand], np.float64).reshape(-1, 2),
        res_video=np.asarray([r[0] for r in res], np.int64), res_class=np.asarray([r[1] for r in res], np.int64),
        res_score=np.asarray([r[2] for r in res], np.float64),
        res_seg=np.asarray([[r[3], r[4]] for r in res], np.float64).reshape(-1, 2))
    print("proposals", data["v_proposals"].shape, data["v_proposals"].dtype, "candidates", len(cand), "detections", len(res),
          "->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
