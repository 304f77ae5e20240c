"""Golden vectors for the two-stream detection fusion from the reference's own code (build container only).

    python tests/golden/make_golden_twostream.py

Runs the reference's FeatureMeter.update / finalize_metrics (detection/time_interval_machine/utils/meters.py) once per
stream on seeded synthetic logits / regressions, saves the two files and runs eval_detection/
format_two_stream_predictions_epic.py main() on them: 3 batches of 2 windows, 3 videos of which one spans two batches,
Nq = 19 queries, Cv = 11 verbs, Cn = 23 nouns; rows where only the verb passes, only the noun passes, where the blend of the
two segments is reversed or rounds to zero width, both clamps and a window start above 3000 s.  Three result sets:
top_k = 1 and top_k = 3 at the reference's verb_alpha 0.65, and top_k = 2 at verb_alpha 1.3 - for 0 <= alpha <= 1 the fused
score is a weighted geometric mean and cannot fall below the smaller of two scores that both passed, so the case "both pass,
the fused score fails" exists only outside that range.  Stubs and the compiled nms_1d_cpu as in make_golden_detect.py; main()
runs in a temporary directory with n_jobs=1, its final subprocess.run (the scoring script) patched out and filter_nms
wrapped to record the candidate list.

The maker asserts the conditions under which the reference is well defined (no tie at the k boundary of a row, no score
within 1e-5 of the threshold, no blended endpoint within 1e-3 ms of a rounding tie, no two final scores of a video equal)
and measures how far the restatement's float64 forms (tests/twostream_ref.py) are from the reference's torch sigmoid and
libm powf: `max_ulp_vs_reference`.

tests/golden/twostream_small.npz holds the seed, the NumPy version, the inputs, the candidate lists and the final `results`
- numbers only, nothing of the reference.
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

from tests import twostream_ref as T  # noqa: E402
from tests.detect_ref import sigmoid32  # noqa: E402

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
import format_two_stream_predictions_epic as fp  # noqa: E402

assert (np.float32(.3) ** 0.65).dtype == np.float32         # NEP 50: the reference's scalars stay fp32 (NumPy >= 2)

SEED, NB, B, NQ, CV, CN = 20262, 3, 2, 19, 11, 23
THRESHOLD, SIGMA = 0.03, 0.25
SETS = {"k1": (1, 0.65), "k3": (3, 0.65), "k2a": (2, 1.3)}      # name -> (top_k, verb_alpha)
KMAX = 3
WINDOW_SIZE = 10.24                                     # not an fp32 number: the product is taken with its fp32 rounding
VIDEOS = [["P03_01", "P03_01"], ["P03_01", "P01_07"], ["P02_05", "P02_05"]]      # first-seen order differs from sorted order
STARTS = [[1.0625, 12.3456789], [17.4657913, 3000.1234567], [0.0004999, 2.7182818]]
LOGIT_THR = float(np.log(THRESHOLD / (1 - THRESHOLD)))


def _pairs(vl, nl, vr, nr, queries, alpha):
    """all KMAX x KMAX pairs of every row of every batch with the restatement: (vs, ns, score, unrounded blend)"""
    out = []
    for b in range(NB):
        sv, sn = sigmoid32(vl[b]), sigmoid32(nl[b])
        vs = np.take_along_axis(sv, T.select_top_k(sv, KMAX), 1)
        ns = np.take_along_axis(sn, T.select_top_k(sn, KMAX), 1)
        pv = T.proposals(vr[b], STARTS[b], WINDOW_SIZE, queries.max(), NQ)
        pn = T.proposals(nr[b], STARTS[b], WINDOW_SIZE, queries.max(), NQ)
        score, _, _ = T.fuse_rows(vs, ns, pv, pn, THRESHOLD, alpha)
        w = (vs[:, :, None] / (vs[:, :, None] + ns[:, None, :])).astype(np.float32)
        w1 = (np.float32(1) - w).astype(np.float32)
        blend = w.astype(np.float64)[..., None] * pv[:, None, None, :] + w1.astype(np.float64)[..., None] * pn[:, None, None, :]
        out.append((vs, ns, score, blend))
    return out


def _near_half(blend):
    x = blend * 1000.0
    return np.abs(x - np.floor(x) - 0.5) < 1e-3


def make_inputs():
    rng = np.random.default_rng(SEED)
    centre = rng.uniform(0.05, 0.9, size=NQ)
    half = rng.uniform(0.01, 0.07, size=NQ)
    queries = np.stack([centre - half, centre + half], axis=1).clip(0.0, 0.97).astype(np.float32)
    vl = rng.normal(-5.2, 1.6, size=(NB, B * NQ, CV)).astype(np.float32)
    nl = rng.normal(-5.6, 1.6, size=(NB, B * NQ, CN)).astype(np.float32)
    base = np.tile(queries, (NB, B, 1)).astype(np.float32)
    vr = base + rng.normal(0, 0.02, size=base.shape).astype(np.float32)
    nr = base + rng.normal(0, 0.03, size=base.shape).astype(np.float32)
    hot = lambda C, at, x: np.where(np.arange(C) == at, np.float32(x), np.float32(-8.0)) + 0.01 * np.arange(C, dtype=np.float32)
    # ---- crafted rows (batch 0, window 0 starts at 1.0625)
    vl[0, 0], nl[0, 0] = hot(CV, 4, 0.5), hot(CN, 7, -8.0)                # only the verb passes
    vl[0, 1], nl[0, 1] = hot(CV, 2, -8.0), hot(CN, 20, 1.0)               # only the noun passes
    vl[0, 2], nl[0, 2] = hot(CV, 9, LOGIT_THR + 0.05), hot(CN, 3, 2.5)    # both pass; at alpha 1.3 the fused score fails
    vl[0, 3], nl[0, 3] = hot(CV, 1, 1.5), hot(CN, 11, 2.0)                # both clamps
    vr[0, 3], nr[0, 3] = (-0.3, 1.4), (0.02, 1.2)         # (both lower ends clamped would blend 1.0625 with itself: a rounding tie)
    vl[0, 4], nl[0, 4] = hot(CV, 0, -1.0), hot(CN, 22, 3.0)               # the noun's reversed segment outweighs the verb's
    vr[0, 4], nr[0, 4] = (0.30, 0.34), (0.80, 0.20)
    vl[0, 5], nl[0, 5] = hot(CV, 10, 0.0), hot(CN, 0, 0.0)                # the blend rounds to zero width
    vr[0, 5], nr[0, 5] = (0.41, 0.41001), (0.41001, 0.41002)
    vl[0, 6], nl[0, 6] = hot(CV, 5, 2.0), hot(CN, 5, -1.0)                # both reversed
    vr[0, 6], nr[0, 6] = (0.7, 0.5), (0.6, 0.4)
    vl[0, 7, :4] = (1.0, 0.5, 0.0, -0.5)                                  # several verbs and nouns of one row pass (top_k 3)
    nl[0, 7, 10:14] = (0.2, 1.2, -0.3, 0.7)
    vl[1, NQ + 5], nl[1, NQ + 5] = hot(CV, 6, 1.0), hot(CN, 17, 0.3)      # upper clamp in the window that starts at 3000.1234567
    vr[1, NQ + 5], nr[1, NQ + 5] = (0.1, 1.2), (0.12, 0.95)
    vl[1, NQ + 6, 3], nl[1, NQ + 6, 8] = 0.8, 1.1
    vr[2, 7], nr[2, 7] = (0.03, 0.3), (-0.05, 0.33)                       # lower clamp (the noun stream's)
    vl[2, 7, 2], nl[2, 7, 19] = 1.4, 0.6
    vl[2, NQ:2 * NQ] -= 1.5                                               # a window with few candidates
    # ---- the conditions under which the reference is well defined, on the restatement's values (main() checks them again
    #      on the reference's own): nudge what is in the way
    for _ in range(50):
        bad = 0
        for lg in (vl, nl):
            near = np.abs(1.0 / (1.0 + np.exp(-lg.astype(np.float64))) - THRESHOLD) < 2e-5
            lg[near] += np.float32(0.01)
            bad += int(near.sum())
        for b, (vs, ns, score, blend) in enumerate(_pairs(vl, nl, vr, nr, queries, 0.65)):
            rows = np.nonzero(_near_half(blend).any(axis=(1, 2, 3)))[0]
            vr[b, rows] += rng.uniform(1e-4, 3e-4, size=(len(rows), 2)).astype(np.float32)
            bad += len(rows)
        for alpha in (0.65, 1.3):
            for b, (vs, ns, score, blend) in enumerate(_pairs(vl, nl, vr, nr, queries, alpha)):
                rows = np.nonzero((np.abs(score - THRESHOLD) < 2e-5).any(axis=(1, 2)))[0]
                vl[b, rows] += np.float32(0.003)
                bad += len(rows)
        if not bad:
            break
    else:
        raise AssertionError("the inputs do not settle")
    return queries, vl, nl, vr, nr


def run_meter(C, logits, reg, queries):
    args = argparse.Namespace(data_modality="visual", include_verb_noun=False, num_class=[C, 5])
    meter = FeatureMeter(args)
    qt = torch.from_numpy(queries)[None].repeat(B, 1, 1)                 # [B, Nq, 2]
    for b in range(NB):
        metadata = {"video_id": list(VIDEOS[b]),
                    "window_start": torch.tensor(STARTS[b], dtype=torch.float64),          # what default_collate makes of
                    "window_size": torch.tensor([WINDOW_SIZE] * B, dtype=torch.float64)}   # Python floats
        meter.update((None, None, torch.from_numpy(logits[b]), None), (torch.from_numpy(reg[b]), None), (qt, None), metadata)
    return meter.finalize_metrics()


def run_reference(verb_data, noun_data, top_k, alpha):
    recorded = {}
    orig_filter = fp.filter_nms

    def recording_filter(results_in_vid, vid, **kw):
        recorded[vid] = [(int(d["verb"]), int(d["noun"]), np.float32(d["score"]), float(d["segment"][0]), float(d["segment"][1]))
                         for d in results_in_vid]
        assert all(isinstance(d["score"], np.float32) for d in results_in_vid)
        return orig_filter(results_in_vid=results_in_vid, vid=vid, **kw)

    fp.filter_nms = recording_filter
    orig_subprocess = fp.subprocess
    fp.subprocess = types.SimpleNamespace(run=lambda *a, **k: None)
    orig_load = torch.load
    fp.torch.load = lambda f, **k: orig_load(f, weights_only=False, **k)   # the files hold numpy arrays (pickled objects)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            torch.save(verb_data, "verb.pt")
            torch.save(noun_data, "noun.pt")
            fp.main(argparse.Namespace(path_to_verb_preds="verb.pt", path_to_noun_preds="noun.pt", path_to_gt="",
                                       score_threshold=THRESHOLD, verb_alpha=alpha, top_k=top_k, sigma=SIGMA, n_jobs=1))
            results = json.load(open("tim.json"))["results"]
        finally:
            os.chdir(cwd)
            fp.torch.load = orig_load
            fp.filter_nms = orig_filter
            fp.subprocess = orig_subprocess
    return recorded, results


def check_well_defined(verb_data, noun_data, top_k, alpha):
    """on the reference's own scores and proposals, over every pair of the top_k selections"""
    sv, sn = verb_data["action"], noun_data["action"]
    assert sv.dtype == np.float32 and verb_data["v_proposals"].dtype == np.float64
    for s in (sv, sn):
        d = -np.sort(-s, axis=1)
        assert (d[:, top_k - 1] != d[:, top_k]).all(), "tie at the k boundary"
    vs = np.take_along_axis(sv, T.select_top_k(sv, top_k), 1)[:, :, None]
    ns = np.take_along_axis(sn, T.select_top_k(sn, top_k), 1)[:, None, :]
    score = (vs ** np.float32(alpha)) * (ns ** np.float32(1.0 - alpha))                 # libm powf, as the reference
    assert score.dtype == np.float32
    for x in (vs, ns, score):
        assert not (np.abs(x.astype(np.float64) - THRESHOLD) < 1e-5).any(), "a score within 1e-5 of the threshold"
    w = vs / (vs + ns)
    blend = (w.astype(np.float64)[..., None] * verb_data["v_proposals"][:, None, None, :]
             + (1 - w).astype(np.float64)[..., None] * noun_data["v_proposals"][:, None, None, :])
    assert not _near_half(blend).any(), "a blended endpoint on a rounding tie"


def main():
    queries, vl, nl, vr, nr = make_inputs()
    verb_data, noun_data = run_meter(CV, vl, queries=queries, reg=vr), run_meter(CN, nl, queries=queries, reg=nr)
    assert list(verb_data["video_ids"]) == list(noun_data["video_ids"])
    names = sorted(set(v for row in VIDEOS for v in row))
    save = {}
    worst = 0
    for tag, (top_k, alpha) in SETS.items():
        check_well_defined(verb_data, noun_data, top_k, alpha)
        recorded, results = run_reference(verb_data, noun_data, top_k, alpha)
        cand = [(names.index(v),) + e for v in names for e in recorded.get(v, [])]
        res = [(names.index(v), int(e["verb"]), int(e["noun"]), float(e["score"]), float(e["segment"][0]), float(e["segment"][1]))
               for v in names for e in results.get(v, [])]
        for v in results:                                     # no two final scores of a video tie
            sc = [e["score"] for e in results[v]]
            assert len(set(sc)) == len(sc), v
            assert all(e["action"] == "%d,%d" % (e["verb"], e["noun"]) for e in results[v])
        # ---- the restatement on the same inputs: the same candidates per row, and how far its scores are
        col = T.Collector(CV, CN, THRESHOLD, alpha, top_k)
        for b in range(NB):
            col.update(vl[b], nl[b], vr[b], nr[b], queries, VIDEOS[b], STARTS[b], WINDOW_SIZE)
        c = col.candidates()
        for v, vid in enumerate(col.video_ids):
            m = c["video"] == v
            want = {(e[0], e[1], e[3], e[4]): e[2] for e in recorded.get(vid, [])}
            got = {(int(a), int(n), float(s[0]), float(s[1])): sc
                   for a, n, s, sc in zip(c["verb"][m], c["noun"][m], c["seg64"][m], c["score"][m])}
            assert set(got) == set(want) and len(got) == int(m.sum()) == len(recorded.get(vid, [])), (tag, vid)
            for key in got:
                worst = max(worst, abs(int(np.float32(got[key]).view(np.int32)) - int(np.float32(want[key]).view(np.int32))))
        save.update({
            tag + "_top_k": top_k, tag + "_alpha": alpha,
            tag + "_cand_video": np.asarray([x[0] for x in cand], np.int64), tag + "_cand_verb": np.asarray([x[1] for x in cand], np.int64),
            tag + "_cand_noun": np.asarray([x[2] for x in cand], np.int64), tag + "_cand_score": np.asarray([x[3] for x in cand], np.float32),
            tag + "_cand_seg": np.asarray([[x[4], x[5]] for x in cand], np.float64).reshape(-1, 2),
            tag + "_res_video": np.asarray([r[0] for r in res], np.int64), tag + "_res_verb": np.asarray([r[1] for r in res], np.int64),
            tag + "_res_noun": np.asarray([r[2] for r in res], np.int64), tag + "_res_score": np.asarray([r[3] for r in res], np.float64),
            tag + "_res_seg": np.asarray([[r[4], r[5]] for r in res], np.float64).reshape(-1, 2)})
        print(tag, "top_k", top_k, "alpha", alpha, "candidates", len(cand), "detections", len(res), "videos", sorted(results))
    print("max_ulp_vs_reference", worst)
    out = os.path.join(HERE, "twostream_small.npz")
    np.savez_compressed(
        out, seed=SEED, numpy_version=np.__version__, threshold=THRESHOLD, sigma=SIGMA, window_size=WINDOW_SIZE, num_queries=NQ,
        sets=np.asarray(list(SETS)), max_ulp_vs_reference=worst, queries=queries, verb_logits=vl, noun_logits=nl, verb_reg=vr,
        noun_reg=nr, window_start=np.asarray(STARTS, np.float64), video_ids=np.asarray(VIDEOS), video_names=np.asarray(names),
        verb_proposals=verb_data["v_proposals"].astype(np.float64), noun_proposals=noun_data["v_proposals"].astype(np.float64),
        **save)
    print("->", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
