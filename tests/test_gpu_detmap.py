"""Detection scoring on the HIP kernels (tim_amd/detmap.py -> tim_amd/csrc/detmap.hip) against its numpy restatement
(tests/detmap_ref.py) and the reference's recorded numbers (tests/golden/detmap_small.npz): the true-positive flags and the
lock table bit for bit, AP within 1e-12 (a sum of at most npos <= 2^13 positive terms that total at most 1: any order of
summation stays within npos * 2^-53)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import detmap_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tim_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
AP_TOL = 1e-12
_cache = {}


def fixture(name):
    """the fixture's inputs and the restatement's outputs on them, computed once"""
    if name not in _cache:
        g = np.load(os.path.join(H.GOLDEN, name + ".npz"))
        seg = g["gt_seconds"] if "gt_seconds" in g else g["gt_seg"]
        _cache[name] = (g, seg) + R.evaluate(g["gt_video"], seg, g["gt_label"], g["pred_video"], g["pred_seg"], g["pred_score"],
                                             g["pred_label"], g["thresholds"])
    return _cache[name]


def run_kernels(tab, thr):
    """the two library calls on the restatement's tables -> tp [T, N], lock [T, G] by input row, ap [T, C]"""
    thr = np.asarray(thr, np.float64)
    T, N, G, C = len(thr), tab["pred_seg"].shape[0], tab["gt_seg"].shape[0], len(tab["classes"])
    d = {k: torch.from_numpy(np.ascontiguousarray(tab[k])).to(DEV)
         for k in ("pred_seg", "group_pred", "group_pred_lo", "group_pred_hi", "group_pos0", "gt_seg", "gt_off", "class_off", "npos")}
    thr_d = torch.from_numpy(thr).to(DEV)
    tp = torch.zeros((T, N), dtype=torch.uint8, device=DEV)
    lock = torch.full((T, G), -1, dtype=torch.int32, device=DEV)
    work = torch.full((G,), -1, dtype=torch.int32, device=DEV)          # need not be cleared: every bit set
    ap = torch.zeros((T, C), dtype=torch.float64, device=DEV)
    L.call("timhip_det_match", L.ptr(d["pred_seg"]), N, L.ptr(d["group_pred"]), L.ptr(d["group_pred_lo"]),
           L.ptr(d["group_pred_hi"]), L.ptr(d["group_pos0"]), L.ptr(d["gt_seg"]), G, L.ptr(d["gt_off"]), len(tab["gt_off"]) - 1,
           L.ptr(thr_d), T, L.ptr(tp), L.ptr(lock), L.ptr(work), None)
    L.call("timhip_det_ap", L.ptr(tp), N, L.ptr(d["class_off"]), L.ptr(d["npos"]), C, T, L.ptr(ap), None)
    torch.cuda.synchronize()
    lock_in = np.empty((T, G), np.int32)
    lock_in[:, tab["gt_order"]] = lock.cpu().numpy()
    return tp.cpu().numpy(), lock_in, ap.cpu().numpy()


def check(got, want, what=""):
    tp, lock, ap = got
    wtp, wlock, wap = want
    err = float(np.abs(ap - wap).max()) if ap.size else 0.0
    print("%s: %d predictions, %d true positives at thr[0], max |ap - restatement| = %.3g" % (what, tp.shape[1], int(tp[0].sum()), err))
    assert np.array_equal(tp, wtp), what
    assert np.array_equal(lock, wlock), what
    assert ap.shape == wap.shape and err <= AP_TOL, (what, err)


@pytest.mark.parametrize("name", ["detmap_small", "detmap_ties"])
def test_kernels_match_the_restatement_on_the_fixtures(name):
    g, seg, tp, lock, ap, tab = fixture(name)
    check(run_kernels(tab, g["thresholds"]), (tp, lock, ap), name)
    if name == "detmap_small":
        assert np.abs(ap - g["ap"]).max() <= AP_TOL                       # and so the reference's own numbers
    else:
        assert np.array_equal(tp, g["tp"]) and np.array_equal(lock, g["lock"])


def synthetic(seed, groups, n_pred, labels=None, videos=None, length=3.0, span=200.0, quantum=None):
    """ground truth with `groups` = {(label, video): segments}; predictions: half jittered copies, half anywhere, with labels
    from `labels` and videos from `videos` (default: those of the ground truth).  `quantum`: snap every time to a multiple
    of it, which makes exactly equal tIoUs and tIoUs that sit on a threshold common."""
    rng = np.random.default_rng(seed)
    gv, gs, gl = [], [], []
    for (lab, v), n in groups.items():
        s = rng.uniform(0.0, span, size=n)
        gv += [v] * n
        gl += [lab] * n
        gs += [(a, a + rng.uniform(0.5, length)) for a in s]
    gs = np.asarray(gs, np.float64).reshape(-1, 2)
    o = rng.permutation(len(gl))
    gv, gs, gl = np.asarray(gv)[o], gs[o], np.asarray(gl, np.int64)[o]
    labels = sorted(set(gl.tolist())) if labels is None else labels
    videos = sorted(set(gv.tolist())) if videos is None else videos
    i = rng.integers(0, len(gl), size=n_pred)
    copy = rng.random(n_pred) < 0.5
    ps = np.where(copy[:, None], gs[i] + rng.normal(0, 0.4, size=(n_pred, 2)), 0.0)
    a = rng.uniform(0.0, span, size=n_pred)
    ps = np.where(copy[:, None], ps, np.stack([a, a + rng.uniform(0.5, length, size=n_pred)], axis=1))
    ps[:, 0] = np.maximum(ps[:, 0], 0.0)
    ps[:, 1] = np.maximum(ps[:, 1], ps[:, 0] + 0.01)
    pv = np.where(copy & np.isin(gv[i], videos), gv[i], rng.choice(videos, size=n_pred))
    pl = np.where(copy & np.isin(gl[i], labels), gl[i], rng.choice(labels, size=n_pred)).astype(np.int64)
    pc = rng.uniform(0.01, 1.0, size=n_pred).astype(np.float32).astype(np.float64)
    if quantum:
        gs, ps = np.round(gs / quantum) * quantum, np.round(ps / quantum) * quantum
        ps[:, 1] = np.maximum(ps[:, 1], ps[:, 0] + quantum)
        gs[:, 1] = np.maximum(gs[:, 1], gs[:, 0] + quantum)
        pc = np.round(pc * 8) / 8
    return (gv, gs, gl), (pv, ps, pc, pl)


LIN5 = np.linspace(0.1, 0.5, 5)
EDGES = {
    # groups of 1, 64, 65 and 130 segments: one lane, a full wave, the second register slot, (130 <= 256) three slots
    "groups_1_64_65_130": dict(groups={(1, "a"): 1, (1, "b"): 64, (1, "c"): 65, (2, "a"): 130}, n_pred=600, thr=LIN5),
    # more than 256 segments: the lock words live in the workspace; 257 is the first such size
    "groups_256_257_300": dict(groups={(1, "a"): 256, (1, "b"): 257, (2, "a"): 300}, n_pred=1500, thr=LIN5, span=900.0),
    "groups_300_on_a_grid": dict(groups={(1, "a"): 300, (2, "a"): 70}, n_pred=600, thr=[0.2, 0.5, 1.0], span=300.0, quantum=0.5),
    "one_threshold": dict(groups={(1, "a"): 20, (3, "b"): 70}, n_pred=300, thr=[0.3]),
    "sixteen_thresholds_repeated": dict(groups={(1, "a"): 20, (3, "b"): 70}, n_pred=300,
                                        thr=[0.1, 0.1, 0.2, 0.3, 0.3, 0.3, 0.4, 0.5, 0.5, 0.6, 0.7, 0.7, 0.8, 0.9, 0.05, 0.1]),
    "on_a_grid": dict(groups={(1, "a"): 30, (1, "b"): 66, (4, "a"): 9}, n_pred=500, thr=[0.25, 1.0 / 3.0, 0.5, 0.5, 1.0],
                      span=40.0, quantum=0.5),
    # a class whose range spans eight chunks of the AP block, next to a small one
    "long_class": dict(groups={(1, "a"): 100, (1, "b"): 40, (2, "a"): 5}, n_pred=2100, thr=LIN5, labels=[1, 1, 1, 1, 1, 1, 1, 1, 1, 2]),
    "chunk_edges_255_256_257": dict(groups={(1, "a"): 30, (2, "a"): 30, (3, "a"): 30}, n_pred=768, thr=LIN5, exact_classes=(255, 256, 257)),
    "npos_one": dict(groups={(5, "a"): 1, (6, "a"): 4}, n_pred=80, thr=LIN5, span=10.0),
    "all_in_videos_without_ground_truth": dict(groups={(1, "a"): 10, (2, "b"): 10}, n_pred=200, thr=LIN5, videos=["x", "y"]),
    "labels_absent_from_the_ground_truth": dict(groups={(1, "a"): 10, (7, "b"): 10}, n_pred=300, thr=LIN5, labels=[0, 1, 3, 7, 9]),
}


def edge_case(name):
    if name not in _cache:
        kw = dict(EDGES[name])
        thr, exact = np.asarray(kw.pop("thr"), np.float64), kw.pop("exact_classes", None)
        gt, pred = synthetic(len(name), **kw)
        if exact:                                                         # class sizes of exactly these many predictions
            pv, ps, pc, pl = pred
            pl = np.repeat(sorted(set(gt[2].tolist())), exact)[np.random.default_rng(1).permutation(sum(exact))]
            pred = (pv, ps, pc, pl)
        _cache[name] = (gt, pred, thr) + R.evaluate(*gt, *pred, thr)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_shapes(name):
    from tim_amd import DetectionScorer
    (gv, gs, gl), (pv, ps, pc, pl), thr, tp, lock, ap, tab = edge_case(name)
    if name == "all_in_videos_without_ground_truth":
        assert tp.sum() == 0 and ap.max() == 0.0 and tab["pred_seg"].shape[0] == 200
    if name == "labels_absent_from_the_ground_truth":
        assert 0 < tab["pred_seg"].shape[0] < 300
    if name == "long_class":
        assert tab["class_off"][1] > 7 * 256
    if name == "chunk_edges_255_256_257":
        assert np.diff(tab["class_off"]).tolist() == [255, 256, 257]
    if name == "npos_one":
        assert tab["npos"].tolist() == [1, 4] and tp[:, :tab["class_off"][1]].sum(axis=1).max() == 1
    if "grid" in name:
        assert tp[-1].sum() > 0                                           # tIoU == 1.0 == thr: >= matches
    check(run_kernels(tab, thr), (tp, lock, ap), name + " (kernels)")
    # the same through the class: the device sorts and tables instead of the restatement's
    videos = sorted(set(pv.tolist()))
    sc = DetectionScorer(gv, gs, gl, tiou_thresholds=thr, round_segments=False)
    mAP, avg = sc.evaluate(torch.from_numpy(ps).to(DEV), torch.from_numpy(pc).to(DEV), torch.from_numpy(pl).to(DEV),
                           torch.from_numpy(np.asarray([videos.index(v) for v in pv], np.int64)).to(DEV), videos)
    N = tab["pred_seg"].shape[0]
    stp = sc.tp.cpu().numpy()
    assert np.array_equal(sc.order.cpu().numpy()[:N], tab["pred_input_row"])
    assert stp[:, N:].sum() == 0                                          # dropped labels: at the end, never matched
    check((stp[:, :N], sc.lock.cpu().numpy(), sc.ap.cpu().numpy()), (tp, lock, ap), name + " (class)")
    assert sc.classes.tolist() == tab["classes"].tolist()
    assert mAP.dtype == np.float64 and mAP.shape == thr.shape and isinstance(avg, float)
    assert np.abs(mAP - ap.mean(axis=1)).max() <= AP_TOL and abs(avg - ap.mean(axis=1).mean()) <= AP_TOL


def test_zero_predictions():
    from tim_amd import DetectionScorer
    lib = L.load()
    (gv, gs, gl), _, thr, *_ = edge_case("npos_one")
    sc = DetectionScorer(gv, gs, gl, tiou_thresholds=thr)
    e = torch.zeros((0,), device=DEV)
    mAP, avg = sc.evaluate(torch.zeros((0, 2), device=DEV), e, e.to(torch.int64), e.to(torch.int64), [])
    assert mAP.tolist() == [0.0] * 5 and avg == 0.0 and sc.ap.shape == (5, 2) and float(sc.ap.abs().max()) == 0.0
    assert sc.tp.shape == (5, 0) and int((sc.lock != -1).sum()) == 0
    assert sc.evaluate_results({"a": [], "zz": []})[1] == 0.0
    # the entries themselves: no prediction / no group / no class is a successful no-op, whatever the pointers
    assert lib.timhip_det_match(None, 0, None, None, None, None, None, 5, None, 2, None, 5, None, None, None, None) == 0
    assert lib.timhip_det_match(None, 9, None, None, None, None, None, 5, None, 0, None, 5, None, None, None, None) == 0
    assert lib.timhip_det_ap(None, 0, None, None, 3, 5, None, None) == 0
    assert lib.timhip_det_ap(None, 7, None, None, 0, 5, None, None) == 0


def test_scorer_gives_the_reference_numbers_on_the_submission():
    from tim_amd import DetectionScorer
    from tim_amd.detmap import timestamp_to_seconds
    g, seg, tp, lock, ap, tab = fixture("detmap_small")
    sec = np.asarray([[timestamp_to_seconds(a), timestamp_to_seconds(b)] for a, b in zip(g["gt_start"], g["gt_stop"])])
    results = {str(v): [] for v in g["video_ids"]}
    for v, s, c, lab in zip(g["pred_video"], g["pred_seg"], g["pred_score"], g["pred_label"]):
        results[str(v)].append({"action": int(lab), "score": float(c), "segment": [float(s[0]), float(s[1])]})
    sc = DetectionScorer(g["gt_video"], sec, g["gt_label"])
    mAP, avg = sc.evaluate_results(results)
    print("mAP", mAP, "reference", g["mAP"], "max diff", np.abs(mAP - g["mAP"]).max(), "avg diff", abs(avg - float(g["average_mAP"])))
    assert np.abs(mAP - g["mAP"]).max() <= AP_TOL and abs(avg - float(g["average_mAP"])) <= AP_TOL
    assert np.abs(sc.ap.cpu().numpy() - g["ap"]).max() <= AP_TOL
    N = tp.shape[1]
    assert np.array_equal(sc.tp.cpu().numpy()[:, :N], tp) and np.array_equal(sc.lock.cpu().numpy(), lock)
    assert sc.classes.tolist() == [3, 8, 15, 21, 40, 77, 120]


def test_score_of_a_collector_equals_its_results_file():
    """score(collector) = evaluate_results(collector.results()) with the same NMS arguments: the device path rounds the
    segments with rint(x * 1000) / 1000, the file carries Python's round(x, 3); flags bit-exact"""
    from tim_amd import DetectionCollector, DetectionScorer
    g = np.load(os.path.join(H.GOLDEN, "detect_small.npz"))
    nb, nrow, ncls = g["logits"].shape
    B = g["window_start"].shape[1]
    col = DetectionCollector([ncls, 5], head="action", score_threshold=float(g["threshold"]))
    qt = torch.from_numpy(np.tile(g["queries"][None], (B, 1, 1))).to(DEV)
    for b in range(nb):
        meta = {"video_id": list(g["video_ids"][b]), "window_start": torch.tensor(g["window_start"][b], dtype=torch.float64),
                "window_size": torch.tensor([float(g["window_size"])] * B, dtype=torch.float64)}
        col.update((None, None, torch.from_numpy(g["logits"][b]).to(DEV), None), (torch.from_numpy(g["reg"][b]).to(DEV), None),
                   (qt, None), meta)
    nms = dict(sigma=float(g["sigma"]))
    segs, scores, labels, video = (t.cpu().numpy() for t in col.detections(**nms))
    assert scores.shape[0] > 50
    rng = np.random.default_rng(3)
    pick = np.arange(0, scores.shape[0], 2)                               # ground truth: jittered detections, one video left out
    pick = pick[video[pick] != 2]
    gt_seg = np.round(segs[pick].astype(np.float64) + rng.normal(0, 0.2, size=(len(pick), 2)), 2)
    gt_seg[:, 1] = np.maximum(gt_seg[:, 1], gt_seg[:, 0] + 0.01)
    gt_video = [col.video_ids[int(v)] for v in video[pick]]
    a = DetectionScorer(gt_video, gt_seg, labels[pick])
    b = DetectionScorer(gt_video, gt_seg, labels[pick])
    mAP_a, avg_a = a.score(col, **nms)
    mAP_b, avg_b = b.evaluate_results(col.results(**nms))
    assert torch.equal(a.tp, b.tp) and torch.equal(a.lock, b.lock) and torch.equal(a.order, b.order)
    assert torch.equal(a.ap, b.ap) and np.array_equal(mAP_a, mAP_b) and avg_a == avg_b
    assert int(a.tp[0].sum()) > 10 and 0.0 < avg_a <= 1.0
    # and the restatement on the file's numbers
    res = col.results(**nms)
    rows = [(v, d["segment"], d["score"], d["action"]) for v in res for d in res[v]]
    tp, lock, ap, tab = R.evaluate(gt_video, gt_seg, labels[pick], [r[0] for r in rows], np.asarray([r[1] for r in rows]),
                                   np.asarray([r[2] for r in rows]), np.asarray([r[3] for r in rows]), a.tiou_thresholds)
    N = tp.shape[1]
    check((a.tp.cpu().numpy()[:, :N], a.lock.cpu().numpy(), a.ap.cpu().numpy()), (tp, lock, ap), "collector")


def test_argument_checks():
    from tim_amd import DetectionScorer
    lib = L.load()
    z = torch.zeros(64, device=DEV)
    p = L.ptr(z)

    def match(n_pred=4, n_gt=4, n_groups=1, T=5, pred_seg=p, lock=p):
        return lib.timhip_det_match(pred_seg, n_pred, p, p, p, p, p, n_gt, p, n_groups, p, T, p, lock, p, None)
    assert match(T=0) == -1 and match(T=17) == -1
    assert match(n_pred=-1) == -1 and match(n_gt=-1) == -1 and match(n_groups=-1) == -1
    assert match(pred_seg=None) == -1 and match(lock=None) == -1
    assert match(n_pred=1 << 31) == L.EUNSUPPORTED
    assert lib.timhip_det_ap(p, 4, p, p, 1, 0, p, None) == -1 and lib.timhip_det_ap(p, 4, p, p, 1, 17, p, None) == -1
    assert lib.timhip_det_ap(p, -1, p, p, 1, 5, p, None) == -1 and lib.timhip_det_ap(p, 4, p, p, -1, 5, p, None) == -1
    assert lib.timhip_det_ap(None, 4, p, p, 1, 5, p, None) == -1 and lib.timhip_det_ap(p, 4, p, p, 1, 5, None, None) == -1
    torch.cuda.synchronize()
    seg = np.asarray([[0.0, 1.0], [2.0, 3.0]])
    with pytest.raises(ValueError):
        DetectionScorer(["a", "a"], seg, [1, 2], tiou_thresholds=np.linspace(0.05, 0.95, 17))
    sc = DetectionScorer(["a", "a"], seg, [1, 2])
    d2, d1, i1 = torch.zeros((3, 2), device=DEV), torch.zeros(3, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(L.TimHipError, match="no CPU fallback"):
        sc.evaluate(d2.cpu(), d1, i1, i1, ["a"])
    with pytest.raises(L.TimHipError, match="no CPU fallback"):
        sc.evaluate(d2, d1, i1.cpu(), i1, ["a"])
    with pytest.raises(ValueError):
        sc.evaluate(d2, d1[:2], i1, i1, ["a"])
    with pytest.raises(ValueError):
        sc.evaluate(d2[:2], d1, i1, i1, ["a"])
    with pytest.raises(ValueError):
        sc.evaluate(d2, d1, i1, i1[:1], ["a"])


def test_score_detection_synthetic_example_prints_five_maps(capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import score_detection_synthetic
    mAP, avg = score_detection_synthetic.main(["--videos", "3", "--windows", "3", "--batch", "4"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "mAP @ tIoU" in ln]
    assert len(lines) == 5
    vals = [float(ln.split(":")[1]) for ln in lines]
    assert all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in vals) and all(0.0 <= float(m) <= 1.0 for m in mAP)
    assert 0.0 < avg < 1.0 and mAP[0] >= mAP[-1]
