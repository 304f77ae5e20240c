"""The detection inference tail on the HIP kernels (tim_amd/detect.py -> tim_amd/csrc/detect.hip) against its numpy
restatement tests/detect_ref.py and the fixture recorded from the reference (tests/golden/detect_small.npz).

Kernels alone: segments, keys, rows and the candidate order bit-exact; scores within 1 ulp and bit-equal on all but one
element in 10^6 (the device's double exp may differ from glibc's in its last bit, which survives the rounding to fp32 about
once in 10^8).  The inputs are built so that no reference score lies within 1 ulp of the threshold, which makes the
candidate membership exact as well.  Behind the NMS the bounds are those of tests/test_gpu_nms.py: kept segments, labels and
their order exact, scores within 2e-5 relative."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import detect_ref as D  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.candidate_helpers import DEV, dv, logit, ulp_apart  # noqa: E402
from tests.candidate_helpers import meta as _meta  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import detect as hd  # noqa: E402

def make_batch(seed, B, nq, ncls, thr, start0=0.0, invalid="some"):
    """one batch of synthetic head outputs; no score within 1 ulp of the threshold"""
    rng = np.random.default_rng(seed)
    R = B * nq
    centre, half = rng.uniform(0.05, 0.9, size=nq), rng.uniform(0.01, 0.08, size=nq)
    queries = np.stack([centre - half, centre + half], axis=1).clip(0.0, 0.98).astype(np.float32)
    reg = (np.tile(queries, (B, 1)) + rng.normal(0, 0.03, size=(R, 2))).astype(np.float32)
    if invalid == "all":
        reg[:, 1] = reg[:, 0] - np.float32(0.01)
    elif R >= 8:
        reg[1] = (0.7, 0.2)                                       # reversed
        reg[2] = (0.33, 0.33)                                     # zero width
        reg[3] = (-0.4, 1.7)                                      # both clamps
        reg[4:7] = ((0.2, 0.6), (0.1, 0.5), (0.3, 0.9))           # the rows with crafted logits below are valid
    logits = rng.normal(logit(thr, -9.0) - 2.4, 1.5, size=(R, ncls)).astype(np.float32)
    if R >= 8:
        logits[4] = logit(thr, -9.0) + 2.0 + rng.uniform(0, 1, size=ncls)      # every class passes
        logits[5] = (logit(thr, -9.0) - 3.0 - rng.uniform(0, 1, size=ncls)) if thr > 0 else -150.0      # none does
        logits[6, ::3] = (-110.0, -30.0, 40.0, 95.0)[seed % 4]            # far tails
    s = D.sigmoid32(logits)
    t32 = np.float32(thr)
    near = (s >= np.nextafter(t32, np.float32(-1))) & (s <= np.nextafter(t32, np.float32(2)))
    logits[near] += np.float32(0.05)
    s = D.sigmoid32(logits)
    assert not ((s >= np.nextafter(t32, np.float32(-1))) & (s <= np.nextafter(t32, np.float32(2)))).any() or thr <= 0.0
    starts = start0 + np.sort(rng.uniform(0, 900, size=B)) + rng.uniform(0, 1e-4, size=B)
    return dict(queries=queries, reg=reg, logits=logits, starts=starts.astype(np.float64), vidx=(np.arange(B) // 2).astype(np.int32))


def run_kernels(b, nq, thr, window_size, logits_dev=None):
    lg = dv(b["logits"]) if logits_dev is None else logits_dev
    mt = dv(b["queries"]).max()
    out = hd.candidates(lg, dv(b["reg"]), dv(b["starts"]), window_size, mt, dv(b["vidx"]), nq, thr)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def check_against_ref(got, b, thr, window_size, first=None):
    """`first`: `got` is the first that many candidates of the list (an emit into a smaller capacity)"""
    seg, score, key, row = got
    ref = D.batch_candidates(b["logits"], b["reg"], b["starts"], window_size, b["queries"].max(), b["vidx"], thr)
    want = {k: ref[k][:first] for k in ("row", "key", "seg", "score")}
    assert row.shape == want["row"].shape, (row.shape, want["row"].shape)
    assert np.array_equal(row, want["row"]) and np.array_equal(key, want["key"])     # membership and order
    assert seg.dtype == np.float32 and np.array_equal(seg.view(np.int32), want["seg"].view(np.int32))
    d = ulp_apart(score, want["score"])
    assert d.max(initial=0) <= 1
    assert int((d != 0).sum()) <= max(1, len(score) // 1000000)
    return ref


@pytest.mark.parametrize("ncls,B,nq,thr", [(1, 1, 1, 0.01), (1, 5, 7, 0.5), (44, 4, 37, 0.01), (63, 3, 19, 0.03),
                                           (64, 3, 19, 0.0), (65, 6, 50, 0.01), (97, 16, 399, 0.01), (97, 2, 33, 0.5),
                                           (300, 8, 100, 0.03), (300, 2, 11, 0.0), (3806, 16, 399, 0.01), (3806, 1, 3, 0.5)])
def test_kernels_match_the_restatement(ncls, B, nq, thr):
    ws = 30.000000000000004 if ncls != 44 else 10.24
    b = make_batch(100 + ncls + B, B, nq, ncls, thr)
    ref = check_against_ref(run_kernels(b, nq, thr, ws), b, thr, ws)
    if B * nq >= 8:
        assert len(ref["row"]) > 0 and (ref["row"] == 4).sum() == ncls and not (ref["row"] == 5).any()
        assert not ref["ok"][1] and not ref["ok"][2]


def test_grid_stride_past_one_pass_of_the_grid():
    """R = 8,200 proposal rows: past the 2,048 blocks * 4 waves = 8,192 rows one pass of the grid covers"""
    B, nq, ncls, thr, ws = 2, 4100, 3, 0.01, 30.000000000000004
    b = make_batch(43, B, nq, ncls, thr)
    ref = check_against_ref(run_kernels(b, nq, thr, ws), b, thr, ws)
    assert len(ref["row"]) > 50 and ref["row"].max() >= 8192          # candidates from the rows of the second pass


def test_a_capacity_below_the_count_clips_the_output():
    """emit with capacity = n // 2 into buffers one guard element longer: the first n // 2 candidates of the full list, and
    everything from the capacity onward keeps its sentinel"""
    B, nq, ncls, thr, ws = 2, 9, 23, 0.01, 10.24
    b = make_batch(29, B, nq, ncls, thr)
    n = len(check_against_ref(run_kernels(b, nq, thr, ws), b, thr, ws)["row"])
    cap = n // 2
    assert n >= 4
    bufs = (torch.full((cap + 1, 2), -7.0, device=DEV), torch.full((cap + 1,), -7.0, device=DEV),
            torch.full((cap + 1,), -7, dtype=torch.int64, device=DEV), torch.full((cap + 1,), -7, dtype=torch.int32, device=DEV))
    res = hd.candidates(dv(b["logits"]), dv(b["reg"]), dv(b["starts"]), ws, dv(b["queries"]).max(), dv(b["vidx"]), nq, thr,
                        out=tuple(t[:cap] for t in bufs))
    torch.cuda.synchronize()
    assert int(res[4].item()) == n                                   # the count is the whole list's
    check_against_ref([t[:cap].cpu().numpy() for t in bufs], b, thr, ws, first=cap)
    for t in bufs:
        assert bool((t[cap:] == -7).all())


def test_window_start_beyond_fp32_resolution():
    """at 3,000 s an fp32 sum would lose the third decimal: the fp64 add keeps it"""
    b = make_batch(7, 4, 25, 23, 0.01, start0=3000.0)
    ref = check_against_ref(run_kernels(b, 25, 0.01, 10.24), b, 0.01, 10.24)
    p32 = (np.clip(b["reg"], 0, b["queries"].max()) * np.float32(10.24)
           + np.repeat(b["starts"], 25)[:, None].astype(np.float32)).astype(np.float32)
    assert (np.round(p32.astype(np.float64), 3).astype(np.float32) != ref["seg32"]).any()     # the case is not vacuous


def test_strided_head_slice_needs_no_copy():
    b = make_batch(11, 3, 21, 97, 0.01)
    wide = torch.full((63, 97 + 40), 50.0, device=DEV)           # anything read outside the slice would pass the threshold
    wide[:, 13:13 + 97] = torch.from_numpy(b["logits"]).to(DEV)
    view = wide[:, 13:13 + 97]
    assert view.stride(0) == 137 and not view.is_contiguous()
    check_against_ref(run_kernels(b, 21, 0.01, 30.0, logits_dev=view), b, 0.01, 30.0)


def test_every_proposal_invalid_gives_no_candidates():
    b = make_batch(13, 2, 30, 44, 0.01, invalid="all")
    seg, score, key, row = run_kernels(b, 30, 0.01, 30.0)
    assert seg.shape == (0, 2) and score.shape == (0,) and key.shape == (0,) and row.shape == (0,)


def test_thresholds_outside_the_unit_interval():
    b = make_batch(17, 2, 16, 20, 0.01)
    b["logits"][7, :4] = (np.nan, -np.inf, np.inf, -200.0)
    for thr in (-1.0, 1.0, 0.0):
        check_against_ref(run_kernels(b, 16, thr, 30.0), b, thr, 30.0)


def test_library_refuses_bad_shapes():
    lib = L.load()
    z = torch.zeros(64, device=DEV)
    assert lib.timhip_det_candidates_count(L.ptr(z), 4, L.ptr(z), L.ptr(z), 1.0, L.ptr(z), 6, 4, 4, 0.01, L.ptr(z), L.ptr(z),
                                           L.ptr(z), None) == -1                       # R not a multiple of Nq
    assert lib.timhip_det_candidates_count(L.ptr(z), 3, L.ptr(z), L.ptr(z), 1.0, L.ptr(z), 8, 4, 4, 0.01, L.ptr(z), L.ptr(z),
                                           L.ptr(z), None) == -1                       # row stride < C
    assert lib.timhip_det_candidates_count(None, 1 << 20, None, None, 1.0, None, 1 << 16, 1 << 16, 1, 0.01, None, None,
                                           L.ptr(z), None) == L.EUNSUPPORTED           # R * C beyond int32


# ---- the collector ------------------------------------------------------------------------------------------------------------
def _same_detections(got, want):
    gs, gc, gl, gv = [t.cpu().numpy() for t in got]
    ws, wc, wl, wv = want
    assert gc.shape == wc.shape
    assert np.array_equal(gv, wv) and np.array_equal(gl, wl) and np.array_equal(gs, ws)       # kept set and order exact
    assert np.allclose(gc, wc, rtol=2e-5, atol=1e-9)


def test_collector_matches_the_reference_fixture():
    from tim_amd import DetectionCollector
    g = np.load(os.path.join(H.GOLDEN, "detect_small.npz"))
    nb, R, ncls = g["logits"].shape
    B = g["window_start"].shape[1]
    col = DetectionCollector([ncls, 5], head="action", score_threshold=float(g["threshold"]))
    qt = torch.from_numpy(np.tile(g["queries"][None], (B, 1, 1))).to(DEV)
    for b in range(nb):
        col.update((None, None, torch.from_numpy(g["logits"][b]).to(DEV), None), (torch.from_numpy(g["reg"][b]).to(DEV), None),
                   (qt, None), _meta(g["video_ids"][b], g["window_start"][b], float(g["window_size"])))
    assert col.video_ids == ["P03_01", "P01_07", "P02_05"]
    seg, score, key = [t.cpu().numpy() for t in col.candidates()]
    names = list(g["video_names"])
    for v, vid in enumerate(col.video_ids):                         # the list the reference handed its NMS, per video
        m, r = key // ncls == v, g["cand_video"] == names.index(vid)
        assert np.array_equal(key[m] % ncls, g["cand_class"][r])
        assert np.array_equal(seg[m], g["cand_seg"][r].astype(np.float32))
        assert ulp_apart(score[m], g["cand_score"][r]).max() <= 2    # torch's CPU sigmoid: see tests/test_detect_ref.py
    res = col.results(sigma=float(g["sigma"]))
    assert sorted(res) == sorted(names)
    for vid, entries in res.items():
        r = g["res_video"] == names.index(vid)
        want = {(int(a), float(s0), float(s1)): float(sc)
                for a, s0, s1, sc in zip(g["res_class"][r], g["res_seg"][r, 0], g["res_seg"][r, 1], g["res_score"][r])}
        got = {(e["action"], e["segment"][0], e["segment"][1]): e["score"] for e in entries}
        assert len(entries) == int(r.sum()) and set(got) == set(want)
        assert all(abs(got[k] - want[k]) <= 2e-5 * max(abs(want[k]), 1e-3) for k in got)
        assert [e["score"] for e in entries] == sorted((e["score"] for e in entries), reverse=True)


def test_collector_on_a_stream_in_two_batch_splits():
    """40 batches of 3 windows over 9 videos whose lengths put a batch boundary at every position inside a video; the same
    windows again in batches of 5 and 1: identical candidates and detections"""
    from tim_amd import DetectionCollector
    nq, ncls, thr, ws = 19, 31, 0.01, 10.24
    W = 120
    big = make_batch(23, W, nq, ncls, thr)
    lens = [13, 14, 12, 16, 11, 17, 10, 15, 12]
    assert sum(lens) == W
    vids = [("vid_%02d" % (9 - i)) for i, n in enumerate(lens) for _ in range(n)]
    qt = torch.from_numpy(np.tile(big["queries"][None], (1, 1, 1))).to(DEV)
    lg, rg = torch.from_numpy(big["logits"]).to(DEV), torch.from_numpy(big["reg"]).to(DEV)

    def collect(sizes):
        col, ref, w = DetectionCollector(ncls, "audio", thr), D.Collector(ncls, thr), 0
        for n in sizes:
            rows = slice(w * nq, (w + n) * nq)
            col.update((None, None, None, lg[rows]), (None, rg[rows]), (None, qt.expand(n, nq, 2)),
                       _meta(vids[w:w + n], big["starts"][w:w + n], ws))
            ref.update(big["logits"][rows], big["reg"][rows], big["queries"], vids[w:w + n], big["starts"][w:w + n], ws)
            w += n
        assert w == W
        return col, ref

    a, ref = collect([3] * 40)
    b, _ = collect([5, 1] * 20)
    ca, cb, cr = a.candidates(), b.candidates(), ref.candidates()
    for x, y in zip(ca, cb):
        assert torch.equal(x, y)
    assert np.array_equal(ca[2].cpu().numpy(), cr["key"]) and np.array_equal(ca[0].cpu().numpy(), cr["seg"])
    assert ulp_apart(ca[1].cpu().numpy(), cr["score"]).max() <= 1
    da, db = a.detections(sigma=0.1), b.detections(sigma=0.1)
    for x, y in zip(da, db):
        assert torch.equal(x, y)
    _same_detections(da, ref.detections(sigma=0.1))
    assert a.results(sigma=0.1).keys() == ref.results(sigma=0.1).keys()
    a.reset()
    assert a.video_ids == [] and a.candidates()[1].numel() == 0 and a.results() == {}


def test_detection_model_to_results():
    """DetectionTIM (tiny, eval(), evaluation route) -> collector -> results(): equal to the restatement fed the same logits"""
    from tim_amd import DetectionCollector
    from tim_amd.detection import TIM
    im, dm, nc, _ = H.DET_CASES[2]                                 # audio_visual, verb / noun / action + audio heads
    cfg = H.tiny_cfg("detection", im, dm, True, num_class=nc)
    sd, _ = H.synth_torch(cfg, 1, 0, 0, seed=3, dtype=torch.float32)
    m = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
            nhead=cfg.nhead, num_layers=cfg.num_layers, input_modality=im, data_modality=dm, num_feats=cfg.num_feats,
            include_verb_noun=True, precision="fp32")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    heads = {"verb": nc[0][0], "action": nc[0][2], "audio": nc[1]}
    cols = {h: DetectionCollector(cfg.num_class, head=h, score_threshold=0.3) for h in heads}
    refs = {h: D.Collector(n, 0.3) for h, n in heads.items()}
    ws, B = 30.0, 3
    for step in range(3):
        _, inp = H.synth_torch(cfg, B, 0, 0, seed=10 + step, dtype=torch.float32)
        vids = ["v%d" % ((3 * step + i) // 4) for i in range(B)]
        starts = [7.5 * (3 * step + i) + 0.0001234 for i in range(B)]
        with torch.no_grad():
            output, _, _, query_times, _ = m([inp["visual"].to(DEV), inp["audio"].to(DEV)], "encoder", inp["times"].to(DEV), None)
        meta = _meta(vids, starts, ws)
        for h in heads:
            slot, rslot = hd.HEADS[h]
            cols[h].update(output[0], output[1], query_times, meta)
            refs[h].update(output[0][slot].cpu().numpy(), output[1][rslot].cpu().numpy(), query_times[rslot].cpu().numpy(), vids,
                           starts, ws)
    total = 0
    for h in heads:
        cand, rc = cols[h].candidates(), refs[h].candidates()
        assert np.array_equal(cand[2].cpu().numpy(), rc["key"]) and np.array_equal(cand[0].cpu().numpy(), rc["seg"])
        assert ulp_apart(cand[1].cpu().numpy(), rc["score"]).max(initial=0) <= 1
        _same_detections(cols[h].detections(sigma=0.1), refs[h].detections(sigma=0.1))
        got, want = cols[h].results(sigma=0.1), refs[h].results(sigma=0.1)
        assert got.keys() == want.keys()
        for vid in got:
            assert [(e["action"], e["segment"]) for e in got[vid]] == [(e["action"], e["segment"]) for e in want[vid]]
            total += len(got[vid])
    assert total > 0


def test_both_calls_replay_in_a_graph_on_new_logits():
    """count + emit captured once with a worst-case-sized output (R * C slots) and replayed after the logits changed in place;
    slots past the total keep their sentinel"""
    nq, ncls, thr, ws, B = 21, 65, 0.03, 30.0, 4
    R = B * nq
    b1, b2 = make_batch(31, B, nq, ncls, thr), make_batch(32, B, nq, ncls, thr)
    logits, reg, starts, vidx = dv(b1["logits"]), dv(b1["reg"]), dv(b1["starts"]), dv(b1["vidx"])
    mt = dv(b1["queries"]).max().reshape(1)
    cap = R * ncls
    out = (torch.empty((cap, 2), device=DEV), torch.empty(cap, device=DEV), torch.empty(cap, dtype=torch.int64, device=DEV),
           torch.empty(cap, dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hd.candidates(logits, reg, starts, ws, mt, vidx, nq, thr, out=out)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = hd.candidates(logits, reg, starts, ws, mt, vidx, nq, thr, out=out)
    for b in (b1, b2, b1):
        logits.copy_(dv(b["logits"])); reg.copy_(dv(b["reg"])); starts.copy_(dv(b["starts"]))
        mt.copy_(dv(b["queries"]).max().reshape(1))
        for t, fill in zip(out, (-7.0, -7.0, -7, -7)):
            t.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        n = int(res[4].item())
        got = [t[:n].cpu().numpy() for t in out]
        check_against_ref(got, b, thr, ws)
        assert 0 < n < cap
        assert bool((out[1][n:] == -7.0).all()) and bool((out[2][n:] == -7).all()) and bool((out[3][n:] == -7).all())
