"""The two-stream detection fusion on the HIP kernels (tim_amd/twostream.py -> tim_amd/csrc/twostream.hip) against its numpy
restatement tests/twostream_ref.py and the fixture recorded from the reference (tests/golden/twostream_small.npz).

Kernels alone: selected indices and pass bits exact, selected scores within 1 ulp (the device's double exp may differ from
glibc's in its last bit, which survives the rounding to fp32 about once in 10^8).  On every row whose selected scores equal
the restatement's bit for bit: fused scores within 3 ulp (each fp32 power may differ by 1 ulp where the device's double pow
and glibc's straddle an fp32 rounding boundary, and the product adds one rounding), segments bit-equal, the emitted order,
keys and rows exact; at most 1 row in 1,000 may fall outside that condition.  The inputs are nudged so that no score of the
restatement - selected or fused - lies within 4 ulp of the threshold, which makes the membership exact for every row.
Behind the NMS the bounds are those of tests/test_gpu_nms.py: kept segments, labels and their order exact, scores within
2e-5 relative."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import twostream_ref as T  # noqa: E402
from tests.candidate_helpers import DEV, dv, logit, ulp_apart  # noqa: E402
from tests.candidate_helpers import meta as _meta  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import twostream as ts  # noqa: E402

def _near(x, thr):
    """within 4 ulp of the threshold (NaN: no)"""
    x = np.ascontiguousarray(x, np.float32)
    return ~np.isnan(x) & (ulp_apart(x, np.full_like(x, np.float32(thr))) <= 4)


def reference(b, thr, alpha, k, ws):
    return T.batch_candidates(b["vl"], b["nl"], b["vr"], b["nr"], b["starts"], ws, b["queries"].max(), b["vidx"], thr, alpha, k)


def settle(b, thr, alpha, k, ws):
    """nudge the rows that carry a selected or fused score within 4 ulp of the threshold; -> the restatement of the result"""
    for _ in range(20):
        ref = reference(b, thr, alpha, k, ws)
        rows = _near(ref["sel_score"], thr).any(axis=(1, 2)) | _near(ref["pair_score"], thr).any(axis=1)
        if not rows.any():
            return ref
        b["vl"][rows] += np.float32(0.05)
        b["nl"][rows] += np.float32(0.03)
    raise AssertionError("the inputs do not settle")


def make_batch(seed, B, nq, Cv, Cn, thr, invalid="some", start0=0.0):
    rng = np.random.default_rng(seed)
    R = B * nq
    centre, half = rng.uniform(0.05, 0.9, size=nq), rng.uniform(0.01, 0.08, size=nq)
    queries = np.stack([centre - half, centre + half], axis=1).clip(0.0, 0.98).astype(np.float32)
    vr = (np.tile(queries, (B, 1)) + rng.normal(0, 0.03, size=(R, 2))).astype(np.float32)
    nr = (np.tile(queries, (B, 1)) + rng.normal(0, 0.04, size=(R, 2))).astype(np.float32)
    if invalid == "all":
        vr[:, 1] = vr[:, 0] - np.float32(0.01)
        nr[:, 1] = nr[:, 0] - np.float32(0.02)
    elif R >= 5:
        vr[1], nr[1] = (0.7, 0.2), (0.8, 0.1)                     # reversed
        vr[2], nr[2] = (0.33, 0.33), (0.33, 0.33)                 # zero width
        vr[3], nr[3] = (-0.4, 1.7), (0.05, 1.3)                   # clamps
    # the best of C normal draws sits near the threshold's logit: rows where the verb, the noun, both or neither pass
    lift = lambda C: 0.0 if C < 2 else 1.5 * np.sqrt(2 * np.log(C))
    vl = rng.normal(logit(thr, -3.0) - lift(Cv) + 1.0, 1.5, size=(R, Cv)).astype(np.float32)
    nl = rng.normal(logit(thr, -3.0) - lift(Cn) + 1.0, 1.5, size=(R, Cn)).astype(np.float32)
    if R >= 5:
        vl[4] += 6.0                                              # many classes of both streams pass in a valid row
        nl[4] += 6.0
        if invalid != "all":
            vr[4], nr[4] = (0.2, 0.6), (0.1, 0.5)
    starts = start0 + np.sort(rng.uniform(0, 900, size=B)) + rng.uniform(0, 1e-4, size=B)
    return dict(queries=queries, vl=vl, nl=nl, vr=vr, nr=nr, starts=starts.astype(np.float64),
                vidx=(np.arange(B) // 2).astype(np.int32))


def run_kernels(b, nq, thr, alpha, k, ws, vl_dev=None, nl_dev=None):
    out = ts.candidates(dv(b["vl"]) if vl_dev is None else vl_dev, dv(b["nl"]) if nl_dev is None else nl_dev, dv(b["vr"]),
                        dv(b["nr"]), dv(b["starts"]), ws, dv(b["queries"]).max(), dv(b["vidx"]), nq, thr, alpha, k, records=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out[:4]], [t.cpu().numpy() for t in out[4]]


def _same_bits(a, b):
    """bit-equal where both are numbers; a NaN only against a NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return (na == nb) & (na | (a.view(np.int32) == b.view(np.int32)))


def _ulps(a, b):
    """ulp distance, 0 for a NaN against a NaN, huge for a NaN against a number"""
    na, nb = np.isnan(a), np.isnan(b)
    d = ulp_apart(np.where(na, 0, a), np.where(nb, 0, b))
    d[na != nb] = 1 << 40
    d[na & nb] = 0
    return d


def check_against_ref(got, ref, k, self_check=False):
    (seg, score, key, row), (sel_idx, sel_score, pair_score, pair_seg, pair_mask, off) = got
    R, kk = ref["sel_idx"].shape[0], k * k
    # ---- records
    assert np.array_equal(sel_idx, ref["sel_idx"])
    bits = ((pair_mask.view(np.uint64)[:, None] >> np.arange(kk, dtype=np.uint64)[None]) & np.uint64(1)).astype(bool)
    assert np.array_equal(bits, ref["pair_ok"])
    assert (pair_mask.view(np.uint64) >> np.uint64(kk) == 0).all() if kk < 64 else True
    assert _ulps(sel_score, ref["sel_score"]).max(initial=0) <= 1
    good = _same_bits(sel_score, ref["sel_score"]).all(axis=(1, 2))
    assert int((~good).sum()) <= R // 1000, "%d of %d rows select a score that differs from the restatement's" % ((~good).sum(), R)
    if self_check:
        assert good.all()
    assert _ulps(pair_score[good], ref["pair_score"][good]).max(initial=0) <= 3
    assert _same_bits(pair_seg[good], ref["pair_seg"][good]).all()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(ref["pair_ok"].sum(axis=1))]))
    # ---- the emitted list
    assert row.shape == ref["row"].shape and np.array_equal(row, ref["row"]) and np.array_equal(key, ref["key"])
    g = good[row]
    assert seg.dtype == np.float32 and np.array_equal(seg[g].view(np.int32), ref["seg"][g].view(np.int32))
    assert ulp_apart(score[g], ref["score"][g]).max(initial=0) <= 3
    return ref


SHAPES = [(1, 1), (2, 64), (63, 65), (64, 256), (97, 300), (257, 255)]
CASES = [(cv, cn, k) for cv, cn in SHAPES for k in sorted({1, 2, 3, 8, min(cv, cn, 8)}) if k <= min(cv, cn)]


@pytest.mark.parametrize("Cv,Cn,k", CASES)
def test_kernels_match_the_restatement(Cv, Cn, k):
    thr, alpha, ws, B, nq = 0.03, 0.65, 10.24, 3, 7
    b = make_batch(1000 + 10 * Cv + k, B, nq, Cv, Cn, thr)
    ref = settle(b, thr, alpha, k, ws)
    check_against_ref(run_kernels(b, nq, thr, alpha, k, ws), ref, k)
    assert not ref["pair_ok"][1:3].any()                       # reversed, zero width
    if min(Cv, Cn) >= 8:
        assert ref["pair_ok"][4].sum() == k * k and 0 < ref["pair_ok"].sum() < B * nq * k * k


@pytest.mark.parametrize("B,nq", [(1, 1), (2, 2), (5, 1), (5, 205), (2, 4100)])
@pytest.mark.parametrize("Cv,Cn,k", [(97, 300, 1), (97, 300, 3), (63, 65, 8)])
def test_row_counts_one_block_the_scan_carry_and_the_grid_stride(B, nq, Cv, Cn, k):
    """R = 1, 4 (one block), 5 (two), 1025 (the scan's carry) and 8,200 (past the 2,048 * 4 rows of one grid pass)"""
    thr, alpha, ws = 0.03, 0.65, 30.000000000000004
    b = make_batch(7 + B * nq + k, B, nq, Cv, Cn, thr)
    ref = settle(b, thr, alpha, k, ws)
    check_against_ref(run_kernels(b, nq, thr, alpha, k, ws), ref, k)
    if B * nq > 1000:
        assert len(ref["row"]) > 50 and ref["row"].max() > B * nq - 50


def test_the_restatement_against_itself_excludes_no_row():
    thr, alpha, ws, k = 0.03, 0.65, 10.24, 3
    b = make_batch(3, 4, 9, 11, 23, thr)
    ref = settle(b, thr, alpha, k, ws)
    kk = k * k
    mask = (ref["pair_ok"].astype(np.uint64) << np.arange(kk, dtype=np.uint64)[None]).sum(axis=1).astype(np.uint64).view(np.int64)
    off = np.concatenate([[0], np.cumsum(ref["pair_ok"].sum(axis=1))])
    got = ([ref["seg"], ref["score"], ref["key"], ref["row"]],
           [ref["sel_idx"], ref["sel_score"], ref["pair_score"], ref["pair_seg"], mask, off])
    check_against_ref(got, ref, k, self_check=True)


@pytest.mark.parametrize("alpha", [0.0, 0.65, 1.0])
def test_alpha_at_its_ends(alpha):
    thr, ws, k = 0.03, 10.24, 2
    b = make_batch(41, 4, 25, 23, 31, thr)
    ref = settle(b, thr, alpha, k, ws)
    (seg, score, key, row), rec = got = run_kernels(b, 25, thr, alpha, k, ws)
    check_against_ref(got, ref, k)
    if alpha in (0.0, 1.0):                                    # pow(x, 1) = x and pow(x, 0) = 1: the fused score is one stream's
        one = rec[1][:, 1 if alpha == 0.0 else 0, :]           # sel_score of the noun (alpha 0) or the verb (alpha 1)
        want = np.repeat(one, k, axis=1) if alpha == 1.0 else np.tile(one, (1, k))
        assert np.array_equal(rec[2], want)


def test_window_start_beyond_fp32_resolution():
    thr, alpha, ws, k = 0.03, 0.65, 10.24, 2
    b = make_batch(7, 4, 25, 11, 23, thr, start0=3000.0)
    check_against_ref(run_kernels(b, 25, thr, alpha, k, ws), settle(b, thr, alpha, k, ws), k)


def test_strided_head_slices_need_no_copy():
    thr, alpha, ws, k, nq = 0.03, 0.65, 30.0, 3, 21
    b = make_batch(11, 3, nq, 97, 300, thr)
    ref = settle(b, thr, alpha, k, ws)
    wide = torch.full((63, 97 + 300 + 40), 50.0, device=DEV)     # anything read outside the slices would win the selection
    wide[:, 13:13 + 97] = torch.from_numpy(b["vl"]).to(DEV)
    wide[:, 120:120 + 300] = torch.from_numpy(b["nl"]).to(DEV)
    vv, nv = wide[:, 13:13 + 97], wide[:, 120:120 + 300]
    assert vv.stride(0) == 437 and not vv.is_contiguous() and not nv.is_contiguous()
    check_against_ref(run_kernels(b, nq, thr, alpha, k, ws, vl_dev=vv, nl_dev=nv), ref, k)


def test_equal_scores_go_to_the_lower_class():
    """integer logits: every row repeats its scores; saturated logits tie at score 1.0 and at score 0"""
    thr, alpha, ws, k, nq = 0.03, 0.65, 10.24, 3, 8
    b = make_batch(19, 2, nq, 70, 130, thr)
    rng = np.random.default_rng(2)
    b["vl"] = rng.integers(-6, 3, size=b["vl"].shape).astype(np.float32)
    b["nl"] = rng.integers(-6, 3, size=b["nl"].shape).astype(np.float32)
    b["vl"][6] = np.where(np.arange(70) % 5 == 3, 110.0, -110.0)            # ties at 1.0 (first at class 3) and at 0
    b["nl"][6] = np.where(np.isin(np.arange(130), (1, 65)), 95.0, -110.0)   # two ones (1 and 65), then zeros from class 0
    b["vl"][7] = -110.0                                                     # every score 0: classes 0, 1, 2; w = 0 / 0
    b["nl"][7] = np.where(np.arange(130) == 129, 110.0, 100.0)              # 110 and 100 both round to 1.0: class 0 first
    b["vr"][6:8], b["nr"][6:8] = (0.2, 0.6), (0.1, 0.5)
    ref = reference(b, thr, alpha, k, ws)
    assert not (_near(ref["sel_score"], thr).any() or _near(ref["pair_score"], thr).any())
    assert ref["sel_idx"][6, 0].tolist() == [3, 8, 13] and ref["sel_idx"][6, 1].tolist() == [1, 65, 0]
    assert ref["sel_idx"][7, 0].tolist() == [0, 1, 2] and ref["sel_idx"][7, 1].tolist() == [0, 1, 2]
    assert (ref["sel_score"][6, 0] == 1.0).all() and ref["sel_score"][6, 1].tolist() == [1.0, 1.0, 0.0]
    dup = [len(set(r.tolist())) < 3 for r in ref["sel_score"][:6, 0]]
    assert any(dup)                                                         # the tie rule decides inside the selection
    check_against_ref(run_kernels(b, nq, thr, alpha, k, ws), ref, k)


def test_a_nan_logit_costs_its_slot_and_nothing_else():
    thr, alpha, ws, k, nq = 0.03, 0.65, 10.24, 2, 8
    b = make_batch(23, 2, nq, 20, 90, thr)
    b["vl"][4:8] += 4.0
    b["nl"][4:8] += 4.0
    b["vr"][4:8], b["nr"][4:8] = (0.2, 0.6), (0.1, 0.5)
    b["vl"][5, 7] = np.nan
    b["nl"][6, 77] = np.nan
    b["vl"][7, 0] = b["nl"][7, 89] = np.nan
    ref = settle(b, thr, alpha, k, ws)
    assert ref["sel_idx"][5, 0, 0] == 7 and ref["sel_idx"][6, 1, 0] == 77 and np.isnan(ref["sel_score"][5, 0, 0])
    assert ref["pair_ok"][5].tolist() == [False, False, True, True] and ref["pair_ok"][6].tolist() == [False, True, False, True]
    assert ref["pair_ok"][7].tolist() == [False, False, False, True]
    check_against_ref(run_kernels(b, nq, thr, alpha, k, ws), ref, k)


@pytest.mark.parametrize("thr", [0.0, 1.0, 1.5])
def test_thresholds_at_the_ends_of_the_unit_interval(thr):
    alpha, ws, k, nq = 0.65, 10.24, 2, 16
    b = make_batch(17, 2, nq, 20, 33, 0.03)
    ref = settle(b, thr, alpha, k, ws)
    (seg, score, key, row), _ = got = run_kernels(b, nq, thr, alpha, k, ws)
    check_against_ref(got, ref, k)
    assert (len(row) == 0) if thr >= 1.0 else (len(row) > 2 * nq)          # thr 0: every pair of a valid row


def test_every_proposal_invalid_gives_no_candidates():
    b = make_batch(13, 2, 30, 44, 50, 0.03, invalid="all")
    ref = settle(b, 0.03, 0.65, 3, 30.0)
    (seg, score, key, row), _ = got = run_kernels(b, 30, 0.03, 0.65, 3, 30.0)
    check_against_ref(got, ref, 3)
    assert seg.shape == (0, 2) and score.shape == (0,) and key.shape == (0,) and row.shape == (0,)


def test_a_capacity_below_the_count_clips_the_output():
    """out= buffers shorter than the list, inside a guard band: the first `cap` candidates and not a word more"""
    thr, alpha, ws, k, nq, B = 0.03, 0.65, 10.24, 3, 21, 4
    b = make_batch(29, B, nq, 40, 60, thr)
    ref = settle(b, thr, alpha, k, ws)
    n = len(ref["row"])
    cap, G = n - 17, 64
    assert cap > 20
    big = (torch.full((cap + 2 * G, 2), -7.0, device=DEV), torch.full((cap + 2 * G,), -7.0, device=DEV),
           torch.full((cap + 2 * G,), -7, dtype=torch.int64, device=DEV), torch.full((cap + 2 * G,), -7, dtype=torch.int32, device=DEV))
    out = tuple(t[G:G + cap] for t in big)
    res = ts.candidates(dv(b["vl"]), dv(b["nl"]), dv(b["vr"]), dv(b["nr"]), dv(b["starts"]), ws, dv(b["queries"]).max(),
                        dv(b["vidx"]), nq, thr, alpha, k, out=out)
    torch.cuda.synchronize()
    assert int(res[4].item()) == n                                           # the count is the whole list's
    assert np.array_equal(out[3].cpu().numpy(), ref["row"][:cap]) and np.array_equal(out[2].cpu().numpy(), ref["key"][:cap])
    assert np.array_equal(out[0].cpu().numpy(), ref["seg"][:cap]) and ulp_apart(out[1].cpu().numpy(), ref["score"][:cap]).max() <= 3
    for t in big:
        assert bool((t[:G] == -7).all()) and bool((t[G + cap:] == -7).all())


def test_library_argument_checks():
    lib = L.load()
    z = torch.zeros(4096, device=DEV)
    # one region of z per argument: logits, regressions, window starts, max_time, the records, the offsets, the outputs
    at = lambda i: z[256 * i:].data_ptr()
    ALL = tuple(at(i) for i in range(16))

    def count(R=8, Cv=4, Cn=6, Nq=4, k=2, ld_v=4, ld_n=6, ptrs=ALL, off=at(15)):
        a = ptrs if ptrs is not None else (None,) * 16
        return lib.timhip_ts_candidates_count(a[0], ld_v, a[1], ld_n, a[2], a[3], a[4], 1.0, a[5], R, Cv, Cn, Nq, k, 0.03, 0.65, 0.35,
                                              a[6], a[7], a[8], a[9], a[10], off, None)

    def emit(R=8, Cv=4, Cn=6, Nq=4, k=2, cap=16, ptrs=ALL):
        a = ptrs if ptrs is not None else (None,) * 16
        return lib.timhip_ts_candidates_emit(a[6], a[8], a[9], a[10], a[15], a[5], R, Cv, Cn, Nq, k, cap, a[11], a[12], a[13], a[14], None)

    assert count() == 0 and emit() == 0
    EINVAL = -1
    assert count(ptrs=None) == EINVAL and emit(ptrs=None) == EINVAL          # null pointers with R > 0
    assert count(off=None) == EINVAL
    assert count(k=0) == EINVAL and emit(k=0) == EINVAL
    assert count(k=5) == EINVAL and emit(k=5) == EINVAL                      # top_k > min(Cv, Cn)
    assert count(R=6) == EINVAL and emit(R=6) == EINVAL                      # R not a multiple of Nq
    assert count(ld_v=3) == EINVAL and count(ld_n=5) == EINVAL               # row stride < C
    assert emit(cap=-1) == EINVAL
    assert count(Cv=20, Cn=20, ld_v=20, ld_n=20, k=9) == L.EUNSUPPORTED and emit(Cv=20, Cn=20, k=9) == L.EUNSUPPORTED
    assert count(R=1 << 26, Nq=1, Cv=8, Cn=8, ld_v=8, ld_n=8, k=8, ptrs=None) == L.EUNSUPPORTED      # R * k * k beyond int32
    assert count(Cv=4000, Cn=97, ld_v=4000, ld_n=97) == L.EUNSUPPORTED       # the block's scores do not fit its LDS
    z.fill_(5.0)
    torch.cuda.synchronize()
    assert count(R=0, ptrs=None) == 0 and emit(R=0, ptrs=None) == 0          # a valid empty call ...
    torch.cuda.synchronize()
    assert z.view(torch.int32)[256 * 15].item() == 0 and z[256 * 15 + 1].item() == 5.0      # ... that still writes row_offsets[0] = 0


# ---- the collector ------------------------------------------------------------------------------------------------------------
def _fixture():
    return np.load(os.path.join(H.GOLDEN, "twostream_small.npz"))


def _collect(g, tag, sizes=(2, 2, 2), **kw):
    """the fixture's six windows in updates of `sizes` windows"""
    from tim_amd import TwoStreamCollector
    nq = int(g["num_queries"])
    cat = lambda a: torch.from_numpy(np.concatenate(list(a))).to(DEV)
    vl, nl, vr, nr = cat(g["verb_logits"]), cat(g["noun_logits"]), cat(g["verb_reg"]), cat(g["noun_reg"])
    vids, starts = list(g["video_ids"].ravel()), g["window_start"].ravel()
    col = TwoStreamCollector(num_verbs=vl.shape[1], num_nouns=nl.shape[1], score_threshold=float(g["threshold"]),
                             verb_alpha=float(g[tag + "_alpha"]), top_k=int(g[tag + "_top_k"]), **kw)
    w = 0
    for n in sizes:
        rows = slice(w * nq, (w + n) * nq)
        qt = torch.from_numpy(np.tile(g["queries"][None], (n, 1, 1))).to(DEV)
        col.update(((None, None, vl[rows], None), (vr[rows], None)), ((None, None, nl[rows], None), (nr[rows], None)), (qt, None),
                   _meta(vids[w:w + n], starts[w:w + n], float(g["window_size"])))
        w += n
    assert w == len(vids)
    return col


@pytest.mark.parametrize("tag", ["k1", "k3", "k2a"])
def test_collector_matches_the_reference_fixture(tag):
    g = _fixture()
    col = _collect(g, tag)
    assert col.video_ids == ["P03_01", "P01_07", "P02_05"]
    res = col.results(sigma=float(g["sigma"]))
    names = list(g["video_names"])
    assert sorted(res) == sorted(names[i] for i in np.unique(g[tag + "_res_video"]))
    for vid, entries in res.items():
        r = g[tag + "_res_video"] == names.index(vid)
        want = [(int(a), int(n), float(s0), float(s1)) for a, n, s0, s1 in
                zip(g[tag + "_res_verb"][r], g[tag + "_res_noun"][r], g[tag + "_res_seg"][r, 0], g[tag + "_res_seg"][r, 1])]
        assert [(e["verb"], e["noun"], e["segment"][0], e["segment"][1]) for e in entries] == want       # the list, in order
        assert all(e["action"] == "%d,%d" % (e["verb"], e["noun"]) for e in entries)
        for e, w in zip(entries, g[tag + "_res_score"][r]):
            assert abs(e["score"] - w) <= 2e-5 * max(abs(w), 1e-3), (vid, e)
    # the candidates against the restatement's (which tests/test_twostream_ref.py pins to the reference's, row by row)
    ref = T.Collector(11, 23, float(g["threshold"]), float(g[tag + "_alpha"]), int(g[tag + "_top_k"]))
    for b in range(3):
        ref.update(g["verb_logits"][b], g["noun_logits"][b], g["verb_reg"][b], g["noun_reg"][b], g["queries"], list(g["video_ids"][b]),
                   g["window_start"][b], float(g["window_size"]))
    seg, score, key = [t.cpu().numpy() for t in col.candidates()]
    rc = ref.candidates()
    assert np.array_equal(key, rc["key"]) and np.array_equal(seg, rc["seg"]) and ulp_apart(score, rc["score"]).max() <= 3


def test_collector_gives_the_same_candidates_however_the_windows_are_batched():
    g = _fixture()
    a, b, c = _collect(g, "k3", (6,)), _collect(g, "k3", (2, 2, 2)), _collect(g, "k3", (1,) * 6)
    for other in (b, c):
        for x, y in zip(a.candidates(), other.candidates()):
            assert torch.equal(x, y)
        for x, y in zip(a.detections(sigma=0.25), other.detections(sigma=0.25)):
            assert torch.equal(x, y)
    assert a.candidates()[1].numel() == len(g["k3_cand_verb"])
    a.reset()
    assert a.video_ids == [] and a.candidates()[1].numel() == 0 and a.results() == {}


def test_verb_and_noun_task_labels_and_the_scorer():
    """task="verb" / "noun" relabel the same detections; DetectionScorer.score(col) equals evaluate_results on the file's
    numbers with integer action labels, bit for bit"""
    from tim_amd import DetectionScorer
    g = _fixture()
    col = _collect(g, "k3")
    nms = dict(sigma=float(g["sigma"]))
    act, verb, noun = col.detections(**nms), col.detections(task="verb", **nms), col.detections(task="noun", **nms)
    assert torch.equal(verb[2], act[2] // 23) and torch.equal(noun[2], act[2] % 23) and int(act[2].max()) < 11 * 23
    for t in (verb, noun):
        assert all(torch.equal(x, y) for x, y in zip(act[:2] + act[3:], t[:2] + t[3:]))
    segs, scores, labels, video = (t.cpu().numpy() for t in act)
    assert scores.shape[0] > 50
    rng = np.random.default_rng(3)
    pick = np.arange(0, scores.shape[0], 2)                               # ground truth: jittered detections, one video left out
    pick = pick[video[pick] != 2]
    gt_seg = np.round(segs[pick].astype(np.float64) + rng.normal(0, 0.2, size=(len(pick), 2)), 2)
    gt_seg[:, 1] = np.maximum(gt_seg[:, 1], gt_seg[:, 0] + 0.01)
    gt_video = [col.video_ids[int(v)] for v in video[pick]]
    a, b = DetectionScorer(gt_video, gt_seg, labels[pick]), DetectionScorer(gt_video, gt_seg, labels[pick])
    mAP_a, avg_a = a.score(col, **nms)
    res = {vid: [{"action": e["verb"] * 23 + e["noun"], "score": e["score"], "segment": e["segment"]} for e in entries]
           for vid, entries in col.results(**nms).items()}
    mAP_b, avg_b = b.evaluate_results(res)
    assert torch.equal(a.tp, b.tp) and torch.equal(a.lock, b.lock) and torch.equal(a.order, b.order)
    assert torch.equal(a.ap, b.ap) and np.array_equal(mAP_a, mAP_b) and avg_a == avg_b
    assert int(a.tp[0].sum()) > 10 and 0.0 < avg_a <= 1.0
    v = DetectionScorer(gt_video, gt_seg, labels[pick] // 23)
    assert 0.0 < v.score(col, task="verb", **nms)[1] <= 1.0               # one collector feeds the scorer per task


def test_one_model_with_verb_and_noun_heads_passed_twice():
    g = _fixture()
    from tim_amd import TwoStreamCollector
    nq = int(g["num_queries"])
    two = _collect(g, "k3")
    one = TwoStreamCollector(11, 23, float(g["threshold"]), 0.65, 3, verb_head="verb", noun_head="noun")
    for b in range(3):
        output = ((dv(g["verb_logits"][b]), dv(g["noun_logits"][b]), None, None), (dv(g["verb_reg"][b]), None))
        qt = torch.from_numpy(np.tile(g["queries"][None], (2, 1, 1))).to(DEV)
        one.update(output, output, (qt, None), _meta(g["video_ids"][b], g["window_start"][b], float(g["window_size"])))
    # the same scores; the noun stream's segment is now the verb stream's, so the blend is that segment (w + w1 = 1 up to an ulp)
    (s1, c1, k1), (s2, c2, k2) = one.candidates(), two.candidates()
    ref = T.Collector(11, 23, float(g["threshold"]), 0.65, 3)
    for b in range(3):
        ref.update(g["verb_logits"][b], g["noun_logits"][b], g["verb_reg"][b], g["verb_reg"][b], g["queries"], list(g["video_ids"][b]),
                   g["window_start"][b], float(g["window_size"]))
    rc = ref.candidates()
    assert np.array_equal(k1.cpu().numpy(), rc["key"]) and np.array_equal(s1.cpu().numpy(), rc["seg"])
    assert ulp_apart(c1.cpu().numpy(), rc["score"]).max() <= 3 and k1.numel() > 100 and not torch.equal(k1, k2)


def test_update_checks_its_arguments_and_host_tensors_raise():
    from tim_amd import TwoStreamCollector
    col = TwoStreamCollector(11, 23)
    z = lambda *s: torch.zeros(*s, device=DEV)
    stream = lambda R, C: ((None, None, z(R, C), None), (z(R, 2), None))
    meta = _meta(["a", "b"], [0.0, 1.0], 10.0)
    with pytest.raises(ValueError, match="proposal rows"):
        col.update(stream(8, 11), stream(6, 23), (z(2, 4, 2), None), meta)           # the streams differ in rows
    with pytest.raises(ValueError, match="divide"):
        col.update(stream(7, 11), stream(7, 23), (z(2, 4, 2), None), meta)           # 7 rows, 2 windows
    with pytest.raises(ValueError, match="classes"):
        col.update(stream(8, 12), stream(8, 23), (z(2, 4, 2), None), meta)
    host = ((None, None, torch.zeros(8, 11), None), (torch.zeros(8, 2), None))
    with pytest.raises(L.TimHipError, match="no CPU fallback"):
        col.update(host, stream(8, 23), (z(2, 4, 2), None), meta)
    assert col.video_ids == [] and col._chunks == []
    with pytest.raises(L.TimHipError):                                               # the library's own refusal surfaces
        ts.candidates(z(8, 11), z(8, 23), z(8, 2), z(8, 2), z(2).double(), 10.0, z(()), z(2).int(), 4, 0.03, 0.65, 9)


def test_both_calls_replay_in_a_graph_on_new_inputs():
    """count + emit captured once with a worst-case-sized output (R * k * k slots) and replayed after the inputs changed in
    place; slots past the total keep their sentinel"""
    nq, Cv, Cn, thr, alpha, ws, B, k = 21, 40, 65, 0.03, 0.65, 30.0, 4, 3
    R = B * nq
    b1, b2 = make_batch(31, B, nq, Cv, Cn, thr), make_batch(32, B, nq, Cv, Cn, thr)
    refs = {id(b): settle(b, thr, alpha, k, ws) for b in (b1, b2)}
    vl, nl, vr, nr, starts, vidx = dv(b1["vl"]), dv(b1["nl"]), dv(b1["vr"]), dv(b1["nr"]), dv(b1["starts"]), dv(b1["vidx"])
    mt = dv(b1["queries"]).max().reshape(1)
    cap = R * k * k
    out = (torch.empty((cap, 2), device=DEV), torch.empty(cap, device=DEV), torch.empty(cap, dtype=torch.int64, device=DEV),
           torch.empty(cap, dtype=torch.int32, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ts.candidates(vl, nl, vr, nr, starts, ws, mt, vidx, nq, thr, alpha, k, out=out)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ts.candidates(vl, nl, vr, nr, starts, ws, mt, vidx, nq, thr, alpha, k, out=out)
    for b in (b1, b2, b1):
        vl.copy_(dv(b["vl"])); nl.copy_(dv(b["nl"])); vr.copy_(dv(b["vr"])); nr.copy_(dv(b["nr"])); starts.copy_(dv(b["starts"]))
        mt.copy_(dv(b["queries"]).max().reshape(1))
        for t, fill in zip(out, (-7.0, -7.0, -7, -7)):
            t.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        n = int(res[4].item())
        ref = refs[id(b)]
        seg, score, key, row = [t[:n].cpu().numpy() for t in out]
        assert n == len(ref["row"]) and 0 < n < cap
        assert np.array_equal(row, ref["row"]) and np.array_equal(key, ref["key"]) and np.array_equal(seg, ref["seg"])
        assert ulp_apart(score, ref["score"]).max() <= 3
        assert bool((out[1][n:] == -7.0).all()) and bool((out[2][n:] == -7).all()) and bool((out[3][n:] == -7).all())
