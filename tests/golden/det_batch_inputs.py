"""Seeded in-memory tables of a small DETECTION sliding-window dataset (what the reference's detection constructor builds from
its pickles and .npy files), shared by make_golden_det_batch.py and the tests.

The tables are built to carry the cases the time normalisation `clamp(round(t - start, decimals=3) / window_size, 0)` can get
wrong (tests/test_det_batch_ref.py asserts that they are there):

  video 0   window 0 starts at 0.0 and reads feature rows whose times are PLANTED: fp32 values d for which rounding to three
            decimals in float64 gives another fp32 result than the fp32 steps rint(d * 1000) / 1000 (found by a seeded search);
            the other rows are arbitrary fp32 times, where a product with 0.001f instead of the division differs about half
            the time
  video 1   window starts in the thousands of seconds, feature times on a 1/16 s grid: (t - start) * 1000 lands exactly on .5
            with an even and an odd neighbour (0.0625 -> 0.062, 0.1875 -> 0.188), and a feature time before the window's start
  video 2   times of a 0.2 s hop as fp32, window starts that are no fp32 numbers (1234.2)

Windows carry 0, 1 and the maximum number of actions per modality; some ground-truth segments begin before their window.
"""
import numpy as np

from tim_amd import synth

NF, V_NUM_AUG, A_NUM_AUG, MAX_V, MAX_A = 6, 3, 2, 3, 2
VIDEOS = ["P01_00", "P01_01", "P02_00"]
F32 = np.float32


def round3_f32(d):
    """torch.round(d, decimals=3) on fp32: a correctly rounded product, round half to even, a correctly rounded division"""
    d = np.asarray(d, F32)
    return (np.rint(d * F32(1000.0)) / F32(1000.0)).astype(F32)


def round3_f64(d):
    """the same steps in float64, rounded to fp32 at the end (NOT what torch computes)"""
    return (np.rint(np.asarray(d, F32).astype(np.float64) * 1000.0) / 1000.0).astype(F32)


def round3_mul(d):
    """a product with 0.001f in place of the division (NOT what torch computes)"""
    d = np.asarray(d, F32)
    return (np.rint(d * F32(1000.0)) * F32(0.001)).astype(F32)


def planted(seed, count):
    """`count` fp32 values in (0.05, 2.3), ascending, on which round3_f64 differs from round3_f32"""
    cand = np.random.RandomState(seed + 90001).uniform(0.05, 2.3, 400000).astype(F32)
    hit = cand[round3_f32(cand) != round3_f64(cand)]
    assert hit.size >= count, hit.size
    return np.sort(hit[:count])


def make_tables(seed, modality, nf=NF, Cv=8, Ca=12):
    rs = np.random.RandomState(seed)
    has_v, has_a = "visual" in modality, "audio" in modality
    n_rows = [40, 48, 57]
    ft = []
    # video 0: rows 0 .. nf-1 planted (start = w[i], end = w[i + nf]), the rest arbitrary ascending fp32 times
    w = planted(seed, 2 * nf)
    st = np.sort(rs.uniform(2.5, 30.0, n_rows[0])).astype(F32)
    t0 = np.stack([st, st + F32(1.0), st + F32(0.5)], 1).astype(F32)
    t0[:nf, 0], t0[:nf, 1] = w[:nf], w[nf:]
    ft.append(t0)
    # video 1: a 1/16 s grid, rows 0 .. 23 from 2047.875 s (row 2 is 2048.0) and rows 24 .. from 3000.9375 s (row 25 is 3001.0)
    st = (F32(2047.875) + np.arange(n_rows[1], dtype=F32) * F32(0.0625)).astype(F32)
    t1 = np.stack([st, st + F32(1.125), st], 1).astype(F32)
    t1[24:, :2] += F32(3000.9375 - 2049.375)
    ft.append(t1)
    # video 2: a 0.2 s hop from 1230 s
    st = (F32(1230.0) + np.arange(n_rows[2]) * 0.2).astype(F32)
    ft.append(np.stack([st, st + F32(1.0), st + F32(0.5)], 1).astype(F32))
    v_feats, v_ft, a_feats, a_ft = {}, {}, {}, {}
    for k, v in enumerate(VIDEOS):
        if has_v:
            v_feats[v] = synth.normal(seed, "dvf" + v, (n_rows[k], V_NUM_AUG, Cv)).astype(F32); v_ft[v] = ft[k]
        if has_a:
            a_feats[v] = synth.normal(seed, "daf" + v, (n_rows[k], A_NUM_AUG, Ca)).astype(F32); a_ft[v] = ft[k].copy()
    # (video, start_sec, first feature row, row stride, visual actions, audio actions)
    plan = [(0, 0.0, 0, 1, MAX_V, MAX_A), (1, 2048.0, 1, 1, 0, 0), (2, 1234.2, 21, 2, 1, 1), (0, 5.0, 8, 2, 2, 0),
            (1, 2047.0, 0, 2, 1, 2), (1, 3001.0, 24, 1, 0, 1), (2, 1231.0, 3, 2, MAX_V, 0), (0, 11.25, 20, 2, 2, 1)]
    n_win = 7 + int(rs.randint(0, 3))
    while len(plan) < n_win:
        plan.append((2, 1236.4, 30, 2, int(rs.randint(0, MAX_V + 1)), int(rs.randint(0, MAX_A + 1))))
    plan = plan[:n_win]
    windows = []
    for vid, start, first, stride, nv, na in plan:
        fi = np.arange(first, first + stride * nf, stride).astype(np.int64)
        assert fi[-1] < n_rows[vid]
        seg = lambda m: (F32(start) - F32(0.3) + np.sort(rs.rand(m, 2) * 2.8, axis=1)).astype(F32).reshape(m, 2)   # noqa: E731  (some begin before the window)
        v_lab = np.stack([rs.randint(0, 97, nv), rs.randint(0, 300, nv), rs.randint(0, 3806, nv), np.full(nv, -1)], 1).astype(np.int64).reshape(nv, 4)
        a_lab = np.stack([np.full(na, -1), np.full(na, -1), np.full(na, -1), rs.randint(0, 44, na)], 1).astype(np.int64).reshape(na, 4)
        windows.append({"video_id": VIDEOS[vid], "start_sec": float(start), "stop_sec": float(start) + nf * 0.4, "feat_indices": fi,
                        "v_gt_segments": seg(nv), "a_gt_segments": seg(na), "v_labels": v_lab, "a_labels": a_lab})
    return {"windows": windows, "v_feats": v_feats if has_v else None, "v_feat_times": v_ft if has_v else None,
            "a_feats": a_feats if has_a else None, "a_feat_times": a_ft if has_a else None, "num_feats": nf,
            "window_size": nf * 0.2 * 2, "max_visual_actions": MAX_V, "max_audio_actions": MAX_A, "v_num_aug": V_NUM_AUG,
            "a_num_aug": A_NUM_AUG, "model_modality": modality, "video_ids": sorted(VIDEOS)}
