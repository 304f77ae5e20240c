"""Seeded inputs shared by make_golden_nms.py (generation, build container) and the NMS tests (regeneration)."""
import numpy as np

from tim_amd import synth


def make_segments(seed, n, ties):
    """segments in [0, 100) s with lengths 0.2 .. 20 s; scores in (0, 1); `ties`: quantise scores so that equal values occur"""
    u = synth.uniform01(seed, "nms", (n, 3))
    start = (u[:, 0] * 100.0).astype(np.float32)
    length = (0.2 + u[:, 1] * u[:, 1] * 19.8).astype(np.float32)
    segs = np.stack([start, start + length], 1).astype(np.float32)
    scores = u[:, 2].astype(np.float32)
    if ties:
        scores = (np.floor(scores * 16) / 16 + 1 / 32).astype(np.float32)
    return segs, scores


def make_clustered(seed, n, ncl):
    """make_segments(seed, n, ties=False) with the starts gathered into `ncl` clusters: every segment of a cluster starts within
    one second of the others, so one selection suppresses most of its cluster (hundreds or thousands of prunes in one step)"""
    segs, scores = make_segments(seed, n, ties=False)
    start = (np.floor(segs[:, 0] / np.float32(100.0) * np.float32(ncl)) * np.float32(100.0 / ncl)
             + segs[:, 0] % np.float32(1.0)).astype(np.float32)
    length = segs[:, 1] - segs[:, 0]
    return np.stack([start, start + length], 1).astype(np.float32), scores


def make_degenerate(seed, n):
    """make_segments(seed, n, ties=False) with one change per quarter of the rows (row r belongs to quarter r % 4):
    quarter 1: an exact duplicate, segment and score, of the row before it (which is of quarter 0 and left as generated);
    quarter 2: zero length (x2 == x1);  quarter 3: a score <= 0, cycling through +0.0, -0.0, -0.25 and the row's own score negated.
    No NaN (the CPU routine's behaviour there is an accident of comparison order, and the product's scores are sigmoids)."""
    segs, scores = make_segments(seed, n, ties=False)
    segs, scores = segs.copy(), scores.copy()
    r = np.arange(n)
    dup = r[r % 4 == 1]
    segs[dup], scores[dup] = segs[dup - 1], scores[dup - 1]
    zero = r[r % 4 == 2]
    segs[zero, 1] = segs[zero, 0]
    neg = r[r % 4 == 3]
    kind = (neg // 4) % 4
    scores[neg] = np.where(kind == 0, np.float32(0.0), np.where(kind == 1, np.float32(-0.0),
                           np.where(kind == 2, np.float32(-0.25), -scores[neg]))).astype(np.float32)
    return segs, scores


def make_classes(seed, n, ncls):
    return np.floor(synth.uniform01(seed, "nms_cls", (n,)) * ncls).astype(np.int64)
