"""1-D segment NMS: oracle/nms_oracle.c against vectors produced by the reference's own nms_cpu.cpp and
nms.py (tests/golden/make_golden_nms.py).  CPU only; bit-exact.  Then the oracle's two weight modes against each other over
every input of tests/nms_cases.py (same selection; the measured distance of the gaussian scores, which is the bound the GPU tests
use against glibc), and the proof, from the oracle's pruned-per-step counts, that each new input reaches the kernel path it is
meant for."""
import glob
import os

import numpy as np
import pytest

from oracle import nms_oracle as N
from tests import nms_cases as K
from tests.helpers import GOLDEN, NMS_GLIBC_RTOL, NMS_GLIBC_ULP
from tests.golden.make_golden_nms_inputs import make_degenerate, make_segments, make_classes

CASES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "nms_*.npz")) if "batched" not in f)
BATCHED = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "nms_batched_*.npz")))


@pytest.mark.parametrize("case", CASES)
def test_nms_oracle_matches_reference(case):
    g = np.load(os.path.join(GOLDEN, case))
    segs, scores = make_segments(int(g["seed"]), int(g["n"]), bool(g["ties"]))
    keep = N.nms_1d(segs, scores, float(g["iou"]), order=g["order"])
    assert np.array_equal(keep, g["keep"])
    inds, dets = N.softnms_1d(segs, scores, float(g["iou"]), float(g["sigma"]), float(g["min_score"]), int(g["method"]))
    assert np.array_equal(inds, g["soft_inds"])
    assert np.array_equal(dets, g["soft_dets"])           # bit-exact scores too (same libm expf on the same host)


@pytest.mark.parametrize("case", BATCHED)
def test_batched_nms_oracle_matches_reference(case):
    g = np.load(os.path.join(GOLDEN, case))
    segs, scores = make_segments(int(g["seed"]), int(g["n"]), False)
    cls = make_classes(int(g["seed"]), int(g["n"]), int(g["ncls"]))
    assert np.array_equal(cls, g["cls"])
    S, Cc, Ll = N.batched_nms(segs, scores, cls, 0.1, 0.001, sigma=0.4, method=2, nms=str(g["kind"]))
    assert np.array_equal(Cc, g["scores"]) and np.array_equal(S, g["segs"]) and np.array_equal(Ll, g["labels"])


# ---- the two weight modes of the oracle: "glibc" (expf, the reference's arithmetic) and "rn" ((float)exp((double)x), the
# ---- arithmetic of tim_amd/csrc/nms.hip), over every input of tests/nms_cases.py

def ulp_distance(a, b):
    """distance of two float32 arrays in units of the last place (the floats of one sign are ordered like their bit patterns)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def reach(n, pruned):
    """per selection step of a group of n elements: (pruned, alive), `alive` being the elements that survive the step's
    decay (the length of the front the compaction scans; `pruned` is the length of the tail it scans)"""
    pruned = np.asarray(pruned)
    before = n - np.concatenate([[0], np.cumsum(pruned)[:-1]])          # nsegs at the start of each step
    return pruned, before - np.arange(len(pruned)) - 1 - pruned


def test_the_first_entries_keep_their_arguments():
    """nms_1d_oracle (5) and softnms_1d_oracle (9) are called through ctypes by every earlier front of this library: an argument
    added to one of them is read from whatever the caller left in its slot.  New outputs come as new entries."""
    import re
    src = open(os.path.join(os.path.dirname(N.__file__), "nms_oracle.c")).read()
    for name, count in (("nms_1d_oracle", 5), ("softnms_1d_oracle", 9), ("softnms_1d_oracle_rn", 9),
                        ("softnms_1d_oracle_pruned", 10), ("softnms_1d_oracle_rn_pruned", 10)):
        m = re.search(r"^int64_t %s\(([^)]*)\)" % name, src, flags=re.M)
        assert m and len(m.group(1).split(",")) == count, name
        assert hasattr(N._load(), name), name


def test_pruned_per_step_accounts_for_every_element():
    for c in K.all_cases():
        inds, dets, pruned = K.oracle(c.name, "rn")
        assert len(pruned) == len(inds) and len(inds) + pruned.sum() == len(c.scores), c.name
        assert len(np.unique(inds)) == len(inds), c.name
        plain = N.softnms_1d(c.segs, c.scores, c.iou, c.sigma, c.min_score, c.method)      # the nullable argument left out
        assert np.array_equal(plain[0], K.oracle(c.name, "glibc")[0]) and np.array_equal(plain[1], K.oracle(c.name, "glibc")[1])


def test_both_modes_select_the_same():
    for c in K.all_cases():
        gi, gd, gp = K.oracle(c.name, "glibc")
        ri, rd, rp = K.oracle(c.name, "rn")
        assert np.array_equal(gi, ri), c.name
        assert np.array_equal(gd[:, :2], rd[:, :2]) and np.array_equal(gp, rp), c.name
        if c.method != 2:                                               # no exponential is evaluated: one arithmetic
            assert np.array_equal(gd[:, 2].view(np.int32), rd[:, 2].view(np.int32)), c.name


def test_gaussian_scores_of_the_two_modes_within_the_recorded_bound():
    """Reference against reference: the largest distance between the glibc and the rn scores over all method 2 inputs.
    Measured (docs/measurement_log.md, 7s): 8 ulp, 9.39e-7 relative, both on degenerate/4097 with min_score 0 (3585 selections,
    nothing positive ever pruned: the longest chain of decay steps of the set); the bounds are twice that."""
    worst_ulp, worst_rel, where = 0, 0.0, None
    differing = 0
    for c in K.all_cases():
        if c.method != 2:
            continue
        g, r = K.oracle(c.name, "glibc")[1][:, 2], K.oracle(c.name, "rn")[1][:, 2]
        d = ulp_distance(g, r)
        if not d.any():
            continue
        differing += 1
        ne = d > 0
        rel = (np.abs(g[ne].astype(np.float64) - r[ne]) / np.abs(r[ne].astype(np.float64))).max()
        if rel > worst_rel:
            where = c.name
        worst_ulp, worst_rel = max(worst_ulp, int(d.max())), max(worst_rel, float(rel))
    print("glibc vs rn: %d ulp, %.3e relative (worst: %s), %d inputs differ" % (worst_ulp, worst_rel, where, differing))
    assert differing > 0                       # the modes are two arithmetics: "bit-identical to glibc" is not what holds
    assert worst_ulp <= NMS_GLIBC_ULP and worst_rel <= NMS_GLIBC_RTOL, (worst_ulp, worst_rel, where)


@pytest.mark.parametrize("method", [0, 1, 2])
def test_clustered_inputs_reach_the_repeated_compaction_pass(method):
    """Conditions on the oracle alone.  The compaction of a step scans the pruned tail and the alive front in chunks of one block
    (512 threads for 1025 .. 4096 elements, 1024 beyond); a chunk loop takes a second iteration, with its running offset, only
    when the step prunes (tail) or keeps (front) more elements than the block is wide."""
    big = [c for c in K.clustered_cases(method) if len(c.scores) in K.BLOCK_WIDTH]       # distinct scores, then quantised ones
    assert [c.name.split("/")[0] for c in big] == ["clustered"] * 2 + ["clustered_ties"] * 2
    for c in big[2:]:                                                   # many equal scores meet in one group
        assert len(np.unique(c.scores)) == 16
    for c in big:
        n = len(c.scores)
        pruned, alive = reach(n, K.oracle(c.name, "rn")[2])
        if method == 0:
            assert pruned.max() > K.BLOCK_WIDTH[n], (c.name, pruned.max())        # the tail loop runs a second iteration
        else:
            assert pruned.max() > 64, (c.name, pruned.max())                      # the rank of a tail element crosses a wave
            # ... and so does the front loop, in a step that moves something.  (Not with method 0: a step that prunes 955 of 1100
            # leaves a front of 144.  There the front's second iteration comes from the scattered groups, see below.)
            assert ((alive > K.BLOCK_WIDTH[n]) & (pruned > 0)).any(), c.name
    # the figures of the table these inputs were chosen by (seed 7, iou 0.1, sigma 0.4)
    table = {0: [(4, 955), (8, 1809)], 1: [(22, 327), (44, 519)], 2: [(25, 364), (50, 666)]}[method]
    got = [(len(K.oracle(c.name, "rn")[0]), int(K.oracle(c.name, "rn")[2].max())) for c in big[:2]]
    assert got == table, got


def test_scattered_groups_reach_only_the_front_loops_second_iteration():
    """What the scattered groups (make_segments) of 1025 elements and more do and do not reach: their steps prune while more than
    a block's width stays alive (the front loop iterates, its offset carried along), but no step prunes more than 195 elements
    (the tail loop never iterates twice): that is what the clustered and the degenerate groups add."""
    for c in K.many_cases():
        n = len(c.scores)
        if n <= 1024:
            continue
        width = 512 if n <= 4096 else 1024
        pruned, alive = reach(n, K.oracle(c.name, "rn")[2])
        assert ((alive > width) & (pruned > 0)).any() and pruned.max() <= 195 < width, c.name


def test_tie_inputs_keep_everything_at_zero():
    for c in K.tie_cases():
        inds, dets, pruned = K.oracle(c.name, "rn")
        n = len(c.scores)
        assert len(inds) == n and pruned.sum() == 0
        assert 2 * int((dets[:, 2] == 0.0).sum()) >= n, c.name
        # among equal scores the first of the CURRENT order wins, which the swaps of the selections before have permuted: the
        # order of the zero-score selections is not the order of the rows
        z = inds[dets[:, 2] == 0.0]
        assert (np.diff(z) < 0).any(), c.name


def test_degenerate_inputs_are_what_they_say():
    for n in K.DEGENERATE_SIZES:
        segs, scores = make_degenerate(5, n)
        base_s, base_c = make_segments(5, n, ties=False)
        r = np.arange(n)
        q0, q1, q2, q3 = (r[r % 4 == k] for k in range(4))
        assert np.array_equal(segs[q0], base_s[q0]) and np.array_equal(scores[q0], base_c[q0])
        assert np.array_equal(segs[q1], segs[q1 - 1]) and np.array_equal(scores[q1], scores[q1 - 1])
        assert np.array_equal(segs[q2, 0], segs[q2, 1]) and np.array_equal(scores[q2], base_c[q2])
        assert (scores[q3] <= 0).all() and np.signbit(scores[q3][scores[q3] == 0]).any() and (scores[q3] < 0).any()
        assert (scores[q3] == 0).any() and not np.signbit(scores[q3][scores[q3] == 0]).all()
        assert min(len(q1), len(q2), len(q3)) >= n // 4 and not np.isnan(scores).any() and not np.isnan(segs).any()


def test_degenerate_groups_reach_both_loops_in_one_step():
    """min_score 0.001: the first step prunes the scores <= 0, more than the block's width, while more than the block's width
    stays alive, and hundreds of selections among duplicates follow (where the order the compaction left decides).  4097 elements
    on 1024 threads with method 0; 2200 elements on 512 threads with every method."""
    for method, n, width in [(0, 4097, 1024), (0, 2200, 512), (1, 2200, 512), (2, 2200, 512)]:
        c = K.degenerate_cases(method, 0.001)[K.DEGENERATE_SIZES.index(n)]
        inds, _, pr = K.oracle(c.name, "rn")
        pruned, alive = reach(len(c.scores), pr)
        assert len(c.scores) == n and pruned[0] > width and alive[0] > width and len(inds) > 500, (c.name, pruned[0], alive[0])
