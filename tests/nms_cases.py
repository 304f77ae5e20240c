"""Inputs of the soft-NMS tests (test infrastructure), shared by tests/test_nms_oracle.py (CPU: the two weight modes of the
oracle against each other, and the proof that each input reaches the code it is meant for) and tests/test_gpu_nms.py (the HIP
kernels against the oracle).  Every input is seeded; every oracle result is computed once per process and shared."""
import collections
import functools
import glob
import os

import numpy as np

from oracle import nms_oracle as N
from tests.helpers import GOLDEN
from tests.golden.make_golden_nms_inputs import make_clustered, make_degenerate, make_segments

Case = collections.namedtuple("Case", "name segs scores iou sigma min_score method")

IOU, SIGMA = 0.1, 0.4
GOLDEN_CASES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLDEN, "nms_*.npz")) if "batched" not in f)
# the sixteen groups of test_many_groups_all_size_classes, then the smallest group on 512 threads and the smallest on the
# global scratch with 1024 threads
MANY_SIZES = [1, 2, 63, 64, 65, 200, 256, 257, 900, 1024, 1500, 4096, 4100, 6000, 17, 300]
BORDER_SIZES = [1025, 4097]
# clustered groups: (n, ncl); per method the min_score of the issue's table; the 200-element group puts the 64-thread launch
# into the same call
CLUSTER_SEED = 7
CLUSTERED = [(1100, 1), (4200, 2)]
CLUSTER_SMALL = (200, 1)
CLUSTER_MIN_SCORE = {0: 0.001, 1: 0.05, 2: 0.05}
BLOCK_WIDTH = {1100: 512, 4200: 1024}            # threads of the block that runs a group of that size (nms.hip: size classes)
# 2200: with min_score 0.001 its first step prunes the quarter with scores <= 0, more than the 512 threads of its block, and
# hundreds of selections among duplicates follow: the one input where the order of the tail loop's second iteration at 512
# threads decides a later selection
DEGENERATE_SIZES = [300, 1025, 4097, 2200]
DEGENERATE_MIN_SCORES = [0.0, 0.001]
SMALL_GROUPS, SMALL_SEED = 3000, 31


@functools.lru_cache(maxsize=None)
def golden_case(fname):
    g = np.load(os.path.join(GOLDEN, fname))
    segs, scores = make_segments(int(g["seed"]), int(g["n"]), bool(g["ties"]))
    return Case("golden/" + fname, segs, scores, float(g["iou"]), float(g["sigma"]), float(g["min_score"]), int(g["method"]))


@functools.lru_cache(maxsize=None)
def many_cases():
    out = []
    for i, n in enumerate(MANY_SIZES + BORDER_SIZES):
        s, c = make_segments(100 + i, n, ties=(i % 3 == 0))
        out.append(Case("many/%d" % n, s, c, IOU, SIGMA, 0.001, 2))
    return out


@functools.lru_cache(maxsize=None)
def clustered_cases(method):
    """the two large clustered groups and the small one, at the method's min_score of the table"""
    out = []
    for n, ncl in CLUSTERED + [CLUSTER_SMALL]:
        s, c = make_clustered(CLUSTER_SEED, n, ncl)
        out.append(Case("clustered/%d/m%d" % (n, method), s, c, IOU, SIGMA, CLUSTER_MIN_SCORE[method], method))
    # The same groups with the scores quantised to 16 levels, as make_segments(ties=True) does.  The order in which the compaction
    # leaves the array shows in the result only where equal scores meet (the first of the current order wins): with distinct
    # scores a compaction that moved the right elements to the wrong slots would select the same segments in the same order.
    for n, ncl in CLUSTERED + [CLUSTER_SMALL]:
        s, c = make_clustered(CLUSTER_SEED, n, ncl)
        c = (np.floor(c * 16) / 16 + 1 / 32).astype(np.float32)
        out.append(Case("clustered_ties/%d/m%d" % (n, method), s, c, IOU, SIGMA, CLUSTER_MIN_SCORE[method], method))
    return out


@functools.lru_cache(maxsize=None)
def tie_cases():
    """method 0 with min_score 0: every suppressed score becomes 0.0 and stays, so the later steps choose among
    hundreds or thousands of exactly equal scores"""
    out = []
    for n, ncl in CLUSTERED:
        s, c = make_clustered(CLUSTER_SEED, n, ncl)
        out.append(Case("ties/%d" % n, s, c, IOU, SIGMA, 0.0, 0))
    return out


@functools.lru_cache(maxsize=None)
def degenerate_cases(method, min_score):
    out = []
    for i, n in enumerate(DEGENERATE_SIZES):
        s, c = make_degenerate(200 + i, n)
        out.append(Case("degenerate/%d/m%d/%g" % (n, method, min_score), s, c, IOU, SIGMA, min_score, method))
    return out


@functools.lru_cache(maxsize=None)
def small_group_cases():
    """about 3000 groups of 1 .. 5 segments (slices of one seeded draw), with one group of 1025 and one of 4097 among them"""
    sizes = 1 + (np.arange(SMALL_GROUPS) * 7 + 3) % 5
    segs, scores = make_segments(SMALL_SEED, int(sizes.sum()), ties=True)
    out, at = [], 0
    for g, n in enumerate(sizes):
        out.append(Case("small/%d" % g, segs[at:at + n], scores[at:at + n], IOU, SIGMA, 0.001, 2))
        at += n
    for where, (n, seed) in ((1000, (1025, 41)), (2001, (4097, 42))):
        s, c = make_segments(seed, n, ties=False)
        out.insert(where, Case("small/big%d" % n, s, c, IOU, SIGMA, 0.001, 2))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = [golden_case(f) for f in GOLDEN_CASES] + many_cases() + tie_cases()
    for method in (0, 1, 2):
        out += clustered_cases(method)
        for ms in DEGENERATE_MIN_SCORES:
            out += degenerate_cases(method, ms)
    return out + small_group_cases()


_by_name = {}


@functools.lru_cache(maxsize=None)
def oracle(name, exp):
    """(inds, dets, pruned_per_step) of the named case in the weight mode `exp` ("glibc" | "rn"); read-only arrays"""
    if not _by_name:
        _by_name.update((c.name, c) for c in all_cases())
    c = _by_name[name]
    out = N.softnms_1d(c.segs, c.scores, c.iou, c.sigma, c.min_score, c.method, exp=exp, return_pruned=True)
    for a in out:
        a.setflags(write=False)
    return out
