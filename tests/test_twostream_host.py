"""CPU-only checks of the two-stream fusion's host side: `tim_amd.TwoStreamCollector` resolves lazily and fails loudly
without a GPU, the two library entry points are declared in the header, bound, and exported under the unchanged ABI number,
and the kernels are in the spill gate's table."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import tim_amd
from tests.candidate_helpers import ROOT, check_entry_points
from tim_amd import _lib

def test_collector_is_a_lazy_export():
    assert "TwoStreamCollector" not in vars(tim_amd)
    from tim_amd.twostream import TwoStreamCollector
    assert tim_amd.TwoStreamCollector is TwoStreamCollector
    col = TwoStreamCollector()
    assert (col.num_verbs, col.num_nouns, col.top_k, col.score_threshold, col.verb_alpha) == (97, 300, 1, 0.03, 0.65)
    assert col.num_classes == 97 * 300 and col.video_ids == [] and (col.verb_head, col.noun_head) == ("action", "action")
    for bad in (dict(top_k=0), dict(top_k=9), dict(num_verbs=3, top_k=4), dict(verb_head="verbs"), dict(num_nouns=0)):
        with pytest.raises(ValueError):
            TwoStreamCollector(**bad)
    with pytest.raises(ValueError):
        col.detections(task="actions")


def test_cpu_tensors_fail_loudly():
    col = tim_amd.TwoStreamCollector(num_verbs=11, num_nouns=23)
    B, nq = 2, 7
    meta = {"video_id": ["a", "b"], "window_start": torch.tensor([0.0, 1.5], dtype=torch.float64),
            "window_size": torch.tensor([30.0, 30.0], dtype=torch.float64)}
    verb = ((None, None, torch.zeros(B * nq, 11), None), (torch.zeros(B * nq, 2), None))
    noun = ((None, None, torch.zeros(B * nq, 23), None), (torch.zeros(B * nq, 2), None))
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        col.update(verb, noun, (torch.zeros(B, nq, 2), None), meta)
    assert col.video_ids == [] and col._chunks == []
    if not torch.cuda.is_available():
        with pytest.raises(_lib.TimHipError):
            col.detections()


def test_exponents_match_the_restatement():
    from tests import twostream_ref as T
    from tim_amd.twostream import exponents
    for alpha in (0.0, 0.65, 1.0, 1.3, 1 / 3):
        a, b = T.exponents(alpha)
        assert exponents(alpha) == (float(a), float(b))
    assert exponents(0.65)[1] == float(np.float32(1.0 - 0.65)) != float(np.float32(1) - np.float32(0.65))


def test_entry_points_are_declared_bound_and_exported():
    check_entry_points("timhip_ts_", {"timhip_ts_candidates_count": 24, "timhip_ts_candidates_emit": 17}, "twostream.hip")


def test_kernels_are_in_the_spill_table_and_the_unit_in_the_makefile():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_spills
    finally:
        sys.path.pop(0)
    pats = dict(check_spills.BUDGET["twostream.hip"])
    assert pats["ts_select_kernel"] == 0 and pats["ts_emit_kernel"] == 0
    mk = open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\btwostream\.hip\b", mk, re.M)
