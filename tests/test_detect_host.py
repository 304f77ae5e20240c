"""CPU-only checks of the detection inference tail's host side: `tim_amd.DetectionCollector` resolves lazily and fails loudly
without a GPU, and the two library entry points are declared in the header, bound, and exported under the unchanged ABI
number."""
import os

import numpy as np
import pytest
import torch

import tim_amd
from tests import helpers as H
from tests.candidate_helpers import check_entry_points
from tim_amd import _lib

def test_collector_is_a_lazy_export():
    assert "DetectionCollector" not in vars(tim_amd)
    from tim_amd.detect import DetectionCollector
    assert tim_amd.DetectionCollector is DetectionCollector
    col = DetectionCollector([[97, 300, 3806], 44], head="noun", score_threshold=0.02)
    assert col.num_classes == 300 and col.video_ids == []
    assert DetectionCollector((13, 5), head="action").num_classes == 13
    assert DetectionCollector((13, 5), head="audio").num_classes == 5
    assert DetectionCollector(23).num_classes == 23
    with pytest.raises(ValueError):
        DetectionCollector((13, 5), head="verb")
    with pytest.raises(ValueError):
        DetectionCollector((13, 5), head="actions")


def test_cpu_tensors_fail_loudly():
    col = tim_amd.DetectionCollector((13, 5), head="action")
    B, nq = 2, 7
    meta = {"video_id": ["a", "b"], "window_start": torch.tensor([0.0, 1.5], dtype=torch.float64),
            "window_size": torch.tensor([30.0, 30.0], dtype=torch.float64)}
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        col.update((None, None, torch.zeros(B * nq, 13), None), (torch.zeros(B * nq, 2), None), (torch.zeros(B, nq, 2), None), meta)
    assert col.video_ids == [] and col._chunks == []
    if not torch.cuda.is_available():
        with pytest.raises(_lib.TimHipError):
            col.detections()


def test_entry_points_are_declared_bound_and_exported():
    check_entry_points("timhip_det_candidates", {"timhip_det_candidates_count": 14, "timhip_det_candidates_emit": 16}, "detect.hip")


def test_restatement_and_host_agree_on_the_class_key():
    """key = video_index * C + class on both sides (the grouped NMS runs one group per key)"""
    from tests import detect_ref as D
    from tim_amd.detect import HEADS, head_classes
    assert HEADS == {"verb": (0, 0), "noun": (1, 0), "action": (2, 0), "audio": (3, 1)}
    assert head_classes([[7, 11, 13], 5], "action") == 13
    g = np.load(os.path.join(H.GOLDEN, "detect_small.npz"))
    c = D.batch_candidates(g["logits"][1], g["reg"][1], g["window_start"][1], float(g["window_size"]), g["queries"].max(),
                           [4, 9], float(g["threshold"]))
    assert set(np.unique(c["key"] // 23)) == {4, 9} and np.array_equal(c["key"] % 23, c["cls"])
