"""Host side of the recognition inference tail, no GPU: the C ABI is declared, bound and built, the accuracy
expressions are the restatement's, and without a device the collector refuses instead of falling back."""
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import recog_ref as RR
from tim_amd import _lib, recog

ROOT = os.path.dirname(os.path.dirname(H.GOLDEN))
NAMES = {"timhip_rec_accumulate", "timhip_rec_finalize", "timhip_rec_counts"}


def test_abi_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    assert NAMES <= set(re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", hdr))
    assert NAMES <= set(_lib.exported_symbols())
    assert re.search(r"#define\s+TIMHIP_REC_MAX_HEADS\s+3\b", hdr) and _lib.REC_MAX_HEADS == 3
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)
    assert re.search(r"^SRCS\s*=.*\brecog\.hip\b", open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read(), re.M)
    import ctypes
    assert ctypes.sizeof(_lib.TimRecHead) == 32             # two pointers, one int64, two int32: no padding to disagree on


def test_accuracy_expressions_are_the_restatements():
    for size in (1, 3, 7, 28, 199, 9668):
        for c1 in (0, 1, size // 3, size):
            c5 = min(size, c1 + size // 5)
            rank = np.array([0] * c1 + [3] * (c5 - c1) + [9] * (size - c5))
            assert recog.accuracy_floats(c1, c5, size) == RR.accuracy(rank)
            assert recog.multitask_floats(c1, c5, size) == RR.multitask_accuracy(rank, np.zeros_like(rank))
    assert recog.accuracy_floats(0, 0, 0) == (0.0, 0.0)


def test_no_device_no_collector(monkeypatch):
    import tim_amd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        tim_amd.RecognitionCollector([[5, 7, 23], 11], 10)
