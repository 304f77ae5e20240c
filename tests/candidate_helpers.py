"""TEST INFRASTRUCTURE ONLY: what the tests of the two candidate units (detect, twostream) share - the small numeric and
host-to-device helpers of their GPU tests and the "declared, bound, exported" check of their host tests."""
import os
import re
import subprocess

import numpy as np
import torch

from tim_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def logit(t, outside):
    """log(t / (1 - t)) of a threshold inside (0, 1), `outside` for any other"""
    return np.log(t / (1.0 - t)) if 0.0 < t < 1.0 else outside


def ulp_apart(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def meta(video_ids, starts, window_size):
    return {"video_id": list(video_ids), "window_start": torch.tensor(np.asarray(starts), dtype=torch.float64),
            "window_size": torch.tensor([window_size] * len(video_ids), dtype=torch.float64)}


def check_entry_points(prefix, nargs, unit):
    """the entry points `nargs` = {name: number of arguments} are exactly what the header declares under `prefix`, bound with
    that many arguments and exported under ABI 6; `unit` compiles the shared header with contraction off"""
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    declared = {n for n in re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", hdr) if n.startswith(prefix)}
    assert declared == set(nargs)
    assert set(nargs) <= set(_lib.exported_symbols())
    for n, k in nargs.items():
        assert len(_lib._SIGS[n][1]) == k, n
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6      # additive: the version stays
    so = _lib.LIB_PATH
    if os.path.exists(so):
        syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        for n in nargs:
            assert re.search(r"\bT %s\b" % n, syms), n
    src = open(os.path.join(ROOT, "tim_amd", "csrc", unit)).read()
    assert "#pragma clang fp contract(off)" in src and '#include "candidates.h"' in src
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "candidates.h"')
