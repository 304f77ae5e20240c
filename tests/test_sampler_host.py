"""The device-side batch sampler's entry points: declared in include/timhip.h, bound in tim_amd/_lib.py, exported by the built
library.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tim_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"timhip_sampler_draw": 18, "timhip_window_batch": 2, "timhip_drloc_draw": 9}


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, k in NARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, code)
        assert m, n
        assert len(m.group(1).split(",")) == k == len(_lib._SIGS[n][1]), n
    assert set(NARGS) <= set(_lib.exported_symbols())
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert C.sizeof(_lib.TimWindowBatch) == 27 * 8 + 11 * 4 + 4
    assert [int(re.search(r"#define\s+%s\s+(.+)" % d, code).group(1).strip("() ").replace("1 << ", "")) for d in
            ("TIMHIP_SAMPLER_WRAP", "TIMHIP_SAMPLER_DROP", "TIMHIP_SAMPLER_MAX_AUG", "TIMHIP_DRLOC_MAX_SAMPLES")] == [0, 1, 24, 25]
    assert (_lib.SAMPLER_WRAP, _lib.SAMPLER_DROP, _lib.SAMPLER_MAX_AUG, _lib.DRLOC_MAX_SAMPLES) == (0, 1, 1 << 24, 1 << 25)
    common = open(os.path.join(ROOT, "tim_amd", "csrc", "common.h")).read()
    assert re.search(r"\bSITE_SAMPLER = 9\b", common) and re.search(r"\bSITE_DRLOC = 10\b", common)
    assert (_lib.SITE_SAMPLER, _lib.SITE_DRLOC) == (9, 10)
    assert re.search(r"^SRCS\s*=.*\bsampler\.hip\b", open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read(), re.M)
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NARGS:
        assert re.search(r"\bT %s\b" % n, syms), n


def test_the_classes_are_lazily_importable():
    import tim_amd
    from tim_amd.data import DeviceWindowDataset, WindowSampler
    from tim_amd.losses import DrlocPositions
    assert tim_amd.WindowSampler is WindowSampler and tim_amd.DrlocPositions is DrlocPositions
    assert callable(DeviceWindowDataset.sampler) and callable(DeviceWindowDataset.narration_ids)
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        DrlocPositions(2, 3, 4, device="cpu")
