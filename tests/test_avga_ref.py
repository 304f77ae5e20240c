"""`tests/avga_ref.py` pinned to what the reference's AVGA module computed: the fp32 record (avga_tiny.npz) and the
float64 record with parameter gradients (avga_grads.npz, tests/golden/make_golden_avga.py)."""
import os

import numpy as np
import torch

from tests import helpers as H
from tests.avga_ref import PARAMS, avga_f64, avga_rounded


def test_f64_restatement_matches_the_fp32_record():
    g = np.load(os.path.join(H.GOLDEN, "avga_tiny.npz"))
    P = {k[5:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("pool/")}
    assert set(P) == set(PARAMS)
    r = avga_f64(P, g["audio"], g["video"])
    want = torch.from_numpy(g["pooled"]).double().reshape(r["out"].shape)
    assert (r["out"] - want).abs().max().item() <= 1e-6
    assert (r["alpha"].sum(1) - 1).abs().max().item() <= 1e-12


def test_f64_restatement_matches_the_float64_record_with_gradients():
    g = np.load(os.path.join(H.GOLDEN, "avga_grads.npz"))
    assert os.path.getsize(os.path.join(H.GOLDEN, "avga_grads.npz")) < 400 * 1024
    P = {k: torch.from_numpy(g["param/" + k]) for k in PARAMS}
    assert g["video"].shape == (3, 2, 7, 7, 64) and g["audio"].shape == (3, 2, 40)
    r = avga_f64(P, g["audio"], g["video"], cot=g["cot"])
    assert (r["out"] - torch.from_numpy(g["out"]).reshape(6, 64)).abs().max().item() <= 1e-11
    assert (r["alpha"] - torch.from_numpy(g["alpha"])).abs().max().item() <= 1e-11
    for k in PARAMS:
        want = torch.from_numpy(g["grad/" + k])
        assert r["grads"][k].shape == want.shape
        assert (r["grads"][k] - want).abs().max().item() <= 1e-10, k


def test_rounding_model_is_close_to_and_different_from_f64():
    g = np.load(os.path.join(H.GOLDEN, "avga_grads.npz"))
    P = {k: torch.from_numpy(g["param/" + k]) for k in PARAMS}
    ref = avga_f64(P, g["audio"], g["video"], cot=g["cot"])
    scale = ref["out"].abs().max().item()
    for dtype, lo, hi in ((torch.float16, 1e-6, 2e-3), (torch.bfloat16, 1e-5, 2e-2)):
        r = avga_rounded(dtype)(P, g["audio"], g["video"], cot=g["cot"])
        err = (r["out"] - ref["out"]).abs().max().item() / scale
        assert lo < err < hi, (dtype, err)
        for k in PARAMS:   # straight-through: every parameter still gets a gradient of the right shape
            assert r["grads"][k].shape == ref["grads"][k].shape and torch.isfinite(r["grads"][k]).all()
