"""The CPU restatement of the device-side mixup (tests/mixup_ref.py) against the reference's own mixup_data
(tests/golden/mixup_small.npz) and against the exact moments of Beta(alpha, alpha).  No GPU."""
import os

import numpy as np
import pytest

from tests import mixup_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixup_small.npz")
# (seed, alpha) of the 4096-draw runs tests/test_gpu_mixup.py compares with the device
GPU_DRAW_RUNS = [(11, 0.2), (12, 1.0)]
N_DRAWS = 4096

_RUNS = {}


def draws(seed, alpha):
    if (seed, alpha) not in _RUNS:
        lam, _, _, margin = R.draw(seed, 0, alpha, 2, N_DRAWS)
        lam.setflags(write=False)
        margin.setflags(write=False)
        _RUNS[(seed, alpha)] = (lam, margin)
    return _RUNS[(seed, alpha)]


def test_philox_restatement_known_properties():
    a = R.philox4x32_7(5, R.SITE_MIXUP, np.arange(4096, dtype=np.uint64))
    assert a.dtype == np.uint32 and a.shape == (4096, 4)
    assert np.array_equal(a, R.philox4x32_7(5, R.SITE_MIXUP, np.arange(4096, dtype=np.uint64)))
    assert len(np.unique(a.reshape(-1))) > 4 * 4096 - 8                 # 16384 words of 32 bits: collisions are rare
    assert not np.array_equal(a, R.philox4x32_7(6, R.SITE_MIXUP, np.arange(4096, dtype=np.uint64)))
    assert not np.array_equal(a, R.philox4x32_7(5, 3, np.arange(4096, dtype=np.uint64)))
    bits = np.unpackbits(a.view(np.uint8)).mean()
    assert abs(bits - 0.5) < 5 * 0.5 / np.sqrt(a.size * 32)


def test_restated_mix_equals_the_reference():
    g = np.load(GOLDEN)
    lam, index = float(g["lam"]), g["index"]
    assert sorted(index.tolist()) == list(range(5)) and 0.0 <= lam <= 1.0
    for i in range(3):
        x, want = g["x%d" % i], g["mixed%d" % i]
        assert x.dtype == np.float32 and want.dtype == np.float32
        got = R.mix(x, lam, index)
        err = np.abs(got - want.astype(np.float64))
        bound = R.mix_bound(x, lam, index)       # the reference mixes in fp32: two rounded products, one rounded sum
        print("tensor %d: max err / bound %.3f" % (i, (err / bound).max()))
        assert (err <= bound).all()
    for k in ("verb", "noun", "action", "class_id"):
        assert np.array_equal(g["yb_" + k], g["y_" + k][index])
        assert (g["y_" + k] == -1).any()


def test_mix_backward_is_the_adjoint():
    rs = np.random.RandomState(0)
    lam = 0.3
    perm, inv = R.permutation(1, 0, 6)
    x, dy = rs.randn(6, 4), rs.randn(6, 4)
    assert abs((R.mix(x, lam, perm) * dy).sum() - (x * R.mix_backward(dy, lam, inv)).sum()) < 1e-12


@pytest.mark.parametrize("B", [1, 2, 3, 64, 257])
def test_restated_permutation(B):
    seen = set()
    for d in range(6):
        perm, inv = R.permutation(9, d, B)
        assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(B))
        assert np.array_equal(inv[perm], np.arange(B)) and np.array_equal(perm[inv], np.arange(B))
        seen.add(tuple(perm.tolist()))
    if B >= 64:
        assert len(seen) == 6


def test_small_permutations_are_uniform():
    counts = {}
    n = 3000
    for d in range(n):
        p = tuple(R.permutation(4, d, 3)[0].tolist())
        counts[p] = counts.get(p, 0) + 1
    assert len(counts) == 6
    for c in counts.values():      # binomial(n, 1/6): five standard deviations
        assert abs(c - n / 6) < 5 * np.sqrt(n * (1 / 6) * (5 / 6))


@pytest.mark.parametrize("alpha", [0.0, -1.0])
def test_alpha_off_gives_lam_one(alpha):
    lam, perm, inv, _ = R.draw(3, 0, alpha, 7, 4)
    assert (lam == 1.0).all()
    assert any(not np.array_equal(p, np.arange(7)) for p in perm)      # the permutation is still drawn


@pytest.mark.parametrize("seed,alpha", GPU_DRAW_RUNS)
def test_beta_moments(seed, alpha):
    lam, _ = draws(seed, alpha)
    assert ((lam >= 0) & (lam <= 1)).all()
    m, v = R.moments(lam)
    em, dm, ev, dv = R.beta_moment_bounds(alpha, N_DRAWS)
    print("alpha %g: mean %.5f (0.5 +- %.4f), variance %.5f (%.5f +- %.4f)" % (alpha, m, dm, v, ev, dv))
    assert abs(m - em) <= dm and abs(v - ev) <= dv


def test_moment_bounds_are_the_stated_ones():
    _, dm, ev, dv = R.beta_moment_bounds(0.2, 4096)
    assert abs(dm - 0.033) < 5e-4 and abs(ev - 0.17857) < 1e-5 and abs(dv - 0.0068) < 1e-4
    _, dm, ev, dv = R.beta_moment_bounds(1.0, 4096)
    assert abs(dm - 0.0226) < 1e-4 and abs(ev - 1 / 12) < 1e-12 and abs(dv - 0.0058) < 1e-4


@pytest.mark.parametrize("alpha", [0.1, 4.0])
def test_beta_moments_at_the_ends_of_the_required_range(alpha):
    lam, _, _, _ = R.draw(21, 0, alpha, 1, 2048)
    m, v = R.moments(lam)
    em, dm, ev, dv = R.beta_moment_bounds(alpha, 2048)
    assert abs(m - em) <= dm and abs(v - ev) <= dv


@pytest.mark.parametrize("seed,alpha", GPU_DRAW_RUNS)
def test_gpu_seeds_keep_clear_of_the_accept_boundary(seed, alpha):
    """a condition on the seeds the GPU test uses: at most 1 % of their draws lie within 1e-4 of an accept / reject decision"""
    _, margin = draws(seed, alpha)
    share = (margin < R.NEAR).mean()
    print("alpha %g: %.3f %% of the draws are near the boundary" % (alpha, 100 * share))
    assert share <= 0.01


def test_draw_sequence_continues():
    a = R.draw(5, 0, 0.2, 5, 8)
    b, c = R.draw(5, 0, 0.2, 5, 3), R.draw(5, 3, 0.2, 5, 5)
    assert np.array_equal(a[0], np.concatenate([b[0], c[0]])) and np.array_equal(a[1], np.concatenate([b[1], c[1]]))


# ---- the unit's host side: declared, built, bound, gated; constants in one agreement ------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"timhip_mixup_draw", "timhip_mixup_apply", "timhip_ce_mixup_fwd_dev", "timhip_ce_mixup_bwd_dev"}


def test_unit_is_declared_built_bound_and_gated():
    import re
    import sys
    from tim_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    assert NAMES <= set(re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", hdr)) and NAMES <= set(_lib.exported_symbols())
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES)
    assert re.search(r"^SRCS\s*=.*\bmixup\.hip\b", open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read(), re.M)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_spills
    assert dict(check_spills.BUDGET["mixup.hip"])["mixup_apply_kernel"] == 0
    common = open(os.path.join(ROOT, "tim_amd", "csrc", "common.h")).read()
    site = int(re.search(r"SITE_MIXUP\s*=\s*(\d+)", common).group(1))
    assert site == _lib.SITE_MIXUP == R.SITE_MIXUP
    in_use = {1, 2, 3} | {_lib.layer_site(layer, k) for layer in range(64) for k in range(8)}
    assert site not in in_use
    lo = float(re.search(r"TIMHIP_MIXUP_ALPHA_MIN\s+([0-9.]+)f", hdr).group(1))
    hi = float(re.search(r"TIMHIP_MIXUP_ALPHA_MAX\s+([0-9.]+)f", hdr).group(1))
    assert (lo, hi) == (_lib.MIXUP_ALPHA_MIN, _lib.MIXUP_ALPHA_MAX) == (R.ALPHA_MIN, R.ALPHA_MAX)
    assert lo <= 0.1 and hi >= 4.0                                       # the range every build must support
    assert int(re.search(r"TIMHIP_MIXUP_MAX_TENSORS\s+(\d+)", hdr).group(1)) == _lib.MIXUP_MAX_TENSORS == 4


def test_no_cpu_fallback():
    import torch
    import tim_amd
    from tim_amd import _lib
    assert tim_amd.Mixup is tim_amd.mixup.Mixup and tim_amd.mixup_data is tim_amd.mixup.mixup_data
    with pytest.raises(_lib.TimHipError):
        tim_amd.Mixup(4, device="cpu")
    with pytest.raises(_lib.TimHipError):
        tim_amd.mixup_data([torch.zeros(4, 3)], torch.zeros(4, dtype=torch.int64), alpha=0.2)
