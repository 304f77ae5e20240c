"""The numpy restatement of the attention weights (tests/attn_maps_ref.py) against the reference's own: for every layer of every
fixture of tests/golden/make_golden_attn.py, the recorded layer input through the layer's in-projection and the restatement
reproduces the reference's dense [B, S, S] weights, values and zero pattern.  No GPU."""
import numpy as np
import pytest

from tests import attn_maps_ref as R


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_the_references_weights(name):
    z, cfg = R.load_fixture(name)
    S, F, H, Bw = int(z["S"]), cfg.F, cfg.nhead, int(z["windows"])
    assert 1 <= Bw <= int(z["B"])
    for l in range(cfg.num_layers):
        want = z["attn/layer%d" % l]
        assert want.dtype == np.float64 and want.shape == (Bw, S, S)
        w = R.weights(R.fixture_qkv(z, cfg, l), Bw, S, F, H)
        assert w.shape == (Bw, S, F + 1)
        got = R.to_dense(w, S, F, 0)
        err = np.abs(got - want).max()
        print("%s layer %d: restatement against the reference, max abs %.3g" % (name, l, err))
        assert err <= 1e-12
        # the zero pattern, exactly: F feature columns in every row and the own key of the S - F query rows
        assert np.array_equal(got != 0, want != 0)
        assert all(int(np.count_nonzero(want[b])) == S * F + (S - F) for b in range(Bw))
        assert np.all(w[:, :F, F] == 0.0)
        assert np.abs(w.sum(-1) - 1.0).max() <= 1e-14


def test_rows_and_per_head_forms_agree_with_the_full_mean():
    rng = np.random.default_rng(0)
    B, S, F, H, Dh = 2, 11, 4, 3, 5
    qkv = rng.standard_normal((B * S, 3 * H * Dh))
    full = R.weights(qkv, B, S, F, H)
    for s0 in (0, 2, F, F + 3):
        assert np.array_equal(R.weights(qkv, B, S, F, H, s0=s0), full[:, s0:])
        ph = R.weights(qkv, B, S, F, H, s0=s0, per_head=True)
        assert ph.shape == (B, H, S - s0, F + 1)
        assert np.abs(ph.mean(1) - full[:, s0:]).max() <= 1e-15
    dense = R.to_dense(full[:, F:], S, F, F)
    assert dense.shape == (B, S - F, S) and np.array_equal(dense[:, :, :F], full[:, F:, :F])
    for s in range(F, S):
        assert np.array_equal(dense[:, s - F, s], full[:, s, F])
    assert np.count_nonzero(dense) == B * (S - F) * (F + 1)
    f32 = R.weights(qkv, B, S, F, H, dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - full).max() <= 1e-6
