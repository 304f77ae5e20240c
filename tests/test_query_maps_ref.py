"""The numpy restatement of `timhip_attention_query_weights` (tests/query_maps_ref.py): pinned to tests/attn_maps_ref.weights on a
full qkv assembled from the same pieces (exactly, in float64), pinned to the reference's recorded weights of the three golden
fixtures (query rows, every recorded layer), and shown to tell three wrong kernels from the right one.  No GPU."""
import numpy as np
import pytest

from tests import attn_maps_ref as R
from tests import query_maps_ref as QM


def _pieces(rng, G, Q, W, F, H, Dh):
    """values on a grid of 1/64 in [-4, 4): every product and every sum of a score is exact in float64, whatever the order - the
    two restatements can then differ only where their formulas do"""
    E = H * Dh

    def grid(*shape):
        return rng.integers(-256, 256, size=shape).astype(np.float64) / 64.0
    return grid(G, Q, E), grid(G, Q, E), grid(W, F, E)


@pytest.mark.parametrize("G,Q,W,F,H,Dh,widx", [(7, 5, 3, 12, 2, 8, [2, 0, 0, 1, 2, 1, 1]), (3, 1, 3, 1, 1, 4, None),
                                               (4, 9, 2, 33, 8, 16, [1, 1, 0, 1]), (2, 33, 2, 100, 4, 32, [1, 0])])
def test_restatement_equals_the_full_one_on_an_assembled_qkv(G, Q, W, F, H, Dh, widx):
    rng = np.random.default_rng(G * 100 + F)
    q, k_own, k_cache = _pieces(rng, G, Q, W, F, H, Dh)
    qkv = QM.full_qkv(q, k_own, k_cache, widx, rng)
    for per_head in (False, True):
        got = QM.query_weights(q, k_own, k_cache, widx, H, per_head=per_head)
        want = R.weights(qkv, G, F + Q, F, H, s0=F, per_head=per_head)
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want)
    assert np.abs(QM.query_weights(q, k_own, k_cache, widx, H).sum(-1) - 1.0).max() <= 1e-14
    # and back: the pieces of the assembled matrix are the pieces
    q2, o2, c2 = QM.split_qkv(qkv, G, F + Q, F)
    idx = np.arange(G) if widx is None else np.asarray(widx)
    assert np.array_equal(q2, q) and np.array_equal(o2, k_own) and np.array_equal(c2, k_cache[idx])
    f32 = QM.query_weights(q, k_own, k_cache, widx, H, dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - QM.query_weights(q, k_own, k_cache, widx, H)).max() <= 1e-6


@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_reproduces_the_references_query_rows(name):
    z, cfg = R.load_fixture(name)
    S, F, H, Bw = int(z["S"]), cfg.F, cfg.nhead, int(z["windows"])
    assert S > F
    for l in range(cfg.num_layers):
        want = QM.compact(z["attn/layer%d" % l], F)
        q, k_own, k_cache = QM.split_qkv(R.fixture_qkv(z, cfg, l), Bw, S, F)
        got = QM.query_weights(q, k_own, k_cache, None, H)
        err = float(np.abs(got - want).max())
        print("%s layer %d: query-row restatement against the reference, max abs %.3g" % (name, l, err))
        assert got.shape == (Bw, S - F, F + 1) and err <= 1e-12
        assert np.all(got > 0)                                   # F + 1 non-zeros in every query row, as the reference has
        # the windows as one cache read through a permuting index: group g = window perm[g]
        perm = np.roll(np.arange(Bw), 1)
        again = QM.query_weights(q[perm], k_own[perm], k_cache, perm, H)
        assert np.array_equal(again, got[perm])


# ---- three wrong kernels ---------------------------------------------------------------------------------------------------------
def _softmax(sc):
    p = np.exp(sc - sc.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def _scores(q, k_own, k_cache, idx, H):
    G, Q, E = q.shape
    F, Dh = k_cache.shape[1], E // H
    qh = q.reshape(G, Q, H, Dh)
    sc = np.einsum("bnhd,bjhd->bhnj", qh, k_cache[idx].reshape(G, F, H, Dh)) / np.sqrt(Dh)
    own = np.einsum("bnhd,bnhd->bhn", qh, k_own.reshape(G, Q, H, Dh)) / np.sqrt(Dh)
    return sc, own


def wrong_no_self(q, k_own, k_cache, widx, H):
    """drops the self column from the softmax (writes 0 there)"""
    sc, _ = _scores(q, k_own, k_cache, np.asarray(widx), H)
    w = _softmax(sc).mean(1)
    return np.concatenate([w, np.zeros(w.shape[:2] + (1,))], -1)


def wrong_window(q, k_own, k_cache, widx, H):
    """reads window g where widx[g] names another"""
    G = q.shape[0]
    sc, own = _scores(q, k_own, k_cache, np.arange(G) % k_cache.shape[0], H)
    return _softmax(np.concatenate([sc, own[..., None]], -1)).mean(1)


def wrong_mean_first(q, k_own, k_cache, widx, H):
    """averages the heads' scores before the softmax"""
    sc, own = _scores(q, k_own, k_cache, np.asarray(widx), H)
    return _softmax(np.concatenate([sc, own[..., None]], -1).mean(1))


def test_restatement_rejects_three_wrong_kernels():
    rng = np.random.default_rng(5)
    G, Q, W, F, H, Dh = 4, 6, 3, 12, 4, 16
    widx = [2, 0, 2, 1]                                          # groups 0, 1 and 3 read a window that is not their own number
    q, k_own, k_cache = (rng.standard_normal(s) for s in ((G, Q, H * Dh), (G, Q, H * Dh), (W, F, H * Dh)))
    want = QM.query_weights(q, k_own, k_cache, widx, H)
    # the bound a right kernel is held to on these inputs (tests/test_gpu_query_weights.py builds it the same way)
    bound = 4.0 * float(np.abs(QM.query_weights(q, k_own, k_cache, widx, H, dtype=np.float32) - want).max()) + 8 * 2.0 ** -23
    sc, own = _scores(q, k_own, k_cache, np.asarray(widx), H)
    right = _softmax(np.concatenate([sc, own[..., None]], -1)).mean(1)
    assert np.abs(right - want).max() <= bound                  # (the helpers above are right when used rightly)
    for wrong in (wrong_no_self, wrong_window, wrong_mean_first):
        got = wrong(q, k_own, k_cache, widx, H)
        assert got.shape == want.shape and np.abs(got.sum(-1) - 1.0).max() <= 1e-12      # each is a plausible map: rows sum to 1
        err = float(np.abs(got - want).max())
        print("%s: max abs error %.3g against a bound of %.3g" % (wrong.__name__, err, bound))
        assert err > 100 * bound, wrong.__name__
    # the wrong window is wrong only where the index differs from the group number
    ww = wrong_window(q, k_own, k_cache, widx, H)
    assert np.abs(ww[2] - want[2]).max() <= bound and all(np.abs(ww[g] - want[g]).max() > 100 * bound for g in (0, 1, 3))
