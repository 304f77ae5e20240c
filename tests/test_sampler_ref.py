"""The CPU restatement of the device-side batch sampler and DRLoc draw (tests/sampler_ref.py): the structure of the order
(DistributedSampler's lists with a keyed permutation), and the uniformity of its draws as conditions.  No GPU."""
import numpy as np
import pytest

from tests import sampler_ref as S

GEOMETRIES = ((7, 1, 3), (7, 3, 2), (7, 8, 1), (64, 2, 8), (65, 4, 8))     # (N, world, batch)


def _five_sigma(counts, n, p):
    return np.abs(np.asarray(counts, np.float64) - n * p).max() / np.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize("N", (1, 2, 3, 7, 64, 65, 1000, 4097))
def test_perm_is_a_bijection_and_changes_with_the_epoch(N):
    p0, passes = S.perm(5, 0, np.arange(N), N)
    assert p0.dtype == np.int64 and sorted(p0.tolist()) == list(range(N))
    assert 1 <= passes <= 64                               # (the longest walk: 40 at N = 4097)
    p1 = S.perm(5, 1, np.arange(N), N)[0]
    assert sorted(p1.tolist()) == list(range(N))
    if N >= 3:
        assert not np.array_equal(p0, p1)                  # consecutive epochs differ
    if N >= 64:                                            # (below, two of a handful of permutations may coincide)
        assert not np.array_equal(p0, S.perm(6, 0, np.arange(N), N)[0])
    assert np.array_equal(p0, S.perm(5, 1 << S.EPOCH_BITS, np.arange(N), N)[0])       # the epoch counts modulo 2^23


@pytest.mark.parametrize("last", ("wrap", "drop"))
@pytest.mark.parametrize("N,W,B", GEOMETRIES)
def test_an_epoch_over_all_ranks_is_the_distributed_samplers_lists(N, W, B, last):
    per_rank, I = S.geometry(N, W, B, last)
    assert per_rank == -(-N // W)
    if I == 0:
        assert last == "drop" and per_rank < B
        return
    seed = 3
    for e in (0, 2):
        perm = S.perm(seed, e, np.arange(N), N)[0]
        for r in range(W):
            got = []
            for k in range(I):
                d = S.draw(seed, e * I + k, N, W, r, B, True, last)
                assert (d["epoch"], d["iteration"]) == (e, k) and d["window"].dtype == np.int32 and d["valid"].dtype == np.uint8
                assert ((0 <= d["window"]) & (d["window"] < N)).all()            # absent rows carry a real window too
                if last == "drop" or k < I - 1:
                    assert d["valid"].all()                                      # absent rows: only the last iteration of "wrap"
                else:
                    n_present = per_rank - k * B
                    assert d["valid"].tolist() == [1] * n_present + [0] * (B - n_present)
                    wrapped = [perm[((p % per_rank) * W + r) % N] for p in range(per_rank, I * B)]
                    assert d["window"][n_present:].tolist() == wrapped
                got += d["window"][d["valid"] != 0].tolist()
            want = [perm[g % N] for g in range(r, per_rank * W, W)]              # rank r holds g = r (mod W)
            assert got == want[:I * B]                                            # ("drop": minus the dropped tail)
            if last == "wrap":
                assert len(got) == per_rank


def test_without_shuffle_the_order_ascends():
    for N, W, B in GEOMETRIES:
        per_rank, I = S.geometry(N, W, B, "wrap")
        for r in range(min(W, 3)):
            rows = np.concatenate([S.draw(9, 5 * I + k, N, W, r, B, False, "wrap")["window"] for k in range(I)])[:per_rank]
            assert rows.tolist() == [(p * W + r) % N for p in range(per_rank)]
    assert S.draw(9, 0, 7, 1, 0, 7, False, "wrap")["window"].tolist() == list(range(7))


def test_drop_with_too_few_windows_has_no_iteration():
    assert S.geometry(7, 1, 8, "drop") == (7, 0) and S.geometry(7, 1, 8, "wrap") == (7, 1) and S.geometry(7, 3, 2, "drop") == (3, 1)


@pytest.mark.parametrize("num_aug", (1, 3, 5))
def test_aug_indices_lie_in_range_and_are_uniform(num_aug):
    B, nf, n = 64, 64, 1 << 16
    v = np.concatenate([S.aug(21, t, 0, B, nf, num_aug).reshape(-1) for t in range(n // (B * nf))])
    a = np.concatenate([S.aug(21, t, 1, B, nf, num_aug).reshape(-1) for t in range(n // (B * nf))])
    for x in (v, a):
        assert x.size == n and x.min() >= 0 and x.max() < num_aug
        if num_aug > 1:
            assert _five_sigma(np.bincount(x, minlength=num_aug), n, 1.0 / num_aug) < 5.0
    assert num_aug == 1 or not np.array_equal(v, a)                                  # the modalities draw independently
    d0, d1 = S.draw(21, 0, 7, 1, 0, 8, True, "wrap", 6, num_aug, num_aug), S.draw(21, 1, 7, 1, 0, 8, True, "wrap", 6, num_aug, num_aug)
    assert d0["v_aug"].shape == (8, 6) and d0["v_aug"].dtype == np.int32
    assert np.array_equal(d0["v_aug"], S.aug(21, 0, 0, 64, 64, num_aug).reshape(-1)[:48].reshape(8, 6))   # addressed by (t, modality, b * nf + j)
    assert num_aug == 1 or not np.array_equal(d0["v_aug"], d1["v_aug"])


@pytest.mark.parametrize("l", (1, 6, 50))
def test_drloc_positions_lie_in_range_and_are_uniform(l):
    n, m = 2048, 32                                                                  # 2^16 draws of each position
    p1, p2, dx = S.drloc(13, 0, n, m, l)
    assert p1.shape == p2.shape == dx.shape == (n, m) and p1.dtype == np.int64 and dx.dtype == np.float32
    for p in (p1, p2):
        assert p.min() >= 0 and p.max() < l
        if l > 1:
            assert _five_sigma(np.bincount(p.reshape(-1), minlength=l), n * m, 1.0 / l) < 5.0
    assert np.array_equal(dx, np.abs(p1 - p2).astype(np.float32) * (np.float32(1.0) / np.float32(l)))
    assert np.abs(dx.astype(np.float64) - np.abs(p1 - p2) / l).max() <= 2.0 ** -24                # within an ulp of the quotient
    assert dx.min() >= 0 and dx.max() < 1
    q1, _, _ = S.drloc(13, 1, n, m, l)
    assert l == 1 or not np.array_equal(p1, q1)
    assert np.array_equal(S.drloc(13, 0, 3, 5, l)[0].reshape(-1), p1.reshape(-1)[:15])   # element i of a draw: the shape takes no part


@pytest.mark.parametrize("seed", (11, 1))
def test_perm_places_every_element_everywhere_equally_often(seed):
    N, epochs = 7, 7000
    e = np.repeat(np.arange(epochs), N).reshape(epochs, N)
    v = S.perm(seed, e, np.tile(np.arange(N), (epochs, 1)), N)[0]
    assert (np.sort(v, axis=1) == np.arange(N)).all()
    counts = np.zeros((N, N))
    for i in range(N):
        counts[i] = np.bincount(v[:, i], minlength=N)
    assert _five_sigma(counts, epochs, 1.0 / N) < 5.0                                # (3.6 at seed 11)
    assert len({tuple(r) for r in v.tolist()}) > 3500                                # a uniform draw of 5040 expects about 3780
    four = S.perm(seed, np.repeat(np.arange(2000), 4).reshape(2000, 4), np.tile(np.arange(4), (2000, 1)), 4)[0]
    assert len({tuple(r) for r in four.tolist()}) == 24
