"""TEST INFRASTRUCTURE ONLY: numpy restatement of `timhip_attention_query_weights` - the attention weights of query rows whose F
feature keys are those of window widx[g] of a cache and whose last key is the row's own.  float64 by default;
`dtype=np.float32` restates the kernel's own arithmetic (tests/attn_maps_ref.py: what another summation order moves is what the
GPU tests' bound is made of).  Written from the pieces, not through tests/attn_maps_ref.weights: tests/test_query_maps_ref.py
pins the two to each other and both to the reference's recorded weights."""
import numpy as np


def query_weights(q, k_own, k_cache, widx, H, per_head=False, dtype=np.float64):
    """q, k_own [G, Q, E]: the query rows' q and own-key columns; k_cache [W, F, E]: the K columns of the cached windows; widx: G
    window numbers (None: group g reads window g) -> [G, Q, F + 1] (per_head: [G, H, Q, F + 1]): softmax over the F keys of window
    widx[g] and, in column F, the row's own key; mean over the heads as a sum in ascending head order times 1 / H"""
    q, k_own, k_cache = (np.asarray(a, dtype=dtype) for a in (q, k_own, k_cache))
    G, Q, E = q.shape
    W, F, _ = k_cache.shape
    Dh = E // H
    idx = np.arange(G) if widx is None else np.asarray(widx)
    assert idx.shape == (G,) and idx.min() >= 0 and idx.max() < W
    scale = dtype(1.0) / np.sqrt(dtype(Dh))
    qh, oh = q.reshape(G, Q, H, Dh), k_own.reshape(G, Q, H, Dh)
    kh = k_cache[idx].reshape(G, F, H, Dh)
    sc = np.full((G, H, Q, F + 1), -np.inf, dtype=dtype)
    sc[..., :F] = np.einsum("bnhd,bjhd->bhnj", qh, kh) * scale
    sc[..., F] = np.einsum("bnhd,bnhd->bhn", qh, oh) * scale
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    tot = p.sum(axis=-1, keepdims=True, dtype=dtype)
    w = p / tot if dtype == np.float64 else p * (dtype(1.0) / tot)     # (the kernel multiplies by the rounded reciprocal)
    if per_head:
        return w
    acc = np.zeros((G, Q, F + 1), dtype=dtype)
    for h in range(H):
        acc += w[:, h]
    return acc * (dtype(1.0) / dtype(H))


def full_qkv(q, k_own, k_cache, widx, rng):
    """the [G (F + Q), 3E] matrix `timhip_attention_weights` reads, assembled from the same pieces: window g's feature rows carry
    the keys of cache window widx[g] (their q and every v column are never read by a query row's weights: random), its query
    rows q | own k | random v"""
    q, k_own, k_cache = np.asarray(q), np.asarray(k_own), np.asarray(k_cache)
    G, Q, E = q.shape
    F = k_cache.shape[1]
    idx = np.arange(G) if widx is None else np.asarray(widx)
    qkv = rng.standard_normal((G, F + Q, 3 * E)).astype(q.dtype)
    qkv[:, :F, E:2 * E] = k_cache[idx]
    qkv[:, F:, :E] = q
    qkv[:, F:, E:2 * E] = k_own
    return qkv.reshape(G * (F + Q), 3 * E)


def split_qkv(qkv, B, S, F):
    """the pieces of a full [B S, 3E] qkv: (q [B, S - F, E], k_own [B, S - F, E], k_cache [B, F, E]) - window b is its own cache"""
    qkv = np.asarray(qkv)
    E = qkv.shape[1] // 3
    x = qkv.reshape(B, S, 3 * E)
    return x[:, F:, :E], x[:, F:, E:2 * E], x[:, :F, E:2 * E]


def compact(dense, F):
    """the reference's dense rows of the query tokens [B, S, S] -> [B, S - F, F + 1]: feature columns, the diagonal last"""
    dense = np.asarray(dense)
    S = dense.shape[-1]
    out = np.empty(dense.shape[:1] + (S - F, F + 1), dtype=dense.dtype)
    out[..., :F] = dense[:, F:, :F]
    for s in range(F, S):
        out[:, s - F, F] = dense[:, s, s]
    return out
