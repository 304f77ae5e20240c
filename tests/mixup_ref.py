"""CPU restatement of tim_amd/csrc/mixup.hip (contract: include/timhip.h, "mixup of the inputs on the device").

  * philox4x32_7 in numpy integers (csrc/common.h)
  * the draw: the permutation in integers (bit for bit what the kernel computes), the Beta sampler in float64 from the same
    words, and for every draw its distance from the sampler's accept / reject decisions - a device value computed a few ulps
    away can only decide differently when that distance is tiny, so the GPU test skips (and counts) such draws
  * the mix and its backward in float64, and the error bound of the fp32 kernel
"""
import numpy as np

SITE_MIXUP = 8
JOHNK_TRIALS, MT_TRIALS, PERM_BLOCK0, DRAW_BITS = 64, 32, 256, 24
ALPHA_MIN, ALPHA_MAX = 0.05, 16.0
NEAR = 1e-4          # a draw whose margin is below this is "near the accept boundary"
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_7(seed, site, ctr):
    """ctr: array of 64-bit counters -> uint32 [len, 4] (the words x, y, z, w)"""
    ctr = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
    seed = int(seed) & (2 ** 64 - 1)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2 = np.full_like(ctr, int(site))
    c3 = np.full_like(ctr, 0x7149)
    for _ in range(7):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2     # (32 x 32 bits: no overflow in 64)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _M32, p1 >> np.uint64(32), p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def _uniform(r):
    return (np.float64(r) + 0.5) / 4294967296.0


def _base(draw):
    return (int(draw) << DRAW_BITS) & (2 ** 64 - 1)


def _gamma(words, alpha):
    """Marsaglia-Tsang on the [MT_TRIALS, 4] words of one variate -> (value, margin)"""
    d = alpha - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    margin = np.inf
    for r in words:
        x = np.sqrt(-2.0 * np.log(_uniform(r[0]))) * np.cos(6.283185307179586476925 * _uniform(r[1]))
        w = 1.0 + c * x
        v = w * w * w
        margin = min(margin, abs(w))      # (v <= 0 exactly when w <= 0: the distance of that decision is |w|, not |w|^3)
        if v <= 0.0:
            continue
        gap = 0.5 * x * x + d - d * v + d * np.log(v) - np.log(_uniform(r[2]))
        margin = min(margin, abs(gap))
        if gap > 0.0:
            return d * v, margin
    return d, margin


def beta(seed, draw, alpha):
    """-> (lam as float64 BEFORE the rounding to fp32, margin: the smallest distance of an examined trial from its decision)"""
    alpha = float(np.float32(alpha))
    if not alpha > 0:
        return 1.0, np.inf
    assert ALPHA_MIN <= alpha <= ALPHA_MAX
    base = _base(draw)
    words = philox4x32_7(seed, SITE_MIXUP, np.uint64(base) + np.arange(64, dtype=np.uint64))
    if np.float32(alpha) < np.float32(1):
        e = 1.0 / alpha
        margin = np.inf
        for r in words[:JOHNK_TRIALS]:
            X, Y = np.power(_uniform(r[0]), e), np.power(_uniform(r[1]), e)
            margin = min(margin, abs(X + Y - 1.0))
            if X + Y <= 1.0:
                return X / (X + Y), margin
        return 0.5, margin
    g1, m1 = _gamma(words[:MT_TRIALS], alpha)
    g2, m2 = _gamma(words[MT_TRIALS:2 * MT_TRIALS], alpha)
    return g1 / (g1 + g2), min(m1, m2)


def permutation(seed, draw, B):
    """-> (perm, inv) int32 [B]: Fisher-Yates from the identity, j = (r * (i + 1)) >> 32 on one word per swap"""
    perm = np.arange(B, dtype=np.int64)
    if B > 1:
        nblk = ((B - 1) >> 2) + 1
        words = philox4x32_7(seed, SITE_MIXUP, np.uint64(_base(draw) + PERM_BLOCK0) + np.arange(nblk, dtype=np.uint64)).reshape(-1)
        for i in range(B - 1, 0, -1):
            j = (int(words[i]) * (i + 1)) >> 32
            perm[i], perm[j] = perm[j], perm[i]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(B)
    return perm.astype(np.int32), inv.astype(np.int32)


def draw(seed, counter, alpha, B, n=1):
    """what one timhip_mixup_draw launch with the counter word at `counter` writes -> lam float64 [n] (unrounded), perm / inv
    int32 [n, B], margin float64 [n]; the counter afterwards is counter + n"""
    lam, margin = np.empty(n), np.empty(n)
    perm, inv = np.empty((n, B), np.int32), np.empty((n, B), np.int32)
    for s in range(n):
        lam[s], margin[s] = beta(seed, counter + s, alpha)
        perm[s], inv[s] = permutation(seed, counter + s, B)
    return lam, perm, inv, margin


def mix(x, lam, index):
    """float64: lam x + (1 - lam) x[index]"""
    x = np.asarray(x, np.float64)
    return lam * x + (1.0 - lam) * x[np.asarray(index)]


def mix_backward(dy, lam, inverse):
    dy = np.asarray(dy, np.float64)
    return lam * dy + (1.0 - lam) * dy[np.asarray(inverse)]


def half_ulp(v, dtype):
    """half a unit in the last place of `dtype` ("fp32" / "fp16" / "bf16") at magnitude |v| (subnormals: the fixed spacing)"""
    bits, emin = {"fp32": (24, -126), "fp16": (11, -14), "bf16": (8, -126)}[dtype]
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - (bits - 1))


def mix_bound(x, lam, index, dtype="fp32"):
    """two rounded products and one rounded sum in fp32: |out - ref| <= 4 * 2^-24 * (lam |x| + (1 - lam) |x[index]|); 16-bit
    storage adds half an ulp of the output (taken one binade up: the rounded value may sit just above the exact one's binade)"""
    x = np.asarray(x, np.float64)
    b = 4.0 * 2.0 ** -24 * mix(np.abs(x), lam, index)
    if dtype != "fp32":
        b = b + half_ulp(np.abs(mix(x, lam, index)) + b, dtype)
    return b


def moments(v):
    v = np.asarray(v, np.float64)
    m = v.mean()
    return m, ((v - m) ** 2).mean()


def beta_moment_bounds(alpha, n):
    """(mean, 5 standard errors of it, variance, 5 standard errors of it) of n draws of Beta(alpha, alpha): mean 1/2, variance
    1 / (4 (2 alpha + 1)), kurtosis 3 - 6 / (2 alpha + 3); se(mean) = sqrt(var / n), se(var) = var sqrt((kurt - 1) / n)"""
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    kurt = 3.0 - 6.0 / (2.0 * alpha + 3.0)
    return 0.5, 5.0 * np.sqrt(var / n), var, 5.0 * var * np.sqrt((kurt - 1.0) / n)
