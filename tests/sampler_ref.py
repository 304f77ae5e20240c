"""CPU restatement of tim_amd/csrc/sampler.hip (contract: include/timhip.h, "device-side batch sampler"), in numpy integers:

  * the sampler draw: iteration t of a seeded, epoch-shuffled, rank-sharded order -> window numbers, valid flags, augmentation
    indices, epoch and iteration words (bit for bit what timhip_sampler_draw writes)
  * the DRLoc draw: pos_1, pos_2 and deltax (numpy float32: the distance times the rounded reciprocal of l)

and of nothing else: what a batch must CONTAIN comes from oracle/data_oracle.py.
"""
import numpy as np

from tests.mixup_ref import philox4x32_7

SITE_SAMPLER, SITE_DRLOC = 9, 10
ROUNDS = 6                     # Feistel rounds of the permutation
EPOCH_BITS = 23                # the epoch enters the Philox counter modulo 2^23
AUG_FLAG = 1 << 63             # counter bit 63: an augmentation word (clear: a round function of the permutation)
DRLOC_DRAW_BITS = 24           # Philox counter of a DRLoc draw = (draw number << 24) | block
_U64 = 2 ** 64 - 1


def geometry(N, world, batch, last):
    """-> (per_rank, iterations per epoch); 0 iterations: the constructor refuses"""
    per_rank = -(-N // world)
    return per_rank, (-(-per_rank // batch) if last == "wrap" else per_rank // batch)


def half_bits(N):
    bits = max(2, int(N - 1).bit_length())
    return (bits + 1) // 2


def perm(seed, e, idx, N):
    """the keyed bijection of [0, N) at epoch e, elementwise on `idx`: a balanced Feistel network over 2 * half_bits(N) bits,
    walked until the value is back inside [0, N) (e: one epoch, or an array of the shape of idx).  -> (values int64, the
    longest walk in passes)"""
    v = np.array(idx, dtype=np.uint64).reshape(-1)
    h = half_bits(N)
    mask = np.uint64((1 << h) - 1)
    ebits = (np.broadcast_to(np.asarray(e, dtype=np.uint64), np.shape(idx)).reshape(-1) & np.uint64((1 << EPOCH_BITS) - 1)) << np.uint64(40)
    todo = np.ones(v.shape, bool)
    passes = 0
    while todo.any():
        x = v[todo]
        L, R = x >> np.uint64(h), x & mask
        for rnd in range(ROUNDS):
            f = philox4x32_7(seed, SITE_SAMPLER, ebits[todo] | np.uint64(rnd << 32) | R)[:, 0].astype(np.uint64) & mask
            L, R = R, L ^ f
        v[todo] = (L << np.uint64(h)) | R
        todo = v >= np.uint64(N)
        passes += 1
    return v.astype(np.int64).reshape(np.shape(idx)), passes


def aug_words(seed, t, modality, count):
    """the Philox words of draw t's augmentation indices of one modality (0 visual, 1 audio), elements 0 .. count-1"""
    nblk = (count + 3) >> 2
    ctr = np.uint64(AUG_FLAG | ((int(t) << 23) & (AUG_FLAG - 1)) | (modality << 22)) + np.arange(nblk, dtype=np.uint64)
    return philox4x32_7(seed, SITE_SAMPLER, ctr).reshape(-1)[:count].astype(np.uint64)


def aug(seed, t, modality, batch, nf, num_aug):
    return ((aug_words(seed, t, modality, batch * nf) * np.uint64(num_aug)) >> np.uint64(32)).astype(np.int32).reshape(batch, nf)


def draw(seed, t, N, world, rank, batch, shuffle, last, nf=0, v_num_aug=0, a_num_aug=0):
    """what one timhip_sampler_draw launch that reads the counter value t writes (the counter afterwards holds t + 1) ->
    dict(window int32 [B], valid uint8 [B], v_aug / a_aug int32 [B, nf] or None, epoch, iteration)"""
    per_rank, I = geometry(N, world, batch, last)
    assert I >= 1
    e, k = divmod(int(t), I)
    p = k * batch + np.arange(batch, dtype=np.int64)
    valid = (p < per_rank).astype(np.uint8)
    i = ((p % per_rank) * world + rank) % N
    window = perm(seed, e, i, N)[0] if shuffle else i
    return {"window": window.astype(np.int32), "valid": valid, "epoch": e, "iteration": k,
            "v_aug": aug(seed, t, 0, batch, nf, v_num_aug) if v_num_aug else None,
            "a_aug": aug(seed, t, 1, batch, nf, a_num_aug) if a_num_aug else None}


def drloc(seed, c, n, m, l):
    """what the timhip_drloc_draw launch that reads the counter value c writes -> (pos_1, pos_2 int64 [n, m], deltax float32)"""
    cnt = n * m
    nblk = (cnt + 1) >> 1
    ctr = np.uint64((int(c) << DRLOC_DRAW_BITS) & _U64) + np.arange(nblk, dtype=np.uint64)
    w = philox4x32_7(seed, SITE_DRLOC, ctr).astype(np.uint64)          # element i: words (x, y) of block i / 2 if i is even, (z, w) if odd
    p = (w * np.uint64(l)) >> np.uint64(32)
    pos_1 = p[:, 0::2].reshape(-1)[:cnt].astype(np.int64).reshape(n, m)
    pos_2 = p[:, 1::2].reshape(-1)[:cnt].astype(np.int64).reshape(n, m)
    deltax = np.abs(pos_1 - pos_2).astype(np.float32) * (np.float32(1.0) / np.float32(l))      # (what torch's `/= l` is on the device)
    return pos_1, pos_2, deltax
