"""`timhip_attention_query_weights` on a real MI355X: the attention weights of query rows against keys read from a cache through a
window index, held bit for bit against `timhip_attention_weights` on the full qkv assembled from the same cache rows and query
rows (the two entries share their kernel bodies), elementwise against the float64 restatement (tests/query_maps_ref.py, pinned to
the reference's recorded weights by tests/test_query_maps_ref.py) on the STORED operand values, and for everything a window index
adds: regrouping, out-of-range entries, refusals.

The bound per shape is that of tests/test_gpu_attn_maps.py, restated: the restatement once more in float32 numpy on the test's own
inputs, its largest deviation from float64, times 4 (another summation order, the fast exp), plus 8 fp32 ulps of 1.0."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import query_maps_ref as QM  # noqa: E402
from tests.candidate_helpers import ulp_apart  # noqa: E402
from tests.test_gpu_parity import DEV  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd.functional import Runtime  # noqa: E402

ULPS8 = 8 * 2.0 ** -23
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -5
PRECS = ["fp16", "bf16", "fp32"]
W, G = 3, 7
WIDX = [2, 0, 0, 1, 2, 1, 1]                      # repeats and permutes the three windows

# head width x F: every width meets every F (key-block edges and the limit; 48 and F = 192 and the (width, blocks) pairs absent
# from attn_for_shape run the generic kernel); Q in {1, 25, 32, 33, 65} and H in {1, 8} rotate through them so that every width
# sees every Q and both H.  flags = 1: TIMHIP_DESC_ATTN_FP32 on a matrix-core shape
_FS, _QS = (1, 31, 32, 33, 100, 192), (1, 25, 32, 33, 65)
SHAPES = [(Dh, (1, 8)[(i + j) % 2], F, _QS[(i + j) % 5], 0) for i, Dh in enumerate((32, 64, 128, 48)) for j, F in enumerate(_FS)]
SHAPES += [(128, 8, 100, 25, 1), (32, 1, 33, 65, 1)]
SMALL = [(32, 8, 33, 33, 0), (64, 1, 100, 65, 0), (128, 8, 100, 25, 0), (48, 1, 31, 25, 0), (128, 8, 100, 25, 1)]


def st():
    return torch.cuda.current_stream().cuda_stream


def desc_of(Dh, Hh, F, S, B, prec, p_drop=0.0, flags=0):
    E = Dh * Hh
    return L.TimDesc(B, S, F, max(E // 2, 1), E, Hh, 4 * E, L.PRECISIONS[prec], p_drop, 0, 0, flags)


@functools.lru_cache(maxsize=None)
def case(Dh, Hh, F, Q, prec):
    """random pieces with scores of ordinary size (unit normal q and k), in the operand dtype (CPU); the float64 restatement on the
    stored values for WIDX, once, shared by every test of the shape; the bound from the float32 restatement of the same inputs"""
    E = Dh * Hh
    dt = Runtime(prec).op_dtype
    g = torch.Generator().manual_seed(1000 * Dh + 10 * F + Q + Hh)
    q, ko, vo = (torch.randn((G, Q, E), generator=g).to(dt) for _ in range(3))
    kc, vc = (torch.randn((W, F, E), generator=g).to(dt) for _ in range(2))
    wide = [t.to(torch.float64).numpy() for t in (q, ko, kc)]
    mean64 = QM.query_weights(*wide, WIDX, Hh)
    ph64 = QM.query_weights(*wide, WIDX, Hh, per_head=True)
    dev32 = max(np.abs(QM.query_weights(*wide, WIDX, Hh, dtype=np.float32) - mean64).max(),
                np.abs(QM.query_weights(*wide, WIDX, Hh, per_head=True, dtype=np.float32) - ph64).max())
    for a in (mean64, ph64):
        a.setflags(write=False)
    return {"qkv_q": torch.cat([q, ko, vo], -1).reshape(G * Q, 3 * E), "kv": torch.cat([kc, vc], -1).reshape(W * F, 2 * E),
            "fillers": torch.randn((G, F, 3 * E), generator=g).to(dt),
            "mean64": mean64, "ph64": ph64, "dev32": float(dev32), "bound": 4.0 * float(dev32) + ULPS8}


def full_qkv(c, Dh, Hh, F, Q, widx):
    """the [G' (F + Q), 3E] matrix timhip_attention_weights reads, from the same cache rows and query rows: window g' carries the
    K | V rows of cache window widx[g'] in its feature rows (their q columns: never read by a query row's weights)"""
    E, n = Dh * Hh, len(widx)
    kv = c["kv"].reshape(W, F, 2 * E)[torch.tensor(widx)]
    feats = torch.cat([c["fillers"][:n, :, :E], kv], -1)
    return torch.cat([feats, c["qkv_q"].reshape(G, Q, 3 * E)[:n]], 1).reshape(n * (F + Q), 3 * E).contiguous()


def run_query(desc, qkv_q, kv, ldkv, wrows, nW, widx, per_head, pad=0, guard=5, fill=float("nan")):
    """-> (rc, [G, (H,) Q, F + 1] weights, the whole padded buffer) - the output sits between `fill`-ed guard rows, with `pad`
    `fill`-ed guard columns behind every row; the caller checks what it expects of them"""
    Gn, Q, F, Hh = desc.B, desc.S, desc.F, desc.H
    ld = F + 1 + pad
    rows = Gn * (Hh if per_head else 1) * Q
    buf = torch.full(((rows + 2 * guard), ld), fill, dtype=torch.float32, device=DEV)
    w = buf[guard:guard + rows]
    idx = None if widx is None else torch.tensor(widx, dtype=torch.int32, device=DEV)
    rc = L.load().timhip_attention_query_weights(C.byref(desc), L.ptr(qkv_q), L.ptr(kv), ldkv, wrows, nW, L.ptr(idx), int(per_head),
                                                 L.ptr(w), ld, st())
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    body = out[guard:guard + rows, :F + 1].reshape((Gn, Hh, Q, F + 1) if per_head else (Gn, Q, F + 1))
    return rc, body, (out, guard, rows)


def untouched(padded, F, fill=float("nan")):
    out, guard, rows = padded
    same = np.isnan if np.isnan(fill) else (lambda a: a == fill)
    return bool(same(out[:guard]).all() and same(out[guard + rows:]).all() and same(out[guard:guard + rows, F + 1:]).all())


def run_ok(desc, qkv_q, kv, widx, per_head, pad=0, **kw):
    rc, body, padded = run_query(desc, qkv_q, kv, 2 * desc.E, desc.F, W, widx, per_head, pad, **kw)
    assert rc == 0, rc
    assert untouched(padded, desc.F), "guard words or columns past F written"
    return body


def run_full(desc, qkv, s0, per_head):
    B, S, F, Hh = desc.B, desc.S, desc.F, desc.H
    n = S - s0
    w = torch.full((B * (Hh if per_head else 1) * n, F + 1), float("nan"), dtype=torch.float32, device=DEV)
    rc = L.load().timhip_attention_weights(C.byref(desc), L.ptr(qkv), s0, int(per_head), L.ptr(w), F + 1, st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return w.cpu().numpy().reshape((B, Hh, n, F + 1) if per_head else (B, n, F + 1))


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the bits of timhip_attention_weights --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,Q,flags", SHAPES)
def test_rows_are_the_bits_of_attention_weights_on_the_assembled_qkv(Dh, Hh, F, Q, flags, prec):
    c = case(Dh, Hh, F, Q, prec)
    E, S = Dh * Hh, F + Q
    qd = desc_of(Dh, Hh, F, Q, G, prec, flags=flags)
    fd = desc_of(Dh, Hh, F, S, G, prec, flags=flags)
    qkv_q, kv, full = c["qkv_q"].to(DEV), c["kv"].to(DEV), full_qkv(c, Dh, Hh, F, Q, WIDX).to(DEV)
    for per_head in (False, True):
        want = run_full(fd, full, F, per_head)
        got = run_ok(qd, qkv_q, kv, WIDX, per_head)
        assert not np.isnan(got).any() and np.array_equal(u32(got), u32(want)), (per_head, float(np.abs(got - want).max()))
        # the NULL / G == W form, reading the keys where timhip_attention_fwd's qkv keeps them: kv = qkv + E, ldkv = 3E, wrows = S
        rc, inplace, padded = run_query(qd, qkv_q, full[:, E:], 3 * E, S, G, None, per_head)
        assert rc == 0 and untouched(padded, F) and np.array_equal(u32(inplace), u32(want))


# ---- 2. float64 accuracy and guards -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,Q,flags", SHAPES)
def test_weights_match_the_restatement_on_the_stored_values(Dh, Hh, F, Q, flags, prec):
    c = case(Dh, Hh, F, Q, prec)
    bound = c["bound"]
    desc = desc_of(Dh, Hh, F, Q, G, prec, flags=flags)
    qkv_q, kv = c["qkv_q"].to(DEV), c["kv"].to(DEV)
    worst = 0.0
    for pad in (0, 7):                                             # ld = F + 1, and a padded pitch (run_ok: the padding stays NaN)
        mean = run_ok(desc, qkv_q, kv, WIDX, False, pad)
        ph = run_ok(desc, qkv_q, kv, WIDX, True, pad)
        for got, want in ((mean, c["mean64"]), (ph, c["ph64"])):
            assert got.dtype == np.float32 and not np.isnan(got).any()
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= bound, (pad, err, bound)
            assert float(np.abs(got.sum(-1, dtype=np.float64) - 1.0).max()) <= bound * (F + 1)
        acc = np.zeros_like(mean)
        for h in range(Hh):                                        # the kernel's own mean of the per-head form
            acc += ph[:, h]
        assert int(ulp_apart(acc * (np.float32(1.0) / np.float32(Hh)), mean).max()) <= 2
    print("QUERYMAP kernel Dh=%d H=%d F=%d Q=%d flags=%d %s: float32-numpy deviation %.3g, bound %.3g, GPU max abs error %.3g"
          % (Dh, Hh, F, Q, flags, prec, c["dev32"], bound, worst))


# ---- 3. the same bits under regrouping -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,Q,flags", SMALL)
def test_a_group_gives_the_same_bits_alone_in_any_launch_and_on_every_run(Dh, Hh, F, Q, flags, prec):
    c = case(Dh, Hh, F, Q, prec)
    E = Dh * Hh
    rows, kv = c["qkv_q"].reshape(G, Q, 3 * E), c["kv"].to(DEV)

    def run(groups, per_head):
        """the launch made of these groups of the case, in this order"""
        sub = rows[torch.tensor(groups)].reshape(len(groups) * Q, 3 * E).contiguous().to(DEV)
        return run_ok(desc_of(Dh, Hh, F, Q, len(groups), prec, flags=flags), sub, kv, [WIDX[g] for g in groups], per_head)
    for per_head in (False, True):
        base = run(list(range(G)), per_head)
        assert np.array_equal(u32(run(list(range(G)), per_head)), u32(base))            # a second run
        for g in (0, 3, G - 1):
            assert np.array_equal(u32(run([g], per_head)[0]), u32(base[g]))             # alone
        perm = [4, 6, 0, 2, 5, 1, 3]
        assert np.array_equal(u32(run(perm, per_head)), u32(base[perm]))                # any permutation of the groups
        some = [5, 5, 1]
        assert np.array_equal(u32(run(some, per_head)), u32(base[some]))                # inside another G, a group twice


# ---- 4. out-of-range entries of widx --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,Q,flags", SMALL)
def test_an_out_of_range_window_gives_nan_rows_and_touches_nothing_else(Dh, Hh, F, Q, flags, prec):
    c = case(Dh, Hh, F, Q, prec)
    desc = desc_of(Dh, Hh, F, Q, G, prec, flags=flags)
    qkv_q, kv = c["qkv_q"].to(DEV), c["kv"].to(DEV)
    bad = {1: -1, 3: W, 6: 2 ** 31 - 1}
    widx = [bad.get(g, w) for g, w in enumerate(WIDX)]
    for per_head in (False, True):
        good = run_ok(desc, qkv_q, kv, WIDX, per_head)
        # a finite prefill: "not written" and "written as NaN" are different things here
        rc, got, padded = run_query(desc, qkv_q, kv, 2 * desc.E, F, W, widx, per_head, pad=3, fill=7.0)
        assert rc == 0 and untouched(padded, F, fill=7.0)
        for g in range(G):
            if g in bad:
                assert np.isnan(got[g]).all(), g                                        # columns 0 .. F of every row (and head)
            else:
                assert np.array_equal(u32(got[g]), u32(good[g])), g


# ---- 5. edge inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,Q,flags", SMALL)
def test_edge_inputs(Dh, Hh, F, Q, flags, prec):
    E = Dh * Hh
    dt = Runtime(prec).op_dtype
    desc = desc_of(Dh, Hh, F, Q, G, prec, flags=flags)
    g = torch.Generator().manual_seed(3)
    kv = torch.randn((W * F, 2 * E), generator=g).to(dt).to(DEV)
    # q = 0: every score is 0, every weight of every row the same value - 1 / (F + 1) as fp32 computes it where the head sum is
    # exact (H = 1; at H = 8 the fixed-order sum v, 2v, 3v, .. rounds: all equal, within 2 ulps)
    qkv_q = torch.randn((G * Q, 3 * E), generator=g)
    qkv_q[:, :E] = 0.0
    w = run_ok(desc, qkv_q.to(dt).to(DEV), kv, WIDX, False)
    v = np.float32(1.0) / np.float32(F + 1)
    assert np.all(w == w[0, 0, 0])
    assert w[0, 0, 0] == v if Hh == 1 else int(ulp_apart(w[0, 0, 0], v).max()) <= 2
    assert np.all(run_ok(desc, qkv_q.to(dt).to(DEV), kv, WIDX, True) == v)
    # one key's score far above the rest (scale * Dh * c^2 >= 90 against 0): that weight is 1.0, the others underflow to exact 0 -
    # the dominant key is key j0 of window 1 only, so groups of the other windows stay uniform over their F keys ... and their own
    c = 4.5 if Dh >= 32 else 6.0
    assert c * c * Dh / np.sqrt(Dh) >= 90.0
    j0 = F // 2
    qkv_q = torch.zeros((G * Q, 3 * E))
    qkv_q[:, :E] = c
    kvz = torch.zeros((W, F, 2 * E))
    kvz[1, j0, :E] = c
    w = run_ok(desc, qkv_q.to(dt).to(DEV), kvz.reshape(W * F, 2 * E).to(dt).to(DEV), WIDX, False)
    assert not np.isnan(w).any()
    for gi, win in enumerate(WIDX):
        if win == 1:
            assert np.all(w[gi, :, j0] == 1.0) and np.all(np.delete(w[gi], j0, axis=-1) == 0.0), gi
        else:
            assert np.abs(w[gi] - v).max() <= ULPS8, gi
    # the own key dominant: column F is 1.0, the cached keys exact zeros
    qkv_q[:, E:2 * E] = c
    w = run_ok(desc, qkv_q.to(dt).to(DEV), torch.zeros((W * F, 2 * E)).to(dt).to(DEV), WIDX, False)
    assert np.all(w[..., F] == 1.0) and np.all(w[..., :F] == 0.0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,Q,flags", SMALL)
def test_scores_at_the_operand_types_largest_finite_magnitude_stay_finite(Dh, Hh, F, Q, flags, prec):
    """Raw scores of +max and -max of the operand type (q = max in one component of every head, k = +1 for key j0 and -1 for key
    j1 there, 0 elsewhere): finite weights, 1.0 (within 8 ulps) at j0, exact zeros elsewhere.

    What this case is about: p = exp2(fma(score, c, -(max * c))) has, at the row's largest score, the rounding error of max * c
    as its exponent - at most 2^-24 |max * c|, a common factor the normalisation cancels while exp2 can take it.  fp16's max
    (65504, |max * c| <= 1.7e4) is far inside that range.  bf16's and fp32's (3.4e38, |max * c| = 4.3e37 .. 8.7e37) are not: the
    error is 3.6e29 .. 5.0e30 there (host arithmetic) and that line alone gave NaN in column j0 of every row, or in the whole
    row where the error is negative (measured on the MI355X before the kernel's wide-row path existed).  The query kernels
    therefore take exp2((score - max) * c) on rows with |max * c| >= 2^30 (attn_maps.hip: map_p_wide); every other row keeps the
    line above, which is what test_rows_are_the_bits_of_attention_weights_on_the_assembled_qkv holds."""
    E = Dh * Hh
    dt = Runtime(prec).op_dtype
    desc = desc_of(Dh, Hh, F, Q, G, prec, flags=flags)
    big = float(torch.finfo(dt).max)
    j0 = F // 2
    j1 = j0 + 1
    assert j1 < F
    qkv_q = torch.zeros((G * Q, 3 * E))
    qkv_q[:, 0:E:Dh] = big                                                     # component 0 of every head
    kvb = torch.zeros((W, F, 2 * E))
    kvb[:, j0, 0:E:Dh] = 1.0
    kvb[:, j1, 0:E:Dh] = -1.0
    c2 = np.float32(np.float32(1.0) / np.sqrt(np.float32(Dh))) * np.float32(1.4426950408889634)
    for per_head in (False, True):
        w = run_ok(desc, qkv_q.to(dt).to(DEV), kvb.reshape(W * F, 2 * E).to(dt).to(DEV), WIDX, per_head)
        bad = ~np.isfinite(w)
        print("QUERYMAP largest magnitude Dh=%d H=%d F=%d Q=%d flags=%d %s per_head=%d: |max * c| = %.3g, non-finite weights %d of %d "
              "(columns %s), weight at the largest score %r" % (Dh, Hh, F, Q, flags, prec, per_head, big * float(c2), int(bad.sum()), w.size,
                                                                sorted(set(np.nonzero(bad)[-1].tolist()))[:4], float(w.reshape(-1, F + 1)[0, j0])))
        assert not bad.any()
        assert np.abs(w[..., j0] - 1.0).max() <= ULPS8 and np.all(np.delete(w, j0, axis=-1) == 0.0)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_and_write_nothing():
    Dh, Hh, F, Q = 32, 2, 12, 5
    E = Dh * Hh
    lib = L.load()
    qkv_q = torch.zeros((G * Q, 3 * E), dtype=torch.float16, device=DEV)
    kv = torch.zeros((W * F, 2 * E), dtype=torch.float16, device=DEV)
    widx = torch.tensor(WIDX, dtype=torch.int32, device=DEV)
    buf = torch.full((G * Hh * Q * (F + 1) + 4,), float("nan"), dtype=torch.float32, device=DEV)
    d = desc_of(Dh, Hh, F, Q, G, "fp16")

    def rc(desc=d, q=L.ptr(qkv_q), k=L.ptr(kv), ldkv=2 * E, wrows=F, nW=W, idx=L.ptr(widx), per_head=0, w=L.ptr(buf), ld=F + 1):
        return lib.timhip_attention_query_weights(C.byref(desc) if desc is not None else None, q, k, ldkv, wrows, nW, idx, per_head, w,
                                                  ld, st())
    assert rc(desc=None) == EINVAL and rc(q=None) == EINVAL and rc(k=None) == EINVAL and rc(w=None) == EINVAL
    assert rc(desc=desc_of(Dh, Hh, F, Q, G, "fp16", p_drop=0.1)) == EINVAL
    assert rc(nW=0) == EINVAL and rc(idx=None) == EINVAL                        # NULL widx with G != W
    assert rc(ld=F) == EINVAL and rc(ldkv=2 * E - 1) == EINVAL and rc(wrows=F - 1) == EINVAL
    assert rc(desc=desc_of(Dh, Hh, 193, Q, G, "fp16"), ld=194, wrows=193) == EUNSUPPORTED
    assert rc(w=L.ptr(buf) + 2) == EALIGN and rc(w=L.ptr(buf) + 2, per_head=1) == EALIGN
    assert rc(k=L.ptr(kv) + 1) == EALIGN and rc(q=L.ptr(qkv_q) + 1) == EALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert int((~torch.isnan(buf)).sum()) == G * Q * (F + 1)
