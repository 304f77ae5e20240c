"""The eight C entry points of tim_amd/csrc/losses.hip, called on their own (tim_amd._lib) and held elementwise to their float64
restatements (tests/losses_ref.py, pinned on the CPU by tests/test_losses_ref.py), at the product's sizes and at the edges where
such kernels go wrong: grids that wrap, row pitches wider than the row, exact DIoU ties, saturated logits.

Rules of this file:
  * every output matrix sits between guard rows, NaN filled, with a padded pitch where the entry point takes one; after the call
    the guard rows and the padding columns are bit-identical to before.  Scalar outputs (loss, accum, block, normaliser) are words
    of a NaN-filled 16-float buffer of which only the documented words may change.  Padding columns of the INPUT matrices hold
    NaN: a read past column C shows up as a NaN result;
  * bounds are derived next to the assert from u = 2^-24: a sum of n fp32 terms in any order is within n u sum|terms|; the number
    of terms is (terms per thread) + 6 (wave tree) + 2 (four waves) + (atomic joins).  The fast intrinsics (__expf, __logf, powf)
    get an explicit allowance of a few u relative to their result and |argument| u for the rounding of their argument;
  * for saturated / large inputs the kernel is also allowed 8x the error of a torch-CPU float32 evaluation of the same formulas
    against float64, per element (docs/measurement_log.md records those figures and the kernel's observed worst ratios);
  * no element is excluded, and every kernel value must be finite where the reference is;
  * the existing whole-tensor tolerances (2e-6 relative CE loss, 1e-5 of the gradient's largest element, 2e-5 relative focal)
    stay as an outer check: for cross entropy on the ordinary inputs, for focal and the side loss at every shape.
RATIOS collects the worst observed |kernel - ref| / bound per family; a module fixture prints it after the last test.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import losses_ref as R  # noqa: E402
from tests.helpers import GOLDEN  # noqa: E402
from tests.test_gpu_rowops import Out, ia, pa, same_bits, st, sync  # noqa: E402
from tim_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
U = R.EPS32
NAN = float("nan")
OK, EINVAL, EALIGN = 0, -1, -5
RATIOS = {}      # family -> worst |kernel - ref| / bound seen
F32ERR = {}      # family -> worst float32-CPU error against float64 seen (absolute)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    """after the module's last test: the worst |kernel - ref| / bound and the float32-CPU errors seen (docs/measurement_log.md; every
    ratio is asserted where it is computed)"""
    yield
    for k in sorted(RATIOS):
        print("ratio %-32s %.3g%s" % (k, RATIOS[k], "   f32-cpu err %.3g" % F32ERR[k] if k in F32ERR else ""))


def note(key, err, bound, f32err=None):
    r = float((err / bound.clamp(min=1e-300)).max()) if torch.is_tensor(err) else float(err / max(bound, 1e-300))
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    if f32err is not None:
        F32ERR[key] = max(F32ERR.get(key, 0.0), float(f32err.max()) if torch.is_tensor(f32err) else float(f32err))
    return r


def within(got, ref, bound, key, f32err=None):
    """elementwise |got - ref| <= bound with every element finite; records the worst ratio"""
    got, ref = got.to(F64), ref.to(F64)
    assert bool(torch.isfinite(got).all()), key + ": non-finite kernel value"
    err = (got - ref).abs()
    r = note(key, err, bound if torch.is_tensor(bound) else torch.full_like(err, bound), f32err)
    assert r <= 1.0, "%s: worst |kernel - ref| / bound = %.3g" % (key, r)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def raw(name):
    return getattr(L.load(), name)


class Scal:
    """16 NaN floats; the entry points get pointers to words of it; `changed()` lists the words that are no longer the NaN"""

    def __init__(self):
        self.buf = torch.full((16,), NAN, device=DEV)
        self.before = self.buf.clone()

    def p(self, word):
        return self.buf.data_ptr() + 4 * word

    def changed(self):
        a, b = self.buf.cpu().view(torch.int32), self.before.cpu().view(torch.int32)
        return [i for i in range(16) if a[i] != b[i]]

    def get(self, lo, n=1):
        return self.buf[lo:lo + n].cpu().to(F64)


def padded(x, ld, fill=NAN):
    """[rows, C] -> device fp32 view [rows, C] of a [rows, ld] buffer whose padding columns hold `fill`"""
    rows, Cn = x.shape
    buf = torch.full((rows, ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :Cn] = x.to(DEV)
    return buf


def out_ok(o, Cn):
    """guards intact, padding columns untouched"""
    return o.guards_intact() and same_bits(o.v[:, Cn:], o.pre[:, Cn:])


# =============================================================================================== cross entropy under mixup
CE_SHAPES = [(1, 5), (3, 13), (5, 1023), (4, 1024), (96, 3806), (960, 3806), (640, 44), (2, 9000)]


def _ce_case(rows, Cn, variant, seed):
    x = torch.randn(rows, Cn, generator=gen(seed)) * 2.0
    edge = torch.tensor([-1, Cn - 1, Cn, Cn + 7, 0])
    ya = torch.randint(Cn, (rows,), generator=gen(seed + 1))
    yb = torch.randint(Cn, (rows,), generator=gen(seed + 2))
    if rows >= 2:      # (a single row keeps its valid target)
        k = min(rows, 5)
        ya[:k] = edge.roll(1)[:k]
        yb[rows - k:] = edge[:k]
    lam = 0.3
    if variant == "nob":
        yb, lam = None, 1.0
    elif variant == "emptyb":          # side b has no valid row while lam < 1: its term is 0 and its rows get no gradient
        yb = torch.where(torch.arange(rows) % 2 == 0, torch.full((rows,), -1), torch.full((rows,), Cn + 7))
    elif variant == "emptya":
        ya = torch.full((rows,), -1)
    elif variant == "sat":             # one logit at +60, the rest 0, the target on it: CE is 0 up to rounding, never negative
        hot = torch.randint(Cn, (rows,), generator=gen(seed + 3))
        x.zero_()
        x[torch.arange(rows), hot] = 60.0
        ya = hot.clone()
        yb = hot.clone()
        yb[::2] = (hot[::2] + 1) % Cn if Cn > 1 else hot[::2]
    elif variant == "big":
        x = x * 1e3
    return x, ya, yb, lam


def _ce_bounds(x64, ref, rows, Cn, smoothing, g):
    """fp32 bounds for stats, accum, loss and dlogits from the float64 values (see the module docstring for the counting)"""
    nt = 256 if Cn >= 1024 else 64
    T = (Cn + nt - 1) // nt + 8                                       # terms per thread + wave tree + four waves
    lse, mean = ref["stats"][:, 0], ref["stats"][:, 1]
    b_mean = T * U * x64.abs().sum(1) / Cn + U * mean.abs()
    d = x64 - x64.max(1, keepdim=True).values                         # <= 0; the subtraction rounds by u |d|
    e = d.exp()
    se = e.sum(1)
    # __expf(d): relative (2 |d| + 8) u (argument rounding through x log2(e), a few ulp of the exp2 unit); sum of C terms: T u se
    b_se = (e * (2 * d.abs() + 8)).sum(1) * U + T * U * se
    b_lse = b_se / se + 8 * U * se.log().clamp(min=1.0) + U * lse.abs()   # __logf: a few ulp of max(1, log se); mx + log: one rounding
    b_ce = []
    for k in (2, 3):
        ce = ref["stats"][:, k]
        b_ce.append(torch.where(ce >= 0, (1 - smoothing) * (b_lse + 2 * U * lse.abs()) + smoothing * (2 * b_lse + b_mean)
                                + 4 * U * ce.abs(), torch.zeros_like(ce)))
    Tr = (rows + 255) // 256 + 8
    acc = ref["accum"]
    b_acc = torch.zeros(4, dtype=F64)
    for k in (0, 1):
        ce = ref["stats"][:, 2 + k]
        b_acc[2 * k] = b_ce[k].sum() + Tr * U * ce.clamp(min=0).sum()
    return b_mean, b_lse, b_ce, b_acc


@pytest.mark.parametrize("smoothing", [0.0, 0.2])
@pytest.mark.parametrize("rows,Cn", CE_SHAPES)
def test_ce_mixup_kernels(rows, Cn, smoothing):
    """ce_rows_kernel<1> (C < 1024, four rows per block) / <4> (one row per block), ce_finish_kernel, ce_bwd_kernel (its grid capped at
    8 blocks per row from C > 8192): stats rows, accum, loss, full gradient; ld = C and C + 12, ldd = C + 4; targets -1, C - 1,
    C and C + 7; yb NULL; a side with no valid row under lam = 0.3; saturated rows; logits scaled by 1e3; two calls repeat bit
    for bit (no atomics in this family)."""
    g = 1.7
    for vi, variant in enumerate(["mix", "nob", "emptyb", "emptya", "sat", "big"]):
        x, ya, yb, lam = _ce_case(rows, Cn, variant, seed=rows + Cn + vi)
        x64 = x.to(F64)
        ref = R.ce_mixup(x64, ya, yb, lam, smoothing, g=g)
        hard = variant in ("sat", "big")
        f32 = R.ce_mixup(x, ya, yb, lam, smoothing, g=g) if hard else None
        b_mean, b_lse, b_ce, b_acc = _ce_bounds(x64, ref, rows, Cn, smoothing, g)
        yad, ybd = ya.to(DEV), None if yb is None else yb.to(DEV)
        gout = torch.tensor([g], device=DEV)
        for ld in (Cn, Cn + 12):
            xd = padded(x, ld)
            keep = xd.clone()
            runs = []
            for rep in range(2):
                stats, dx, sc = Out(rows, 4), Out(rows, Cn + 4), Scal()
                L.call("timhip_ce_mixup_fwd", xd.data_ptr(), rows, Cn, ld, L.ptr(yad), L.ptr(ybd), lam, smoothing, stats.ptr, sc.p(4),
                       sc.p(10), st())
                L.call("timhip_ce_mixup_bwd", xd.data_ptr(), rows, Cn, ld, L.ptr(yad), L.ptr(ybd), lam, smoothing, stats.ptr, sc.p(4),
                       L.ptr(gout), dx.ptr, Cn + 4, st())
                runs.append((stats, dx, sc))
            sync()
            stats, dx, sc = runs[0]
            key = "ce/" + variant
            assert same_bits(xd, keep) and stats.guards_intact() and out_ok(dx, Cn)
            assert sc.changed() == [4, 5, 6, 7, 10], sc.changed()
            assert same_bits(stats.v, runs[1][0].v) and same_bits(dx.v, runs[1][1].v) and same_bits(sc.buf, runs[1][2].buf)
            s = stats.v.cpu().to(F64)
            e32 = (lambda k: 8 * (f32[k].to(F64) - ref[k]).abs()) if hard else (lambda k: 0.0)
            es = e32("stats")
            within(s[:, 0], ref["stats"][:, 0], b_lse + (es[:, 0] if hard else 0.0), key + "/lse")
            within(s[:, 1], ref["stats"][:, 1], b_mean + (es[:, 1] if hard else 0.0), key + "/mean")
            for k in (2, 3):
                ign = ref["stats"][:, k] < 0
                assert bool((s[ign, k] == -1.0).all()) and bool((s[~ign, k] >= 0.0).all()), "ignored <-> -1, counted <-> >= 0"
                within(s[:, k], ref["stats"][:, k], b_ce[k - 2] + (es[:, k] if hard else 0.0) + R.TINY32, key + "/ce",
                       None if not hard else (f32["stats"][:, k].to(F64) - ref["stats"][:, k]).abs())
            acc = sc.get(4, 4)
            assert acc[1].item() == ref["accum"][1].item() and acc[3].item() == ref["accum"][3].item()      # counts: exact
            ea = e32("accum")
            within(acc, ref["accum"], b_acc + (ea if hard else 0.0) + R.TINY32, key + "/accum")
            n_a, n_b = max(ref["accum"][1].item(), 1.0), max(ref["accum"][3].item(), 1.0)
            b_loss = lam * b_acc[0] / n_a + (1 - lam) * b_acc[2] / n_b + 4 * U * abs(ref["loss"].item()) + R.TINY32
            loss = sc.get(10)[0]
            within(loss, ref["loss"], b_loss + (e32("loss") if hard else 0.0), key + "/loss")
            # gradient, per element, v = w exp(x - lse) - w eps / C [- wa (1 - eps) at c = ya] [- wb (1 - eps) at c = yb]:
            #   * the softmax term sm = w exp(x - lse) moves relatively by (3 |x - lse| + 8) u (the rounded difference, the fast exp's
            #     product with a rounded log2(e), a few ulp of its exp2 unit), by the absolute error of the stored lse, and by 8 u
            #     for w itself (lam, 1 - lam and g as floats, g lam, the division by the count, wa + wb) and the product;
            #   * the constant terms rest = v - sm (w eps / C everywhere, the one-hot terms at the target columns ALONE) carry the
            #     same roundings of w plus those of eps or 1 - eps, their product and / C: 10 u relative to their own size;
            #   * each subtraction rounds its result: 3 u |v| covers the three of them (a partial result is no larger than
            #     sm + |rest|, which the 8 u above leave room for);
            #   * a term below the smallest normal may be flushed to zero: (1 + w) 2^-126.
            # Nothing here scales with the row's weight except at the target columns: a tail element w exp(x - lse) of 1e-7 w is
            # held to a few u of ITSELF plus u w eps / C.
            wsum = torch.zeros(rows, dtype=F64)
            for y, coef, cnt in ((ya, lam, ref["accum"][1].item()), (yb, 1 - lam, ref["accum"][3].item())):
                if y is not None and cnt > 0:
                    wsum += torch.where((y >= 0) & (y < Cn), torch.full((rows,), g * coef / cnt, dtype=F64), torch.zeros(rows, dtype=F64))
            dl = x64 - ref["stats"][:, :1]
            sm = wsum[:, None] * dl.exp()
            rest = (ref["dlogits"] - sm).abs()
            b_d = sm * ((3 * dl.abs() + 8) * U + b_lse[:, None] + (es[:, :1] if hard else 0.0) + 8 * U) \
                + 10 * U * rest + 3 * U * ref["dlogits"].abs()
            b_tiny = (1 + wsum[:, None]) * R.TINY32
            d = dx.v[:, :Cn].cpu().to(F64)
            within(d, ref["dlogits"], b_d + b_tiny + (e32("dlogits") if hard else 0.0), key + "/dlogits",
                   None if not hard else (f32["dlogits"].to(F64) - ref["dlogits"]).abs())
            norow = wsum == 0
            assert bool((d[norow] == 0).all()), "a row no side counts gets an exactly zero gradient"
            if variant == "sat":
                assert acc[1].item() == rows, "saturated rows stay counted in n_a"
            if variant == "mix":       # grad_out == NULL stands for 1: the same gradient without its factor g
                d1 = Out(rows, Cn + 4)
                L.call("timhip_ce_mixup_bwd", xd.data_ptr(), rows, Cn, ld, L.ptr(yad), L.ptr(ybd), lam, smoothing, stats.ptr, sc.p(4),
                       None, d1.ptr, Cn + 4, st())
                sync()
                assert out_ok(d1, Cn)
                within(d1.v[:, :Cn].cpu(), ref["dlogits"] / g, b_d / g + b_tiny, key + "/dlogits-no-grad_out")
            if not hard:     # the whole-tensor tolerances of tests/test_gpu_losses.py as an outer check
                assert abs(loss.item() - ref["loss"].item()) < 2e-6 * max(1.0, abs(ref["loss"].item()))
                assert (d - ref["dlogits"]).abs().max().item() <= 1e-5 * max(ref["dlogits"].abs().max().item(), 1e-30)


# =============================================================================================== sigmoid focal loss
def _focal_inputs(rows, Cn, seed, device_side=False):
    """logits ~ 3 N(0, 1) with +-20, +-90, +-200 planted; targets: smoothed values with exact 0 and 1 planted"""
    if device_side:
        gd = torch.Generator(device=DEV).manual_seed(seed)
        x = (torch.randn(rows, Cn, generator=gd, device=DEV) * 3.0)
        t = torch.rand(rows, Cn, generator=gd, device=DEV).pow(8.0)
        w = torch.rand(rows, generator=gd, device=DEV) + 0.5
        valid = (torch.rand(rows, generator=gd, device=DEV) > 0.25)
        x, t, w, valid = x.cpu(), t.cpu(), w.cpu(), valid.cpu()
    else:
        x = torch.randn(rows, Cn, generator=gen(seed)) * 3.0
        t = torch.rand(rows, Cn, generator=gen(seed + 1)).pow(8.0)
        w = torch.rand(rows, generator=gen(seed + 2)) + 0.5
        valid = torch.rand(rows, generator=gen(seed + 3)) > 0.25
    n = rows * Cn
    xf, tf = x.view(-1), t.view(-1)
    ext = torch.tensor([20.0, -20.0, 90.0, -90.0, 200.0, -200.0])
    tv = torch.tensor([0.0, 1.0, 0.9, 0.001])
    k = 0
    for e in ext:                      # every extreme logit against every kind of target, at the front and at the very end
        for tt in tv:
            for pos in (k % n, n - 1 - (k % n)):
                xf[pos], tf[pos] = e, tt
            k += 1
    tf[(torch.arange(n) % 11) == 3] = 0.0
    tf[(torch.arange(n) % 97) == 5] = 1.0
    valid[0] = True
    valid[rows - 1] = True
    return x, t, w, valid


def _focal_check(x, t, w, valid, alpha, gamma, want_elem, key, g=0.6):
    """g = None: grad_out == NULL, which stands for 1"""
    rows, Cn = x.shape
    gout = None if g is None else torch.tensor([g], device=DEV)
    g = 1.0 if g is None else g
    chunk = max(512, (1 << 21) // Cn)          # rows per float64 reference chunk
    n = rows * Cn
    xd, td = x.to(DEV), t.to(DEV)
    wd = None if w is None else w.to(DEV)
    vd = None if valid is None else valid.to(device=DEV, dtype=torch.uint8)
    keep = (xd.clone(), td.clone())
    elem = Out(rows, Cn) if want_elem else None
    dx = Out(rows, Cn)
    sc = Scal()
    L.call("timhip_focal_loss_fwd", L.ptr(xd), L.ptr(td), rows, Cn, L.ptr(wd), L.ptr(vd), alpha, gamma, sc.p(3),
           None if elem is None else elem.ptr, st())
    L.call("timhip_focal_loss_bwd", L.ptr(xd), L.ptr(td), rows, Cn, L.ptr(wd), L.ptr(vd), alpha, gamma, L.ptr(gout), dx.ptr, st())
    sync()
    assert same_bits(xd, keep[0]) and same_bits(td, keep[1]) and dx.guards_intact() and (elem is None or elem.guards_intact())
    assert sc.changed() == [3], sc.changed()
    got_e = None if elem is None else elem.v.cpu()
    got_d = dx.v.cpu()
    tot = b_tot = mag = 0.0
    dmax = emax = 0.0
    for r0 in range(0, rows, chunk):
        sl = slice(r0, min(rows, r0 + chunk))
        x64, t64 = x[sl].to(F64), t[sl].to(F64)
        ww = None if w is None else w[sl].to(F64)
        vv = None if valid is None else valid[sl]
        re, _, rd = R.focal(x64, t64, ww, vv, alpha, gamma, g=g)
        fe, _, fd = R.focal(x[sl], t[sl], None if w is None else w[sl], vv, alpha, gamma, g=g)          # float32, kernel's order
        bl, bd = R.focal_bound(x64, t64, alpha, gamma)
        f = R._row_factor(x64.shape[0], ww, vv, F64)[:, None]
        e_f32, d_f32 = (fe.to(F64) - re).abs(), (fd.to(F64) - rd).abs()
        assert bool(torch.isfinite(re).all() and torch.isfinite(rd).all())
        b_e = f * bl + 8 * e_f32 + 2 * U * re.abs() + R.TINY32
        b_d = g * f * bd + 8 * d_f32 + 3 * U * rd.abs() + R.TINY32
        within(got_d[sl], rd, b_d, key + "/dx", d_f32)
        if vv is not None:
            assert bool((got_d[sl][~vv] == 0).all())
        if got_e is not None:
            within(got_e[sl], re, b_e, key + "/elem", e_f32)
            if vv is not None:
                assert bool((got_e[sl][~vv] == 0).all())
        tot += re.sum().item()
        b_tot += b_e.sum().item()
        mag += re.abs().sum().item()
        dmax, emax = max(dmax, rd.abs().max().item()), max(emax, (got_d[sl].to(F64) - rd).abs().max().item())
    blocks = min((n + 255) // 256, 512)
    T = (n + blocks * 256 - 1) // (blocks * 256) + 8 + blocks           # per thread + trees + one atomic join per block
    got = sc.get(3)[0].item()
    assert np.isfinite(got)
    r = note(key + "/sum", abs(got - tot), b_tot + T * U * mag + R.TINY32)
    assert r <= 1.0, (key, got, tot, r)
    # the whole-tensor tolerances of tests/test_gpu_losses.py as an outer check, at every shape
    print("outer %s %dx%d: sum rel %.3g (2e-5), dx err / largest %.3g (1e-5)" % (key, rows, Cn, abs(got - tot) / max(abs(tot), 1e-300),
                                                                              emax / max(dmax, 1e-300)))
    assert abs(got - tot) <= 2e-5 * abs(tot) and emax <= 1e-5 * dmax


@pytest.mark.parametrize("alpha", [-1.0, 0.25])
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 3.0])
@pytest.mark.parametrize("rows,Cn", [(131073, 1), (3, 43691), (1001, 97), (5, 1), (1, 300)])
def test_focal_kernels(rows, Cn, gamma, alpha):
    """focal_fwd_kernel / focal_bwd_kernel: 131 073 elements (one past the forward grid's 512 x 256) as C = 1 and as three long rows,
    an element count that is no multiple of 256, tiny shapes; w / valid / elem / grad_out each NULL or given; every gamma branch of focal_term
    (q * q, powf, the q > 0 guard) and both alpha branches; logits of +-20, +-90, +-200 against targets 0, 1 and smoothed."""
    x, t, w, valid = _focal_inputs(rows, Cn, seed=rows + Cn)
    for ww, vv, want_elem, g in ((w, valid, True, 0.6), (None, None, False, None), (w, None, False, 0.6), (None, valid, True, 0.6)):
        _focal_check(x, t, ww, vv, alpha, gamma, want_elem, "focal/g%g" % gamma, g=g)


def test_focal_full_size():
    """the product's 16 x 399 query rows x 3806 action classes = 24.3 M elements: the forward's 512-block grid walks 186 elements per
    thread and joins 512 atomics, the backward's 4096-block grid wraps 24 times, i / C runs past 2^24"""
    rows, Cn = 6384, 3806
    x, t, w, valid = _focal_inputs(rows, Cn, seed=5, device_side=True)
    _focal_check(x, t, w, valid, 0.25, 2.0, True, "focal/full")


def test_focal_element_index_past_2_31():
    """focal_fwd_kernel walks i = 0 .. rows * C - 1 in 64 bits and looks its row up as i / C.  At the product's 24.3 M elements an
    index kept in 32 bits gives the same values; it differs from element 2^31 on.  (2^30 + 8) rows x 2 classes is 2^31 + 16
    elements; every row is switched off through `valid` except four below row 2^30 and three from it on (the last row among
    them), so the float64 reference has 14 terms.  An `int` element index turns negative for those three rows and looks their
    flag up 2^30 bytes in front of `valid`: the flags therefore sit behind 2^30 zero bytes of the same allocation, and such a
    kernel finds "switched off" there and loses their terms, half of the sum.  One 8 GiB buffer serves as logits and as
    targets (values in [0, 1]; both are only read); elem and the backward, 8 GiB each, are left out.
    What this pins: the ELEMENT index.  A kernel that keeps i in 64 bits and only narrows the quotient i / C to `int` computes the
    same values for every rows < 2^31 the entry point accepts, with or without the 512-block cap, and passes here as it should.
    The test holds about 10 GiB of device memory (8 GiB + 2 GiB) and does not look at what is free first: on a card that
    others fill it ends in torch's out-of-memory error, which is then no finding about the kernel."""
    rows, Cn = (1 << 30) + 8, 2
    n = rows * Cn
    on = torch.tensor([0, 5, (1 << 29) + 3, (1 << 30) - 1, 1 << 30, (1 << 30) + 3, rows - 1])
    v = torch.tensor([[0.0, 1.0], [0.25, 0.9], [0.001, 0.5], [1.0, 0.0], [0.75, 0.125], [0.9, 1.0], [0.5, 0.0625]])
    front = 1 << 30
    xt = torch.zeros(n, device=DEV)
    vbuf = torch.zeros(front + rows + 64, dtype=torch.uint8, device=DEV)
    idx = (on[:, None] * Cn + torch.arange(Cn)).to(DEV)
    xt[idx] = v.to(DEV)
    vbuf[(front + on).to(DEV)] = 1
    sc = Scal()
    L.call("timhip_focal_loss_fwd", xt.data_ptr(), xt.data_ptr(), rows, Cn, None, vbuf.data_ptr() + front, 0.25, 2.0, sc.p(3), None, st())
    sync()
    assert sc.changed() == [3], sc.changed()
    assert int(xt.count_nonzero()) == int(v.count_nonzero()) and int(vbuf.sum(dtype=torch.int64)) == on.numel()      # inputs only read
    got = sc.get(3)[0].item()
    del xt, vbuf
    torch.cuda.empty_cache()
    v64 = v.to(F64)
    re, tot, _ = R.focal(v64, v64, None, None, 0.25, 2.0)
    fe, _, _ = R.focal(v, v, None, None, 0.25, 2.0)
    bl, _ = R.focal_bound(v64, v64, 0.25, 2.0)
    # every other term is an exact 0, and adding 0 is exact: 14 terms, the trees, and at most 14 non-zero atomic joins
    bound = (bl + 8 * (fe.to(F64) - re).abs() + 2 * U * re.abs()).sum().item() + (14 + 8 + 14) * U * re.abs().sum().item()
    lost = re[4:].sum().item()
    print("focal 2^31: kernel %.9g, float64 %.9g, bound %.3g, the rows from 2^30 on hold %.3g of it" % (got, tot.item(), bound, lost))
    assert lost > 1e4 * bound
    assert note("focal/index-2^31/sum", abs(got - tot.item()), bound) <= 1.0, (got, tot.item())


# =============================================================================================== 1-D DIoU
def _tie_rows():
    g = np.load(os.path.join(GOLDEN, "loss_det_ties.npz"))
    return torch.from_numpy(g["pred"]), torch.from_numpy(g["off"]), g


def _diou_bounds(loss, scale, g):
    """per row: loss = 1 - I / Uc + z^2 with each term <= 1 in a dozen roundings: 16 u; the gradient's terms sum to at most `scale`
    = 2 / Uc + 1 / Lcc in magnitude (tests/losses_ref.py), each through at most 8 roundings"""
    return 16 * U * torch.ones_like(loss), abs(g) * 8 * U * scale[:, None] + R.TINY32


@pytest.mark.parametrize("n", [1, 44, 255, 256, 65537])
def test_diou_kernel(n):
    """diou_kernel on the tie fixture (n = 44: the reference's compiled-call gradient itself) and on it tiled among random rows up to
    65 537 rows (the 256-block grid wraps); with and without `valid`; forward only, backward only, both.  At an exact tie the
    strict rule gives the tied side nothing: a split-tie gradient is off by half a term, orders of magnitude past the bound."""
    p44, o44, fx = _tie_rows()
    if n <= 44:
        pred, off = p44[:n].clone(), o44[:n].clone()
    else:
        pred, off = torch.rand(n, 2, generator=gen(n)) * 2.0, torch.rand(n, 2, generator=gen(n + 1)) * 2.0
        for s in (0, n // 2 - 7, n - 44):          # the special rows at the front, in the middle and at the very end
            pred[s:s + 44], off[s:s + 44] = p44, o44
    g = 0.7
    pd, od = pred.to(DEV), off.to(DEV)
    gout = torch.tensor([g], device=DEV)
    for valid in (None, torch.arange(n) % 5 != 2):
        vd = None if valid is None else valid.to(device=DEV, dtype=torch.uint8)
        loss, d, br, scale = R.diou_1d(pred.to(F64), off.to(F64), valid, 1e-8, g=g)
        b_l, b_d = _diou_bounds(loss, scale, g)
        blocks = min((n + 255) // 256, 256)
        T = (n + blocks * 256 - 1) // (blocks * 256) + 6 + blocks * 4           # per thread + wave tree + one atomic per wave
        b_sum = b_l.sum().item() + T * U * loss.abs().sum().item()
        for mode in ("fwd", "bwd", "both"):
            sc, dp = Scal(), Out(n, 2)
            L.call("timhip_diou_1d", L.ptr(pd), L.ptr(od), n, L.ptr(vd), 1e-8, L.ptr(gout), sc.p(2) if mode != "bwd" else None,
                   dp.ptr if mode != "fwd" else None, st())
            sync()
            assert dp.guards_intact()
            assert sc.changed() == ([2] if mode != "bwd" else []), (mode, sc.changed())
            if mode != "bwd":
                got = sc.get(2)[0].item()
                assert note("diou/sum", abs(got - loss.sum().item()), b_sum) <= 1.0, (got, loss.sum().item())
                assert abs(got - loss.sum().item()) <= 1e-5 * abs(loss.sum().item())
            if mode != "fwd":
                within(dp.v.cpu(), d, b_d, "diou/dpred")
                if valid is not None:
                    assert bool((dp.v.cpu()[~valid] == 0).all())
            else:
                assert same_bits(dp.v, dp.pre)
        if n == 44 and valid is None:     # the reference's own compiled-call numbers (fp32: 8 more roundings of the same scale)
            sc, dp = Scal(), Out(n, 2)
            L.call("timhip_diou_1d", L.ptr(pd), L.ptr(od), n, None, 1e-8, None, sc.p(2), dp.ptr, st())
            sync()
            within(dp.v.cpu(), torch.from_numpy(fx["dpred"]), 16 * U * scale[:, None] + R.TINY32, "diou/dpred-vs-reference")
            assert abs(sc.get(2)[0].item() - float(fx["diou"])) <= 1e-6 * float(fx["diou"])
            assert float(np.abs(fx["dpred_first_call"] - fx["dpred"]).max()) > 0.1       # a split-tie gradient is a different one


# =============================================================================================== detection side loss
def _side_inputs(rows, Cs, seed, npos, all_outside=False, ties=False, device_side=False):
    gg = gen(seed)
    if device_side:
        gd = torch.Generator(device=DEV).manual_seed(seed)
        xs = [(torch.randn(rows, c, generator=gd, device=DEV) * 3.0).cpu() for c in Cs]
        ts = [torch.rand(rows, c, generator=gd, device=DEV).pow(8.0).cpu() for c in Cs]
    else:
        xs = [torch.randn(rows, c, generator=gg) * 3.0 for c in Cs]
        ts = [torch.rand(rows, c, generator=gg).pow(8.0) for c in Cs]
    ext = torch.tensor([20.0, -20.0, 90.0, -90.0, 200.0, -200.0])
    for x, t in zip(xs, ts):
        xf, tf = x.view(-1), t.view(-1)
        for k in range(min(6, xf.numel())):
            xf[k], tf[k] = ext[k], (0.0, 1.0, 0.9)[k % 3]
        tf[(torch.arange(tf.numel()) % 13) == 4] = 0.0
    iou = torch.rand(rows, generator=gg)
    iou[torch.randperm(rows, generator=gg)[:rows // 10]] = -1.0
    iou[0] = 0.9
    if all_outside:
        iou[:] = -1.0
    off = torch.full((rows, 2), float("inf"))
    reg = torch.rand(rows, 2, generator=gg) * 3.0
    pos = torch.nonzero(iou >= 0.6).flatten()[:npos] if not all_outside else torch.arange(min(npos, rows))
    off[pos] = torch.rand(pos.numel(), 2, generator=gg) * 3.0
    if ties:
        p44, o44, _ = _tie_rows()
        s = rows - 44 - 3
        reg[s:s + 44], off[s:s + 44] = p44, o44
    return xs, ts, iou, off, reg


def _side_check(xs, ts, iou, off, reg, gamma, alpha, null_head, key, null_gout=False, chunk=512):
    """null_gout: grad_out == NULL, which stands for 1"""
    K, rows = len(xs), iou.numel()
    Cs = [x.shape[1] for x in xs]
    thr, eps, lam, mom, norm0, g = 0.6, 1e-8, 0.5, 0.9, 250.0, (1.0 if null_gout else 0.7)
    xd, td = [x.to(DEV) for x in xs], [t.to(DEV) for t in ts]
    ud, od, rd = iou.to(DEV), off.to(DEV), reg.to(DEV)
    gout = None if null_gout else torch.tensor([g], device=DEV)
    valid, pos = iou >= 0, off[:, 0] != float("inf")
    w = torch.where(iou < thr, torch.ones_like(iou), iou).to(F64)
    npos = float(pos.sum())
    dl, dd, _, dscale = R.diou_1d(reg.to(F64), off.to(F64), pos, eps)
    sc = Scal()
    sc.buf[15] = norm0                                        # the running normaliser: word 15, in / out
    norm_in = norm0
    for call in range(2):                                     # two consecutive calls: the normaliser is a running value
        nm = mom * norm_in + (1 - mom) * max(npos, 1.0)
        dxs = [None if k == null_head else Out(rows, Cs[k]) for k in range(K)]
        dreg = Out(rows, 2)
        sc.buf[:15] = NAN
        sc.before = sc.buf.clone()
        L.call("timhip_det_side_loss_fwd", pa(xd), pa(td), ia(Cs), K, rows, L.ptr(ud), L.ptr(od), L.ptr(rd), thr, alpha, gamma, eps, lam,
               mom, sc.p(15), sc.p(4), st())
        L.call("timhip_det_side_loss_bwd", pa(xd), pa(td), ia(Cs), K, rows, L.ptr(ud), L.ptr(od), L.ptr(rd), thr, alpha, gamma, eps, lam,
               sc.p(4), L.ptr(gout), (C.c_void_p * K)(*[None if o is None else o.ptr for o in dxs]), dreg.ptr, st())
        sync()
        assert sc.changed() == [4, 5, 6, 7, 8, 9, 10, 11, 15], sc.changed()
        blk = sc.get(4, 8)
        assert blk[3].item() == npos and bool((blk[5:] == 0).all())
        assert abs(blk[4].item() - nm) <= 4 * U * nm and sc.get(15)[0].item() == blk[4].item()
        fsum = b_fsum = fmag = 0.0
        for k in range(K):
            n = rows * Cs[k]
            gk = g / (K * nm)
            o = dxs[k]
            assert o is None or o.guards_intact()
            got_d = None if o is None else o.v.cpu()
            emax = dmax = 0.0
            for r0 in range(0, rows, chunk):
                sl = slice(r0, min(rows, r0 + chunk))
                x64, t64 = xs[k][sl].to(F64), ts[k][sl].to(F64)
                re, _, rdx = R.focal(x64, t64, w[sl], valid[sl], alpha, gamma, g=gk)
                fe, _, fd = R.focal(xs[k][sl], ts[k][sl], w[sl].float(), valid[sl], alpha, gamma, g=gk)
                bl, bd = R.focal_bound(x64, t64, alpha, gamma)
                f = R._row_factor(x64.shape[0], w[sl], valid[sl], F64)[:, None]
                e_f32, d_f32 = (fe.to(F64) - re).abs(), (fd.to(F64) - rdx).abs()
                b_e = f * bl + 8 * e_f32 + 2 * U * re.abs() + R.TINY32
                fsum += re.sum().item()
                fmag += re.abs().sum().item()
                blocks = min((n + 255) // 256, 512)
                b_fsum += b_e.sum().item() + ((n + blocks * 256 - 1) // (blocks * 256) + 8 + blocks) * U * re.abs().sum().item()
                if got_d is not None:
                    b_d = gk * f * bd + 8 * d_f32 + 8 * U * rdx.abs() + R.TINY32          # (g / (K nm): three more roundings)
                    within(got_d[sl], rdx, b_d, key + "/dlogits", d_f32)
                    assert bool((got_d[sl][~valid[sl]] == 0).all()), "rows with iou < 0: exactly 0"
                    emax, dmax = max(emax, (got_d[sl].to(F64) - rdx).abs().max().item()), max(dmax, rdx.abs().max().item())
            if got_d is not None:      # the whole-tensor tolerance as an outer check: 1e-5 of the gradient's largest element
                print("outer %s head %d: dlogits err / largest %.3g (1e-5)" % (key, k, emax / max(dmax, 1e-300)))
                assert emax <= 1e-5 * dmax
        assert note(key + "/focal_sum", abs(blk[1].item() - fsum), b_fsum + R.TINY32) <= 1.0, (blk[1].item(), fsum)
        blocks = min((rows + 255) // 256, 256)
        b_dsum = 16 * U * npos + ((rows + blocks * 256 - 1) // (blocks * 256) + 6 + 4 * blocks) * U * dl.abs().sum().item()
        assert note(key + "/diou_sum", abs(blk[2].item() - dl.sum().item()), b_dsum + R.TINY32) <= 1.0, (blk[2].item(), dl.sum().item())
        want = fsum / (K * nm) + (lam * dl.sum().item() / nm if npos > 0 else 0.0)
        b_loss = b_fsum / (K * nm) + lam * b_dsum / nm + 8 * U * (abs(fsum) / (K * nm) + lam * abs(dl.sum().item()) / nm) + R.TINY32
        assert note(key + "/loss", abs(blk[0].item() - want), b_loss) <= 1.0, (blk[0].item(), want)
        print("outer %s: loss rel %.3g, focal sum rel %.3g (2e-5)" % (key, abs(blk[0].item() - want) / max(abs(want), 1e-300),
                                                                    abs(blk[1].item() - fsum) / max(abs(fsum), 1e-300)))
        assert abs(blk[0].item() - want) <= 2e-5 * abs(want) and abs(blk[1].item() - fsum) <= 2e-5 * abs(fsum)
        assert dreg.guards_intact()
        gr = g * lam / nm
        within(dreg.v.cpu(), dd * gr, gr * 12 * U * dscale[:, None] + R.TINY32, key + "/dreg")
        assert bool((dreg.v.cpu()[~pos] == 0).all()), "non-positive rows: exactly 0"
        norm_in = nm


@pytest.mark.parametrize("gamma,alpha", [(2.0, 0.25), (0.5, -1.0), (1.0, 0.25), (3.0, -1.0)])
@pytest.mark.parametrize("heads,npos,mode", [(1, 40, ""), (3, 40, "null1"), (4, 40, "ties"), (3, 0, ""), (2, 40, "outside"), (1, 40, "ties")])
def test_det_side_loss_kernels(heads, npos, mode, gamma, alpha):
    """timhip_det_side_loss_fwd / _bwd with 1, 3 and 4 heads (C = 97, 1, 437, 13: 131 100 elements in the third, one past the
    forward cap), without a positive row, with every row outside (iou < 0), with dlogits[1] == NULL, and with the DIoU tie fixture
    among the positive rows (det_rows_kernel's copy of the tie / clamp rule); twice in a row; grad_out NULL in the one-head case."""
    rows = 300
    Cs = [97, 1, 437, 13][:heads]
    xs, ts, iou, off, reg = _side_inputs(rows, Cs, seed=heads * 10 + npos, npos=npos, all_outside=(mode == "outside"), ties=(mode == "ties"))
    _side_check(xs, ts, iou, off, reg, gamma, alpha, 1 if mode == "null1" else -1, "side/g%g" % gamma,
                null_gout=(heads == 1 and mode == ""))


def test_det_side_loss_full_size():
    """one head at the product's 6384 rows x 3806 action classes, the tie fixture among its positive rows"""
    xs, ts, iou, off, reg = _side_inputs(6384, [3806], seed=9, npos=700, ties=True, device_side=True)
    _side_check(xs, ts, iou, off, reg, 2.0, 0.25, -1, "side/full")


# =============================================================================================== DRLoc
DR_SHAPES = [(64, 50, 1024, 8), (3, 12, 64, 7), (2, 5, 4, 1)]        # m = 8: what examples/train_synthetic.py samples
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _positions(n, l, m, kind, seed):
    if kind == "random":
        return torch.randint(l, (n, m), generator=gen(seed)), torch.randint(l, (n, m), generator=gen(seed + 1))
    if kind == "equal":                # every sample of a window on one position: worst-case atomic contention
        return torch.randint(l, (n, 1), generator=gen(seed)).expand(n, m).contiguous(), torch.randint(l, (n, 1), generator=gen(seed + 1)).expand(n, m).contiguous()
    return torch.full((n, m), l - 1), torch.full((n, m), l - 1)             # "last": the final row of every window


@pytest.mark.parametrize("kind", ["random", "equal", "last"])
@pytest.mark.parametrize("layout", ["halves", "same"])
@pytest.mark.parametrize("n,l,D,m", DR_SHAPES)
def test_drloc_kernels(n, l, D, m, layout, kind):
    """drloc_gather_kernel (an exact cast of the gathered rows, all three operand types, ld = 2D and 2D + 8) and
    drloc_scatter_kernel (adds onto a pre-filled dx; each element within (its number of terms) u sum|terms|); x1 / x2 as the two
    halves of one [n, 2l, D] tensor (batch stride 2 l D) and as one and the same tensor."""
    rowsN = 2 * l if layout == "halves" else l
    feats = torch.randn(n * rowsN + 2 * 4, D, generator=gen(n + D))           # 4 guard rows on each side, one flat buffer
    o1 = 4 * D
    o2 = o1 + (l * D if layout == "halves" else 0)
    sb, sl = rowsN * D, D
    p1, p2 = _positions(n, l, m, kind, seed=m)
    fd, p1d, p2d = feats.to(DEV), p1.to(DEV), p2.to(DEV)
    keep = fd.clone()
    base = fd.view(-1)
    ref = R.drloc_gather(feats.view(-1), o1, o2, sb, sl, D, p1, p2, m)
    for prec in ("fp32", "bf16", "fp16"):
        for ld in (2 * D, 2 * D + 8):
            o = Out(n * m, ld, TDT[prec])
            L.call("timhip_drloc_gather", L.PRECISIONS[prec], base.data_ptr() + 4 * o1, base.data_ptr() + 4 * o2, sb, sl, n, l, D,
                   L.ptr(p1d), L.ptr(p2d), m, o.ptr, ld, st())
            sync()
            assert out_ok(o, 2 * D) and same_bits(fd, keep)
            assert same_bits(o.v[:, :2 * D].cpu().contiguous(), ref.to(TDT[prec])), "the gather is an exact cast"
    for ldg in (2 * D, 2 * D + 8):
        gr = torch.randn(n * m, ldg, generator=gen(ldg))
        grd = gr.to(DEV)
        grd[:, 2 * D:] = NAN
        pre = torch.randn(feats.numel(), generator=gen(3))
        dxd = pre.to(DEV)
        L.call("timhip_drloc_scatter_add", L.ptr(grd), ldg, dxd.data_ptr() + 4 * o1, dxd.data_ptr() + 4 * o2, sb, sl, n, l, D,
               L.ptr(p1d), L.ptr(p2d), m, st())
        sync()
        want, mag, cnt = R.drloc_scatter_add(gr.to(F64), pre.to(F64), o1, o2, sb, sl, D, p1, p2, m)
        got = dxd.cpu()
        within(got, want, cnt * U * (mag + pre.abs().to(F64)), "drloc/scatter")
        assert same_bits(got[cnt == 0], pre[cnt == 0]), "elements no sample points at keep their bits (guard rows included)"
        assert bool((cnt[:o1] == 0).all() and (cnt[-4 * D:] == 0).all())
        if kind != "random":
            assert cnt.max().item() >= m


# =============================================================================================== argument checks
def test_loss_entry_points_refuse_bad_arguments():
    """every TIMHIP_EINVAL / TIMHIP_EALIGN condition of the launchers returns its code and leaves the NaN-filled outputs untouched;
    rows == 0 for focal and DIoU returns OK with the loss word zeroed and nothing else written"""
    rows, Cn = 6, 12
    x = torch.randn(rows, Cn + 4, device=DEV)
    t = torch.rand(rows, Cn + 4, device=DEV)
    y = torch.randint(Cn, (rows,), device=DEV)
    u = torch.rand(rows, device=DEV)
    off = torch.rand(rows, 2, device=DEV)
    outs = [Out(rows, Cn + 4) for _ in range(3)]
    sc = Scal()

    def untouched():
        sync()
        return sc.changed() == [] and all(same_bits(o.whole, o.before) for o in outs)

    ce_f, ce_b = raw("timhip_ce_mixup_fwd"), raw("timhip_ce_mixup_bwd")
    stats = outs[0]
    for smoothing, ld in ((1.0, Cn), (-0.1, Cn), (0.2, Cn - 1)):
        assert ce_f(x.data_ptr(), rows, Cn, ld, y.data_ptr(), None, 1.0, smoothing, stats.ptr, sc.p(4), sc.p(10), st()) == EINVAL
    assert ce_f(x.data_ptr(), 0, Cn, Cn, y.data_ptr(), None, 1.0, 0.2, stats.ptr, sc.p(4), sc.p(10), st()) == EINVAL
    assert ce_f(x.data_ptr(), rows, Cn, Cn, None, None, 1.0, 0.2, stats.ptr, sc.p(4), sc.p(10), st()) == EINVAL
    for ld, ldd in ((Cn - 1, Cn), (Cn, Cn - 1)):
        assert ce_b(x.data_ptr(), rows, Cn, ld, y.data_ptr(), None, 1.0, 0.2, stats.ptr, sc.p(4), None, outs[1].ptr, ldd, st()) == EINVAL
    assert untouched()
    # focal: NULL operands, C = 0; DIoU: neither output asked for
    f_f, f_b, di = raw("timhip_focal_loss_fwd"), raw("timhip_focal_loss_bwd"), raw("timhip_diou_1d")
    assert f_f(x.data_ptr(), t.data_ptr(), rows, 0, None, None, 0.25, 2.0, sc.p(3), None, st()) == EINVAL
    assert f_f(x.data_ptr(), t.data_ptr(), rows, Cn, None, None, 0.25, 2.0, None, outs[0].ptr, st()) == EINVAL
    assert f_b(x.data_ptr(), None, rows, Cn, None, None, 0.25, 2.0, None, outs[1].ptr, st()) == EINVAL
    assert di(off.data_ptr(), off.data_ptr(), rows, None, 1e-8, None, None, None, st()) == EINVAL
    assert di(off.data_ptr(), off.data_ptr(), -1, None, 1e-8, None, sc.p(2), outs[2].ptr, st()) == EINVAL
    assert untouched()
    # side loss: 0 and 5 heads; a NULL logits[k] / targets[k] or C[k] = 0 in the last of three heads (refused before the first launch)
    s_f, s_b = raw("timhip_det_side_loss_fwd"), raw("timhip_det_side_loss_bwd")
    five = [x] * 5
    for K in (0, 5):
        assert s_f(pa(five), pa(five), ia([Cn] * 5), K, rows, u.data_ptr(), off.data_ptr(), off.data_ptr(), 0.6, 0.25, 2.0, 1e-8, 0.5,
                   0.9, sc.p(15), sc.p(4), st()) == EINVAL
        assert s_b(pa(five), pa(five), ia([Cn] * 5), K, rows, u.data_ptr(), off.data_ptr(), off.data_ptr(), 0.6, 0.25, 2.0, 1e-8, 0.5,
                   sc.p(4), None, pa([o.v for o in outs] + [outs[0].v] * 2), None, st()) == EINVAL
    three, holed = [x] * 3, pa([x, x, None])
    dl3 = pa([o.v for o in outs])
    for lg, tg, cs in ((holed, pa(three), [Cn] * 3), (pa(three), holed, [Cn] * 3), (pa(three), pa(three), [Cn, Cn, 0])):
        assert s_f(lg, tg, ia(cs), 3, rows, u.data_ptr(), off.data_ptr(), off.data_ptr(), 0.6, 0.25, 2.0, 1e-8, 0.5, 0.9, sc.p(15),
                   sc.p(4), st()) == EINVAL
        assert s_b(lg, tg, ia(cs), 3, rows, u.data_ptr(), off.data_ptr(), off.data_ptr(), 0.6, 0.25, 2.0, 1e-8, 0.5, sc.p(4), None,
                   dl3, None, st()) == EINVAL
    assert untouched()
    # DRLoc: D % 4, ld < 2D, ld % 4, strides % 4, pointers 4 bytes off a 16-byte boundary
    n, l, D, m = 2, 3, 8, 2
    f = torch.randn(n * l * D + 8, device=DEV)
    pos = torch.zeros(n, m, dtype=torch.int64, device=DEV)
    o = Out(n * m, 2 * D + 8)
    outs.append(o)
    ga, sa = raw("timhip_drloc_gather"), raw("timhip_drloc_scatter_add")
    P = L.PRECISIONS["fp32"]
    fp, pp = f.data_ptr(), pos.data_ptr()
    assert ga(P, fp, fp, l * D, D, n, l, 6, pp, pp, m, o.ptr, 2 * D, st()) == EINVAL                  # D % 4
    assert ga(P, fp, fp, l * D, D, n, l, D, pp, pp, m, o.ptr, 2 * D - 4, st()) == EINVAL              # ld < 2D
    assert ga(P, fp, fp, l * D, D, n, l, D, pp, pp, m, o.ptr, 2 * D + 2, st()) == EINVAL              # ld % 4
    assert ga(P, fp, fp, l * D + 2, D, n, l, D, pp, pp, m, o.ptr, 2 * D, st()) == EINVAL              # batch stride % 4
    assert ga(P, fp, fp, l * D, D + 2, n, l, D, pp, pp, m, o.ptr, 2 * D, st()) == EINVAL              # row stride % 4
    assert ga(P, fp + 4, fp, l * D, D, n, l, D, pp, pp, m, o.ptr, 2 * D, st()) == EALIGN
    assert ga(P, fp, fp + 4, l * D, D, n, l, D, pp, pp, m, o.ptr, 2 * D, st()) == EALIGN
    assert ga(P, fp, fp, l * D, D, n, l, D, pp, pp, m, o.ptr + 4, 2 * D, st()) == EALIGN
    assert ga(P, fp, fp, l * D, D, n, l, D, pp, pp, 0, o.ptr, 2 * D, st()) == EINVAL
    assert sa(o.ptr, 2 * D - 1, outs[0].ptr, outs[1].ptr, l * D, D, n, l, D, pp, pp, m, st()) == EINVAL   # ldg < 2D
    assert sa(o.ptr, 2 * D, None, outs[1].ptr, l * D, D, n, l, D, pp, pp, m, st()) == EINVAL
    assert untouched()
    # rows == 0: OK, the loss word zeroed, nothing else written
    assert f_f(x.data_ptr(), t.data_ptr(), 0, Cn, None, None, 0.25, 2.0, sc.p(3), outs[0].ptr, st()) == OK
    assert f_b(x.data_ptr(), t.data_ptr(), 0, Cn, None, None, 0.25, 2.0, None, outs[1].ptr, st()) == OK
    assert di(off.data_ptr(), off.data_ptr(), 0, None, 1e-8, None, sc.p(2), outs[2].ptr, st()) == OK
    sync()
    assert sc.changed() == [2, 3] and sc.get(2, 2).tolist() == [0.0, 0.0]
    assert all(same_bits(o.whole, o.before) for o in outs)
