"""The three fused-optimizer kernels (tim_amd/csrc/optim.hip) against float64 with ELEMENTWISE bounds (tests/optim_ref.py holds the
reference, the bounds with their derivation and the input families; tests/test_optim_ref.py shows on the CPU that the inputs keep
the bounds honest).  The C entry points are driven directly over TimOptItem tables and state blocks the test owns, so the STEP and
LR words, the flag words and every alignment are free.  Every case is ONE step from injected state and asserts
  * p, m, v of every item element by element within `optim_ref.bounds`, computed from the COEF the kernel wrote (itself held to
    its own limit) - the comparison measures the update's arithmetic alone;
  * NORM and COEF within their limits, STEP / SKIPPED / FOUND_INF / LR exact, BC1 and BC2_SQRT bit for bit;
  * operand copies bit-equal to the cast of the master the kernel wrote; their padding columns and two NaN guard rows on either
    side, the 8 NaN guard words on either side of every p, m, v, g and state block, and g itself, bit-identical;
  * a skipped step leaves every byte but NORM / COEF / FOUND_INF / SKIPPED as it was.
The float64 work runs on the CPU.  Largest problems: one flat item of 16,781,315 elements, one (2944, 2880) weight with copies."""
import ctypes as C
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import optim_ref as R  # noqa: E402
from tim_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
GUARD = 8                        # guard words on either side of a flat array and of a state block
NAN_BITS = {torch.float32: (torch.int32, 0x7FC00A5A), torch.float16: (torch.int16, 0x7E5A), torch.bfloat16: (torch.int16, 0x7FDA)}
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PRECS = ["fp16", "bf16", "fp32"]
OPT_GRID, OPT_TILE, OPT_MAX = 2048, 4096, 48      # optim.hip: block cap, elements per tile, items per launch
WORST = {}                       # (quantity, route) -> (largest |kernel - float64| / bound, the case it came from)


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def worst():
    yield
    for key in sorted(WORST):
        print("\nlargest |kernel - float64| / bound  %-5s %-5s %.3f  (%s)" % (key + WORST[key]))
    path = os.environ.get("TIM_OPTIM_RATIOS")      # a measurement run keeps the table
    if path:
        with open(path, "w") as f:
            json.dump({"%s %s" % k: v for k, v in sorted(WORST.items())}, f, indent=1)


def _note(what, route, r, case):
    if r > WORST.get((what, route), (-1.0, ""))[0]:
        WORST[(what, route)] = (r, case)


def _bits(t):
    return t.contiguous().view(NAN_BITS[t.dtype][0])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    _bits(t).fill_(NAN_BITS[dtype][1])
    return t


def _ru64(n):
    return (n + 63) // 64 * 64


class Item:
    """One TimOptItem over guarded device buffers.  data: fp32 CPU tensors (p, g, m, v) of rows * cols elements; offs: the start
    of p, g, m, v in words past a 16-byte boundary; copies: the operand dtype of plain [rows, ldp] / tr [cols, ldt], or None."""

    def __init__(self, shape, data, offs=(0, 0, 0, 0), copies=None, ldp=None, ldt=None):
        self.rows, self.cols = shape if len(shape) == 2 else (1, shape[0])
        self.n = self.rows * self.cols
        self.data = dict(zip("pgmv", (t.reshape(-1).float().clone() for t in data)))
        self.offs = dict(zip("pgmv", offs))
        self.whole, self.view = {}, {}
        for k in "pgmv":
            off = self.offs[k]
            w = _poison(GUARD + off + self.n + GUARD, torch.float32)
            self.whole[k], self.view[k] = w, w[GUARD + off:GUARD + off + self.n]
            self.view[k].copy_(self.data[k])
            assert self.view[k].data_ptr() % 16 == 4 * off
        self.copies = copies
        if copies is not None:
            self.ldp, self.ldt = ldp or _ru64(self.cols), ldt or _ru64(self.rows)
            self.whole["plain"] = _poison((self.rows + 4, self.ldp), copies)
            self.whole["tr"] = _poison((self.cols + 4, self.ldt), copies)

    def c_item(self):
        v = self.view
        if self.copies is None:
            return L.TimOptItem(L.ptr(v["p"]), L.ptr(v["g"]), L.ptr(v["m"]), L.ptr(v["v"]), None, None, self.rows, self.cols, 0, 0)
        return L.TimOptItem(L.ptr(v["p"]), L.ptr(v["g"]), L.ptr(v["m"]), L.ptr(v["v"]), L.ptr(self.whole["plain"][2:]),
                            L.ptr(self.whole["tr"][2:]), self.rows, self.cols, self.ldp, self.ldt)

    def expected_whole(self, k, before, new):
        """the buffer `k` as it must come back when its payload is `new`: everything else as before"""
        want = before.clone()
        if k == "plain":
            want[2:2 + self.rows, :self.cols] = new
        elif k == "tr":
            want[2:2 + self.cols, :self.rows] = new
        else:
            off = GUARD + self.offs[k]
            want[off:off + self.n] = new
        return want


class Table:
    """the items of one parameter group with its state block (guarded) and the launch arguments of its update"""
    PRESET = 123.25      # NORM, COEF, BC1, BC2_SQRT before the step: a skipped step must leave the bias corrections alone

    def __init__(self, items, step=0, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=0.01, skipped=3):
        self.items, self.step, self.betas, self.eps, self.wd, self.skipped = items, step, betas, eps, wd, skipped
        self.lr32 = R.f32(lr)
        words = torch.full((GUARD + L.OPT_STATE_WORDS + GUARD,), NAN_BITS[torch.float32][1], dtype=torch.int64)
        blk = words[GUARD:GUARD + L.OPT_STATE_WORDS]
        blk[:] = R.bits32(self.PRESET)
        blk[L.OPT_STEP], blk[L.OPT_LR], blk[L.OPT_FOUND_INF], blk[L.OPT_SKIPPED] = step, R.bits32(self.lr32), 0, skipped
        self.state_whole = words.to(torch.int32).to(DEV)
        self.state = self.state_whole[GUARD:GUARD + L.OPT_STATE_WORDS]

    def launch_table(self):
        arr = (L.TimOptItem * len(self.items))(*[it.c_item() for it in self.items])
        cnt = L.load().timhip_optim_norm_partials(C.cast(arr, C.c_void_p), len(self.items))
        assert cnt > 0, cnt
        return arr, cnt


def _parr(ptrs):
    return (C.c_void_p * max(1, len(ptrs)))(*ptrs)


def _snapshot(tables):
    return [[{k: w.clone() for k, w in it.whole.items()} for it in t.items] + [t.state_whole.clone()] for t in tables]


def _step(tables, max_norm, flags=(), prec="fp32"):
    """norm over every table, ONE finish, update per table -> the partial count of each table"""
    launch = [t.launch_table() for t in tables]
    total = sum(cnt for _, cnt in launch)
    partials = torch.full((total + 2,), float("nan"), dtype=torch.float64, device=DEV)     # (one guard on either side)
    at = 1
    for t, (arr, cnt) in zip(tables, launch):
        L.call("timhip_optim_norm", C.cast(arr, C.c_void_p), len(t.items), partials.data_ptr() + 8 * at, st())
        at += cnt
    words = [torch.tensor([f], dtype=torch.int32, device=DEV) for f in flags]
    L.call("timhip_optim_finish", partials.data_ptr() + 8, total, _parr([w.data_ptr() for w in words]), len(words), float(max_norm),
           _parr([t.state.data_ptr() for t in tables]), (C.c_double * len(tables))(*[t.betas[0] for t in tables]),
           (C.c_double * len(tables))(*[t.betas[1] for t in tables]), len(tables), st())
    for t, (arr, _) in zip(tables, launch):
        L.call("timhip_optim_update", L.PRECISIONS[prec], C.cast(arr, C.c_void_p), len(t.items), t.state.data_ptr(),
               float(t.betas[0]), float(t.betas[1]), float(t.eps), float(t.wd), st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(partials[0])) and bool(torch.isnan(partials[-1]))      # nothing written outside the `total` partials
    if not any(bool(torch.isnan(it.view["g"]).any()) for t in tables for it in t.items):
        assert not bool(torch.isnan(partials[1:-1]).any())                         # ... and every one of them written
    return [cnt for _, cnt in launch]


def _check(tables, before, max_norm, case, flags=(), route="flat", norm64=None):
    """every assertion of the module's docstring on the state the step left behind -> whether the step was applied"""
    n64 = R.norm([it.data["g"] for t in tables for it in t.items]) if norm64 is None else norm64
    applied = None
    for ti, t in enumerate(tables):
        n32, coef, bad, step1, bc1, bc2s = R.finish(n64, max_norm, flags, t.step, *t.betas)
        applied = not bad
        whole = t.state_whole.cpu()
        was = before[ti][-1].cpu()
        assert torch.equal(whole[:GUARD], was[:GUARD]) and torch.equal(whole[-GUARD:], was[-GUARD:]), (case, "state guards")
        blk = whole[GUARD:GUARD + L.OPT_STATE_WORDS]
        f = blk.view(torch.float32)
        assert int(blk[L.OPT_STEP]) == step1 and int(blk[L.OPT_FOUND_INF]) == int(bad), (case, blk.tolist())
        assert int(blk[L.OPT_SKIPPED]) == t.skipped + int(bad) and R.bits32(f[L.OPT_LR].item()) == R.bits32(t.lr32), (case, blk.tolist())
        k_norm, k_coef = f[L.OPT_NORM].item(), f[L.OPT_COEF].item()
        if math.isfinite(n32):
            r_norm = abs(k_norm - n64) / (R.NORM_LIMIT * n64) if n64 > 0 else (0.0 if k_norm == 0.0 else math.inf)
            r_coef = abs(k_coef - coef) / (R.COEF_LIMIT * coef)
            print("%s: norm %.9g (float64 %.17g, %.3f of its limit), coef %.9g (%.3f)" % (case, k_norm, n64, r_norm, k_coef, r_coef))
            _note("norm", route, r_norm, case)
            _note("coef", route, r_coef, case)
            assert r_norm <= 1.0 and r_coef <= 1.0, (case, k_norm, n64, k_coef, coef)
            if coef == 1.0:
                assert k_coef == 1.0, (case, k_coef)
        else:
            assert (math.isnan(k_norm) and math.isnan(n32)) or (k_norm == n32), (case, k_norm, n32)
        if bad:
            assert torch.equal(blk[L.OPT_BC1:], was[GUARD + L.OPT_BC1:GUARD + L.OPT_STATE_WORDS]), (case, "bias corrections moved")
            for ii, it in enumerate(t.items):
                for k, w in it.whole.items():
                    assert _same(w, before[ti][ii][k]), (case, ti, ii, k, "a skipped step wrote")
            continue
        assert (R.bits32(f[L.OPT_BC1].item()), R.bits32(f[L.OPT_BC2_SQRT].item())) == (R.bits32(bc1), R.bits32(bc2s)), \
            (case, f[L.OPT_BC1].item(), bc1, f[L.OPT_BC2_SQRT].item(), bc2s)
        for ii, it in enumerate(t.items):
            args = (it.data["p"], it.data["g"], it.data["m"], it.data["v"], k_coef, t.lr32, bc1, bc2s, t.betas[0], t.betas[1], t.eps, t.wd)
            ref, lim = R.update(*args), R.bounds(*args)
            where = (case, ti, ii, (it.rows, it.cols), tuple(it.offs.values()))
            for k, rf, lm in zip("pmv", ref, lim):
                out = it.view[k].cpu()
                r = R.ratio(out, rf, lm)
                _note(k, route, r, case)
                assert r <= 1.0, where + (k, r)
                assert _same(it.whole[k], it.expected_whole(k, before[ti][ii][k], it.view[k])), where + (k, "guard words")
            assert _same(it.whole["g"], before[ti][ii]["g"]), where + ("the gradient was written",)
            if it.copies is not None:
                cast = it.view["p"].reshape(it.rows, it.cols).to(it.copies)
                assert _same(it.whole["plain"], it.expected_whole("plain", before[ti][ii]["plain"], cast)), where + ("plain",)
                assert _same(it.whole["tr"], it.expected_whole("tr", before[ti][ii]["tr"], cast.t())), where + ("tr",)
    return applied


def _run(tables, max_norm, case, flags=(), prec="fp32", route=None, norm64=None):
    before = _snapshot(tables)
    counts = _step(tables, max_norm, flags, prec)
    applied = _check(tables, before, max_norm, case, flags, route or ("flat" if all(it.copies is None for t in tables for it in t.items) else prec),
                     norm64)
    return counts, applied, before


def _flat(n, seed, offs=(0, 0, 0, 0), family="normal"):
    return Item((n,), R.FAMILIES[family](n, seed), offs)


def _weight(shape, seed, prec, offs=(0, 0, 0, 0), family="normal", ldp=None, ldt=None):
    return Item(shape, R.FAMILIES[family](shape[0] * shape[1], seed), offs, DT[prec], ldp, ldt)


# ---------------------------------------------------------------------------------------------- 1. flat route
NUMELS = (1, 3, 4, 5, 4092, 4093, 4095, 4096, 4097, 4100, 8191, 8193)


def test_flat_route_offsets_and_tile_edges():
    """Element counts around one and two 4096-element tiles x the start offset s of p in {0, 1, 2, 3} words x three layouts: all
    four arrays at s (16-byte accesses with a shifted start), moments at other offsets, p and g at different offsets (both
    scalar).  144 items in one table: three launches, and the item walk crosses items of every kind."""
    items = []
    for n in NUMELS:
        for s in range(4):
            for offs in ((s, s, s, s), (s, s, (s + 1) % 4, (s + 2) % 4), (s, (s + 1) % 4, s, s)):
                items.append(_flat(n, 1000 + len(items), offs, "wide" if len(items) % 2 else "normal"))
    assert len(items) == 144 > 2 * OPT_MAX
    counts, applied, _ = _run([Table(items, step=4, betas=(0.9, 0.99), wd=0.05)], 1.0, "flat offsets")
    # the norm's tiles are cut in the index space shifted by g's offset: (offset + numel) elements, rounded up, every one a block
    assert applied and counts == [sum((it.offs["g"] + it.n + OPT_TILE - 1) // OPT_TILE for it in items)]


# ---------------------------------------------------------------------------------------------- 2. grid stride, flat
def test_flat_route_grid_stride():
    """A chunk of more than 2048 tiles: one item of 2 * 2048 * 4096 + 4099 elements at offset 1 (4098 tiles in the norm and in the
    update), then three small items at tiles 4098 .. 4101 - blocks 0 .. 5 take three tiles, and blocks 2 .. 5 reach the small items
    on their second stride, so the item walk advances after a stride.  A second table adds six tiles: the finish kernel sums
    2048 + 6 partials, eight or nine to a thread."""
    big = 2 * OPT_GRID * OPT_TILE + 4099
    first = [_flat(big, 1, (1, 1, 1, 1)), _flat(5, 2, (3, 3, 3, 3)), _flat(4097, 3, (0, 1, 0, 0), "wide"), _flat(1, 4)]
    second = [_flat(4097, 5), _flat(63, 6), _flat(4094, 7, (3, 3, 3, 3)), _flat(2, 8, (2, 2, 2, 2))]
    assert (1 + big + OPT_TILE - 1) // OPT_TILE == 4098
    tables = [Table(first, step=9, betas=(0.9, 0.999), wd=0.01), Table(second, step=2, lr=3e-3, betas=(0.8, 0.99), wd=0.0)]
    counts, applied, _ = _run(tables, 1.0, "flat stride")
    # first: 4098 + 1 + 2 + 1 = 4102 tiles, capped at 2048 blocks; second: 2 + 1 + 2 + 1 = 6 blocks
    assert applied and counts == [2048, 6]


# ---------------------------------------------------------------------------------------------- 3. grid stride, copies
@pytest.mark.parametrize("prec", PRECS)
def test_copy_route_grid_stride(prec):
    """A (2944, 2880) weight = 46 x 45 = 2070 tiles of 64 x 64, then (100, 52) and (7, 3) with copies in the same chunk: blocks
    0 .. 24 take a second tile through the same LDS tile, the last three of them ragged ones of other items."""
    items = [_weight((2944, 2880), 1, prec), _weight((100, 52), 2, prec, family="wide"), _weight((7, 3), 3, prec)]
    assert 46 * 45 + 2 + 1 > OPT_GRID
    counts, applied, _ = _run([Table(items, step=1, betas=(0.9, 0.999), wd=0.02)], 1.0, "copy stride " + prec, prec=prec)
    assert applied and counts == [OPT_GRID]     # (the norm pass cuts the same chunk into 2070 + 2 + 1 flat tiles: capped too)


# ---------------------------------------------------------------------------------------------- 4. copy route, ragged / scalar
RAGGED = ((1, 1), (7, 3), (63, 65), (64, 64), (65, 63), (100, 52), (52, 100), (129, 68), (8, 1028))


@pytest.mark.parametrize("prec", PRECS)
def test_copy_route_ragged_and_scalar_shapes(prec):
    """cols = 52, 68, 100, 1028: cols % 8 == 4, the last octet of a row goes scalar while the others stay 16-byte; cols = 1, 3, 63,
    65: cols % 4 != 0, scalar throughout (rows are not 16-byte aligned); a master 4 bytes past a boundary with cols % 4 == 0: scalar
    masters, 16-byte copies; pitches as the runtime allocates them (the next multiple of 64) and one pair of larger ones; a flat
    item between the weights."""
    items = [_weight(s, 10 + i, prec, family="wide" if i % 2 else "normal") for i, s in enumerate(RAGGED)]
    items.append(_weight((66, 72), 30, prec, offs=(1, 0, 0, 0)))
    items.append(_flat(4097, 31, (1, 1, 1, 1)))
    items.append(_weight((66, 72), 32, prec, offs=(0, 0, 2, 0)))
    items.append(_weight((100, 52), 33, prec, ldp=192, ldt=256))
    counts, applied, _ = _run([Table(items, step=0, betas=(0.9, 0.999), wd=0.05)], 0.5, "copy ragged " + prec, prec=prec)
    assert applied and counts == [sum((it.offs["g"] + it.n + OPT_TILE - 1) // OPT_TILE for it in items)]


# ---------------------------------------------------------------------------------------------- 5. scalars of the step
def _mixed(prec="fp16", family="normal", seed=50):
    return [_flat(4097, seed, (1, 1, 1, 1), family), _weight((65, 63), seed + 1, prec, family=family),
            _weight((100, 52), seed + 2, prec, family=family), _flat(3, seed + 3, (2, 2, 0, 0), family)]


@pytest.mark.parametrize("betas", R.BETAS, ids=lambda b: "betas%g_%g" % b)
@pytest.mark.parametrize("step", R.STEPS)
def test_bias_corrections_at_preset_steps(step, betas):
    """the STEP word preset to t - 1: BC1 = fp32(1 - beta1^t), BC2_SQRT = fp32(sqrt(1 - beta2^t)) bit for bit (float64, rounded
    once), and the update they scale within its bounds"""
    _, applied, _ = _run([Table(_mixed(), step=step, betas=betas, lr=1e-3)], 1.0, "t=%d betas=%s" % (step + 1, betas), prec="fp16")
    assert applied


def test_two_state_blocks_in_one_finish():
    """two groups with their own betas, step counts, learning rates and decays share one norm and one finish"""
    tables = [Table(_mixed("bf16", seed=60), step=999, betas=(0.9, 0.999), lr=1e-2, wd=0.05, skipped=0),
              Table(_mixed("bf16", "wide", seed=70), step=9, betas=(0.8, 0.99), lr=3e-3, wd=0.0, skipped=41)]
    _, applied, _ = _run(tables, 2.0, "two blocks", prec="bf16")
    assert applied


@pytest.mark.parametrize("what", ["lr0", "wd0", "max_norm0", "below_max_norm", "zero_grad"])
def test_degenerate_scalars(what):
    fam = {"zero_grad": "zero_grad", "below_max_norm": "small_grad"}.get(what, "normal")
    t = Table(_mixed("fp16", fam, seed=80), step=5, lr=0.0 if what == "lr0" else 1e-2, wd=0.0 if what == "wd0" else 0.05)
    _, applied, before = _run([t], 0.0 if what == "max_norm0" else 1.0, what, prec="fp16")
    assert applied
    coef = t.state.view(torch.float32)[L.OPT_COEF].item()
    if what == "lr0":     # decay = 1 - 0 * wd and step_size = 0: p does not change at all, the moments still move
        for ii, it in enumerate(t.items):
            assert _same(it.whole["p"], before[0][ii]["p"])
            assert not _same(it.whole["m"], before[0][ii]["m"]) and not _same(it.whole["v"], before[0][ii]["v"])
    if what in ("max_norm0", "below_max_norm", "zero_grad"):
        assert coef == 1.0
    if what == "zero_grad":
        assert t.state.view(torch.float32)[L.OPT_NORM].item() == 0.0
        for it in t.items:
            assert all(bool(torch.isfinite(it.view[k]).all()) for k in "pmv")


# ---------------------------------------------------------------------------------------------- 6. large / non-finite gradients
def test_huge_gradients_are_clipped_not_skipped():
    """entries of size 1e15 everywhere: g * g = 1e30 .. 2e31 stays inside fp32, the norm is finite (~1e17), coef ~1e-17, and the
    update of g * coef meets the ordinary bounds"""
    t = Table(_mixed("fp16", "huge", seed=90), step=7)
    _, applied, _ = _run([t], 1.0, "huge", prec="fp16")
    coef = t.state.view(torch.float32)[L.OPT_COEF].item()
    assert applied and 1e-18 < coef < 1e-16, coef


def test_square_overflow_counts_as_non_finite():
    """one entry of 1e20: finite, but g * g overflows fp32 inside the norm's tile sum - NORM is inf and the step is skipped
    (include/timhip.h: found_inf = the norm is inf / nan), every byte of every item as it was"""
    t = Table(_mixed("fp16", seed=100), step=7)
    it = t.items[1]
    it.data["g"][it.n // 2] = 1e20
    it.view["g"].copy_(it.data["g"])
    assert math.isfinite(R.f32(R.norm([i.data["g"] for i in t.items])))          # (the float64 norm would fit)
    _, applied, _ = _run([t], 1.0, "1e20", prec="fp16", norm64=math.inf)
    assert not applied and math.isinf(t.state.view(torch.float32)[L.OPT_NORM].item())


def test_a_non_finite_entry_anywhere_skips_every_table():
    """NaN and +inf, one at a time, at the last element of an offset-3 tensor of 4097 elements, the first element of an offset-1
    tensor, the last element of the last item of a second 48-item launch, and element (rows - 1, cols - 1) of a ragged weight
    with copies: the step is a no-op on every item of both tables.  With the plants removed the same tables take the step."""
    first = [_flat(4097, 200, (3, 3, 3, 3)), _flat(1000, 201, (1, 1, 1, 1))] + [_flat(1 + (7 * i) % 50, 202 + i) for i in range(48)]
    second = [_weight((65, 63), 300, "bf16"), _weight((100, 52), 301, "bf16"), _flat(9, 302)]
    assert OPT_MAX < len(first) <= 2 * OPT_MAX
    tables = [Table(first, step=3), Table(second, step=11, betas=(0.8, 0.99))]
    places = [(first[0], 4096), (first[1], 0), (first[-1], first[-1].n - 1), (second[0], 65 * 63 - 1)]
    for pi, (it, at) in enumerate(places):
        for bad in (math.nan, math.inf):
            it.view["g"][at] = bad
            _, applied, _ = _run(tables, 1.0, "plant %d %s" % (pi, bad), prec="bf16", norm64=bad)
            assert not applied
            it.view["g"][at] = it.data["g"][at]
            for t in tables:
                t.skipped += 1
    _, applied, _ = _run(tables, 1.0, "plants removed", prec="bf16")
    assert applied


def test_thirty_two_flag_words():
    """the finish kernel reads up to 32 external non-finite words: only the last one raised skips the step; all clear applies it"""
    t = Table(_mixed("fp32", seed=110), step=2)
    _, applied, _ = _run([t], 1.0, "flag 31 raised", flags=[0] * 31 + [1], prec="fp32")
    assert not applied
    t.skipped += 1
    _, applied, _ = _run([t], 1.0, "32 flags clear", flags=[0] * 32, prec="fp32")
    assert applied


# ---------------------------------------------------------------------------------------------- 7. through FusedAdamW
def test_fused_adamw_continues_a_loaded_state():
    """`load_state_dict` with step = 999 and given moments on two groups with different betas, then one `step()`: masters and
    moments within the bounds, the operand copies the cast of the masters, and the state_dict reports step 1000"""
    from tim_amd import functional as F
    from tim_amd.optim import FusedAdamW
    shapes = [[(65, 63), (4097,)], [(100, 52), (3,)]]
    hyper = [dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=0.05), dict(lr=3e-3, betas=(0.8, 0.99), weight_decay=0.0)]
    data = [[R.family_wide(math.prod(s), 400 + 10 * gi + i) for i, s in enumerate(grp)] for gi, grp in enumerate(shapes)]
    ps = [[d[0].reshape(s).to(DEV).requires_grad_(True) for d, s in zip(dg, grp)] for dg, grp in zip(data, shapes)]
    rt = F.Runtime("fp16")
    for grp in ps:
        for p in grp:
            if p.dim() == 2:
                rt.weight(p)
    opt = FusedAdamW([dict(params=grp, **h) for grp, h in zip(ps, hyper)], eps=1e-8, max_grad_norm=1.0, runtime=rt)
    sd = opt.state_dict()
    flat = [(d, s) for dg, grp in zip(data, shapes) for d, s in zip(dg, grp)]
    sd["state"] = {i: {"step": torch.tensor(999.0), "exp_avg": d[2].reshape(s).clone(), "exp_avg_sq": d[3].reshape(s).clone()}
                   for i, (d, s) in enumerate(flat)}
    opt.load_state_dict(sd)
    for grp, dg, sh in zip(ps, data, shapes):
        for p, d, s in zip(grp, dg, sh):
            p.grad = d[1].reshape(s).to(DEV)
    opt.step()
    torch.cuda.synchronize()
    n64 = R.norm([d[1] for d, _ in flat])
    assert abs(opt.last_grad_norm.item() - n64) <= R.NORM_LIMIT * n64
    k_coef = opt.last_clip_coef.item()
    for gi, h in enumerate(hyper):
        _, coef, bad, t, bc1, bc2s = R.finish(n64, 1.0, [], 999, *h["betas"])
        assert not bad and t == 1000 and abs(k_coef - coef) <= R.COEF_LIMIT * coef
        for p, d in zip(ps[gi], data[gi]):
            args = (d[0], d[1], d[2], d[3], k_coef, R.f32(h["lr"]), bc1, bc2s, h["betas"][0], h["betas"][1], 1e-8, h["weight_decay"])
            outs = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
            for k, out, rf, lm in zip("pmv", outs, R.update(*args), R.bounds(*args)):
                r = R.ratio(out, rf, lm)
                _note(k, "adamw", r, "FusedAdamW")
                assert r <= 1.0, (gi, tuple(p.shape), k, r)
            if p.dim() == 2:
                plain, tr = next((a, b) for q, a, b in rt.copies.pairs(p.device) if q is p)
                want = p.detach().half()
                assert torch.equal(plain[:, :p.shape[1]], want) and torch.equal(tr[:, :p.shape[0]], want.t())
    got = opt.state_dict()["state"]
    assert all(float(got[i]["step"]) == 1000.0 for i in range(len(flat)))
    assert int(opt.skipped_steps) == 0 and int(opt.found_inf) == 0
