"""Every C entry point of tim_amd/csrc/rowops.hip outside the encoder layers, called on its own (tim_amd._lib.call) and held
to its float64 restatement (tests/rowops_ref.py), at the shapes that reach every branch of the kernels.

Rules of this file:
  * outputs sit between guard rows; outputs the header documents as WRITTEN start as NaN, outputs documented as ACCUMULATED
    start as a non-zero pattern; after the call the guard rows are bit-identical, padding columns hold what the header says;
  * tolerances are derived next to the assert (u = 2^-24, the unit roundoff of fp32; a sum of n fp32 terms in any order is within
    n u sum|terms|; a 16-bit store adds half an ulp of the stored type); pure moves are bit-exact;
  * kernels without atomics are run twice and must repeat bit for bit;
  * a `scale` / `out_scale` argument is a pointer into the 8-word block timhip_grad_scale lays out ({S, 1/S, scratch, scratch,
    non-finite flag, ...}): `scale` arguments point at word 0, `out_scale` arguments at word 1 (the kernels OR the flag into the
    third word after it).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rowops_ref as R  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.functional import EncoderPlan  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
U = R.EPS32
PRECS = ["fp32", "bf16", "fp16"]
DT = {"fp32": torch.float32, "bf16x3": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
G = 4   # guard rows on either side of an output


def st():
    return torch.cuda.current_stream().cuda_stream


def sync():
    torch.cuda.synchronize()


def ia(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def pa(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def rn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Out:
    """an output buffer [rows, ld] between G guard rows; fill: "nan" (the entry point writes it) or "acc" (it accumulates)"""

    def __init__(self, rows, ld, dtype=torch.float32, fill="nan"):
        self.whole = torch.empty((rows + 2 * G, ld), dtype=dtype, device=DEV)
        if fill == "nan":
            self.whole.fill_(float("nan"))
        else:   # multiples of 1/8 between -0.75 and 0.875, never 0: exact in every storage type
            n = self.whole.numel()
            pat = ((torch.arange(n, device=DEV) % 13) - 6).float() * 0.125
            self.whole.copy_(torch.where(pat == 0, torch.full_like(pat, 0.875), pat).view(self.whole.shape).to(dtype))
        self.before = self.whole.clone()
        self.v = self.whole[G:G + rows]
        self.rows = rows

    @property
    def ptr(self):
        return self.v.data_ptr()

    @property
    def pre(self):
        return self.before[G:G + self.rows]

    def guards_intact(self):
        return same_bits(self.whole[:G], self.before[:G]) and same_bits(self.whole[G + self.rows:], self.before[G + self.rows:])


def scale_block(word, value):
    """the 8 words of a timhip_grad_scale block, all zero but `word`"""
    blk = torch.zeros(8, device=DEV)
    blk[word] = value
    return blk


def table_dev(table):
    return torch.tensor(table, dtype=torch.int32).reshape(-1, 4).to(DEV)


# =============================================================================================== time MLP, layer 1
def _l1_inputs(rows, d, seed):
    times = (torch.rand(rows, 2, generator=torch.Generator().manual_seed(seed)) * 2 - 1)
    times[0] = 0.0                                     # a zero time: h = relu(b)
    w, b = rn(d, 2, seed=seed + 1), rn(d, seed=seed + 2)
    if rows > 1:                                       # the relu edge: pre-activations exactly 0, one ulp above, one ulp below
        times[1, 0], times[1, 1] = 1.0, 0.0
        w[0, 0] = w[1, 0] = w[2, 0] = 0.5
        b[0] = -0.5
        b[1] = torch.nextafter(torch.tensor(-0.5), torch.tensor(0.0))
        b[2] = torch.nextafter(torch.tensor(-0.5), torch.tensor(-1.0))
    return times, w, b


L1_ROWS = [1, 3, 511, 512, 515, 4096 + 5]      # one row per block, four, sixteen; each with a ragged last block
L1_SHAPES = [(32, 64), (72, 96), (512, 512), (1000, 1024), (1100, 1152), (30, 30), (513, 513)]


@pytest.mark.parametrize("prec", PRECS + ["bf16x3"])
@pytest.mark.parametrize("d,ld", L1_SHAPES)
def test_time_l1_fwd(prec, d, ld):
    """vector form with up to 256 column quads (several row lanes; 24 quads leave 16 threads idle), with more than 256 quads
    (a thread walks columns), element form (ld % 4 != 0)"""
    T = DT[prec]
    for rows in L1_ROWS:
        times, w, b = _l1_inputs(rows, d, seed=rows)
        td, wd, bd = times.to(DEV), w.to(DEV), b.to(DEV)
        keep = [t.clone() for t in (td, wd, bd)]
        outs = []
        for _ in range(2):
            o = Out(rows, ld, T)
            L.call("timhip_time_l1_fwd", L.PRECISIONS[prec], L.ptr(td), rows, d, L.ptr(wd), L.ptr(bd), o.ptr, ld, st())
            outs.append(o)
        sync()
        o = outs[0]
        assert o.guards_intact() and same_bits(o.v, outs[1].v)
        assert all(same_bits(a, k) for a, k in zip((td, wd, bd), keep))
        got = o.v.cpu().to(F64)
        assert bool((got[:, d:] == 0).all())                                    # padding columns: zero
        ref = R.time_l1(times.to(F64), w.to(F64), b.to(F64))
        # two fused multiply-adds, each rounding once a value below sum|terms|: 2 u sum|terms|; relu does not grow a difference
        e32 = 2 * U * R.time_l1_abs_terms(times.to(F64), w.to(F64), b.to(F64))
        lim = e32 * (1 + R.HALF_ULP[T]) + R.store_bound(ref, T)
        assert bool(((got[:, :d] - ref).abs() <= lim).all()), (rows, ((got[:, :d] - ref).abs() - lim).max().item())
        if rows > 1:
            assert got[1, 0] == 0 and got[1, 2] == 0 and got[1, 1] >= 0


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("d,ld", [(32, 64), (72, 128), (512, 512), (1000, 1024), (1100, 1152)])
def test_time_l1_fwd_split3(prec, d, ld):
    """[hi | lo | hi] blocks of width ld: T(v), T(v - hi), T(v) of the fp32 value v the plain entry point writes, bit for bit"""
    T = DT[prec]
    for rows in L1_ROWS:
        times, w, b = _l1_inputs(rows, d, seed=rows)
        td, wd, bd = times.to(DEV), w.to(DEV), b.to(DEV)
        v = Out(rows, ld, torch.float32)
        L.call("timhip_time_l1_fwd", L.PREC_FP32, L.ptr(td), rows, d, L.ptr(wd), L.ptr(bd), v.ptr, ld, st())
        outs = []
        for _ in range(2):
            o = Out(rows, 3 * ld, T)
            L.call("timhip_time_l1_fwd_split3", L.PRECISIONS[prec], L.ptr(td), rows, d, L.ptr(wd), L.ptr(bd), o.ptr, ld, st())
            outs.append(o)
        sync()
        o = outs[0]
        assert o.guards_intact() and same_bits(o.v, outs[1].v)
        hi, lo = R.split3(v.v, T)
        assert bool((v.v[:, d:] == 0).all())
        assert same_bits(o.v[:, :ld], hi) and same_bits(o.v[:, ld:2 * ld], lo) and same_bits(o.v[:, 2 * ld:], hi), rows
        for blk in range(3):
            assert bool((o.v[:, blk * ld + d:(blk + 1) * ld] == 0).all())
    # refused on the host: an fp32 precision, a block width that is not a multiple of 64 (rowops.hip, timhip_time_l1_fwd_split3: first line)
    lib = L.load()
    assert lib.timhip_time_l1_fwd_split3(L.PREC_FP32, L.ptr(td), rows, d, L.ptr(wd), L.ptr(bd), o.ptr, ld, st()) != 0
    assert lib.timhip_time_l1_fwd_split3(L.PRECISIONS[prec], L.ptr(td), rows, d, L.ptr(wd), L.ptr(bd), o.ptr, ld + 32, st()) != 0


def _l1_bwd_case(prec, rows, d, ld, with_dt, with_scale, poison=False):
    T = DT[prec]
    times = torch.rand(rows, 2, generator=torch.Generator().manual_seed(rows + d)) * 2 - 1
    w = rn(d, 2, seed=d)
    dh = torch.zeros(rows, ld).to(T)
    g = rn(rows, d, seed=rows)
    g = g * (rn(rows, d, seed=rows + 1) > -0.3)          # the relu mask, folded in as the contract says
    dh[:, :d] = g.to(T)
    if poison:
        dh[rows // 2, d // 2] = float("inf")
    td, wd, dhd = times.to(DEV), w.to(DEV), dh.to(DEV)
    keep = [t.clone() for t in (td, wd, dhd)]
    dw, db = Out(d, 2, fill="acc"), Out(1, d, fill="acc")
    dt = Out(rows, 2) if with_dt else None
    osv = 2.0 ** -7 if with_scale else 1.0
    blk = scale_block(1, osv) if with_scale else None
    L.call("timhip_time_l1_bwd", L.PRECISIONS[prec], L.ptr(td), rows, d, L.ptr(wd), L.ptr(dhd), ld, dw.ptr, db.ptr,
           dt.ptr if dt else None, blk.data_ptr() + 4 if with_scale else None, st())
    sync()
    assert dw.guards_intact() and db.guards_intact() and (dt is None or dt.guards_intact())
    assert all(same_bits(a, k) for a, k in zip((td, wd, dhd), keep))
    if with_scale:     # {0, 1/S, 0, 0, flag, 0, 0, 0}: the flag word is the only one a call may change
        want = scale_block(1, osv)
        if poison:
            want.view(torch.int32)[4] = 1
        assert same_bits(blk, want)
    if poison:
        return
    g64 = dh[:, :d].to(F64)                                # the stored operand is the input
    rdw, rdb, rdt = R.time_l1_bwd(times.to(F64), w.to(F64), g64)
    adw, adb, adt = R.time_l1_bwd(times.to(F64).abs(), w.to(F64).abs(), g64.abs())
    nblk = (rows + 31) // 32
    # dw / db: `rows` products summed in fp32 in some order, times os (exact: a power of two), added by one atomic per block onto
    # the pre-filled value: (rows + nblk + 2) u (|pre| + os sum|terms|)
    for got, pre, ref, ab in ((dw.v, dw.pre, rdw, adw), (db.v.view(-1), db.pre.view(-1), rdb, adb)):
        want = pre.cpu().to(F64) + osv * ref
        lim = (rows + nblk + 2) * U * (pre.cpu().to(F64).abs() + osv * ab)
        err = (got.cpu().to(F64) - want).abs()
        assert bool((err <= lim).all()), (rows, d, ld, (err - lim).max().item())
    if dt:
        # dt: d products per row, lane sums then a wave reduction, times os: (d + 8) u os sum|terms|
        err = (dt.v.cpu().to(F64) - osv * rdt).abs()
        assert bool((err <= (d + 8) * U * osv * adt).all()), (rows, d, ld, err.max().item())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("d", [32, 256, 260, 512, 516, 1024, 1028, 30])
def test_time_l1_bwd(prec, d):
    """four row lanes (d <= 256), two (d <= 512), one; the element form (d % 4 != 0, or a row pitch that is not a multiple of 4);
    32 rows per block below 2048 rows, 128 from there on, ragged last blocks; dw / db are added to, dt is written, everything
    written carries the out_scale factor"""
    for rows in (1, 31, 33, 2047, 2048 + 7):
        for ld in ((d, d + 4) if d % 4 == 0 else (d, d + 2)):
            _l1_bwd_case(prec, rows, d, ld, True, True)
            _l1_bwd_case(prec, rows, d, ld, False, False)
    if d == 32:
        _l1_bwd_case(prec, 33, d, d + 2, True, True)      # d % 4 == 0 with an odd pitch: element form
        _l1_bwd_case(prec, 33, d, d, True, False)
        _l1_bwd_case(prec, 33, d, d, False, True)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [32, 30])
def test_time_l1_bwd_non_finite_flag(prec, d):
    """an inf in dh reaches dw / db: the kernel ORs 1 into the flag word of the scale block and changes nothing else in it"""
    _l1_bwd_case(prec, 40, d, d, True, True, poison=True)


# =============================================================================================== sequence assembly
def _asm_inputs(table, B, d, n_e, T, ncls, nmod, seed=0):
    e0, e1, te = rn(B, n_e, d, seed=seed), rn(B, n_e, d, seed=seed + 1), rn(B, T, d, seed=seed + 2)
    cls, mod = rn(max(ncls, 1), d, seed=seed + 3), rn(max(nmod, 1), 2 * d, seed=seed + 4)
    return e0, e1, te, cls, mod


def _asm_fwd(prec, table, B, d, n_e, T, ncls, nmod, form="p", p=0.0, seed=0, site=L.SITE_SEQ):
    """-> (x fp32 [B,S,2d] Out, x_T Out, inputs on the CPU)"""
    S, E, Tt = len(table), 2 * d, DT[prec]
    ins = _asm_inputs(table, B, d, n_e, T, ncls, nmod)
    e0, e1, te, cls, mod = [t.to(DEV) for t in ins]
    keep = [t.clone() for t in (e0, e1, te, cls, mod)]
    tab = table_dev(table)
    x, xt = Out(B * S, E), Out(B * S, E, Tt)
    if form == "p":
        L.call("timhip_assemble_fwd_p", L.PRECISIONS[prec], L.ptr(tab), B, S, d, L.ptr(e0), L.ptr(e1), n_e,
               pa([cls[i] for i in range(ncls)]), ncls, L.ptr(te), T, pa([mod[i] for i in range(nmod)]), nmod, p, seed, site,
               x.ptr, xt.ptr, st())
    else:
        L.call("timhip_assemble_fwd", L.PRECISIONS[prec], L.ptr(tab), B, S, d, L.ptr(e0), L.ptr(e1), n_e, L.ptr(cls), L.ptr(te), T,
               L.ptr(mod), p, seed, site, x.ptr, xt.ptr, st())
    sync()
    assert x.guards_intact() and xt.guards_intact()
    assert all(same_bits(a, k) for a, k in zip((e0, e1, te, cls, mod), keep))
    return x, xt, ins


def _check_asm_fwd(prec, table, B, d, n_e, T, ncls, nmod):
    S, E = len(table), 2 * d
    x, xt, (e0, e1, te, cls, mod) = _asm_fwd(prec, table, B, d, n_e, T, ncls, nmod, "p")
    x2, xt2, _ = _asm_fwd(prec, table, B, d, n_e, T, ncls, nmod, "c")
    assert same_bits(x.v, x2.v) and same_bits(xt.v, xt2.v)           # by pointer == contiguous; also: repeats bit for bit
    ref = R.assemble(table, B, d, e0.to(F64), e1.to(F64), [c.to(F64) for c in cls], te.to(F64), [m.to(F64) for m in mod])
    got = x.v.view(B, S, E).cpu().to(F64)
    # a move and at most ONE fp32 addition (the modality vector): half an ulp of the sum; rows without one are exact
    assert bool(((got - ref).abs() <= U * ref.abs()).all())
    nomod = torch.tensor([r[3] < 0 for r in table])
    assert torch.equal(got[:, nomod], ref[:, nomod])
    assert same_bits(xt.v, x.v.to(DT[prec]))                            # the operand copy is the rounded fp32 row


def _asm_bwd(table, B, d, n_e, T, ncls, nmod, form="p", p=0.0, seed=0, want=("e0", "e1", "te"), null_cls=(), null_mod=(),
             dx=None):
    S, E = len(table), 2 * d
    dx = rn(B, S, E, seed=7) if dx is None else dx
    dxd = dx.to(DEV)
    keep = dxd.clone()
    tab = table_dev(table)
    o = {"e0": Out(B * n_e, d) if "e0" in want else None, "e1": Out(B * n_e, d) if "e1" in want else None,
         "te": Out(B * T, d) if "te" in want else None,        # WRITTEN (include/timhip.h): starts as NaN
         "cls": Out(max(ncls, 1), d, fill="acc"), "mod": Out(max(nmod, 1), 2 * d, fill="acc")}
    optr = lambda k: o[k].ptr if o[k] is not None else None
    if form == "p":
        L.call("timhip_assemble_bwd_p", L.ptr(tab), B, S, d, L.ptr(dxd), n_e, T, p, seed, L.SITE_SEQ, optr("e0"), optr("e1"),
               pa([None if i in null_cls else o["cls"].v[i] for i in range(ncls)]), ncls, optr("te"),
               pa([None if i in null_mod else o["mod"].v[i] for i in range(nmod)]), nmod, st())
    else:
        L.call("timhip_assemble_bwd", L.ptr(tab), B, S, d, L.ptr(dxd), n_e, T, p, seed, L.SITE_SEQ, optr("e0"), optr("e1"),
               o["cls"].ptr, optr("te"), o["mod"].ptr, st())
    sync()
    assert all(v.guards_intact() for v in o.values() if v is not None)
    assert same_bits(dxd, keep)
    return o, dx


def _check_asm_bwd(table, B, d, n_e, T, ncls, nmod, form="p", want=("e0", "e1", "te"), null_cls=(), null_mod=(), dx=None,
                   p=0.0, seed=0, ref_dx=None):
    o, dx = _asm_bwd(table, B, d, n_e, T, ncls, nmod, form, p=p, seed=seed, want=want, null_cls=null_cls, null_mod=null_mod, dx=dx)
    dxr = (dx if ref_dx is None else ref_dx).to(F64)
    g = R.assemble_bwd(table, B, d, dxr, n_e, T, ncls, nmod)
    a, n_cls, n_mod, n_te = R.assemble_abs(table, B, d, dxr, T, ncls, nmod)
    exact = p == 0.0
    # d_e0 / d_e1: a move.  Rows the table names are the dx rows bit for bit, the others are not touched
    for k, kind in (("e0", 0), ("e1", 2)):
        if o[k] is None:
            continue
        got = o[k].v.view(B, n_e, d)
        wrote = g["wrote%d" % (0 if kind == 0 else 1)]
        if exact:
            assert torch.equal(got[:, wrote].cpu().to(F64), g["d_" + k][:, wrote])
        else:
            assert bool(((got[:, wrote].cpu().to(F64) - g["d_" + k][:, wrote]).abs() <= U * g["d_" + k][:, wrote].abs()).all())
        assert same_bits(got[:, ~wrote], o[k].pre.view(B, n_e, d)[:, ~wrote])
    # d_te: WRITTEN - the fixed-order sum over the token rows that read the time row, zero for a time row nobody reads
    if o["te"] is not None:
        got = o["te"].v.view(B, T, d).cpu().to(F64)
        assert bool(torch.isfinite(got).all())
        nt = torch.tensor(n_te, dtype=F64).view(1, T, 1)
        assert bool(((got - g["d_te"]).abs() <= (nt + (0 if exact else 1)) * U * a["d_te"]).all())      # n terms: n u sum|terms|
        assert bool((got[:, nt.view(-1) == 0] == 0).all())
    # d_cls / d_mod: ACCUMULATED - B * (rows of the vector) terms summed in fp32 (window lanes, carried sums, one atomic per block and
    # column onto the pre-filled value): (n + blocks + 2) u (|pre| + sum|terms|), blocks <= S
    S = len(table)
    for k, n_k, nul in (("cls", n_cls, null_cls), ("mod", n_mod, null_mod)):
        for i in range(len(n_k)):
            pre = o[k].pre[i].cpu().to(F64)
            got = o[k].v[i].cpu().to(F64)
            if i in nul:
                assert torch.equal(got, pre)
                continue
            want = pre + g["d_" + k][i]
            lim = (n_k[i] + S + 2 + (0 if exact else n_k[i])) * U * (pre.abs() + a["d_" + k][i])
            assert bool(((got - want).abs() <= lim).all()), (k, i, ((got - want).abs() - lim).max().item())
    return o


def _plan_table(name, nv, na):
    cfg = named_config(name)
    nf = cfg.num_feats
    T = (2 * nf if cfg.input_modality == "audio_visual" else nf) + nv + na
    plan = EncoderPlan(cfg, T, nv, na)
    return [tuple(r) for r in plan.rows], nf, T, len(plan.cls_names), len(plan.mod_names)


def _synthetic_table(S):
    """16 + 16 feature rows of two embedders, then cls rows whose cls / modality target alternates every row, changes at odd and at
    even rows (inside a block's rows and at a block boundary for every rows-per-block), with and without a modality vector; cls
    indices up to 5; time rows 32 .. 38 are read by about 30 token rows each, time row 39 by nobody"""
    t = [(0, s, s, 0) for s in range(16)] + [(2, s, 16 + s, 1) for s in range(16)]
    for s in range(32, S):
        if s < 100:
            cls, mod = s % 2, s % 3 - 1
        elif s < 131:
            cls, mod = 2, 1
        elif s < 162:
            cls, mod = 5, -1
        elif s < 200:
            cls, mod = 3, 0
        else:
            cls, mod = 4, (1 if s < 229 else 2)
        t.append((1, cls, 32 + s % 7, mod))
    return t, 16, 40, 6, 3


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,nv,na,B,d", [("C2a", 10, 5, 3, 32), ("C1", 8, 0, 3, 32), ("C4", 399, 0, 2, 32), ("C4", 399, 0, 2, 512),
                                            ("C2a", 10, 5, 2, 512)])
def test_assemble_fwd_plan_tables(prec, name, nv, na, B, d):
    table, n_e, T, ncls, nmod = _plan_table(name, nv, na)
    _check_asm_fwd(prec, table, B, d, n_e, T, ncls, nmod)


@pytest.mark.parametrize("S", [255, 257])
def test_assemble_fwd_synthetic_table(S):
    table, n_e, T, ncls, nmod = _synthetic_table(S)
    _check_asm_fwd("fp16", table, 3, 32, n_e, T, ncls, nmod)


def test_assemble_fwd_p_refuses_a_null_vector():
    """timhip_assemble_fwd_p checks its pointer tables on the host before the launch (rowops.hip: the two loops over cls[i] / mod[i]
    in front of assemble_fwd_launch): a NULL or misaligned entry is TIMHIP_EALIGN"""
    table, n_e, T, ncls, nmod = _plan_table("C2a", 10, 5)
    B, d, S = 2, 32, len(table)
    e0, e1, te, cls, mod = [t.to(DEV) for t in _asm_inputs(table, B, d, n_e, T, ncls, nmod)]
    x, xt = Out(B * S, 2 * d), Out(B * S, 2 * d)
    for bad_cls, bad_mod in ((0, None), (None, 1)):
        cl = [None if i == bad_cls else cls[i] for i in range(ncls)]
        mo = [None if i == bad_mod else mod[i] for i in range(nmod)]
        rc = L.load().timhip_assemble_fwd_p(L.PREC_FP32, L.ptr(table_dev(table)), B, S, d, L.ptr(e0), L.ptr(e1), n_e, pa(cl), ncls,
                                            L.ptr(te), T, pa(mo), nmod, 0.0, 0, L.SITE_SEQ, x.ptr, xt.ptr, st())
        assert rc != 0
    sync()
    assert same_bits(x.whole, x.before) and same_bits(xt.whole, xt.before)


@pytest.mark.parametrize("form", ["p", "c"])
@pytest.mark.parametrize("name,nv,na,B,d", [("C2a", 10, 5, 3, 32), ("C1", 8, 0, 3, 32), ("C4", 399, 0, 2, 32), ("C4", 399, 0, 3, 512),
                                            ("C2a", 10, 5, 5, 512)])
def test_assemble_bwd_plan_tables(form, name, nv, na, B, d):
    """the tables the host builds; C4 at its real size: 399 query rows that share one cls vector and one modality vector, four
    token rows per block - the carried sums and their flushes, elementwise"""
    table, n_e, T, ncls, nmod = _plan_table(name, nv, na)
    want = ("e0", "e1", "te") if nmod else ("e0", "te")       # one embedder: d_e1 = NULL
    _check_asm_bwd(table, B, d, n_e, T, ncls, nmod, form, want=want)


@pytest.mark.parametrize("S", [255, 256, 257])
@pytest.mark.parametrize("B", [1, 3])
def test_assemble_bwd_synthetic_table(S, B):
    """one, two and three token rows per block; targets that change inside a block, at a block boundary and every row; rows without
    a modality vector; a NULL entry in a pointer table (that gradient is not wanted: skipped, the others unaffected)"""
    table, n_e, T, ncls, nmod = _synthetic_table(S)
    _check_asm_bwd(table, B, 32, n_e, T, ncls, nmod, "p")
    _check_asm_bwd(table, B, 32, n_e, T, ncls, nmod, "c")
    if B == 3:
        _check_asm_bwd(table, B, 32, n_e, T, ncls, nmod, "p", null_cls=(2,), null_mod=(0,))
        _check_asm_bwd(table, B, 32, n_e, T, ncls, nmod, "p", want=("e0",))          # d_e1 = NULL, d_te = NULL


@pytest.mark.parametrize("B", [1, 3, 5, 8, 32, 37])
def test_assemble_bwd_window_shares(B):
    """the four window lanes of the first kernel with 1 .. 37 windows; the 1 / 4 / 16 window shares of the d_te kernel (B < 8, < 32,
    from 32 on) with a ragged last share"""
    table, n_e, T, ncls, nmod = _plan_table("C2a", 10, 5)
    _check_asm_bwd(table, B, 32, n_e, T, ncls, nmod, "p")


@pytest.mark.parametrize("B", [2, 9])
def test_assemble_bwd_time_rows_with_many_readers(B):
    """d_te: the reader list at its limit (8 token rows read one time row) and the form behind it (9 and 20 readers: every table
    row is tested again); a time row nobody reads comes out zero"""
    table = [(0, s, s, -1) for s in range(3)] + [(1, 0, 3, -1)] * 8 + [(1, 1, 4, 0)] * 9 + [(1, 0, 5, -1)] * 20
    o = _check_asm_bwd(table, B, 32, 3, 7, 2, 1, "p", want=("e0", "te"))
    assert bool((o["te"].v.view(B, 7, 32)[:, 6] == 0).all())
    # interleaved readers: the fallback walks the whole table
    table2 = [(0, s, s, -1) for s in range(3)] + [(1, s % 2, 3 + s % 2, -1) for s in range(40)]
    _check_asm_bwd(table2, B, 64, 3, 6, 2, 0, "p", want=("e0", "te"))


def test_assemble_bwd_uses_the_forwards_mask():
    """p > 0: bwd(dx) == ref_bwd(dx * mask / (1 - p)) with the mask timhip_dropout_mask returns for (seed, SITE_SEQ) - the one the
    forward applied"""
    table, n_e, T, ncls, nmod = _plan_table("C2a", 10, 5)
    B, d, S, p, seed = 3, 32, len(table), 0.25, 4242
    mk = torch.empty((B * S, 2 * d), dtype=torch.uint8, device=DEV)
    L.call("timhip_dropout_mask", seed, L.SITE_SEQ, p, B * S, 2 * d, L.ptr(mk), st())
    x0, _, ins = _asm_fwd("fp32", table, B, d, n_e, T, ncls, nmod, "p", p=0.0)
    x1, _, _ = _asm_fwd("fp32", table, B, d, n_e, T, ncls, nmod, "p", p=p, seed=seed)
    sync()
    keep = mk.cpu().to(F64)
    assert 0.7 < keep.mean().item() < 0.8
    f = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32).item()
    assert bool(((x1.v.cpu().to(F64) - x0.v.cpu().to(F64) * keep * f).abs() <= U * x0.v.cpu().to(F64).abs() * f).all())
    dx = rn(B, S, 2 * d, seed=7)
    # exact product (the kernel multiplies by the same fp32 factor), so the error bounds of the p = 0 case hold with one more rounding
    _check_asm_bwd(table, B, d, n_e, T, ncls, nmod, "p", dx=dx, p=p, seed=seed, ref_dx=dx.to(F64) * keep.view(B, S, 2 * d) * f)


# =============================================================================================== row moves
RANGE_SETS = [[(9, 1)], [(9, 2), (11, 3)], [(18, 5), (9, 2), (12, 1)], [(9, 1), (10, 1), (11, 1), (13, 2), (16, 3), (20, 3)]]
#               one row    adjacent          out of order, ends at S     six ranges, rows 12, 15, 19 belong to nobody (S = 23)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", [64, 1024])
def test_gather_and_scatter_ranges(prec, B, E):
    S, T = 23, DT[prec]
    x = rn(B, S, E, seed=E + B).to(T)
    xd = x.to(DEV)
    stream = rn(B, S, E, seed=1)
    for ranges in RANGE_SETS:
        s0, n = [r[0] for r in ranges], [r[1] for r in ranges]
        outs = [Out(B * k, E, T) for k in n]
        L.call("timhip_gather_ranges", L.PRECISIONS[prec], L.ptr(xd), B, S, E, len(ranges), ia(s0), ia(n), pa([o.v for o in outs]), st())
        singles = [Out(B * k, E, T) for k in n]
        for (a, k), o in zip(ranges, singles):
            L.call("timhip_gather_rows", L.PRECISIONS[prec], L.ptr(xd), B, S, E, a, k, o.ptr, st())
        sync()
        for o, o1, want in zip(outs, singles, R.gather_ranges(x, ranges)):
            assert o.guards_intact() and o1.guards_intact()
            assert same_bits(o.v.cpu(), want) and same_bits(o1.v.cpu(), want)
        assert same_bits(xd.cpu(), x)
        if prec != "fp32":
            continue
        # scatter-add (fp32): onto a pre-filled stream; rows of no range stay bit-identical; one addition per element: exact
        # against the same fp32 addition on the host
        rows = [rn(B * k, E, seed=3 + i) for i, k in enumerate(n)]
        rows_d = [r.to(DEV) for r in rows]
        want = R.scatter_ranges_add(stream, ranges, rows)
        dx, dx1 = Out(B * S, E), Out(B * S, E)
        for o in (dx, dx1):
            o.v.copy_(stream.view(B * S, E))
        L.call("timhip_scatter_ranges_add", B, S, E, len(ranges), ia(s0), ia(n), pa(rows_d), dx.ptr, st())
        for (a, k), r in zip(ranges, rows_d):
            L.call("timhip_scatter_rows_add", L.ptr(r), B, S, E, a, k, dx1.ptr, st())
        sync()
        assert dx.guards_intact() and dx1.guards_intact()
        assert same_bits(dx.v.cpu(), want.view(B * S, E)) and same_bits(dx1.v.cpu(), want.view(B * S, E))
        covered = torch.zeros(S, dtype=torch.bool)
        for a, k in ranges:
            covered[a:a + k] = True
        assert same_bits(dx.v.view(B, S, E)[:, ~covered].cpu(), stream[:, ~covered])
        # gather, then scatter-add onto zeros: the identity on the covered rows
        z = Out(B * S, E)
        z.v.zero_()
        L.call("timhip_scatter_ranges_add", B, S, E, len(ranges), ia(s0), ia(n), pa([o.v for o in outs]), z.ptr, st())
        sync()
        back = z.v.view(B, S, E).cpu()
        assert torch.equal(back[:, covered], x[:, covered]) and bool((back[:, ~covered] == 0).all())


@pytest.mark.parametrize("prec", PRECS)
def test_gather_rows_narrow(prec):
    """E % 4 != 0: the element-wise form ([rows, 2] LayerNorm statistics of the evaluation tail; an odd width)"""
    T = DT[prec]
    for E in (2, 7):
        B, S = 3, 19
        x = rn(B, S, E, seed=E).to(T)
        o = Out(B * 5, E, T)
        L.call("timhip_gather_rows", L.PRECISIONS[prec], L.ptr(x.to(DEV)), B, S, E, 14, 5, o.ptr, st())
        sync()
        assert o.guards_intact() and same_bits(o.v.cpu(), x[:, 14:19].reshape(B * 5, E))


ONE_RANGE = [(0, 1), (4, 3), (6, 1)]   # of S = 7 token rows: the first row, a range that ends at S, the last row alone


@pytest.mark.parametrize("prec", PRECS)
def test_gather_single_entry_is_the_one_range_entry(prec):
    """timhip_gather_rows and timhip_gather_ranges with one range are one kernel: both equal x[b, s0:s0+n] bit for bit (a copy: no
    tolerance); E = 260 walks a second column step with a ragged end; E % 4 != 0 is the single entry's alone"""
    B, S, T = 2, 7, DT[prec]
    for E in (4, 8, 260) + ((2, 6) if prec == "fp32" else ()):
        x = rn(B, S, E, seed=E).to(T)
        xd = x.to(DEV)
        for s0, n in ONE_RANGE:
            want = x[:, s0:s0 + n].reshape(B * n, E)
            o1 = Out(B * n, E, T)
            L.call("timhip_gather_rows", L.PRECISIONS[prec], L.ptr(xd), B, S, E, s0, n, o1.ptr, st())
            o = Out(B * n, E, T)
            rc = L.load().timhip_gather_ranges(L.PRECISIONS[prec], L.ptr(xd), B, S, E, 1, ia([s0]), ia([n]), pa([o.v]), st())
            sync()
            assert o1.guards_intact() and same_bits(o1.v.cpu(), want), (E, s0, n)
            if E % 4:
                assert rc == -1 and same_bits(o.whole, o.before)      # TIMHIP_EINVAL, nothing written
            else:
                assert rc == 0 and o.guards_intact() and same_bits(o.v.cpu(), want), (E, s0, n)
        assert same_bits(xd.cpu(), x)


def test_scatter_single_entry_is_the_one_range_entry():
    """timhip_scatter_rows_add and timhip_scatter_ranges_add with one range: one fp32 addition per element of the range onto a
    pre-filled stream, equal to the same addition on the host and to each other bit for bit; every other row bit-unchanged"""
    B, S = 2, 7
    for E in (4, 260):
        for s0, n in ONE_RANGE:
            rows = rn(B * n, E, seed=E + s0)
            rows_d = rows.to(DEV)
            dx1, dx = Out(B * S, E, fill="acc"), Out(B * S, E, fill="acc")
            want = dx.pre.cpu().view(B, S, E).clone()
            want[:, s0:s0 + n] += rows.view(B, n, E)
            L.call("timhip_scatter_rows_add", L.ptr(rows_d), B, S, E, s0, n, dx1.ptr, st())
            L.call("timhip_scatter_ranges_add", B, S, E, 1, ia([s0]), ia([n]), pa([rows_d]), dx.ptr, st())
            sync()
            assert dx1.guards_intact() and dx.guards_intact()
            assert same_bits(dx1.v, dx.v) and same_bits(dx.v.cpu(), want.view(B * S, E)), (E, s0, n)
            outside = [s for s in range(S) if not s0 <= s < s0 + n]
            assert same_bits(dx.v.view(B, S, E)[:, outside], dx.pre.view(B, S, E)[:, outside])
            assert same_bits(rows_d.cpu(), rows)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("E", [64, 1024])
def test_gather_split3_ranges(prec, B, E):
    S, T = 23, DT[prec]
    x = rn(B, S, E, seed=E) * torch.exp2(torch.arange(E) % 9 - 4.0)
    xd = x.to(DEV)
    for ranges in RANGE_SETS:
        s0, n = [r[0] for r in ranges], [r[1] for r in ranges]
        res = []
        for _ in range(2):
            outs = [Out(B * k, 3 * E, T) for k in n]
            L.call("timhip_gather_split3_ranges", L.PRECISIONS[prec], L.ptr(xd), B, S, E, len(ranges), ia(s0), ia(n),
                   pa([o.v for o in outs]), st())
            res.append(outs)
        sync()
        for o, o2, rows in zip(res[0], res[1], R.gather_ranges(x, ranges)):
            hi, lo = R.split3(rows, T)
            assert o.guards_intact() and same_bits(o.v, o2.v)
            assert same_bits(o.v.cpu(), torch.cat([hi, lo, hi], 1))


def test_dx_init_range_shapes():
    """timhip_dx_init / _slabs beyond the two cases of tests/test_gpu_kernels.py: one to six ranges, ranges of one row, adjacent,
    out of order, ending at S, rows of no range, B = 1"""
    for B in (1, 3):
        for E in (64, 1024):
            S, F = 23, 9
            feats = rn(B, F, E, seed=1)
            for ranges in RANGE_SETS:
                s0, n = [r[0] for r in ranges], [r[1] for r in ranges]
                nslab = [1 + (i % 3) for i in range(len(ranges))]
                rows = [rn(z, B * k, E, seed=5 + i) for i, (k, z) in enumerate(zip(n, nslab))]
                rows_d = [r.to(DEV) for r in rows]
                want = torch.zeros(B, S, E)
                want[:, :F] = feats
                for (a, k), r in zip(ranges, rows):
                    acc = r[0].clone()
                    for z in range(1, r.shape[0]):
                        acc += r[z]                      # the documented order: slab after slab
                    want[:, a:a + k] = acc.view(B, k, E)
                dx = Out(B * S, E)
                L.call("timhip_dx_init_slabs", B, S, F, E, L.ptr(feats.to(DEV)), len(ranges), ia(s0), ia(n), pa(rows_d), ia(nslab),
                       dx.ptr, st())
                dx1 = Out(B * S, E)
                L.call("timhip_dx_init", B, S, F, E, None, len(ranges), ia(s0), ia(n), pa([r[0] for r in rows_d]), dx1.ptr, st())
                sync()
                assert dx.guards_intact() and dx1.guards_intact()
                assert same_bits(dx.v.cpu(), want.view(B * S, E))
                w1 = torch.zeros(B, S, E)
                for (a, k), r in zip(ranges, rows):
                    w1[:, a:a + k] = r[0].view(B, k, E)
                assert same_bits(dx1.v.cpu(), w1.view(B * S, E))


# =============================================================================================== small elementwise kernels
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ld", [2, 8, 64])
def test_sigmoid_bwd_rows(prec, ld):
    """dst = T(scale * g * y * (1 - y)), zero from column 2 to ld; y at 0, 1, 0.5 and next to the ends"""
    T, rows, cols = DT[prec], 301, 2
    y = torch.sigmoid(rn(rows, cols, seed=1) * 4)
    y[0, 0], y[0, 1], y[1, 0], y[1, 1] = 0.0, 1.0, 0.5, 1e-38
    y[2, 0], y[2, 1] = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)), 1e-45
    g = rn(rows, cols, seed=2)
    yd, gd = y.to(DEV), g.to(DEV)
    for sv in (None, 2.0 ** -7, 8.0):
        blk = scale_block(0, sv) if sv else None
        res = []
        for _ in range(2):
            o = Out(rows, ld, T)
            L.call("timhip_sigmoid_bwd_rows", L.PRECISIONS[prec], L.ptr(gd), L.ptr(yd), rows, cols, o.ptr, ld, L.ptr(blk), st())
            res.append(o)
        sync()
        o = res[0]
        assert o.guards_intact() and same_bits(o.v, res[1].v)
        assert blk is None or same_bits(blk, scale_block(0, sv))
        got = o.v.cpu().to(F64)
        assert bool((got[:, cols:] == 0).all())
        ref = R.sigmoid_bwd(g.to(F64), y.to(F64), sv or 1.0)
        # 1 - y and two products round in fp32 (the power-of-two scale is exact): 3 u |ref|; below the smallest normal number
        # (2^-126) a product carries no relative bound; then the store
        e32 = 3 * U * ref.abs() + 2.0 ** -126
        assert bool(((got[:, :cols] - ref).abs() <= e32 * (1 + R.HALF_ULP[T]) + R.store_bound(ref, T)).all())
        assert got[0, 0] == 0 and got[0, 1] == 0


@pytest.mark.parametrize("prec", PRECS)
def test_cast_rows_many(prec):
    """six matrices of different shapes in one launch; a row pitch beyond 2048 (8 column blocks per row: a block walks); padding
    columns zero; the scale word multiplied in (a power of two: the cast of the exact product)"""
    T = DT[prec]
    shapes = [(5, 3, 64), (17, 97, 128), (1, 2100, 2112), (33, 300, 320), (2, 1, 4), (9, 2049, 4096)]
    src = [rn(r, c, seed=i) for i, (r, c, _) in enumerate(shapes)]
    src_d = [s.to(DEV) for s in src]
    for sv in (None, 2.0 ** -7):
        for count in (6, 1):
            blk = scale_block(0, sv) if sv else None
            outs = [Out(r, ld, T) for (r, _, ld) in shapes[:count]]
            L.call("timhip_cast_rows_many", L.PRECISIONS[prec], count, pa(src_d[:count]), ia([s[0] for s in shapes[:count]]),
                   ia([s[1] for s in shapes[:count]]), pa([o.v for o in outs]), ia([s[2] for s in shapes[:count]]), L.ptr(blk), st())
            sync()
            for o, s, (r, c, ld) in zip(outs, src, shapes):
                assert o.guards_intact()
                want = torch.zeros(r, ld)
                want[:, :c] = s * (sv or 1.0)
                assert same_bits(o.v.cpu(), want.to(T)), (r, c, ld)
            assert blk is None or same_bits(blk, scale_block(0, sv))
    assert all(same_bits(a.cpu(), b) for a, b in zip(src_d, src))


def _cast_check(got, src, cols, ld, T, p, seed, site, vs):
    """got == the torch restatement of timhip_cast_rows: T(x * mask / (1 - p) * vs), zero from `cols` to `ld`; the mask is
    timhip_dropout_mask's at a row pitch of `cols` rounded up to a multiple of 4 (the kernel draws per column quad).  Equal as
    values everywhere, no tolerance; bit for bit wherever the mask keeps (a dropped x < 0 is x * 0 = -0 on most paths and +0 where
    the compiler fuses the fp16 conversion into a multiply-add with a +0 addend: the sign of that zero is nobody's contract)"""
    rows = src.shape[0]
    v = src[:, :cols].cpu()
    kept = torch.ones(rows, ld, dtype=torch.bool)
    if p > 0:
        pitch = (cols + 3) // 4 * 4
        mk = torch.empty((rows, pitch), dtype=torch.uint8, device=DEV)
        L.call("timhip_dropout_mask", seed, site, p, rows, pitch, L.ptr(mk), st())
        sync()
        kept[:, :cols] = mk.cpu()[:, :cols] != 0
        v = v * (kept[:, :cols].float() / (1 - p))
    want = torch.zeros(rows, ld, dtype=T)
    want[:, :cols] = (v * vs).to(T)
    got = got.cpu()
    return torch.equal(got, want) and same_bits(got[kept], want[kept])


CAST_SHAPES = [(5, 5, 8), (8, 12, 8), (8, 8, 64), (1, 1, 64)]
#  (cols, lds, ld): scalar tail; strided source, 16-byte path; zero padding out to ld; the loss path's one column


@pytest.mark.parametrize("prec", PRECS)
def test_cast_rows_one_item_and_pair(prec):
    """timhip_cast_rows and timhip_cast_rows_pair are one kernel over one or two items: a round-to-nearest cast of x * mask / (1 - p)
    * scale with p = 0.5 and scale = 0.5 (both products exact), so every case equals the torch restatement bit for bit; the pair
    equals two single calls bit for bit"""
    T, rows, seed = DT[prec], 3, 0x1234567
    half = torch.tensor([0.5], device=DEV)
    for cols, lds, ld, off in [c + (0,) for c in CAST_SHAPES] + [(8, 12, 8, 1)]:   # off = 1: the source starts 4 bytes past a
        flat = rn(rows * lds + off, seed=cols + lds + ld).to(DEV)                   # 16-byte boundary: element by element
        src = flat[off:].view(rows, lds)
        assert src.data_ptr() % 16 == 4 * off
        for p in (0.0, 0.5):
            for vs in (None, half):
                o = Out(rows, ld, T)
                L.call("timhip_cast_rows", L.PRECISIONS[prec], L.ptr(src), rows, cols, lds, o.ptr, ld, p, seed, L.SITE_FEAT_V,
                       L.ptr(vs), st())
                sync()
                assert o.guards_intact(), (cols, lds, ld, off, p, vs is not None)
                assert _cast_check(o.v, src, cols, ld, T, p, seed, L.SITE_FEAT_V, 0.5 if vs is not None else 1.0), \
                    (cols, lds, ld, off, p, vs is not None)
                assert bool((o.v[:, cols:] == 0).all())
    assert same_bits(half.cpu(), torch.tensor([0.5]))
    # the pair: two contiguous matrices of different widths and sites
    cols, lds_out, sites = (5, 8), (8, 64), (L.SITE_FEAT_V, L.SITE_FEAT_A)
    srcs = [rn(rows, c, seed=40 + c).to(DEV) for c in cols]
    for p in (0.0, 0.5):
        pair = [Out(rows, ld, T) for ld in lds_out]
        L.call("timhip_cast_rows_pair", L.PRECISIONS[prec], pa(srcs), ia(cols), pa([o.v for o in pair]), ia(lds_out), rows, p, seed,
               (C.c_uint32 * 2)(*sites), st())
        for x, c, ld, site, o2 in zip(srcs, cols, lds_out, sites, pair):
            o1 = Out(rows, ld, T)
            L.call("timhip_cast_rows", L.PRECISIONS[prec], L.ptr(x), rows, c, c, o1.ptr, ld, p, seed, site, None, st())
            sync()
            assert o1.guards_intact() and o2.guards_intact() and same_bits(o1.v, o2.v), (c, p)
            assert _cast_check(o2.v, x, c, ld, T, p, seed, site, 1.0), (c, p)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 9925])
def test_colsum_accumulates(prec, rows):
    """out[c] += sum_r src[r, c] (include/timhip.h: float atomics, one per 64-row block): a pre-filled `out` keeps its value"""
    T = DT[prec]
    for cols in ((1, 255, 257, 1024) if rows < 9925 else (1, 257)):
        ld = cols + 8
        src = torch.full((rows, ld), 3.0).to(T)
        src[:, :cols] = rn(rows, cols, seed=rows + cols).to(T)
        out = Out(1, cols, fill="acc")
        L.call("timhip_colsum", L.PRECISIONS[prec], L.ptr(src.to(DEV)), rows, cols, ld, out.ptr, st())
        sync()
        assert out.guards_intact()
        pre, s64 = out.pre.view(-1).cpu().to(F64), src[:, :cols].to(F64)
        nblk = (rows + 63) // 64
        # at most 64 terms per block in order, then one atomic per block onto the running value: (64 + nblk + 1) u (|pre| + sum|terms|)
        lim = (64 + nblk + 1) * U * (pre.abs() + s64.abs().sum(0))
        err = (out.v.view(-1).cpu().to(F64) - (pre + s64.sum(0))).abs()
        assert bool((err <= lim).all()), (rows, cols, (err - lim).max().item())


# rows per block of the LayerNorm backward as include/timhip.h / DESIGN.md describe them: 4 below 2048 rows ... 20 at 9920 rows
LN_BLOCKS = {77: 20, 1240: 310, 9920: 496}


@pytest.mark.parametrize("rows", sorted(LN_BLOCKS))
@pytest.mark.parametrize("nsets", [1, 16])
def test_ln_partials_reduce(rows, nsets):
    """dgamma[i][c] += sum_b partials[i][b][c], dbeta[i][c] += sum_b partials[i][b][cols + c] over the blocks of a LayerNorm
    backward launch of `rows` rows (set stride = blocks * 2 * cols floats); partials filled by hand"""
    cols, nblk = 64, LN_BLOCKS[rows]
    part = rn(nsets, nblk, 2 * cols, seed=rows)
    # (allocated for one block per four rows, the smallest block the launcher ever picks: nothing can be read past the buffer
    #  should the library's block count differ from this file's - the sums would)
    buf = torch.zeros(nsets * ((rows + 3) // 4) * 2 * cols, device=DEV)
    buf[:part.numel()] = part.view(-1).to(DEV)
    keep = buf.clone()
    dg, db = Out(nsets, cols, fill="acc"), Out(nsets, cols, fill="acc")
    L.call("timhip_ln_partials_reduce", L.ptr(buf), nsets, rows, cols, pa([dg.v[i] for i in range(nsets)]),
           pa([db.v[i] for i in range(nsets)]), st())
    sync()
    assert dg.guards_intact() and db.guards_intact() and same_bits(buf, keep)
    p64 = part.to(F64)
    for o, ref, ab in ((dg, p64[:, :, :cols].sum(1), p64[:, :, :cols].abs().sum(1)), (db, p64[:, :, cols:].sum(1), p64[:, :, cols:].abs().sum(1))):
        pre = o.pre.cpu().to(F64)
        # nblk terms in 32 shares of four running sums, one atomic per share: (nblk + 32 + 4) u (|pre| + sum|terms|)
        lim = (nblk + 36) * U * (pre.abs() + ab)
        assert bool(((o.v.cpu().to(F64) - (pre + ref)).abs() <= lim).all())


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_dp_reduce(wire, world):
    """out = T(scale * sum over ranks in rank order, accumulated in fp32): no atomics, a fixed order - bit for bit the same fp32
    additions on the host"""
    T = DT[wire]
    for per in (4, 1028, 2 ** 20 + 4):
        recv = rn(world, per, seed=world + per % 7).to(T)
        scale = 1.0 / 3.0
        rd = recv.to(DEV)
        res = []
        for _ in range(2):
            o = Out(1, per, T)
            L.call("timhip_dp_reduce", 1 if wire == "bf16" else 0, L.ptr(rd), world, per, scale, o.ptr, st())
            res.append(o)
        sync()
        assert res[0].guards_intact() and same_bits(res[0].v, res[1].v) and same_bits(rd.cpu(), recv)
        acc = torch.zeros(per)
        for w in range(world):
            acc += recv[w].float()
        want = (acc * torch.tensor(scale, dtype=torch.float32)).to(T)
        assert same_bits(res[0].v.view(-1).cpu(), want), (world, per)
        ref = recv.to(F64).sum(0) * scale
        lim = (world + 2) * U * recv.to(F64).abs().sum(0) * scale
        assert bool(((res[0].v.view(-1).cpu().to(F64) - ref).abs() <= lim * (1 + R.HALF_ULP[T]) + R.store_bound(ref, T)).all())
