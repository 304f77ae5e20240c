"""NT GEMM and weight-gradient kernels against float64 with ELEMENTWISE bounds, one small case per route of gemm_plan.h /
wgrad_plan.h (tests/gemm_ref.py holds the references, the bounds and their derivations; tests/test_gemm_ref.py shows on the CPU
what the checker rejects).  Every case
  * first asks the plan (tests/gemm_plan_print.cpp, compiled with g++: host only) which kernel the call gets and asserts the
    family and tile it is meant for - a later routing change cannot silently move a case onto another kernel;
  * runs every epilogue the family carries with its outputs in guarded buffers and ALL pitches different from each other and
    from N (ld0, ld1, ldres, ldaux, ldmask, lda, ldb), operand columns past Kp NaN;
  * makes the call twice: a non-atomic epilogue repeats bit for bit;
  * checks every element against its own bound, and the guard rows and pad columns bit for bit.
The alignment classes (a) - (d) put the one-block-per-CU epilogue (pp_epilogue) and epi_quad / epi_oct on each of their
branches: 8-wide, the N % 8 == 4 tail and the unpaired Philox draw, the quad path, the scalar path.
The fp64 work runs on the device.  Largest problem: 5115 x 6144 x 128."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gemm_ref as G  # noqa: E402
from tests.test_gemm_plan import _ask, _compile, _group, _nt  # noqa: E402
from tests.test_wgrad_plan import _wgroup, _wtn  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd.functional import Runtime  # noqa: E402

DEV = "cuda:0"
H16 = ["bf16", "fp16"]
P, SEED, SITE = 0.3, 1234567, 42
PP_EPI = (L.EPI_STORE_T, L.EPI_RELU_T, L.EPI_STORE_F32, L.EPI_DROP_RES_F32, L.EPI_ADD_F32, L.EPI_GELU_DROP_G2, L.EPI_GELU_T, L.EPI_MULAUX_T)
P8_EPI = (L.EPI_STORE_T, L.EPI_GELU_DROP_G2, L.EPI_GELU_T, L.EPI_MULAUX_T)
F32_EPI = tuple(e for e in G.ALL_EPI if e != L.EPI_RELU_SPLIT3_T)     # (the split-operand epilogue is for 16-bit storage)
SHARES = {}      # family -> largest used share of the (arithmetic part of the) bound


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("gemm_edges") / "gemm_plan_print")
    yield exe
    for fam in sorted(SHARES):
        print("\nlargest used share of the elementwise bound, %-6s %.3f" % (fam, SHARES[fam]))


def _route(printer, knobs, prec, epi, M, N, K, want, splitk=1, a_wrap=0, **kn):
    """set the launcher knobs (TIMHIP_<name>) for the test, ask the plan with the same knobs, assert what the case is meant for"""
    if kn:
        knobs(**{"TIMHIP_" + k: str(v) for k, v in kn.items()})
    plan = _ask(printer, [_nt(L.PRECISIONS[prec], epi, M, N, K, splitk, a_wrap, **kn)])[0]
    assert {k: plan[k] for k in want} == want, (plan, (prec, epi, M, N, K))
    return plan


# ---- the alignment classes ---------------------------------------------------------------------------------------------------
def _pitches(cls, epi, N, Kp, prec, kw=None):
    """(a) / (b): every 16-bit pitch % 8, fp32 pitches % 4 (the class is N % 8 == 0 or == 4); (c): % 4 and not % 8; (d): odd N with
    odd pitches.  All different from each other and from N in every class."""
    p = G.default_pitches(epi, N, Kp, prec, kw)
    r8 = G._ru(N, 8)
    if cls == "c":
        p.update(ld0=r8 + 4, ld1=r8 + 12, ldaux=r8 + 20, ldres=r8 + 28)
    if cls == "d":
        p.update(ld0=N + 2, ld1=N + 6, ldaux=N + 10, ldres=N + 4)
    return p


def _assert_class(cls, c):
    """the precondition the epilogues branch on, so that a case cannot drift out of its class"""
    used = [c.ld0] + ([c.ld1] if c.out1 is not None else []) + ([c.ldaux] if c.aux is not None else []) + ([c.ldres] if c.res is not None else [])
    h16 = [c.ld0] * (c.epi not in G.F32_OUT) + ([c.ld1] if c.out1 is not None else []) + ([c.ldaux] if c.aux is not None and c.epi != L.EPI_DRELU_F32IN_T else [])
    ptrs = [t.data_ptr() for t in (c.out0, c.out1, c.res, c.aux, c.bias_buf) if t is not None]
    if cls in ("a", "b"):     # e.vec and e.vec8; (a): no column tail, the paired Philox draw; (b): the vec8 tail, the unpaired draw
        assert all(v % 4 == 0 for v in used) and all(v % 8 == 0 for v in h16) and all(q % 16 == 0 for q in ptrs)
        assert (c.N & 7) == (0 if cls == "a" else 4)
    elif cls == "c":          # e.vec, not e.vec8: the quad path of the 16-bit outputs
        assert all(v % 4 == 0 for v in used) and all(v % 8 == 4 for v in h16) and all(q % 16 == 0 for q in ptrs)
    else:                     # not e.vec: the scalar path, columns up to an odd N
        assert c.N % 2 == 1 and c.ld0 % 2 == 1 and any(v % 4 for v in used)
    assert len({c.N, c.ld0, c.ld1, c.ldres, c.ldaux, c.lda, c.ldb}) == 7 and c.ldmask != (c.N + 7) // 8


# ---- one call ----------------------------------------------------------------------------------------------------------------
def _epi_struct(c):
    ln = c.ln
    return L.TimEpi(L.ptr(c.out0), L.ptr(c.out1), L.ptr(c.bias_buf), L.ptr(c.res), L.ptr(c.aux), c.ld0, c.ld1, c.ldres, c.ldaux,
                    float(c.p), SITE, SEED, L.ptr(c.mask), c.ldmask, 0, L.ptr(ln.stats) if ln else None, L.ptr(ln.w) if ln else None,
                    L.ptr(ln.b) if ln else None, L.ptr(c.sc_buf), c.kw if c.a_wrap else 0, 0)


def _launch(c):
    e = _epi_struct(c)
    L.call("timhip_gemm_nt", L.PRECISIONS[c.dtype], c.epi, L.ptr(c.Abuf), c.lda, L.ptr(c.Bbuf), c.ldb, c.M, c.N, c.K, C.byref(e),
           c.splitk, st())


def _keep_set(M, N):
    keep = torch.empty((M, N), dtype=torch.uint8, device=DEV)
    L.call("timhip_dropout_mask", SEED, SITE, P, M, N, L.ptr(keep), st())
    torch.cuda.synchronize()
    assert abs(float(keep.float().mean()) - (1 - P)) < 0.05
    return keep


def _twice_and_verify(c, launch=_launch):
    before = G.snapshot(c)
    launch(c)
    torch.cuda.synchronize()
    first = G.snapshot(c)
    share = G.verify(c, before)
    G.reset_outputs(c, before)
    launch(c)
    torch.cuda.synchronize()
    if c.epi == L.EPI_ATOMIC_F32:
        share = max(share, G.verify(c, before))
    else:
        for k, v in first.items():
            assert G._bits_equal(getattr(c, k), v), "the call does not repeat bit for bit: " + k
    return share


def _variants(epi, N, keep_sets, M):
    """the forms of one epilogue: dropout drawn in the epilogue / read from keep-bits, the LayerNorm residual, acc_scale"""
    drop = epi in G.HAS_DROPOUT and N % 4 == 0
    if drop and (M, N) not in keep_sets:
        keep_sets[(M, N)] = _keep_set(M, N)
    kw = dict(p=P, keep=keep_sets[(M, N)]) if drop else {}
    out = [dict(kw)]
    if drop and epi in (L.EPI_GELU_DROP_G2, L.EPI_GELU_DROP_T2, L.EPI_DGELU_T):
        out.append(dict(kw, mask_bits=True))
    if epi == L.EPI_DROP_RES_F32:
        out.append(dict(kw, ln=True))
        out.append(dict())                       # p = 0: the plain residual
    if epi == L.EPI_ADD_F32:
        out.append(dict(acc_scale=0.25))
    return out


def _run_epilogues(family, prec, M, N, K, epis, cls=None, check_route=None, **case_kw):
    """returns the forms that ran: {(epilogue, dropout on, keep-bits handed over)}"""
    keep_sets, forms = {}, set()
    for epi in epis:
        for kw in _variants(epi, N, keep_sets, M):
            if check_route is not None:
                check_route(epi)
            kw.update(case_kw)
            Kp = G._ru(K)
            if cls is not None:
                kw["pitches"] = _pitches(cls, epi, N, Kp, prec, Kp // 2 if kw.get("a_wrap") else None)
            c = G.make_case(epi, M, N, K, prec, device=DEV, seed=11 + epi, **kw)
            if cls is not None:
                _assert_class(cls, c)
            share = _twice_and_verify(c)
            SHARES[family] = max(SHARES.get(family, 0.0), share)
            forms.add((epi, c.p > 0, c.mask is not None))
    return forms


def _assert_dropout_branches(forms):
    """classes (a) and (b) on the one-block-per-CU kernels: the dropout + residual epilogue drew its own Philox numbers - by lane
    pairs when (N & 7) == 0 (TIMHIP_EPI_PAIR, on by default), one quad at a time otherwise - and the GELU epilogue read keep-bits
    (use_mask: all of a row's bytes in class (a), with the n + 7 < N tail left to the quad path in class (b))"""
    assert os.environ.get("TIMHIP_EPI_PAIR", "1") == "1"
    assert (L.EPI_DROP_RES_F32, True, False) in forms and (L.EPI_GELU_DROP_G2, True, True) in forms


# ---- gemm.hip: the two-blocks-per-CU kernel, every epilogue --------------------------------------------------------------------
def _h16(bm, wm, wn, nst):
    return dict(family="h16", bm=bm, bn=128, wm=wm, wn=wn, nst=nst)


H16_ROUTES = [
    ("128x128, M <= 64", _h16(128, 2, 2, 2), [(1, 5, 24), (64, 136, 192)], {}),
    ("64x128, 8 waves, 4 stages", _h16(64, 2, 4, 4), [(70, 136, 192), (130, 136, 64)], {}),
    ("64x128, 4 waves", _h16(64, 1, 4, 4), [(70, 136, 192)], dict(GEMM_SMALL_W8=0)),
    ("64x128, 3 stages", _h16(64, 1, 4, 3), [(2000, 1100, 64)], {}),
    ("128x128", _h16(128, 2, 2, 2), [(2100, 2056, 64)], {}),
    ("160x128", _h16(160, 1, 4, 2), [(1270, 6604, 128)], {}),
]


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("name,want,shapes,kn", H16_ROUTES, ids=[r[0] for r in H16_ROUTES])
def test_h16_routes_every_epilogue(name, want, shapes, kn, prec, printer, knobs):
    for M, N, K in shapes:
        _run_epilogues("h16", prec, M, N, K, G.ALL_EPI, check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, want, **kn))


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("cls,N", [("a", 136), ("b", 132), ("c", 136), ("d", 135)])
def test_h16_alignment_classes(cls, N, prec, printer, knobs):
    M, K = 70, 192
    epis = [e for e in G.ALL_EPI if e != L.EPI_RELU_SPLIT3_T and not (cls == "d" and e in G.HAS_DROPOUT)]   # (odd N: the ABI refuses dropout)
    _run_epilogues("h16", prec, M, N, K, epis, cls=cls,
                   check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, _h16(64, 2, 4, 4)))


@pytest.mark.parametrize("prec", H16)
def test_h16_wrapped_a_operand(prec, printer, knobs):
    """C = [A | A] B^T on the two-blocks-per-CU kernel: K = 2 x 128, A has 128 columns"""
    M, N, K = 70, 136, 256
    epis = [e for e in G.ALL_EPI if e != L.EPI_ATOMIC_F32]
    _run_epilogues("h16", prec, M, N, K, epis, a_wrap=True,
                   check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, _h16(64, 2, 4, 4), a_wrap=2))


@pytest.mark.parametrize("prec", H16)
def test_split_k_atomics(prec, printer, knobs):
    M, N, K = 310, 256, 128
    _route(printer, knobs, prec, L.EPI_ATOMIC_F32, M, N, K, dict(family="h16", grid_z=2, ksteps=1), splitk=2)
    _run_epilogues("h16", prec, M, N, K, [L.EPI_ATOMIC_F32], splitk=2)


# ---- gemm_pp.hip: the one-block-per-CU kernels ---------------------------------------------------------------------------------
PP_ROUTES = {
    "ld128": (dict(family="ld", tm=4, bm=128, tpb=1), dict(GEMM_PP_MIN_TILES=1)),
    "ld160": (dict(family="ld", tm=5, bm=160, tpb=1), dict(GEMM_PP_MIN_TILES=1, GEMM_TMW=5)),
    "pp8w": (dict(family="pp8w", tm=5, bm=160), dict(GEMM_PP_MIN_TILES=1, GEMM_LD=0)),
}


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("cls,N", [("a", 512), ("b", 516), ("c", 516), ("d", 515)])
@pytest.mark.parametrize("route", sorted(PP_ROUTES))
def test_pp_routes_alignment_classes(route, cls, N, prec, printer, knobs):
    """three contraction steps against the three-stage ring, a ragged last row panel (1283 rows) and column tile"""
    want, kn = PP_ROUTES[route]
    M, K = 1283, 192
    epis = [e for e in PP_EPI if not (cls == "d" and e in G.HAS_DROPOUT)]
    forms = _run_epilogues(want["family"], prec, M, N, K, epis, cls=cls,
                           check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, want, **kn))
    if cls in ("a", "b"):
        _assert_dropout_branches(forms)


@pytest.mark.parametrize("prec", H16)
def test_ld_one_contraction_step(prec, printer, knobs):
    M, N, K = 1283, 512, 64
    want, kn = PP_ROUTES["ld128"]
    _run_epilogues("ld", prec, M, N, K, PP_EPI, cls="a", check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, want, **kn))


@pytest.mark.parametrize("prec", H16)
def test_pp8w_wrapped_a_operand(prec, printer, knobs):
    """C = [A | A] B^T: K = 2 x 128, A has 128 columns and lda = 192"""
    M, N, K = 1283, 512, 256
    _run_epilogues("pp8w", prec, M, N, K, PP_EPI, cls="a", a_wrap=True,
                   check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, dict(family="pp8w", tm=5), a_wrap=2, GEMM_PP_MIN_TILES=1))


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("cls,N", [("a", 4096), ("b", 4004), ("c", 4004), ("d", 4003)])
def test_ldp_walk_of_two_alignment_classes(cls, N, prec, printer, knobs):
    """gemm_nt_ldp_kernel at two contraction steps, two column tiles per block, 512 tiles; TIMHIP_GEMM_P8=0 keeps the 16-bit
    store and the GELU epilogues here (by default the eight-phase kernel takes them at this shape)"""
    M, K = 5115, 128
    want = dict(family="ldp", tm=5, tpb=2, grid_x=256)
    epis = [e for e in PP_EPI if not (cls == "d" and e in G.HAS_DROPOUT)]
    forms = _run_epilogues("ldp", prec, M, N, K, epis, cls=cls, check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, want, GEMM_P8=0))
    if cls in ("a", "b"):
        _assert_dropout_branches(forms)


@pytest.mark.parametrize("prec", H16)
def test_ldp_default_knobs_walks_of_two_and_three_and_the_multi_round_ld(prec, printer, knobs):
    for (M, N, K), want, epis in [((5115, 4096, 128), dict(family="ldp", tpb=2), (L.EPI_STORE_F32, L.EPI_DROP_RES_F32, L.EPI_ADD_F32)),
                                  ((5115, 6144, 128), dict(family="ldp", tpb=3, grid_x=256), (L.EPI_STORE_F32,)),
                                  ((5115, 4096, 64), dict(family="ld", tpb=1, grid_x=512, pf_dist=0), (L.EPI_STORE_F32, L.EPI_STORE_T))]:
        _run_epilogues(want["family"], prec, M, N, K, epis, cls="a", check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, want))


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("cls", ["a", "c"])
@pytest.mark.parametrize("K,tm,phases", [(128, 8, 2), (192, 8, 2), (128, 8, 4), (192, 8, 4), (192, 10, 2)])
def test_p8_routes(K, tm, phases, cls, prec, printer, knobs):
    """the eight-phase kernel at Kp = 128 (its two-stage prologue and nothing else) and 192; N must be a multiple of 256 there,
    so only the pitches vary: 8-wide and the quad path"""
    M, N = 1283, 512
    want = dict(family="p8", tm=tm, bm=32 * tm, phases=phases)
    knobs(TIMHIP_GEMM_PP_MIN_TILES="1", TIMHIP_GEMM_P8=str(tm), TIMHIP_GEMM_P8_PH=str(phases))
    for epi in P8_EPI:     # the library itself, with the knobs the printer is given below, answers the same
        assert L.load().timhip_gemm_p8_choice(epi, M, N, K) == tm
    _run_epilogues("p8", prec, M, N, K, P8_EPI, cls=cls,
                   check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, want, GEMM_PP_MIN_TILES=1, GEMM_P8=tm, GEMM_P8_PH=phases))


# ---- fp32 and bf16x3 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,family", [("fp32", "f32"), ("bf16x3", "x3")])
@pytest.mark.parametrize("M,N,K", [(130, 136, 24), (130, 136, 64)])
def test_f32_and_x3_every_epilogue(M, N, K, prec, family, printer, knobs):
    _run_epilogues(family, prec, M, N, K, F32_EPI, check_route=lambda epi: _route(printer, knobs, prec, epi, M, N, K, dict(family=family, bm=128, bn=128)))


# ---- the grouped launch --------------------------------------------------------------------------------------------------------
GROUP_SHAPES = [(960, 97, 192), (960, 300, 192), (960, 3806, 192), (640, 44, 192), (70, 136, 192), (1, 5, 24)]   # test_gemm_group's, K <= 192


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("epi,big,want", [(L.EPI_STORE_F32, True, dict(bn=128, wn=4, nst=2)), (L.EPI_ADD_F32, True, dict(bn=128, wn=4, nst=2)),
                                          (L.EPI_ADD_F32, False, dict(bn=64, wm=2, wn=2, nst=2)), (L.EPI_STORE_F32, False, dict(bn=128, nst=4)),
                                          (L.EPI_STORE_T, False, dict(bn=128, nst=4)), (L.EPI_RELU_T, False, dict(bn=128, nst=4))])
def test_grouped_launch(epi, big, want, prec, printer):
    shapes = [s for s in GROUP_SHAPES if big or s[1] != 3806]
    plan = _ask(printer, [_group(epi, [(m, n) for m, n, _ in shapes])])[0]
    assert {k: plan[k] for k in want} == want, plan
    cases = [G.make_case(epi, M, N, K, prec, device=DEV, seed=50 + i) for i, (M, N, K) in enumerate(shapes)]
    arr = (L.TimGemmItem * len(cases))()
    for a, c in zip(arr, cases):
        a.A, a.B, a.lda, a.ldb, a.M, a.N, a.K, a.reserved, a.e = L.ptr(c.Abuf), L.ptr(c.Bbuf), c.lda, c.ldb, c.M, c.N, c.K, 0, _epi_struct(c)

    def launch():
        L.call("timhip_gemm_nt_group", L.PRECISIONS[prec], epi, C.cast(arr, C.c_void_p), len(cases), st())
        torch.cuda.synchronize()

    before = [G.snapshot(c) for c in cases]
    launch()
    first = [G.snapshot(c) for c in cases]
    for c, b in zip(cases, before):
        SHARES["group"] = max(SHARES.get("group", 0.0), G.verify(c, b))
        G.reset_outputs(c, b)
    launch()
    for c, f in zip(cases, first):
        assert G._bits_equal(c.out0_whole, f["out0_whole"])


# ---- weight gradients ----------------------------------------------------------------------------------------------------------
def _wgrad_items(M, shapes, prec, no_bias=1):
    """per item: guarded operands with ldy > Nout and ldx > Kout (both % 8, all different), a guarded dW and db, their fp64 values"""
    T = G.OP_DTYPE[prec]
    g = torch.Generator(device=DEV).manual_seed(77)
    items = []
    for i, (N, K) in enumerate(shapes):
        ldy, ldx = G._ru(N, 8) + 8 + 16 * i, G._ru(K, 8) + 24 + 16 * i
        assert ldy % 8 == 0 and ldx % 8 == 0 and len({N, K, ldy, ldx}) == 4 - (N == K)
        cy = torch.exp2(torch.randint(-4, 5, (N,), generator=g, device=DEV).float())
        cx = torch.exp2(torch.randint(-3, 4, (K,), generator=g, device=DEV).float())
        dY = (torch.randn(M, N, generator=g, device=DEV) * 0.25 * cy).to(T)
        X = (torch.randn(M, K, generator=g, device=DEV) * cx).to(T)
        yw, yv = G.guarded(M, N, ldy, T, DEV, dY)
        xw, xv = G.guarded(M, K, ldx, T, DEV, X)
        it = dict(N=N, K=K, dY=yv, X=xv, dY64=dY.double(), X64=X.double(), keep=(yw, xw))
        it["dW_whole"], it["dW"] = G.guarded(N, K, K, torch.float32, DEV, torch.full((N, K), 0.5))
        it["db_whole"] = it["db"] = None
        if i != no_bias:
            it["db_whole"], it["db"] = (t.view(-1) for t in G.guarded(1, N, N, torch.float32, DEV, torch.full((1, N), -0.25)))
        items.append(it)
    return items


def _wgrad_check(family, items, splits, accumulate, out_scale, launch):
    before = [(it["dW_whole"].clone(), None if it["db"] is None else it["db_whole"].clone()) for it in items]
    firsts = None
    for _ in range(2):
        for it, (bw, bb) in zip(items, before):
            it["dW_whole"].copy_(bw)
            if bb is not None:
                it["db_whole"].copy_(bb)
        launch()
        torch.cuda.synchronize()
        got = [(it["dW_whole"].clone(), None if it["db"] is None else it["db_whole"].clone()) for it in items]
        if firsts is None:
            firsts = got
    for it, (bw, bb), (fw, fb), (gw, gb) in zip(items, before, firsts, got):
        N, K = it["N"], it["K"]
        assert G.untouched(it["dW_whole"], bw, N, K), "dW: a guard row was written"
        base_w = torch.full((N, K), 0.5, dtype=G.F64, device=DEV) if accumulate else None
        base_b = torch.full((N,), -0.25, dtype=G.F64, device=DEV) if accumulate else None
        (w, lim_w), (b, lim_b) = G.wgrad_reference(it["dY64"], it["X64"], splits, base_w, base_b, out_scale)
        for whole in (fw, gw):      # both calls within the bound; a launch without a split and without atomics repeats bit for bit
            sh = G.share_of_bound(whole[2:2 + N].double(), w, lim_w)
            assert sh <= 1.0, ("dW", N, K, sh)
            SHARES[family] = max(SHARES.get(family, 0.0), sh)
        if it["db"] is not None:
            assert G.untouched(it["db_whole"].view(5, N), bb.view(5, N), 1, N), "db: a guard element was written"
            for whole in (fb, gb):
                sh = G.share_of_bound(whole.view(5, N)[2].double(), b, lim_b)
                assert sh <= 1.0, ("db", N, sh)
                SHARES[family] = max(SHARES.get(family, 0.0), sh)
    return firsts, got


def _out_scale(prec):
    """fp16: a power of two on the outputs, handed over as word 1 of a gradient-scale block (include/timhip.h: timhip_grad_scale)"""
    if prec != "fp16":
        return 1.0, None, None
    gs = torch.zeros(8, device=DEV)
    gs[0], gs[1] = 8.0, 0.125
    return 0.125, gs, gs.data_ptr() + 4


@pytest.mark.parametrize("prec", H16)
def test_wgrad_one_product(prec, printer):
    """timhip_wgrad: one product through the slabs and the reduce kernel; it always accumulates"""
    M, shapes = 523, [(200, 72)]
    plan = _ask(printer, [_wtn(M, *shapes[0])])[0]
    assert plan["family"] == "split" and plan["splits"] == 2 and plan["tiles"] == 2
    rt = Runtime(prec)
    items = _wgrad_items(M, shapes, prec, no_bias=-1)
    scale, gs, sp = _out_scale(prec)
    it = items[0]
    _wgrad_check("wgrad split", items, plan["splits"], True, scale,
                 lambda: rt.wgrad(it["dY"], it["N"], it["X"], it["K"], M, it["dW"], it["db"], out_scale=sp))


WGRAD_ROUTES = [
    ("split, contraction split", 523, [(200, 72), (64, 136), (130, 128)], dict(family="split", splits=2), {}),
    ("split, direct writes", 300, [(128, 128)], dict(family="split", splits=1, ws=0), {}),
    ("ld", 2051, [(3000, 1000), (1000, 3000)], dict(family="ld", tiles=192, splits=1), {}),
    ("pp8w", 2051, [(3000, 1000), (1000, 3000)], dict(family="pp8w", tiles=192, splits=1), dict(WGRAD_LD=0)),
    ("p8, ragged, 2 phases", 2051, [(2048, 2048)] * 3 + [(2048, 1536)], dict(family="p8", tiles=240, ragged=1, phases=2), {}),
    ("p8, ragged, 4 phases", 2051, [(2048, 2048)] * 3 + [(2048, 1536)], dict(family="p8", tiles=240, ragged=1, phases=4), dict(WGRAD_P8_PH=4)),
    ("p8, whole stages", 2048, [(2048, 2048)] * 3 + [(2048, 1536)], dict(family="p8", tiles=240, ragged=0, phases=2), {}),
]


@pytest.mark.parametrize("prec", H16)
@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("name,M,shapes,want,kn", WGRAD_ROUTES, ids=[r[0] for r in WGRAD_ROUTES])
def test_wgrad_group_routes(name, M, shapes, want, kn, accumulate, prec, printer, knobs):
    if kn:
        knobs(**{"TIMHIP_" + k: str(v) for k, v in kn.items()})
    items = _wgrad_items(M, shapes, prec, no_bias=1 if len(shapes) > 1 else -1)
    lds = [(it["dY"].stride(0), it["X"].stride(0)) for it in items]
    plan = _ask(printer, [_wgroup(M, shapes, lds=lds, **kn)])[0]
    assert plan["contract"] == "ok" and {k: plan[k] for k in want} == want, plan
    rt = Runtime(prec)
    scale, gs, sp = _out_scale(prec)
    group = [(it["dY"], it["N"], it["X"], it["K"], it["dW"], it["db"]) for it in items]
    firsts, got = _wgrad_check("wgrad " + want["family"], items, plan["splits"], accumulate, scale,
                               lambda: rt.wgrad_group(group, M, accumulate=accumulate, out_scale=sp))
    if plan["splits"] == 1 and want["family"] != "split":       # one block owns every output element: no atomics, same bits
        for (fw, fb), (gw, gb) in zip(firsts, got):
            assert G._bits_equal(fw, gw) and (fb is None or G._bits_equal(fb, gb))
    if gs is not None:
        assert float(gs[4]) == 0.0      # the non-finite flag stayed clear
