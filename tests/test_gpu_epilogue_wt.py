"""The whole-wave-tile form of the DROP_RES_F32 epilogue on the 160-row loader-wave NT kernel (TIMHIP_EPI_WT=1, the default:
gemm_pp.hip: pp_epilogue_wt_res) against the form it replaces (TIMHIP_EPI_WT=0: pp_epilogue -> epi_quad), BIT FOR BIT: the
output with its guard rows and pad columns, as raw 32-bit words.  The same form of the eight-phase kernel's STORE_T epilogue was
built, measured without a gain and taken out (docs/measurement_log.md); its routes stay here as launches the knob must not touch.

The knob selects a template instance in the launcher.  Each value gets its own child process (`python -m` of this module with
the knob in its environment, so the library reads it the way a product run does); a child runs every case below once - it sets
the case's route knobs and re-reads them (timhip_reload_env) - and saves the outputs, the tests compare the two files.  Two
children for the whole module: a test is a compare.

Routes (all with TIMHIP_GEMM_PP_MIN_TILES=1; test_route asserts each with the plan printer):
    res160   DROP_RES_F32, + TIMHIP_GEMM_TMW=5 -> gemm_nt_ld_kernel, 160 x 256 tile: the instance that carries pp_epilogue_wt_res
    res128   DROP_RES_F32 with that knob alone -> gemm_nt_ld_kernel, 128 x 256 tile: at M = 1280 / 1293 the plan prefers ten
             128-row panels to eight 160-row ones (gemm_plan.h: gemm_pp_tmw), so the shapes as specified do not reach the 160-row
             instance by themselves.  They stay, on the kernel the plan gives them, which the knob must not touch; res160 is the
             same shapes on the kernel the form was built for
    p8_8     STORE_T, + TIMHIP_GEMM_P8=8  -> gemm_nt_p8_kernel, 256 x 256 tile, two phases: the knob must not touch it
    p8_10    STORE_T, + TIMHIP_GEMM_P8=10 -> gemm_nt_p8_kernel, 320 x 256 tile, two phases: the knob must not touch it
    st_ld    STORE_T, + TIMHIP_GEMM_P8=0  -> gemm_nt_ld_kernel: the knob must not touch it
Shapes (M x N x K):
    1280 x 512 x 128    full tiles of every size (160, 256, 320 rows): every wave on the new form
    1293 x 512 x 128    a ragged last row tile: its waves stay on the old path beside new-form tiles
    1280 x 520 x 128    loader-wave routes only (the eight-phase kernel takes N % 256 == 0): a ragged column tile
    1280 x 516 x 128    loader-wave routes only: N % 8 != 0 - the Philox launches fall back as a whole
Inputs: every 16th row of A is zero, so those accumulators are +0; the cases without a bias run with acc_scale = -1, which
turns them into -0.  STORE_T then has to store the word 0x8000 there, and DROP_RES_F32 with a plain residual of -0 in those rows
0x80000000, kept or dropped ((-0) + (-0) k): a bias of +0 where there is none would give +0.  Asserted in both arms.
Dropout (DROP_RES_F32): Philox drawn in the epilogue at p = 0.1 (lane pairs where N % 8 == 0), and p = 0 (thr = 0); the residual
plain and as LayerNorm statistics with affine parameters."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
P = 0.1
ROUTES = {
    "res160": dict(GEMM_PP_MIN_TILES=1, GEMM_TMW=5),
    "res128": dict(GEMM_PP_MIN_TILES=1),
    "p8_8": dict(GEMM_PP_MIN_TILES=1, GEMM_P8=8),
    "p8_10": dict(GEMM_PP_MIN_TILES=1, GEMM_P8=10),
    "st_ld": dict(GEMM_PP_MIN_TILES=1, GEMM_P8=0),
}
WANT = {
    "res160": dict(family="ld", tm=5, bm=160, tpb=1),
    "res128": dict(family="ld", tm=4, bm=128, tpb=1),
    "p8_8": dict(family="p8", tm=8, bm=256, phases=2),
    "p8_10": dict(family="p8", tm=10, bm=320, phases=2),
    "st_ld": dict(family="ld", tpb=1),
}
SHAPES = {"full": (1280, 512, 128), "rows": (1293, 512, 128), "cols": (1280, 520, 128), "n516": (1280, 516, 128)}
PRECS = ("fp16", "bf16")


def _shapes(route):
    return ("full", "rows") if route.startswith("p8") else tuple(SHAPES)


# (route, precision, shape, dropout, LayerNorm residual, bias)
# the routes the knob does not touch launch the same instance in both arms: res128 one case per shape as specified, the STORE_T
# routes fp16 with a bias and without
RES_CASES = [("res160", prec, shape, drop, ln, bias) for prec in PRECS for shape in _shapes("res160")
             for drop in ("philox", "thr0") for ln in (True, False) for bias in (True, False)]
RES_CASES += [("res128", "fp16", shape, "philox", True, True) for shape in _shapes("res128")]
ST_CASES = [(route, "fp16", shape, None, False, bias) for route in ("p8_8", "p8_10", "st_ld") for shape in _shapes(route)
            for bias in (True, False)]
CASES = RES_CASES + ST_CASES


def _id(case):
    route, prec, shape, drop, ln, bias = case
    return "-".join([route, prec, shape] + ([drop, "ln" if ln else "plain"] if drop else []) + ["bias" if bias else "nobias"])


def _epi(route):
    from tim_amd import _lib as L
    return L.EPI_DROP_RES_F32 if route.startswith("res") else L.EPI_STORE_T


# ---- the child: every case once, with the knobs of its environment -------------------------------------------------------------
def _run_case(case):
    from tests import gemm_ref as G
    from tests.test_gpu_gemm_edges import _launch
    from tim_amd import _lib as L

    route, prec, shape, drop, ln, bias = case
    M, N, K = SHAPES[shape]
    epi = _epi(route)
    for k in ("GEMM_PP_MIN_TILES", "GEMM_TMW", "GEMM_P8"):
        os.environ.pop("TIMHIP_" + k, None)
    os.environ.update({"TIMHIP_" + k: str(v) for k, v in ROUTES[route].items()})
    L.reload_env()
    if route.startswith("p8"):
        assert L.load().timhip_gemm_p8_choice(epi, M, N, K) == ROUTES[route]["GEMM_P8"]
    kw = {}
    if drop == "philox":   # (keep: what make_case asks for wherever p > 0; only a reference would read it)
        kw = dict(p=P, keep=torch.ones((1, 1), dtype=torch.uint8, device=DEV))
    c = G.make_case(epi, M, N, K, prec, device=DEV, seed=7, acc_scale=None if bias else -1.0, ln=ln, **kw)
    g = torch.Generator(device=DEV).manual_seed(101)
    a = torch.randn(M, K, generator=g, device=DEV)
    a[::16] = 0
    c.Abuf[:, :K] = a.to(c.T)
    if not bias:
        c.bias_buf = None
        if epi == L.EPI_DROP_RES_F32 and not ln:
            c.res[::16] = -0.0
    assert c.mask is None and (c.ln is not None) == ln
    _launch(c)
    torch.cuda.synchronize()
    words = torch.int32 if epi == L.EPI_DROP_RES_F32 else torch.int16
    out = c.out0_whole.view(words).cpu()
    if not bias and not ln:      # -0 stays -0: no bias is + (-0), and (-0) + (-0) k = -0 for a kept and for a dropped element
        zero = out[2:2 + M][::16, :N]
        assert bool((zero == (-2 ** 31 if words == torch.int32 else -2 ** 15)).all()), "a -0 accumulator did not stay -0"
    return out


def _child(path):
    torch.save({_id(case): _run_case(case) for case in CASES}, path)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    d = tmp_path_factory.mktemp("epi_wt")
    got = {}
    for v in ("0", "1"):
        path = str(d / ("knob%s.pt" % v))
        env = dict(os.environ, TIMHIP_EPI_WT=v)
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_epilogue_wt", path], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, "TIMHIP_EPI_WT=%s: %s" % (v, r.stderr[-3000:])
        got[v] = torch.load(path)
    return got


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    from tests.test_gemm_plan import _compile
    return _compile(tmp_path_factory.mktemp("epi_wt_plan") / "gemm_plan_print")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_route(route, prec, printer):
    """which kernel each case reaches"""
    from tests.test_gemm_plan import _ask, _nt
    from tim_amd import _lib as L
    for shape in _shapes(route):
        M, N, K = SHAPES[shape]
        plan = _ask(printer, [_nt(L.PRECISIONS[prec], _epi(route), M, N, K, **ROUTES[route])])[0]
        assert {k: plan[k] for k in WANT[route]} == WANT[route], (shape, plan)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_output_bit_for_bit(case, arms):
    a, b = arms["0"][_id(case)], arms["1"][_id(case)]
    assert a.shape == b.shape and a.dtype == b.dtype
    diff = a != b
    assert not bool(diff.any()), "%d words differ between TIMHIP_EPI_WT=0 and 1, first at %s" % (int(diff.sum()), diff.nonzero()[0].tolist())
    assert bool((a != a[0, 0]).any())     # the outputs were written (the guard value is not all there is)


if __name__ == "__main__":
    _child(sys.argv[1])
