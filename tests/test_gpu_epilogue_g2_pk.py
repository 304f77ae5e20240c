"""The pair form of the GELU_DROP_G2 epilogue on the eight-phase NT kernel (TIMHIP_EPI_G2_PK=1, the default: whole wave tiles
with keep-bits or without dropout run gemm_pp.hip: pp_epilogue_g2pk on gelu_both_f2) against the form it replaces
(TIMHIP_EPI_G2_PK=0: pp_epilogue -> epi_oct on gelu_both_f), BIT FOR BIT: both outputs - out0 = gelu(x) keep, out1 = gelu'(x)
keep - with their guard rows and pad columns, as raw 16-bit words.

The knob selects a template instance in the launcher.  Each value gets its own child process (`python -m` of this module with
the knob in its environment, so the library reads it the way a product run does); a child runs every case below once and
saves the outputs, the tests compare the two files.  Two children for the whole module: a test is a compare.

Route: TIMHIP_GEMM_PP_MIN_TILES=1 TIMHIP_GEMM_P8=10 as tests/test_gpu_gemm_edges.py::test_p8_routes forces it - the 320 x 256
tile for every shape the one-block-per-CU kernels can take.  They take M >= 1280, N >= 512, and the eight-phase kernel N % 256
== 0 and K >= 128 only (gemm_plan.h: gemm_pp_wins, gemm_p8_tm), so the two shapes the change was specified with cannot reach it
under any knob.  They stay, on the kernel the plan gives them, which the knob must not touch (asserted: not p8, the same bits),
and the smallest shapes with the same properties that DO run the eight-phase kernel stand beside them:
    320 x 256 x 128     as specified: one full tile                          -> the two-blocks-per-CU kernel
    333 x 264 x 64      as specified: ragged rows and columns, one step      -> the two-blocks-per-CU kernel
    1280 x 512 x 128    4 x 2 full tiles: every wave on the pair form
    1293 x 512 x 128    a fifth row tile with 13 live rows: its waves keep epi_oct while the other tiles' take the pair form -
                        the two paths meet in one launch (an edge COLUMN tile does not exist on this kernel: N % 256 == 0)
The last two are asserted to be p8 / tm = 10 by the plan printer here and by timhip_gemm_p8_choice in the children.

Inputs: A's rows are randn scaled by 0 .. 3.5 in row order (B randn K^-1/2), so |x| runs from 0 past 6 in every row tile
(asserted per case: every unit bin of |x| in [0, 6) and |x| >= 6 are populated); every 16th row of A is zero, so x is the
bias there, or +0 without one.  The cases without a bias run with acc_scale = -1, which turns those accumulators into -0:
gelu(-0) = -0 and -0 * keep = -0 for a kept and for a dropped element (a select instead of the product, or a bias of +0
where there is none, would store +0).  Asserted: out0 is the word 0x8000 in all of those rows.
Dropout: keep-bits of timhip_dropout_mask at p = 0.1 handed over as TimEpi.mask bytes, and p = 0 (thr = 0)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
P, SEED, SITE = 0.1, 1234567, 42
ROUTE = dict(GEMM_PP_MIN_TILES=1, GEMM_P8=10)
SHAPES = {"tile": (320, 256, 128), "ragged": (333, 264, 64), "p8full": (1280, 512, 128), "p8rows": (1293, 512, 128)}
CASES = [(prec, shape, drop, bias) for prec in ("fp16", "bf16") for shape in SHAPES for drop in ("bits", "thr0") for bias in (True, False)]


def _id(case):
    prec, shape, drop, bias = case
    return "%s-%s-%s-%s" % (prec, shape, drop, "bias" if bias else "nobias")


# ---- the child: every case once, with the knobs of its environment -------------------------------------------------------------
def _run_case(case):
    from tests import gemm_ref as G
    from tests.test_gpu_gemm_edges import _launch
    from tim_amd import _lib as L

    prec, shape, drop, bias = case
    M, N, K = SHAPES[shape]
    epi = L.EPI_GELU_DROP_G2
    if shape.startswith("p8"):
        assert L.load().timhip_gemm_p8_choice(epi, M, N, K) == 10
    kw = {}
    if drop == "bits":
        keep = torch.empty((M, N), dtype=torch.uint8, device=DEV)
        L.call("timhip_dropout_mask", SEED, SITE, P, M, N, L.ptr(keep), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        kw = dict(p=P, keep=keep, mask_bits=True)
    c = G.make_case(epi, M, N, K, prec, device=DEV, seed=5, acc_scale=None if bias else -1.0, **kw)
    g = torch.Generator(device=DEV).manual_seed(99)
    a = torch.randn(M, K, generator=g, device=DEV) * torch.linspace(0.0, 3.5, M, device=DEV)[:, None]
    a[::16] = 0
    b = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5
    c.Abuf[:, :K] = a.to(c.T)
    c.Bbuf[:, :K] = b.to(c.T)
    if bias:
        c.bias_buf[:N] = torch.randn(N, generator=g, device=DEV) * 0.5
    else:
        c.bias_buf = None
    x = c.Abuf[:, :K].double() @ c.Bbuf[:, :K].double().T
    x = x + c.bias_buf[:N].double() if bias else -x
    hist = torch.histc(x.abs().float().clamp(max=6.5), bins=7, min=0.0, max=7.0)
    assert bool((hist > 0).all()), ("|x| does not cover 0 .. 6 and beyond", hist.tolist())
    assert (c.mask is not None) == (drop == "bits")
    _launch(c)
    torch.cuda.synchronize()
    out = {k: getattr(c, k).view(torch.int16).cpu() for k in ("out0_whole", "out1_whole")}
    if not bias:      # gelu(-0) * scale and gelu(-0) * (+0) are both -0
        assert bool((out["out0_whole"][2:2 + M][::16, :N] == -32768).all()), "gelu(-0) * keep is not -0 everywhere"
    return out


def _child(path):
    torch.save({_id(case): _run_case(case) for case in CASES}, path)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    d = tmp_path_factory.mktemp("g2pk")
    got = {}
    for v in ("0", "1"):
        path = str(d / ("knob%s.pt" % v))
        env = dict(os.environ, TIMHIP_EPI_G2_PK=v, **{"TIMHIP_" + k: str(w) for k, w in ROUTE.items()})
        r = subprocess.run([sys.executable, "-m", "tests.test_gpu_epilogue_g2_pk", path], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, "TIMHIP_EPI_G2_PK=%s: %s" % (v, r.stderr[-3000:])
        got[v] = torch.load(path)
    return got


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    from tests.test_gemm_plan import _compile
    return _compile(tmp_path_factory.mktemp("g2pk_plan") / "gemm_plan_print")


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_route(prec, shape, printer):
    from tests.test_gemm_plan import _ask, _nt
    from tim_amd import _lib as L
    M, N, K = SHAPES[shape]
    plan = _ask(printer, [_nt(L.PRECISIONS[prec], L.EPI_GELU_DROP_G2, M, N, K, **ROUTE)])[0]
    if not shape.startswith("p8"):
        assert plan["family"] != "p8", plan
    else:
        assert (plan["family"], plan["tm"], plan["bm"]) == ("p8", 10, 320), plan


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_both_outputs_bit_for_bit(case, arms):
    a, b = arms["0"][_id(case)], arms["1"][_id(case)]
    for k in ("out0_whole", "out1_whole"):
        diff = a[k] != b[k]
        assert not bool(diff.any()), "%s: %d words differ between TIMHIP_EPI_G2_PK=0 and 1, first at %s" % (
            k, int(diff.sum()), diff.nonzero()[0].tolist())


if __name__ == "__main__":
    _child(sys.argv[1])
