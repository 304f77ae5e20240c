"""CPU-only: which NT GEMM kernel a call gets and with what launch geometry, from tim_amd/csrc/gemm_plan.h alone.  A small
program (tests/gemm_plan_print.cpp: its own main, a TimKnobs with the defaults) is compiled with g++ and asked for the plans of
the C2a / detection layer shapes, the small-problem shapes and the grouped launch; the expected routes are derived by hand
from the launchers as they were before the plan existed."""
import os
import subprocess

import pytest

from tim_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tim_amd", "csrc")
BF16, X3, FP32, F16 = L.PREC_BF16, L.PREC_BF16X3, L.PREC_FP32, L.PREC_F16
ALL_EPI = range(15)
PP_EPI = (L.EPI_STORE_T, L.EPI_RELU_T, L.EPI_STORE_F32, L.EPI_DROP_RES_F32, L.EPI_ADD_F32, L.EPI_GELU_DROP_G2, L.EPI_GELU_T, L.EPI_MULAUX_T)


def _compile(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "gemm_plan_print.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_print")


def _ask(exe, lines):
    out = subprocess.run([exe], input="".join(l + "\n" for l in lines), text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    rows = [dict((k, int(v) if v.lstrip("-").isdigit() else v) for k, v in (f.split("=") for f in r.split())) for r in out.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def _nt(prec, epi, M, N, K, splitk=1, a_wrap=0, **knobs):
    return " ".join(["nt", *map(str, (prec, epi, M, N, K, splitk, a_wrap)), *("%s=%d" % kv for kv in knobs.items())])


def _p8(epi, M, N, K, **knobs):
    return " ".join(["p8", *map(str, (epi, M, N, K)), *("%s=%d" % kv for kv in knobs.items())])


def _group(epi, shapes, **knobs):
    return " ".join(["group", str(epi), str(len(shapes)), *(str(v) for mn in shapes for v in mn), *("%s=%d" % kv for kv in knobs.items())])


# (expected plan fields, call) - a field that is not named is not checked
P8_LDS = {8: 2 * (256 + 256) * 128, 10: 2 * (320 + 256) * 128}
LD_LDS = {5: 3 * (160 + 256) * 128, 4: 3 * (128 + 256) * 128}


def _h16(bm, wm, wn, nst, grid_x, grid_z=1):
    return dict(family="h16", bm=bm, bn=128, wm=wm, wn=wn, nst=nst, tpb=1, grid_x=grid_x, grid_z=grid_z, block=64 * wm * wn,
                lds=nst * (bm + 128) * 64 * 2)


def _routes():
    r = []
    # eight-phase routes (block 512)
    r.append((dict(family="p8", tm=8, bm=256, bn=256, phases=2, nst=2, grid_x=468, grid_z=1, block=512, lds=P8_LDS[8]),
              _nt(F16, L.EPI_STORE_T, 9920, 3072, 1024)))
    r.append((dict(family="p8", tm=10, bm=320, phases=2, grid_x=248, block=512, lds=P8_LDS[10]), _nt(F16, L.EPI_GELU_DROP_G2, 9920, 2048, 1024)))
    r.append((dict(family="p8", tm=10, bm=320, phases=2, grid_x=248, block=512, lds=P8_LDS[10]), _nt(BF16, L.EPI_MULAUX_T, 9920, 2048, 1024, GEMM_P8=2)))
    r.append((dict(family="p8", tm=8, phases=4, grid_x=468, block=512), _nt(F16, L.EPI_STORE_T, 9920, 3072, 1024, GEMM_P8_PH=4)))
    # one-block-per-CU routes: loader waves (block 768), 160- and 128-row tiles
    one_round = dict(family="ld", tm=5, bm=160, bn=256, nst=3, tpb=1, pf_dist=4, pf_mode=1, grid_x=248, grid_z=1, block=768, lds=LD_LDS[5])
    r.append((one_round, _nt(F16, L.EPI_STORE_T, 9920, 1024, 1024)))
    r.append((one_round, _nt(F16, L.EPI_DROP_RES_F32, 9920, 1024, 2048)))
    r.append((dict(family="ldp", tm=5, bm=160, tpb=3, pf_dist=4, grid_x=248, block=768, lds=LD_LDS[5]), _nt(F16, L.EPI_STORE_T, 9920, 3072, 1024, GEMM_P8=0)))
    # (the row tile is priced WITH the walk although TIMHIP_GEMM_LDP=0 turns the walk off: still 160 rows)
    r.append((dict(family="ld", tm=5, bm=160, tpb=1, pf_dist=0, grid_x=744, block=768, lds=LD_LDS[5]),
              _nt(F16, L.EPI_STORE_T, 9920, 3072, 1024, GEMM_P8=0, GEMM_LDP=0)))
    r.append((dict(family="ldp", tm=5, bm=160, tpb=2, pf_dist=4, grid_x=248, block=768), _nt(F16, L.EPI_MULAUX_T, 9920, 2048, 1024)))
    r.append((dict(family="ld", tm=4, bm=128, tpb=1, pf_dist=4, grid_x=252, block=768, lds=LD_LDS[4]), _nt(F16, L.EPI_STORE_T, 7984, 1024, 1024)))
    # (eight-phase refused: its tiles would fill their rounds to 0.73 and 0.58, below 0.85)
    r.append((dict(family="ldp", tm=4, bm=128, tpb=3, pf_dist=4, grid_x=252, block=768, lds=LD_LDS[4]), _nt(F16, L.EPI_STORE_T, 7984, 3072, 1024)))
    for epi in PP_EPI:   # A wraps: the 8-wave kernel, 160 rows; eight-phase refused
        r.append((dict(family="pp8w", tm=5, bm=160, bn=256, tpb=1, grid_x=248, block=512, lds=LD_LDS[5]), _nt(F16, epi, 9920, 1024, 1024, a_wrap=8)))
    # two-blocks-per-CU routes (gemm.hip)
    r.append((_h16(160, 1, 4, 2, 496), _nt(F16, L.EPI_STORE_T, 9920, 1024, 1024, GEMM_PP=0)))
    r.append((_h16(160, 1, 4, 2, 496), _nt(F16, L.EPI_DGELU_T, 9920, 1024, 1024)))   # (pp does not carry the epilogue)
    for epi in ALL_EPI:
        r.append((_h16(64, 2, 4, 4, 160), _nt(BF16, epi, 1240, 1024, 1024)))
        r.append((_h16(64, 1, 4, 4, 160), _nt(BF16, epi, 1240, 1024, 1024, GEMM_SMALL_W8=0)))
        r.append((_h16(64, 1, 4, 3, 312), _nt(F16, epi, 2480, 1024, 1024)))
        r.append((_h16(128, 2, 2, 2, 312), _nt(F16, epi, 4960, 1024, 1024)))   # (124 pp tiles < 192; the tall tile does not win)
        r.append((_h16(128, 2, 2, 2, 8), _nt(F16, epi, 64, 1024, 1024)))
        for prec, fam, ksteps in ((FP32, "f32", 8), (X3, "x3", 2)):
            r.append((dict(family=fam, bm=128, bn=128, grid_x=6, grid_z=1, block=256, lds=0, ksteps=ksteps), _nt(prec, epi, 300, 256, 128)))
    r.append((dict(_h16(64, 2, 4, 4, 10, 4), ksteps=39), _nt(F16, L.EPI_ATOMIC_F32, 300, 256, 9920, splitk=4)))
    return r


def test_gemm_nt_routes(printer):
    """the table of the routing issue: every C2a / detection layer product, the knobs that switch families, the small-problem
    tiles, split-K and the fp32 / bf16x3 kernels"""
    routes = _routes()
    got = _ask(printer, [call for _, call in routes])
    for (want, call), plan in zip(routes, got):
        assert {k: plan[k] for k in want} == want, call


def test_gemm_p8_choice(printer):
    """what timhip_gemm_p8_choice answers: the assertions of test_gemm_eight_phase_choice and of test_gemm_eight_phase_kernel
    (tests/test_gpu_kernels.py), without a GPU"""
    S, G2, MUL, DR = L.EPI_STORE_T, L.EPI_GELU_DROP_G2, L.EPI_MULAUX_T, L.EPI_DROP_RES_F32
    want = [(8, _p8(S, 9920, 3072, 1024, GEMM_P8=1)), (10, _p8(G2, 9920, 2048, 1024, GEMM_P8=1)),
            (0, _p8(MUL, 9920, 2048, 1024, GEMM_P8=1)),            # (measured: no gain with that epilogue)
            (10, _p8(MUL, 9920, 2048, 1024, GEMM_P8=2)),
            (0, _p8(S, 9920, 1024, 3072, GEMM_P8=1)), (0, _p8(S, 1240, 3072, 1024, GEMM_P8=1)),
            (0, _p8(S, 9920, 3072, 64, GEMM_P8=1)),                # one contraction step: the two-buffer prologue needs two
            (0, _p8(S, 9920, 3072, 1024, GEMM_P8=0))]
    for tm in (8, 10):   # forced: that tile for every legal shape and the three epilogues, no other epilogue
        for M, N, K in [(9920, 3072, 1024), (9920, 2048, 1024), (9925, 2048, 192), (3000, 512, 128), (7984, 3072, 1024),
                        (300, 256, 64 * 5), (13120, 1024, 2048)]:
            for ph in (4, 2):
                want += [(tm, _p8(epi, M, N, K, GEMM_P8=tm, GEMM_P8_PH=ph)) for epi in (S, G2, MUL)]
                want.append((0, _p8(DR, M, N, K, GEMM_P8=tm, GEMM_P8_PH=ph)))
    want.append((10, _p8(L.EPI_GELU_T, 9920, 2048, 1024)))   # (test_gpu_infer: GELU_T routes as GELU_DROP_G2)
    got = _ask(printer, [call for _, call in want])
    for (tm, call), g in zip(want, got):
        assert g["tm"] == tm, call


def test_gemm_group_plan(printer):
    """the grouped launch: an ADD_F32 group of at most 512 64 x 128 tiles takes 64 x 64 tiles with two stages; every other group
    64 x 128 tiles with 4 / 3 / 2 stages for up to 256 / up to 512 / more tiles"""
    t64 = lambda shapes: sum(-(-m // 64) * -(-n // 64) for m, n in shapes)
    t128 = lambda shapes: sum(-(-m // 64) * -(-n // 128) for m, n in shapes)
    heads = [(1240, 1024), (1240, 1024), (1240, 300), (1240, 97)]          # 20 x (8 + 8 + 3 + 1) = 400 tiles of 64 x 128
    edge = [(64 * 64, 128 * 8)]                                            # exactly 512
    over = [(64 * 64, 128 * 8), (1, 1)]                                    # 513
    small = [(300, 256), (300, 130)]                                       # 5 x (2 + 2) = 20
    exact256 = [(64 * 32, 128 * 8)]
    assert (t128(heads), t128(edge), t128(over), t128(small), t128(exact256)) == (400, 512, 513, 20, 256)
    w64 = lambda s: dict(bn=64, wm=2, wn=2, nst=2, tiles=t64(s), block=256, lds=2 * (64 + 64) * 64 * 2)
    w128 = lambda s, nst: dict(bn=128, wm=1, wn=4, nst=nst, tiles=t128(s), block=256, lds=nst * (64 + 128) * 64 * 2)
    want = [(w64(heads), _group(L.EPI_ADD_F32, heads)), (w64(edge), _group(L.EPI_ADD_F32, edge)), (w128(over, 2), _group(L.EPI_ADD_F32, over)),
            (w128(heads, 3), _group(L.EPI_STORE_T, heads)), (w128(edge, 3), _group(L.EPI_STORE_T, edge)), (w128(over, 2), _group(L.EPI_STORE_T, over)),
            (w128(small, 4), _group(L.EPI_STORE_T, small)), (w128(exact256, 4), _group(L.EPI_RELU_T, exact256)),
            (w128(small, 4), _group(L.EPI_STORE_F32, small)), (w128(small, 2), _group(L.EPI_STORE_T, small, GEMM_SMALL_NST=2))]
    got = _ask(printer, [call for _, call in want])
    for (w, call), g in zip(want, got):
        assert g == w, call


def test_gemm_plan_header_is_plain_cpp_and_clean_under_sanitizers(tmp_path):
    """gemm_plan.h compiles on its own as plain C++17 (no HIP header, no device qualifier, no environment), and the printer built
    with AddressSanitizer + UBSan runs every call of the tests above without a report"""
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                           os.path.join(CSRC, "gemm_plan.h"), os.devnull])
    for hdr in ("gemm_plan.h", "tim_knobs.h"):
        code = open(os.path.join(CSRC, hdr)).read()
        assert "#include <hip" not in code and "__device__" not in code and "getenv" not in code
    exe = _compile(tmp_path / "gemm_plan_print_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    calls = [call for _, call in _routes()] + [_p8(L.EPI_STORE_T, 9920, 3072, 1024), _group(L.EPI_ADD_F32, [(1240, 1024), (1240, 97)]),
                                               _group(L.EPI_STORE_T, [(64 * 64, 128 * 8), (1, 1)])]
    _ask(exe, calls)
