"""CPU-only: which weight-gradient kernel a group gets, with what launch geometry and workspace, from
tim_amd/csrc/wgrad_plan.h alone.  tests/gemm_plan_print.cpp (its `wgroup` / `wtn` lines) is compiled with g++ and asked for the
plans of the routing issue's table; the expected routes are derived by hand from the launchers as they were before the plan
existed (tim_wgrad_p8_wins, tim_wgrad_pp_wins, splits_for_tiles and the fall-through ladder of tim_wgrad_group_h16)."""
import os
import subprocess

import pytest

from tests.test_gemm_plan import CSRC, _ask, _compile


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("wgrad_plan") / "gemm_plan_print")


def _layer(E, FF):
    """the four products (Nout, Kout) of an encoder layer: linear2, linear1, out-projection, in-projection"""
    return [(E, FF), (FF, E), (E, E), (3 * E, E)]


L = _layer(1024, 2048)
SMALL = [(256, 512), (512, 256), (256, 256), (768, 256)]
ODD = [(200, 72), (64, 136), (130, 128)]
RAGGED_NK = [(2000, 1000), (1000, 2000), (3000, 1000)]


def _wgroup(M, shapes, lds=None, **extra):
    """lds: per item (ldy, ldx); default: the row widths"""
    lds = lds or [(n, k) for n, k in shapes]
    return " ".join(["wgroup", str(M), str(len(shapes)), *(str(v) for (n, k), (ly, lx) in zip(shapes, lds) for v in (n, k, ly, lx)),
                     *("%s=%d" % kv for kv in extra.items())])


def _wtn(M, N, K):
    return "wtn %d %d %d" % (M, N, K)


def _al(x):
    return (x + 255) // 256 * 256


LD_LDS, P8_LDS, SPLIT_LDS = 3 * 48 * 1024, 2 * 64 * 1024, 65536


def _routes():
    r = []
    ok = dict(contract="ok")
    # 1 / 2: a C2a layer: 64 + 64 + 32 + 96 = 256 loader-wave tiles of 128 x 256, one per CU; WGRAD_LD=0: the 8-wave kernel
    r.append((dict(ok, family="ld", tn=128, tk=256, tiles=256, grid_x=256, block=768, lds=LD_LDS, pf_dist=4, splits=1, ws=0,
                   tile0="0,64,128,160,256,256,256,256,256"), _wgroup(9920, L)))
    r.append((dict(ok, family="pp8w", grid_x=256, block=512, lds=LD_LDS), _wgroup(9920, L, WGRAD_LD=0)))
    r.append((dict(family="ld", pf_dist=2), _wgroup(9920, L, WGRAD_PF=2)))
    # 3 - 6: a C2a pair: 256 eight-phase tiles of 256 x 256, and what the A/B switches leave of it
    r.append((dict(ok, family="p8", tn=256, tk=256, tiles=256, grid_x=256, block=512, lds=P8_LDS, phases=2, ragged=0, pf_dist=0, splits=1, ws=0,
                   tile0="0,32,64,80,128,160,192,208,256"), _wgroup(9920, L + L)))
    r.append((dict(family="p8", phases=4, grid_x=256, block=512, lds=P8_LDS), _wgroup(9920, L + L, WGRAD_P8_PH=4)))
    r.append((dict(family="ld", tiles=512, grid_x=512, block=768, lds=LD_LDS), _wgroup(9920, L + L, WGRAD_P8=0)))
    r.append((dict(family="split", tn=128, tk=128, tiles=1024, grid_x=1024, block=256, lds=SPLIT_LDS, splits=1, steps_per_split=155, ws=0),
              _wgroup(9920, L + L, WGRAD_P8=0, WGRAD_PP=0)))
    # 7: the ragged instance: C4's M = 7984 = 124 x 64 + 48, and the smallest ragged / whole contraction the kernel is taken for
    r.append((dict(family="p8", ragged=1, phases=2, grid_x=256), _wgroup(7984, L + L)))
    r.append((dict(family="p8", ragged=1, grid_x=256), _wgroup(2051, L + L)))
    r.append((dict(family="p8", ragged=0, tiles=256, grid_x=256), _wgroup(2048, [(1024, 2048)] * 8)))
    # 8: M < 2048: no tiled family (1024 tiles of 128 x 128, 32 steps: not split); a layer alone is half a round of eight-phase tiles
    r.append((dict(family="split", tiles=1024, grid_x=1024, splits=1), _wgroup(2047, L + L)))
    # 9: other layer widths
    r.append((dict(family="p8", tiles=512, grid_x=512, ragged=0), _wgroup(9920, _layer(2048, 4096))))   # two full rounds
    r.append((dict(family="ld", tiles=216, grid_x=216), _wgroup(9920, _layer(768, 3072))))               # 768 % 256 != 0
    r.append((dict(family="split", tiles=128, grid_x=512, splits=4, steps_per_split=39,                  # 64 tiled tiles < 192
                   ws=_al(4 * 2097152 * 4) + _al(4 * 3584 * 4), db_off=_al(4 * 2097152 * 4)), _wgroup(9920, _layer(512, 1024))))
    # 10: ragged n / k tiles: 16 x 4 + 8 x 8 + 24 x 4 = 224 loader-wave tiles
    r.append((dict(ok, family="ld", tiles=224, grid_x=224, block=768, tile0="0,64,128,224,224,224,224,224,224"), _wgroup(2100, RAGGED_NK)))
    # 11 / 12: the split kernel
    r.append((dict(ok, family="split", tiles=32, grid_x=160, block=256, lds=SPLIT_LDS, splits=5, steps_per_split=4,
                   ws=_al(5 * 524288 * 4) + _al(5 * 1792 * 4)), _wgroup(1240, SMALL)))
    r.append((dict(ok, family="split", tiles=6, grid_x=12, splits=2, steps_per_split=5, ws=321280, db_off=_al(2 * 39744 * 4),
                   tile0="0,2,4,6,6,6,6,6,6"), _wgroup(523, ODD, lds=[(200, 72), (64, 136), (136, 128)])))   # (ld: multiples of 8)
    # (a forced count - TIMHIP_WGRAD_SPLITS of a tuning build: 20 steps in 6 splits are 5 splits of 4; the workspace is sized by the 6)
    r.append((dict(family="split", grid_x=160, splits=5, steps_per_split=4, ws=_al(6 * 524288 * 4) + _al(6 * 1792 * 4), db_off=_al(6 * 524288 * 4)),
              _wgroup(1240, SMALL, FORCE_SPLITS=6)))
    # 13: the 32-bit byte offsets of the tiled grids (M * ld * 2 < 2^32): beyond them the split kernel - every item, or one only
    r.append((dict(ok, family="split", tn=128, tiles=1024), _wgroup(700000, L + L)))
    big = [(n, k) for n, k in L + L]
    big[5] = (216488, 1024)   # 9920 x 216488 x 2 = 2^32 + 154624
    r.append((dict(ok, family="split", tiles=1024, grid_x=1024), _wgroup(9920, L + L, lds=big)))
    big[5] = (216480, 1024)   # 2^32 - 4096: still addressable
    r.append((dict(ok, family="p8", grid_x=256), _wgroup(9920, L + L, lds=big)))
    big[5], big[2] = (2048, 1024), (1024, 216488)   # the same through an ldx
    r.append((dict(ok, family="split", tiles=1024), _wgroup(9920, L + L, lds=big)))
    r.append((dict(ok, family="split", tiles=512), _wgroup(9920, L, lds=[(216488, 2048)] + L[1:])))      # the loader-wave grid as well
    return r


def _contracts():
    c = [("einval", _wgroup(9920, L + L, NULL_X=6)), ("einval", _wgroup(9920, L + L + L[:1])),            # n = 9
         ("einval", _wgroup(0, L)), ("eunsupported", _wgroup(523, [(6, 5)], lds=[(8, 8)])),               # Nout * Kout % 4
         ("eunsupported", _wgroup(9920, L[:3] + [(1026, 1023)], lds=L[:3] + [(1032, 1024)])),
         # precedence: the first item at fault decides; within an item EINVAL comes before EALIGN
         ("ealign", _wgroup(9920, L + L, NULL_X=6, ODD_DW=0)), ("einval", _wgroup(9920, L + L, NULL_X=0, ODD_DW=6)),
         ("einval", _wgroup(9920, L + L, NULL_X=3, ODD_DW=3))]
    for i in (0, 5, 7):
        c.append(("ealign", _wgroup(9920, L + L, ODD_DW=i)))
        c.append(("ealign", _wgroup(9920, L + L, lds=[(n, k + 4 * (j == i)) for j, (n, k) in enumerate(L + L)])))   # ldx % 8
        c.append(("ealign", _wgroup(9920, L + L, lds=[(n + 12 * (j == i), k) for j, (n, k) in enumerate(L + L)])))  # ldy % 8
    return c


def test_wgrad_group_routes(printer):
    """the table of the routing issue: the C2a layer and pair, the A/B switches, the ragged instance, the thresholds, other layer
    widths, the split kernel's grids and workspaces, the 32-bit limit of the tiled grids"""
    routes = _routes()
    got = _ask(printer, [call for _, call in routes])
    for (want, call), plan in zip(routes, got):
        assert {k: plan[k] for k in want} == want, call


def test_wgrad_tn_plan(printer):
    """the single product (tim_wgrad_tn_h16): splits, steps per split, grid, LDS and the workspace formula of tim_wgrad_tn_ws -
    [slab sk N K fp32][bias slab sk N fp32], each rounded up to 256 bytes, also with one split"""
    want = [(dict(family="split", tiles=8, splits=5, steps_per_split=4, grid_x=8 * 5, block=256, lds=SPLIT_LDS,
                  ws=_al(5 * 97 * 1024 * 4) + _al(5 * 97 * 4), db_off=_al(5 * 97 * 1024 * 4)), _wtn(1240, 97, 1024)),
            (dict(family="split", tiles=24, splits=16, steps_per_split=10, grid_x=24 * 16, block=256,
                  ws=_al(16 * 300 * 1024 * 4) + _al(16 * 300 * 4), db_off=_al(16 * 300 * 1024 * 4)), _wtn(9920, 300, 1024)),
            # (3 steps: never split - and still through a slab)
            (dict(tiles=1, splits=1, steps_per_split=3, grid_x=1, ws=_al(10 * 6 * 4) + _al(10 * 4), db_off=256), _wtn(130, 10, 6))]
    got = _ask(printer, [call for _, call in want])
    for (w, call), g in zip(want, got):
        assert {k: g[k] for k in w} == w, call


def test_wgrad_group_contract(printer):
    """the argument contract, one copy: a NULL pointer, n = 9 and M = 0 are EINVAL; ldx % 8, ldy % 8 or a misaligned dW on item
    0 / 5 / 7 is EALIGN for the whole group; Nout * Kout % 4 is EUNSUPPORTED; the first item at fault decides"""
    want = _contracts()
    got = _ask(printer, [call for _, call in want])
    for (rc, call), g in zip(want, got):
        assert g["contract"] == rc, call


def test_wgrad_plan_header_is_plain_cpp_and_clean_under_sanitizers(tmp_path):
    """wgrad_plan.h compiles on its own as plain C++17 (no HIP header, no device qualifier, no environment), and the printer built
    with AddressSanitizer + UBSan runs every call of the tests above without a report"""
    hdr = os.path.join(CSRC, "wgrad_plan.h")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include", hdr, os.devnull])
    code = open(hdr).read()
    assert "#include <hip" not in code and "__device__" not in code and "getenv" not in code
    exe = _compile(tmp_path / "gemm_plan_print_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    _ask(exe, [call for _, call in _routes()] + [call for _, call in _contracts()] +
         [_wtn(1240, 97, 1024), _wtn(9920, 300, 1024), _wtn(130, 10, 6), _wtn(0, 10, 6)])
