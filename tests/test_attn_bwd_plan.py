"""CPU-only: the LDS plan of the co-resident fused attention backward (tim_amd/csrc/attn_bwd_plan.h, the helper its launcher
uses), asked through a small stand-alone program (tests/attn_bwd_plan_print.cpp).  Two blocks share the 160 KiB of a CU only
if each takes at most 80 KiB = 81 920 bytes: that figure is pinned for the product geometry (S = 155, F = 100), for a window
without padded keys (160, 128) and for an F that is no multiple of 8 (133, 97), together with the layout the kernel assumes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tim_amd", "csrc")
PINNED = [(155, 100), (160, 128), (133, 97)]


def _compile(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                           os.path.join(ROOT, "tests", "attn_bwd_plan_print.cpp"), "-o", str(out)])
    return str(out)


def _ask(exe, shapes):
    out = subprocess.run([exe], input="".join("%d %d %d\n" % s for s in shapes), text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    rows = [dict((k, int(v)) for k, v in (f.split("=") for f in r.split())) for r in out.stdout.splitlines()]
    assert len(rows) == len(shapes)
    return rows


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("attn_bwd_plan") / "attn_bwd_plan_print")


@pytest.mark.parametrize("S,F", PINNED)
def test_two_blocks_fit_a_cu(printer, S, F):
    p, = _ask(printer, [(S, F, 128)])
    assert p["fits"] == 1
    assert p["lds"] <= 81920
    # every row the reads of the last key block touch exists: fragment rows 96 + 31 and transposing rows 96 + 16 + 4 + 3 + 8
    assert p["kv_rows"] >= max(96 + 31, 96 + 16 + 4 + 3 + 8) + 1 and p["kv_rows"] >= F
    assert p["sweeps"] == (S + 31) // 32 <= 5
    # K | V | dS | P~ back to back, each sweep tile 32 rows of 128 16-bit keys, nothing behind them
    assert p["k_off"] == 0 and p["v_off"] == p["kv_rows"] * 256 and p["ds_off"] == 2 * p["kv_rows"] * 256
    assert p["pt_off"] == p["ds_off"] + 32 * 256 and p["lds"] == p["pt_off"] + 32 * 256


def test_shapes_the_form_does_not_serve(printer):
    """S in (160, 192], other head widths and other key-block counts keep their routes"""
    rows = _ask(printer, [(176, 128, 128), (161, 100, 128), (155, 100, 64), (155, 96, 128), (155, 129, 128), (160, 100, 128), (97, 97, 128)])
    assert [r["fits"] for r in rows] == [0, 0, 0, 0, 0, 1, 1]


def test_plan_header_is_plain_cpp_and_clean_under_sanitizers(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                           os.path.join(CSRC, "attn_bwd_plan.h"), os.devnull])
    src = open(os.path.join(CSRC, "attn_bwd_plan.h")).read()
    assert "#include <hip" not in src and "__device__" not in src and "getenv" not in src
    exe = _compile(tmp_path / "attn_bwd_plan_print_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert all(r["lds"] <= 81920 for r in _ask(exe, [(S, F, 128) for S, F in PINNED]))
