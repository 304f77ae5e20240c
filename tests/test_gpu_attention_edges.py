"""Attention forward and backward against float64 with ELEMENTWISE bounds, per kernel family (tests/attn_ref.py holds the reference,
the bounds with their derivation, the guarded cases and the case list; tests/test_attn_ref.py shows on the CPU what the checker
rejects).  Every case
  * first asserts, from the dispatch rule of tim_attention_fwd / _bwd restated in attn_ref.family_of, the kernel family, row split
    and wave count it is meant for, so that the list cannot drift out of its class.  (The test sees results, not kernel names);
  * runs the forward into NaN-prefilled, guarded o and lse, then the backward IN ISOLATION - handed o = T(reference o) and
    lse = fp32(reference lse) - into a NaN-prefilled, guarded dqkv with a NaN-filled workspace that has a guard behind it;
  * makes each call twice with the outputs re-poisoned: no attention kernel uses atomics, so the bits repeat;
  * checks lse, o and dqkv element by element against their own bounds, every element finite, every guard bit for bit.
The keep set is timhip_dropout_mask's at site 16 + 8 * layer with row pitch LP = round_up(F + 1, 8).
The fp64 work runs on the device.  Largest problem: 1 x 1 x 499 x 100 x 128."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_ref as A  # noqa: E402
from tim_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
SHARES = {}      # (pass, family, precision) -> largest used share of the (arithmetic part of the) bound


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module", autouse=True)
def shares():
    yield
    for key in sorted(SHARES):
        print("\nlargest used share of the elementwise bound, %s %-9s %-6s %.3f" % (key + (SHARES[key],)))


def _desc(cs, prec):
    E = cs.H * cs.Dh
    return L.TimDesc(cs.B, cs.S, cs.F, E // 2, E, cs.H, 4 * E, L.PRECISIONS[prec], cs.p, A.SEED, A.LAYER, L.DESC_ATTN_FP32 if cs.fp32 else 0)


def _keep_set(cs):
    if cs.p == 0:
        return None
    rows, LP = cs.B * cs.H * cs.S, A._ru(cs.F + 1, 8)
    keep = torch.empty((rows, LP), dtype=torch.uint8, device=DEV)
    L.call("timhip_dropout_mask", A.SEED, A.SITE, cs.p, rows, LP, L.ptr(keep), st())
    torch.cuda.synchronize()
    return keep


def _fwd(c, desc):
    return L.load().timhip_attention_fwd(C.byref(desc), L.ptr(c.qkv), L.ptr(c.o), L.ptr(c.lse), st())


def _bwd(c, desc):
    return L.load().timhip_attention_bwd(C.byref(desc), L.ptr(c.qkv), L.ptr(c.o_in), L.ptr(c.lse_in), L.ptr(c.dO_buf), L.ptr(c.dqkv),
                                         L.ptr(c.ws), c.ws.numel(), st())


def _twice(c, desc, launch, names):
    """the call, twice, each time into re-poisoned outputs; asserts equal bits and leaves the second call's results in place"""
    first = None
    for _ in range(2):
        A.repoison(c)
        assert launch(c, desc) == 0
        torch.cuda.synchronize()
        got = [getattr(c, n).clone() for n in names]
        if first is None:
            first = got
    for n, a, b in zip(names, first, got):
        assert A._bits_equal(a, b), "the call does not repeat bit for bit: " + n


def _run(cs, prec, knobs, seed):
    if cs.knobs:
        knobs(**{"TIMHIP_" + k: str(v) for k, v in cs.knobs.items()})
    fam = A.expected_family(cs, prec)
    desc = _desc(cs, prec)
    c = A.make_case(prec, cs.B, cs.S, cs.F, cs.H, cs.Dh, p=cs.p, seed=seed, peaked=cs.peaked, device=DEV, keep=_keep_set(cs), fp32=cs.fp32)
    A.attach_workspace(c, max(16, int(L.load().timhip_attention_bwd_workspace_bytes(C.byref(desc)))))
    _twice(c, desc, _fwd, ("o_whole", "lse_whole"))
    share = A.verify_fwd(c, fam.fwd)
    SHARES[("fwd", fam.fwd, prec)] = max(SHARES.get(("fwd", fam.fwd, prec), 0.0), share)
    _twice(c, desc, _bwd, ("dqkv_whole",))
    share = A.verify_bwd(c, fam.bwd)
    SHARES[("bwd", fam.bwd, prec)] = max(SHARES.get(("bwd", fam.bwd, prec), 0.0), share)


def _params(group):
    return [pytest.param(cs, prec, i, id="%s-%s" % (cs.name.replace(" ", "_"), prec)) for i, cs in enumerate(A.GPU_CASES[group]) for prec in cs.precs]


@pytest.mark.parametrize("cs,prec,i", _params("table"))
def test_shape_table(cs, prec, i, knobs):
    """all ten (head width, key blocks) pairs of attn_for_shape with one real key in the last key block, one padded key and none,
    S = F + 37 (at least two row blocks, the last one ragged), p = 0 and 0.3: the 16-bit matrix-core kernels, and the f32
    matrix-core kernels for fp32 / bf16x3.  (128, 4) is the fused backward - key-split at S <= 160, plain fused above - and is
    repeated with TIMHIP_ATTN_FUSED=0 and TIMHIP_ATTN_KS=0; one `peaked` case per family"""
    _run(cs, prec, knobs, 100 + i)


@pytest.mark.parametrize("cs,prec,i", _params("split"))
def test_row_split_and_wave_walking(cs, prec, i, knobs):
    """a (window, head) spread over two, four and (TIMHIP_ATTN_SPLIT_MIN=1) three workgroups; TIMHIP_ATTN_WAVES = 1 and 2: a wave
    walks several row blocks; ten row blocks on the eight waves of the f32 kernels"""
    _run(cs, prec, knobs, 300 + i)


@pytest.mark.parametrize("cs,prec,i", _params("rows"))
def test_row_count_edges(cs, prec, i, knobs):
    """no query row at all; one query row that opens a row block; one token"""
    _run(cs, prec, knobs, 400 + i)


@pytest.mark.parametrize("cs,prec,i", _params("simple"))
def test_fp32_arithmetic_kernels(cs, prec, i, knobs):
    """what the dispatch rule leaves to attention.hip: head width 16 with three heads, (64, three key blocks), head width 80 (a
    partly filled second pass of the `c += 64` loops), the keys-per-lane edges F = 64, 65, 129 and the KPL limit 192, and a
    (128, 4) shape under TIMHIP_DESC_ATTN_FP32"""
    _run(cs, prec, knobs, 500 + i)


@pytest.mark.parametrize("prec", A.PRECS)
def test_more_than_192_feature_keys_is_unsupported_and_writes_nothing(prec):
    cs = A._case("F = 193", 2, 198, 193, 2, 16, 0.0)
    assert A.family_of(prec, dict(B=cs.B, S=cs.S, F=cs.F, H=cs.H, Dh=cs.Dh)).fwd == "unsupported"
    desc = _desc(cs, prec)
    c = A.make_case(prec, cs.B, cs.S, cs.F, cs.H, cs.Dh, seed=7, device=DEV)
    A.attach_workspace(c, 1 << 20)
    assert _fwd(c, desc) == L.EUNSUPPORTED and _bwd(c, desc) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    for n in ("o_whole", "lse_whole", "dqkv_whole"):
        assert A._bits_equal(getattr(c, n), c.poison[n]), n + " was written"
    assert bool((c.ws_whole == 0xFF).all())
