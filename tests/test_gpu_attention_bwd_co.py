"""The co-resident form of the key-split fused attention backward (TIMHIP_ATTN_BWD_CO=1: four-wave blocks of 80 KiB, two per CU,
dK / dV accumulated per 32-row sweep in registers - attention_bwd2.hip: attn_bwd_co) against float64, element by element.
Every case runs the backward IN ISOLATION (o = T(reference o), lse = fp32(reference lse), as tests/test_gpu_attention_edges.py does)
once with the knob off and once with it on, into NaN-prefilled guarded outputs.  Both runs are held to the same bounds
(tests/attn_ref.py: bwd_bounds of the 16-bit fused family) against the same reference, and that reference is built on
timhip_dropout_mask's keep set for the case's seed and site: a keep decision that differs from it in either run moves dV by a
whole p dO / (1 - p) term, far outside the bound - so the two runs' masks are that set, bit for bit.  Cases with keep-bits hand
timhip_attn_keep_bits' words to the backward as the layer backward does (timhip_attention_bwd_keep_bits); the others make the
kernels draw their own.  Shapes: the smallest at which the new form can go wrong, see CASES.  Largest: 3 x 8 x 155 x 100 x 128."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_ref as A  # noqa: E402
from tim_amd import _lib as L  # noqa: E402

DEV = "cuda:0"

#        name                                                   B  H   S    F    p    prec   keep-bits  family
CASES = [("product geometry: five sweeps, ragged last, 4 keys",  1, 2, 155, 100, 0.1, "fp16", True, "fused_ks"),
         ("the same without dropout (no Philox, no bits)",       1, 2, 155, 100, 0.0, "bf16", False, "fused_ks"),
         ("no padded keys: every K / V row is data",             1, 2, 160, 128, 0.1, "fp16", False, "fused_ks"),
         ("one query row: the self term in its own sweep",       1, 2, 101, 100, 0.1, "fp16", True, "fused_ks"),
         ("F no multiple of 8: one key in the last block",       1, 2, 133, 97, 0.1, "bf16", False, "fused_ks"),
         ("several co-resident blocks per CU",                   3, 8, 155, 100, 0.1, "fp16", True, "fused_ks"),
         ("S = 176 keeps the plain fused route",                 1, 2, 176, 128, 0.1, "fp16", False, "fused")]


def st():
    return torch.cuda.current_stream().cuda_stream


def _desc(B, S, F, H, prec, p):
    E = H * 128
    return L.TimDesc(B, S, F, E // 2, E, H, 4 * E, L.PRECISIONS[prec], p, A.SEED, A.LAYER, 0)


def _keep_set(B, S, F, H, p):
    if p == 0:
        return None
    rows, LP = B * H * S, A._ru(F + 1, 8)
    keep = torch.empty((rows, LP), dtype=torch.uint8, device=DEV)
    L.call("timhip_dropout_mask", A.SEED, A.SITE, p, rows, LP, L.ptr(keep), st())
    torch.cuda.synchronize()
    return keep


def _keep_bits(desc, rows):
    """the words of layer A.LAYER: timhip_attn_keep_bits fills the saved blocks of layers 0 .. A.LAYER"""
    nb = L.load().timhip_layer_saved_bytes(C.byref(desc))
    saved = [torch.zeros(nb, dtype=torch.uint8, device=DEV) for _ in range(A.LAYER + 1)]
    L.call("timhip_attn_keep_bits", C.byref(desc), A.LAYER + 1, (C.c_void_p * (A.LAYER + 1))(*[t.data_ptr() for t in saved]), st())
    off, nbytes = C.c_size_t(), C.c_size_t()
    L.call("timhip_layer_saved_field", C.byref(desc), L.SAVED_ATTN_KEEP_BITS, C.byref(off), C.byref(nbytes))
    assert nbytes.value == rows * 16
    words = torch.empty(rows * 16 + 64, dtype=torch.uint8, device=DEV)   # (a copy that ends where the words end)
    head = (-words.data_ptr()) % 16
    out = words[head:head + rows * 16]
    out.copy_(saved[A.LAYER][off.value:off.value + nbytes.value])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,B,H,S,F,p,prec,kb,family", [pytest.param(*cs, id="S%d-F%d-B%d-%s" % (cs[3], cs[4], cs[1], cs[6])) for cs in CASES])
def test_knob_off_and_on_against_float64(name, B, H, S, F, p, prec, kb, family, knobs):
    assert A.family_of(prec, dict(B=B, S=S, F=F, H=H, Dh=128)).bwd == family, "the case left the route it is meant for"
    desc = _desc(B, S, F, H, prec, p)
    c = A.make_case(prec, B, S, F, H, 128, p=p, seed=700 + S + F, device=DEV, keep=_keep_set(B, S, F, H, p))
    A.attach_workspace(c, max(16, int(L.load().timhip_attention_bwd_workspace_bytes(C.byref(desc)))))
    bits = _keep_bits(desc, B * H * S) if kb else None
    got = {}
    for co in ("0", "1"):
        knobs(TIMHIP_ATTN_BWD_CO=co)
        A.repoison(c)
        rc = L.load().timhip_attention_bwd_keep_bits(C.byref(desc), L.ptr(c.qkv), L.ptr(c.o_in), L.ptr(c.lse_in), L.ptr(c.dO_buf), L.ptr(c.dqkv),
                                                     L.ptr(c.ws), c.ws.numel(), L.ptr(bits), st())
        assert rc == 0
        torch.cuda.synchronize()
        share = A.verify_bwd(c, family)
        print("\n%s, TIMHIP_ATTN_BWD_CO=%s: largest used share of the elementwise bound %.3f" % (name, co, share))
        got[co] = c.dqkv_whole.clone()
    if family != "fused_ks":     # a shape the new form does not serve: the knob changes nothing
        assert A._bits_equal(got["0"], got["1"]), "TIMHIP_ATTN_BWD_CO changed the results of a shape that keeps its route"
