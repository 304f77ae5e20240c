"""timhip_attention_query_fwd on a real MI355X: query rows against keys and values kept elsewhere, held bit for bit against the
query rows of the full kernel it shares its body with (csrc/attention.h).  No tolerance anywhere in this file.

The 16-bit precisions compare with timhip_attention_fwd as it runs.  fp32 / bf16x3 take the fp32-arithmetic kernel here (the
exact-fp32 matrix-core kernels are not shared), so there the full call runs that family's full kernel
(TIMHIP_DESC_ATTN_FP32) - "bit-equal to that family's full kernel"."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import DEV  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd.functional import Runtime  # noqa: E402

PRECS = ["fp16", "bf16", "fp32", "bf16x3"]
SHAPES = [(3, 155, 100, 8, 128),   # four key blocks, padded keys, Q = 55
          (2, 161, 128, 2, 128),   # no padded key, Q = 33: second row block nearly empty
          (2, 151, 150, 2, 128),   # five key blocks (the non-prefetching form), Q = 1
          (2, 499, 100, 8, 128),   # row split across workgroups
          (4, 80, 50, 2, 64),      # Dh = 64
          (2, 40, 12, 2, 32),      # Dh = 32
          (2, 30, 12, 3, 16)]      # no matrix-core instance, plain kernel
GUARD, SENTINEL = 64, -3.0


def st():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def bits(t):
    return t.contiguous().view(torch.uint8)


def full_attention(rt, qkv, B, S, F, H, E):
    """o [B, S, E] of timhip_attention_fwd (fp32-storage modes: the fp32-arithmetic family, see the module docstring)"""
    flags = 0 if rt.h16 else L.DESC_ATTN_FP32
    desc = L.TimDesc(B, S, F, E // 2, E, H, 4 * E, rt.prec, 0.0, 0, 0, flags)
    o = torch.zeros((B * S, E), dtype=rt.op_dtype, device=DEV)
    L.call("timhip_attention_fwd", C.byref(desc), L.ptr(qkv), L.ptr(o), None, st())
    return o.view(B, S, E)


def query_attention(rt, qkv_q, kv_ptr, ldkv, wrows, W, widx, G, Q, F, H, E, expect=0):
    """-> (o [G, Q, E], the guard rows in front, the guard rows behind)"""
    desc = L.TimDesc(G, Q, F, E // 2, E, H, 4 * E, rt.prec, 0.0, 0, 0, 0)
    buf = torch.full((G * Q + 2 * GUARD, E), SENTINEL, dtype=rt.op_dtype, device=DEV)
    o = buf[GUARD:GUARD + G * Q]
    rc = L.load().timhip_attention_query_fwd(C.byref(desc), L.ptr(qkv_q), kv_ptr, ldkv, wrows, W, L.ptr(widx), L.ptr(o), st())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return o.view(G, Q, E), buf[:GUARD], buf[GUARD + G * Q:]


def untouched(*guards):
    return all(bool((g == SENTINEL).all()) for g in guards)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,S,F,H,Dh", SHAPES)
def test_query_rows_are_the_full_kernels_query_rows(prec, B, S, F, H, Dh):
    rt = Runtime(prec)
    E, Q, ts = H * Dh, S - F, torch.empty(0, dtype=rt.op_dtype).element_size()
    qkv = rnd(B * S, 3 * E, seed=5).to(DEV).to(rt.op_dtype)
    want = full_attention(rt, qkv, B, S, F, H, E)[:, F:]
    qkv_q = qkv.view(B, S, 3 * E)[:, F:].reshape(B * Q, 3 * E).contiguous()
    # keys and values read in place from the full qkv
    o, g0, g1 = query_attention(rt, qkv_q, qkv.data_ptr() + E * ts, 3 * E, S, B, None, B, Q, F, H, E)
    assert torch.equal(bits(o), bits(want))
    assert untouched(g0, g1)
    # ... and from the compact [W F, 2E] layout the stack's cache has
    kv = qkv.view(B, S, 3 * E)[:, :F, E:].reshape(B * F, 2 * E).contiguous()
    o, g0, g1 = query_attention(rt, qkv_q, kv.data_ptr(), 2 * E, F, B, None, B, Q, F, H, E)
    assert torch.equal(bits(o), bits(want))
    assert untouched(g0, g1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,F,H,Dh", [(155, 100, 8, 128), (30, 12, 3, 16)])
def test_window_index_picks_the_window(prec, S, F, H, Dh):
    """W = 3 windows, G = 7 groups: group g's rows are the full kernel's rows for (window widx[g], group g's query rows) - the
    expectation is the full kernel on, per group, an S-row qkv of that window's feature rows and the group's query rows"""
    rt = Runtime(prec)
    W, idx = 3, [2, 0, 0, 1, 2, 2, 0]
    G, E, Q = len(idx), H * Dh, S - F
    feat = rnd(W, F, 3 * E, seed=7).to(DEV).to(rt.op_dtype)
    qkv_q = rnd(G, Q, 3 * E, seed=8).to(DEV).to(rt.op_dtype)
    full = torch.cat([feat[idx], qkv_q], dim=1).reshape(G * S, 3 * E).contiguous()
    want = full_attention(rt, full, G, S, F, H, E)[:, F:]
    kv = feat[:, :, E:].reshape(W * F, 2 * E).contiguous()
    widx = torch.tensor(idx, dtype=torch.int32, device=DEV)
    o, g0, g1 = query_attention(rt, qkv_q.reshape(G * Q, 3 * E), kv.data_ptr(), 2 * E, F, W, widx, G, Q, F, H, E)
    assert torch.equal(bits(o), bits(want))
    assert untouched(g0, g1)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,F,H,Dh", [(155, 100, 8, 128), (499, 100, 8, 128), (30, 12, 3, 16)])
def test_an_index_past_the_last_window_gives_nan_rows(prec, S, F, H, Dh):
    """index [0, W], one past the end: group 1 is all NaN, group 0 finite and correct.  The cache tensor carries one spare window
    behind the W the call is told about, so no read could leave the allocation even without the guard."""
    rt = Runtime(prec)
    W, E, Q = 2, H * Dh, S - F
    feat = rnd(W + 1, F, 3 * E, seed=9).to(DEV).to(rt.op_dtype)
    qkv_q = rnd(2, Q, 3 * E, seed=10).to(DEV).to(rt.op_dtype)
    kv = feat[:, :, E:].reshape((W + 1) * F, 2 * E).contiguous()
    widx = torch.tensor([0, W], dtype=torch.int32, device=DEV)
    o, g0, g1 = query_attention(rt, qkv_q.reshape(2 * Q, 3 * E), kv.data_ptr(), 2 * E, F, W, widx, 2, Q, F, H, E)
    full = torch.cat([feat[:1], qkv_q[:1]], dim=1).reshape(S, 3 * E).contiguous()
    want = full_attention(rt, full, 1, S, F, H, E)[:, F:]
    assert torch.equal(bits(o[0]), bits(want[0]))
    assert bool(torch.isfinite(o[0].float()).all())
    assert bool(torch.isnan(o[1].float()).all())
    assert untouched(g0, g1)


def test_refusals_come_before_any_launch():
    rt = Runtime("fp16")
    G, Q, F, H, E, W = 4, 5, 12, 2, 64, 3
    qkv_q = torch.zeros((G * Q, 3 * E), dtype=rt.op_dtype, device=DEV)
    kv = torch.zeros((W * F, 2 * E), dtype=rt.op_dtype, device=DEV)
    o = torch.full((G * Q, E), SENTINEL, dtype=rt.op_dtype, device=DEV)
    widx = torch.zeros(G, dtype=torch.int32, device=DEV)
    lib = L.load()

    def run(p_drop=0.0, idx=widx, ldkv=2 * E, wrows=F):
        desc = L.TimDesc(G, Q, F, E // 2, E, H, 4 * E, rt.prec, p_drop, 0, 0, 0)
        return lib.timhip_attention_query_fwd(C.byref(desc), L.ptr(qkv_q), L.ptr(kv), ldkv, wrows, W, L.ptr(idx), L.ptr(o), st())
    assert run(p_drop=0.1) == L.EINVAL            # evaluation only
    assert run(idx=None) == L.EINVAL              # identity needs G == W
    assert run(ldkv=2 * E - 8) == L.EINVAL        # a row holds K and V
    assert run(wrows=F - 1) == L.EINVAL
    assert lib.timhip_attention_query_fwd(None, L.ptr(qkv_q), L.ptr(kv), 2 * E, F, W, L.ptr(widx), L.ptr(o), st()) == L.EINVAL
    torch.cuda.synchronize()
    assert untouched(o)
    assert run() == 0
