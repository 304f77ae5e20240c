"""CPU test of the GEMM checker itself (tests/gemm_ref.py): an fp32 emulation of a correct kernel - fp32 matmul of the rounded
operands, the epilogue in fp32, every buffer addressed through its own pitch - is accepted for every epilogue and both 16-bit
types and uses under half of the elementwise bound; each of a list of subtly wrong kernels is rejected; and three of them are
shown to pass the max-norm check `tol()` of tests/test_gpu_kernels.py, which is what the elementwise bound adds."""
import math

import pytest
import torch

from tests import gemm_ref as G
from tim_amd import _lib as L

SHAPES = [(1283, 516, 192), (333, 136, 64)]
H16 = ["bf16", "fp16"]
TOL = {"bf16": 4e-3, "fp16": 6e-4}       # tests/test_gpu_kernels.py: tol(), quadrupled as _check_layer_gemm_epilogues takes it
P = 0.3


def _keep(M, N, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, N, generator=g) >= P).to(torch.uint8)


def _case(epi, M, N, K, dtype, **kw):
    if epi in G.HAS_DROPOUT and "p" not in kw:
        kw.update(p=P, keep=_keep(M, N), mask_bits=epi == L.EPI_GELU_DROP_G2)
    return G.make_case(epi, M, N, K, dtype, **kw)


def _read(whole, ld, M, N):
    """[M, N] read from the flat buffer at row pitch ld, from the view's first element on (a wrong pitch reads wrong elements)"""
    base = 2 * whole.shape[1]
    idx = base + torch.arange(M)[:, None] * ld + torch.arange(N)[None, :]
    return whole.reshape(-1)[idx.clamp(max=whole.numel() - 1)]


def _write(whole, ld, vals):
    M, N = vals.shape
    base = 2 * whole.shape[1]
    idx = base + torch.arange(M)[:, None] * ld + torch.arange(N)[None, :]
    ok = idx < whole.numel()
    whole.view(-1)[idx[ok]] = vals.to(whole.dtype)[ok]


def _gelu32(v):
    return 0.5 * v * (1 + torch.erf(v * (1 / math.sqrt(2.0))))


def _dgelu32(v):
    return 0.5 * (1 + torch.erf(v * (1 / math.sqrt(2.0)))) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327


def emulate(c, mut=None):
    """what a correct kernel computes, in fp32; `mut` names one deliberate mistake"""
    M, N, epi, f32 = c.M, c.N, c.epi, torch.float32
    A = c.Abuf[:, :c.kw or c.Kp].float()
    if c.a_wrap:
        A = torch.cat([A, A], 1)
    B = c.Bbuf[:, :c.Kp].float()
    acc = A @ B.t()
    if mut == "last_k_small_row":
        r = int(c.ops.row_scale.argmin())
        acc[r] -= A[r, c.K - 1] * B[:, c.K - 1]
    if mut == "step_in_block":       # one 64-deep contraction step of one 16 x 16 block
        k0 = c.Kp - 64
        acc[32:48, 64:80] -= A[32:48, k0:k0 + 64] @ B[64:80, k0:k0 + 64].t()
    s = torch.ones((), dtype=f32) if c.sc_buf is None else c.sc_buf[0]
    x = acc * s
    v = x
    if c.bias_buf is not None:
        bias = c.bias_buf[:N]
        if mut == "bias_next_col":
            bias = bias.roll(-1)
        v = (acc + bias) * s if mut == "scale_after_bias" else x + bias
    k = None
    if c.p > 0:
        scale = torch.tensor(1.0, dtype=f32) / (torch.tensor(1.0, dtype=f32) - torch.tensor(c.p, dtype=f32))
        if mut == "no_keep_scale":
            scale = torch.tensor(1.0, dtype=f32)
        if c.mask is not None:
            ldm = (N + 7) // 8 if mut == "mask_pitch" else c.ldmask
            base = 2 * c.mask_whole.shape[1]
            idx = base + torch.arange(M)[:, None] * ldm + (torch.arange(N) // 8)[None, :]
            keep = (c.mask_whole.view(-1)[idx].to(torch.int32) >> (torch.arange(N) % 8).to(torch.int32)[None, :]) & 1
        else:
            keep = c.keep
        k = keep.float() * scale
    k1 = k if k is not None else torch.ones((), dtype=f32)
    res = aux = None
    if c.res is not None:
        res = _read(c.res_whole, c.ld0 if mut == "res_pitch" else c.ldres, M, N)
    if c.aux is not None:
        aux = _read(c.aux_whole, c.ld1 if mut == "aux_pitch" else c.ldaux, M, N).float()
    out1 = None
    if epi in (L.EPI_STORE_T, L.EPI_STORE_F32):
        out0 = v
        if mut == "double_round":
            out0 = v.to(c.T).float()
    elif epi == L.EPI_RELU_T:
        out0 = v.clamp(min=0)
    elif epi == L.EPI_GELU_DROP_T2:
        out0, out1 = _gelu32(v) * k1, v
    elif epi == L.EPI_GELU_DROP_G2:
        out0, out1 = _gelu32(v) * k1, _dgelu32(v) * k1
    elif epi == L.EPI_GELU_T:
        out0 = _gelu32(v)
    elif epi == L.EPI_DROP_RES_F32:
        r = res
        if c.ln is not None:
            r = (res - c.ln.stats[:, 0:1]) * c.ln.stats[:, 1:2] * c.ln.w + c.ln.b
        out0 = r + v * k1
    elif epi == L.EPI_ADD_F32:
        out0 = x + res
    elif epi == L.EPI_DGELU_T:
        out0 = x * k1 * _dgelu32(aux)
    elif epi in (L.EPI_DRELU_T, L.EPI_DRELU_F32IN_T):
        out0 = torch.where(aux > 0, x, torch.zeros_like(x))
    elif epi == L.EPI_ATOMIC_F32:
        out0 = c.out0[:, :N] + x
    elif epi == L.EPI_SIGMOID_F32:
        out0 = 1 / (1 + torch.exp(-v))
    elif epi == L.EPI_MULAUX_T:
        out0 = x * aux
    elif epi == L.EPI_RELU_SPLIT3_T:
        r = v.clamp(min=0)
        hi = r.to(c.T)
        for blk, val in ((0, hi), (1, (r - hi.float()).to(c.T)), (2, hi)):
            c.out0[:, blk * c.ld1:blk * c.ld1 + N] = val
        return
    if mut == "col_past_n":          # a store one column past N, made before the row below gets its own values
        c.out0_whole.view(-1)[2 * c.ld0 + 7 * c.ld0 + N] = 1.0
    _write(c.out0_whole, c.ld0, out0)
    if out1 is not None:
        _write(c.out1_whole, c.ld0 if mut == "out1_pitch" else c.ld1, out1)
    if mut == "guard_row":
        c.out0_whole[1, 3] = 1.0
    if mut == "pad_col":
        c.out0_whole[2 + 5, N] = 1.0


def _run(c, mut=None):
    before = G.snapshot(c)
    emulate(c, mut)
    return before


def _rejected(c, mut):
    before = _run(c, mut)
    try:
        G.verify(c, before)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_checker_accepts_the_fp32_emulation_within_half_of_the_bound(M, N, K, dtype):
    worst = 0.0
    for epi in G.ALL_EPI:
        variants = [dict()]
        if epi == L.EPI_DROP_RES_F32:
            variants += [dict(ln=True), dict(p=0.0)]
        if epi == L.EPI_ADD_F32:
            variants.append(dict(acc_scale=0.25))
        if epi == L.EPI_GELU_DROP_G2:
            variants.append(dict(p=P, keep=_keep(M, N), mask_bits=False))
        for kw in variants:
            c = _case(epi, M, N, K, dtype, **kw)
            share = G.verify(c, _run(c))
            assert share < 0.5, (epi, kw, share)
            worst = max(worst, share)
    print("largest used share of the bound, %s (%d, %d, %d): %.3f" % (dtype, M, N, K, worst))


@pytest.mark.parametrize("dtype", H16)
def test_checker_accepts_the_wrapped_a_operand(dtype):
    c = _case(L.EPI_STORE_F32, 333, 136, 256, dtype, a_wrap=True)
    assert G.verify(c, _run(c)) < 0.5
    c = _case(L.EPI_STORE_F32, 333, 136, 256, dtype, a_wrap=True)
    c.a_wrap = False                  # a kernel that read A once: the reference of [A | A] B^T must not accept A B_hi^T ...
    c.Kp, kp = 128, c.Kp
    before = _run(c)
    c.a_wrap, c.Kp = True, kp
    with pytest.raises(AssertionError):
        G.verify(c, before)


# (mutation, epilogue, extra arguments of the case, the types for which the tol() max-norm check of test_gpu_kernels.py must ACCEPT
#  it; the neighbouring bias is let through with bf16 only: fp16's 6e-4 of max|ref| is just below the largest bias step here)
MUTATIONS = [
    ("bias_next_col", L.EPI_STORE_F32, {}, ("bf16",)),
    ("res_pitch", L.EPI_DROP_RES_F32, {}, None),
    ("out1_pitch", L.EPI_GELU_DROP_G2, {}, None),
    ("aux_pitch", L.EPI_MULAUX_T, {}, None),
    ("last_k_small_row", L.EPI_STORE_F32, {}, H16),
    ("step_in_block", L.EPI_STORE_T, {}, None),
    ("double_round", L.EPI_STORE_F32, {}, H16),
    ("scale_after_bias", L.EPI_STORE_F32, dict(acc_scale=0.25), None),
    ("no_keep_scale", L.EPI_DROP_RES_F32, {}, None),
    ("mask_pitch", L.EPI_GELU_DROP_G2, {}, None),
    ("guard_row", L.EPI_STORE_T, {}, None),
    ("pad_col", L.EPI_STORE_F32, {}, None),
    ("col_past_n", L.EPI_STORE_F32, {}, None),
]


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("mut,epi,kw,maxnorm_accepts", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_checker_rejects_a_subtly_wrong_kernel(mut, epi, kw, maxnorm_accepts, dtype):
    M, N, K = SHAPES[0]
    c = _case(epi, M, N, K, dtype, **kw)
    assert G.verify(c, _run(c)) < 0.5            # the same case, unmutated, is accepted
    c = _case(epi, M, N, K, dtype, **kw)
    assert _rejected(c, mut), mut
    if maxnorm_accepts and dtype in maxnorm_accepts:
        assert G.max_norm_accepts(c, TOL[dtype]), "the max-norm check was expected to let this one through"


@pytest.mark.parametrize("dtype", H16)
def test_a_store_past_n_hides_in_the_next_row_unless_the_pitch_is_padded(dtype):
    """why every output pitch of the GPU tests is larger than N: with ld0 = N the stray store lands on element 0 of the next row
    and that row's own store covers it; with ld0 > N it lands in a pad column"""
    M, N, K = SHAPES[1]
    c = _case(L.EPI_STORE_F32, M, N, K, dtype, pitches=dict(ld0=N))
    assert not _rejected(c, "col_past_n")
    c = _case(L.EPI_STORE_F32, M, N, K, dtype)
    assert c.ld0 > N and _rejected(c, "col_past_n")


@pytest.mark.parametrize("dtype", H16)
def test_wgrad_reference_accepts_an_fp32_emulation_and_rejects_a_dropped_row(dtype):
    M, Nout, Kout = 523, 200, 72
    o = G.operands(M, Nout, Kout, dtype, 3)
    dY, X = o.res * 0.25, G.operands(M, Kout, 8, dtype, 4).aux
    dY = dY.to(G.OP_DTYPE[dtype]).double()
    base = torch.full((Nout, Kout), 0.5, dtype=torch.float64)
    (w, bw), (b, bb) = G.wgrad_reference(dY, X, 2, base, torch.full((Nout,), 0.5, dtype=torch.float64))
    got_w = (0.5 + dY.float().t() @ X.float()).double()
    got_b = (0.5 + dY.float().sum(0)).double()
    assert G.share_of_bound(got_w, w, bw) < 0.5 and G.share_of_bound(got_b, b, bb) < 0.5
    r = int((dY.abs().sum(1) * X.abs().sum(1)).argmin())       # the row that matters least
    bad = (0.5 + dY.float().t() @ X.float() - dY[r].float()[:, None] * X[r].float()[None, :]).double()
    assert G.share_of_bound(bad, w, bw) > 1.0
