"""float64 references and ELEMENTWISE error bounds for the NT GEMM epilogues (include/timhip.h, TIMHIP_EPI_* 0 .. 14) and the
weight-gradient products, as pure torch functions: they work on whatever device their tensors are on (tests/test_gemm_ref.py
runs them on the CPU against an fp32 emulation and its mutations, tests/test_gpu_gemm_edges.py on the device against the
kernels - nothing large travels to the host).

A case (`make_case`) owns every buffer of one call:
  * operands: A is randn with its rows scaled by 2^randint(-6, 6), B randn K^-0.5 with rows scaled by 2^randint(-4, 4), the bias
    scaled like B's rows, res and aux randn - all rounded to the operand type, kept as fp64.  The device operand buffers have
    lda != ldb, both multiples of 64 and larger than Kp = K rounded up to 64; columns [K, Kp) are zero, as the ABI asks, columns
    [Kp, ld) are NaN: nothing may read them, and a read shows in the output.
  * outputs in guarded buffers: two rows before and two rows after, and every column at or past N, hold one NaN bit pattern and
    must come back bit for bit (`untouched`).  res, aux, the bias and the keep-bits are padded with NaN / set bits the same way.
  * every pitch is its own number, so an epilogue that indexes `res` with ld0, `out1` with ld0 or `aux` with ld1 reads or
    writes the wrong element, and with ld0 > N a store one column past N lands in a pad column instead of the next row.

The bounds are derived, not fitted.  u = 2^-23 throughout: a whole unit in the last place of fp32, which also covers an
accumulator that truncates instead of rounding to nearest.
"""
import math
from types import SimpleNamespace

import torch

from tests.test_gpu_kernels import HALF_ULP, _bits_equal  # noqa: F401  (the 16-bit rounding steps and the bit compare of _ln_edge)
from tim_amd import _lib as L

F64 = torch.float64
U = 2.0 ** -23
OP_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "bf16x3": torch.float32}
NAN_BITS = {4: 0x7FC00ABC, 2: 0x7FC5, 1: 0xFF}   # one quiet-NaN pattern per element size (uint8 buffers: all bits set)

F32_OUT = (L.EPI_STORE_F32, L.EPI_DROP_RES_F32, L.EPI_ADD_F32, L.EPI_ATOMIC_F32, L.EPI_SIGMOID_F32)
HAS_BIAS = (L.EPI_STORE_T, L.EPI_RELU_T, L.EPI_STORE_F32, L.EPI_GELU_DROP_T2, L.EPI_DROP_RES_F32, L.EPI_SIGMOID_F32,
            L.EPI_GELU_DROP_G2, L.EPI_RELU_SPLIT3_T, L.EPI_GELU_T)
HAS_RES = (L.EPI_DROP_RES_F32, L.EPI_ADD_F32)
HAS_AUX = (L.EPI_DGELU_T, L.EPI_DRELU_T, L.EPI_DRELU_F32IN_T, L.EPI_MULAUX_T)
HAS_OUT1 = (L.EPI_GELU_DROP_T2, L.EPI_GELU_DROP_G2)
HAS_DROPOUT = (L.EPI_GELU_DROP_T2, L.EPI_DROP_RES_F32, L.EPI_DGELU_T, L.EPI_GELU_DROP_G2)
ALL_EPI = tuple(range(15))


def _ru(x, m=64):
    return (x + m - 1) // m * m


def nan_filled(shape, dtype, device):
    """a buffer whose every element is the SAME NaN bit pattern (uint8: 0xFF), so `untouched` can compare bits"""
    size = torch.empty((), dtype=dtype).element_size()
    iv = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[size]
    return torch.full(shape, NAN_BITS[size], dtype=iv, device=device).view(dtype)


def guarded(rows, cols, ld, dtype, device="cpu", src=None):
    """(whole, view): rows + 4 rows of pitch ld filled with one NaN pattern; the view is rows 2 .. rows + 1.  src (optional,
    [rows, cols]) is written into the view's first `cols` columns - an input such as res / aux, or the start value of an
    accumulating output."""
    assert ld >= cols
    whole = nan_filled((rows + 4, ld), dtype, device)
    view = whole[2:2 + rows]
    if src is not None:
        view[:, :cols] = src.to(device).to(dtype)
    return whole, view


def untouched(whole, before, rows, cols):
    """bit for bit: the two guard rows on either side and every column the call does not own.  cols: N (columns at or past it
    are pad), or a bool vector over the pitch that is True where the call writes."""
    ld = whole.shape[1]
    pad = torch.arange(ld, device=whole.device) >= cols if isinstance(cols, int) else ~cols
    ok = _bits_equal(whole[:2], before[:2]) and _bits_equal(whole[2 + rows:], before[2 + rows:])
    return ok and (not bool(pad.any()) or _bits_equal(whole[2:2 + rows][:, pad], before[2:2 + rows][:, pad]))


def operands(M, N, K, dtype, seed, device="cpu"):
    """the fp64 values of one problem, every one of them exactly representable in the operand type `dtype`"""
    g = torch.Generator(device=device).manual_seed(seed)
    T = OP_DTYPE[dtype]

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=device, dtype=torch.float32)

    def p2(n, lo, hi):
        return torch.exp2(torch.randint(lo, hi + 1, (n,), generator=g, device=device).float())

    sa, sb = p2(M, -6, 6), p2(N, -4, 4)
    A = rn(M, K) * sa[:, None]
    B = rn(N, K) * K ** -0.5 * sb[:, None]
    bias = rn(N) * K ** -0.5 * sb
    res, aux = rn(M, N), rn(M, N)
    q = lambda t: t.to(T).to(F64)
    return SimpleNamespace(A=q(A), B=q(B), bias=q(bias), res=q(res), aux=q(aux), row_scale=sa, col_scale=sb)


def device_operand(x64, ld, Kp, dtype):
    """[R, ld] operand buffer: the values, zeros up to Kp, NaN from Kp on"""
    R, K = x64.shape
    assert ld % 64 == 0 and ld >= Kp >= K
    buf = nan_filled((R, ld), dtype, x64.device)
    buf[:, :Kp] = 0
    buf[:, :K] = x64.to(dtype)
    return buf


def pack_keep_bits(keep, ldmask):
    """[M, N] 0/1 -> [M + 4, ldmask] bytes, bit c % 8 of byte [r, c / 8] = element (r, c); every other bit SET (a kept element
    where there is none: an epilogue that reads past its row's bytes keeps what it should drop)"""
    M, N = keep.shape
    nb = (N + 7) // 8
    assert ldmask >= nb
    full = torch.ones((M, nb * 8), dtype=torch.int32, device=keep.device)
    full[:, :N] = keep.to(torch.int32)
    byts = (full.view(M, nb, 8) << torch.arange(8, device=keep.device, dtype=torch.int32)).sum(-1).to(torch.uint8)
    whole = torch.full((M + 4, ldmask), 0xFF, dtype=torch.uint8, device=keep.device)
    whole[2:2 + M, :nb] = byts
    return whole, whole[2:2 + M]


def default_pitches(epi, N, Kp, dtype, kw=None):
    """all different from each other and from N; the 16-bit ones multiples of 8, the fp32 ones of 4 (class (a) of the GPU tests)"""
    n8 = _ru(N, 8)
    p = dict(ld0=n8 + 8, ld1=n8 + 24, ldres=n8 + 12, ldaux=n8 + 40, ldmask=(N + 7) // 8 + 3, lda=(kw or Kp) + 64, ldb=Kp + 128)
    if epi in F32_OUT:
        p["ld0"] = n8 + 4
    if epi == L.EPI_RELU_SPLIT3_T:
        p["ld1"] = _ru(N) + 64
        p["ld0"] = 3 * p["ld1"] + 8
    return p


def make_case(epi, M, N, K, dtype, device="cpu", seed=0, pitches=None, keep=None, p=0.0, acc_scale=None, splitk=1, ln=False,
              a_wrap=False, mask_bits=False, prior=1.0):
    """every buffer of one timhip_gemm_nt call.  keep: [M, N] 0/1 (the site's keep set) when p > 0; mask_bits: hand the keep set
    to the epilogue as TimEpi.mask bytes; ln: the LayerNorm form of DROP_RES_F32; a_wrap: K = 2 * kw, A has kw columns and is
    read twice; prior: what an ATOMIC_F32 output holds before the call."""
    T = OP_DTYPE[dtype]
    Kp = _ru(K)
    kw = Kp // 2 if a_wrap else None
    assert not a_wrap or (K == Kp and kw % 64 == 0)
    o = operands(M, N, K, dtype, seed, device)
    if a_wrap:
        o.A = o.A[:, :kw].contiguous()
    pt = dict(default_pitches(epi, N, Kp, dtype, kw))
    pt.update(pitches or {})
    c = SimpleNamespace(epi=epi, M=M, N=N, K=K, Kp=Kp, dtype=dtype, T=T, device=device, p=p, keep=keep, splitk=splitk, a_wrap=a_wrap,
                        kw=kw, acc_scale=acc_scale, ops=o, prior=prior, ln=None, **pt)
    c.Abuf = device_operand(o.A, c.lda, kw or Kp, T)
    c.Bbuf = device_operand(o.B, c.ldb, Kp, T)
    c.bias_buf = c.res_whole = c.res = c.aux_whole = c.aux = c.out1_whole = c.out1 = c.mask_whole = c.mask = None
    if epi in HAS_BIAS:
        c.bias_buf = nan_filled((N + 8,), torch.float32, device)
        c.bias_buf[:N] = o.bias.float()
    if epi in HAS_RES:
        c.res_whole, c.res = guarded(M, N, c.ldres, torch.float32, device, o.res)
    if epi in HAS_AUX:
        c.aux_whole, c.aux = guarded(M, N, c.ldaux, torch.float32 if epi == L.EPI_DRELU_F32IN_T else T, device, o.aux)
    out_t = torch.float32 if epi in F32_OUT else T
    if epi == L.EPI_RELU_SPLIT3_T:
        col = torch.arange(c.ld0, device=device)
        c.cols0 = (col < 3 * c.ld1) & (col % c.ld1 < N)
    else:
        c.cols0 = N
    src = torch.full((M, N), prior, dtype=F64, device=device) if epi == L.EPI_ATOMIC_F32 else None
    c.out0_whole, c.out0 = guarded(M, N, c.ld0, out_t, device, src)
    if epi in HAS_OUT1:
        c.out1_whole, c.out1 = guarded(M, N, c.ld1, T, device)
    if p > 0:
        assert epi in HAS_DROPOUT and keep is not None and N % 4 == 0
        if mask_bits:
            c.mask_whole, c.mask = pack_keep_bits(keep, c.ldmask)
    if ln:
        assert epi == L.EPI_DROP_RES_F32
        g = torch.Generator(device=device).manual_seed(seed + 1000)
        mean = o.res.mean(-1).float()
        rstd = (o.res.var(-1, unbiased=False) + 1e-5).rsqrt().float()
        w = (1 + 0.1 * torch.randn(N, generator=g, device=device)).float()
        b = (0.1 * torch.randn(N, generator=g, device=device)).float()
        c.ln = SimpleNamespace(stats=torch.stack([mean, rstd], 1).contiguous(), w=w, b=b)
    c.sc_buf = None if acc_scale is None else torch.tensor([acc_scale], dtype=torch.float32, device=device)
    return c


def snapshot(c):
    return {k: getattr(c, k).clone() for k in ("out0_whole", "out1_whole") if getattr(c, k) is not None}


def reset_outputs(c, snap):
    for k, v in snap.items():
        getattr(c, k).copy_(v)


# ---- the accumulators ------------------------------------------------------------------------------------------------------
def acc_coefficient(dtype, Kp):
    """|acc_kernel - acc| <= coefficient * u * S elementwise, S = |A| |B|^T, for ANY order of summation.
    bf16 / fp16: a product of two 8-bit (11-bit) significands has at most 16 (22) bits: exact in fp32.  A sum of Kp exact terms
      in fp32, in any order and any tree, is within (Kp - 1) u of sum|terms| (first order); Kp + 2 leaves room for the second
      order and for the multiplication by acc_scale.
    fp32 (gemm_nt_f32_kernel, v_mfma_f32_32x32x2_f32): every product is rounded as well: Kp + 3.
    bf16x3 (gemm_nt_x3_kernel): a = hi + lo + e with hi = bf16(a), lo = bf16(a - hi) (a - hi is exact in fp32):
      |a - hi| <= 2^-9 |a|, |e| <= 2^-9 |a - hi| <= 2^-18 |a|, |hi| <= (1 + 2^-9) |a|, |lo| <= 2^-9 (1 + 2^-9) |a|.
      The kernel keeps hi_a hi_b + hi_a lo_b + lo_a hi_b; what it drops is
        a b - kept = lo_a lo_b + e_a (hi_b + lo_b) + (hi_a + lo_a) e_b + e_a e_b  <=  (2^-18 + 2 * 2^-18) (1 + 2^-7) |a| |b|
                  <= 3.03 * 2^-18 |a| |b| = 97 u |a| |b|.
      The 3 Kp kept products are exact in fp32 (bf16 x bf16) and their absolute sum is at most (1 + 2^-7) S, so the
      accumulation adds (3 Kp + 2) u 1.01 S: coefficient 97 + 1.01 (3 Kp + 2)."""
    if dtype in ("bf16", "fp16"):
        return Kp + 2
    if dtype == "fp32":
        return Kp + 3
    return 97 + 1.01 * (3 * Kp + 2)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _store(want, d, dtype):
    """a 16-bit store rounds to nearest: HALF_ULP |want|, and fp16 has a smallest step of 2^-24 below 2^-14.  The fp32 'operand
    types' (fp32, bf16x3) store what they computed."""
    if dtype not in HALF_ULP:
        return d
    return d + HALF_ULP[dtype] * want.abs() + (2.0 ** -24 if dtype == "fp16" else 0.0)


def _t(want, d, dtype):
    """an operand-type output: (want, bound with the store's rounding, the arithmetic part of the bound)"""
    return want, _store(want, d, dtype), d


def _f(want, d):
    """an fp32 output: the bound is all arithmetic"""
    return want, d, d


def reference(c):
    """{name: (want, bound, arithmetic part of the bound)} for the outputs of case c, fp64 on c.device.  names: out0, out1; RELU_SPLIT3_T: hi (= block 0 and
    block 2 of out0) and sum (= block 0 + block 1)."""
    u, o, epi, dt = U, c.ops, c.epi, c.dtype
    A = torch.cat([o.A, o.A], 1) if c.a_wrap else o.A
    s = 1.0 if c.acc_scale is None else float(c.acc_scale)
    acc = A @ o.B.t()
    S = A.abs() @ o.B.abs().t()
    x = s * acc
    d = acc_coefficient(dt, c.Kp) * u * S * abs(s)                  # d_acc of the issue: the accumulators, scaled
    kf = None
    if c.p > 0:
        kf = c.keep.to(F64) / (1.0 - c.p)
    k1 = kf if kf is not None else 1.0
    # v = acc + bias: a sum of two terms, each rounding within u of a partial sum <= |x| + |bias|: 2 u of each term's magnitude
    if epi in HAS_BIAS:
        v, dv = x + o.bias, d + 2 * u * (x.abs() + o.bias.abs())
    else:
        v, dv = x, d
    if epi == L.EPI_STORE_T or epi == L.EPI_STORE_F32:
        return {"out0": _t(v, dv, dt) if epi == L.EPI_STORE_T else _f(v, dv)}
    if epi == L.EPI_RELU_T:                                          # relu is 1-Lipschitz and exact
        w = v.clamp(min=0)
        return {"out0": _t(w, dv, dt)}
    if epi in (L.EPI_GELU_DROP_T2, L.EPI_GELU_DROP_G2, L.EPI_GELU_T):
        # gelu(v) = v Phi(v): |gelu'| <= 1.13 carries dv; Phi from the erf approximation of common.h (1.5e-7 absolute, halved by
        # the 0.5) times |v|, and two roundings (the sum 1 + erf, the product): (0.75e-7 + 2 u) |v|.  The keep factor 1 / (1 - p)
        # multiplies value and error and is itself an fp32 quotient: 2 u of the result.
        gl, dgl = gelu64(v), 1.13 * dv + (0.75e-7 + 2 * u) * v.abs()
        w0 = gl * k1
        out = {"out0": _t(w0, dgl * k1 + 2 * u * w0.abs(), dt)}
        if epi == L.EPI_GELU_DROP_T2:                                # out1 = the pre-activation
            out["out1"] = _t(v, dv, dt)
        elif epi == L.EPI_GELU_DROP_G2:                              # out1 = mask * gelu'(v): |gelu''| <= 0.8, gelu' itself within 4e-7
            w1 = dgelu64(v) * k1
            out["out1"] = _t(w1, (0.8 * dv + 4e-7) * k1 + 2 * u * w1.abs(), dt)
        return out
    if epi == L.EPI_DROP_RES_F32:
        r, dr = o.res, 0.0
        if c.ln is not None:
            # residual = (res - mean) rstd w + b at the statistics the kernel is GIVEN: a difference, two products and a sum, each
            # within u of its result (less when the compiler contracts to fma): 4 u of the two terms' magnitudes
            mean, rstd = c.ln.stats[:, 0:1].to(F64), c.ln.stats[:, 1:2].to(F64)
            t = (o.res - mean) * rstd * c.ln.w.to(F64)
            r, dr = t + c.ln.b.to(F64), 4 * u * (t.abs() + c.ln.b.to(F64).abs())
        w = r + v * k1
        return {"out0": _f(w, dv * k1 + dr + 2 * u * ((v * k1).abs() + r.abs()))}
    if epi == L.EPI_ADD_F32:
        w = x + o.res
        return {"out0": _f(w, d + 2 * u * (x.abs() + o.res.abs()))}
    if epi == L.EPI_DGELU_T:
        # acc * keep * gelu'(aux): aux is read exactly, gelu' of it is within 4e-7 (erf 1.5e-7, exp 2 ulp), three products
        gp = dgelu64(o.aux)
        w = x * k1 * gp
        return {"out0": _t(w, (d * gp.abs() + x.abs() * 4e-7) * k1 + 3 * u * w.abs(), dt)}
    if epi in (L.EPI_DRELU_T, L.EPI_DRELU_F32IN_T):                  # the gate is exact
        w = x * (o.aux > 0)
        return {"out0": _t(w, d * (o.aux > 0), dt)}
    if epi == L.EPI_ATOMIC_F32:
        # every split adds its partial sum (the accumulator bound holds for the splits together: their absolute sums add up to S)
        # with one fp32 atomic: (splitk + 1) u |want|
        w = c.prior + x
        return {"out0": _f(w, d + (c.splitk + 1) * u * w.abs())}
    if epi == L.EPI_SIGMOID_F32:
        # s = 1 / (1 + e), e = __expf(-v) = exp2(-v log2 e): the rounded argument moves e by |v| u relative, exp2 itself by 2 ulp,
        # the sum and the quotient by one each: |ds| <= s (1 - s) (|v| + 3) u + 3 u s <= s (|v| + 6) u; sigmoid' <= 0.25 carries dv
        w = torch.sigmoid(v)
        return {"out0": _f(w, 0.25 * dv + w * (v.abs() + 6) * u)}
    if epi == L.EPI_MULAUX_T:
        w = x * o.aux
        return {"out0": _t(w, d * o.aux.abs() + 2 * u * w.abs(), dt)}
    if epi == L.EPI_RELU_SPLIT3_T:
        # hi = T(r), lo = T(r - hi) of the kernel's own r = relu(v): hi is a stored value of r; hi + lo misses r by the rounding of
        # lo alone, HALF_ULP |r - hi| <= HALF_ULP^2 |r| (1 + HALF_ULP), plus fp16's smallest step
        w = v.clamp(min=0)
        h = HALF_ULP[dt]
        return {"hi": _t(w, dv, dt), "sum": (w, dv + h * h * 1.01 * (w.abs() + dv) + (2.0 ** -24 if dt == "fp16" else 0.0), dv)}
    raise ValueError(epi)


def got_outputs(c):
    """the case's outputs as fp64 [M, N] tensors under the names `reference` uses"""
    N = c.N
    if c.epi == L.EPI_RELU_SPLIT3_T:
        b0, b1, b2 = (c.out0[:, i * c.ld1:i * c.ld1 + N] for i in range(3))
        assert _bits_equal(b0, b2), "the third block of the split operand is the first"
        return {"hi": b0.to(F64), "sum": b0.to(F64) + b1.to(F64)}
    out = {"out0": c.out0[:, :N].to(F64)}
    if c.out1 is not None:
        out["out1"] = c.out1[:, :N].to(F64)
    return out


def share_of_bound(got, want, bound, arith=None):
    """max over the elements of the used share of the bound.  arith (the arithmetic part of a bound that also holds a 16-bit
    store's rounding step): the store's own rounding takes up to all of its allowance by nature, so the share is taken of the
    arithmetic part, after the allowance: max(0, |got - want| - (bound - arith)) / arith.  inf for a NaN or an error where the
    bound is zero; 0 where there is no error."""
    err = (got - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    if arith is not None:
        a = arith if torch.is_tensor(arith) else torch.full_like(err, float(arith))
        err, b = (err - (b - a)).clamp(min=0), a
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
    return float(ratio.max())


def verify(c, before):
    """guards and pads bit for bit, then every output element within its bound.  Returns the largest used share of the
    (arithmetic part of the) bound; raises AssertionError with the output's name otherwise."""
    assert untouched(c.out0_whole, before["out0_whole"], c.M, c.cols0), "out0: a guard row or a pad column was written"
    if c.out1 is not None:
        assert untouched(c.out1_whole, before["out1_whole"], c.M, c.N), "out1: a guard row or a pad column was written"
    ref, got, worst = reference(c), got_outputs(c), 0.0
    for name, (want, bound, arith) in ref.items():
        sh = share_of_bound(got[name], want, bound)
        assert sh <= 1.0, "%s: epilogue %d uses %.3g of its elementwise bound" % (name, c.epi, sh)
        worst = max(worst, share_of_bound(got[name], want, bound, arith))
    if c.p > 0:   # a dropped element is an exact zero (DROP_RES_F32: the residual alone is covered by the bound)
        for name in ("out0", "out1"):
            if name in got and c.epi != L.EPI_DROP_RES_F32 and not (c.epi == L.EPI_GELU_DROP_T2 and name == "out1"):
                assert bool((got[name][c.keep == 0] == 0).all()), name + ": a dropped element is not zero"
    return worst


def max_norm_accepts(c, dtype_tol):
    """the older check of tests/test_gpu_kernels.py: max|got - want| <= tol * max(1, max|want|) (+ the store's half ulp of
    max|want|) - what the elementwise bound replaces; tests/test_gemm_ref.py shows which mutations it lets through"""
    ref, got = reference(c), got_outputs(c)
    for name, (want, _, _) in ref.items():
        lim = dtype_tol * max(1.0, float(want.abs().max()))
        if c.epi not in F32_OUT:
            lim += HALF_ULP.get(c.dtype, 0.0) * float(want.abs().max())
        if float((got[name] - want).abs().max()) > lim:
            return False
    return True


# ---- weight gradients ------------------------------------------------------------------------------------------------------
def wgrad_reference(dY, X, splits, base_w=None, base_b=None, out_scale=1.0):
    """dW = base + out_scale dY^T X, db = base + out_scale colsum(dY), fp64, with their bounds: the accumulator rule with the
    contraction length M - M exact products (16-bit operands) summed in fp32 in any order, `splits` partial sums joined by a
    reduce: (M + splits + 2) u S |out_scale|, S = |dY|^T |X| (sum|dY| for the bias) - and, when the call accumulates, the final
    sum with the value that was there: 2 u of each term."""
    M = dY.shape[0]
    coef = (M + splits + 2) * U * abs(out_scale)
    w = out_scale * (dY.t() @ X)
    bw = coef * (dY.abs().t() @ X.abs())
    b = out_scale * dY.sum(0)
    bb = coef * dY.abs().sum(0)
    if base_w is not None:
        bw = bw + 2 * U * (w.abs() + base_w.abs())
        w = w + base_w
    if base_b is not None:
        bb = bb + 2 * U * (b.abs() + base_b.abs())
        b = b + base_b
    return (w, bw), (b, bb)
