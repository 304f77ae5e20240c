"""float64 reference, ELEMENTWISE error bounds, guarded cases and an fp32 emulation (with a list of subtly wrong kernels) for the
structured attention of include/timhip.h: timhip_attention_fwd / timhip_attention_bwd.  Pure torch: everything works on whatever
device the case lives on (tests/test_attn_ref.py runs it on the CPU against the emulation and its mutations,
tests/test_gpu_attention_edges.py on the device against the kernels).

The operation.  Token row i of a (window b, head h) attends to the F feature keys j < F and, when it is a query row (i >= F), to
itself: column F of every [.., F + 1] matrix here is the SELF column (score q_i . k_i, value v_i), dead for feature rows.
    s_ij = scale q_i . k_j,  m_i = max_j s_ij,  P_ij = exp(s_ij - m_i) / sum_j,  lse_i = m_i + log sum_j exp(s_ij - m_i)
    k_ij = keep_ij / (1 - p)  (keep: the site's dropout stream at row pitch LP = round_up(F + 1, 8)),   P~ = P k
    o_i = sum_j P~_ij v_j
    dP_ij = dO_i . v_j,  delta_i = sum_j P_ij (k dP)_ij  (= dO_i . o_i),  dS = P (k dP - delta) scale
    dQ_i = sum_j dS_ij k_j;   feature keys: dK_j = sum_i dS_ij q_i, dV_j = sum_i P~_ij dO_i;
    query rows (the self terms, single products): dK_i = dS_iF q_i, dV_i = P~_iF dO_i.
`reference` writes all of it out in float64 on the STORED operands (16-bit values widened), so that the bounds can use the
intermediates.  It equals oracle.attention_structured + autograd to 1e-12 (tests/test_attn_ref.py).

The bounds are derived, not fitted.  u = 2^-23: a whole unit in the last place of fp32 (covers an accumulator that truncates).
h = HALF_ULP[prec] for 16-bit storage, 0 for fp32 storage (fp32, bf16x3: attention_f32.hip runs exact fp32 arithmetic on the f32
matrix cores, attention.hip plain fp32 fma chains).  A sum of n fp32 terms in any order is within (n - 1) u sum|terms|.

  scores     products of two 16-bit operands are exact in fp32 (8 + 8 / 11 + 11 significand bits); fp32 operands round each
             product.  Dh terms, any order, and the multiplication by scale:  e_s(i,j) = (Dh + 2) u scale sum_c |q_ic| |k_jc|.
  P          relative error eps_ij = e_s(i,j) + max_j e_s(i,.) + (F + 16 + 2 |s_ij - m_i|) u:
             the score's own error in the exponent; the row sum's relative error is at most the largest of its terms'
             (max_j e_s) plus F u of accumulation; the argument (s - m) scale log2 e is formed by one fma with the rounded
             constant scale * log2 e (attention.h: c2) or by a rounded difference and __expf's own product: 2 |s - m| u; the
             exp2 unit, the reciprocal, the products with inv and the keep factor (1 / (1 - p) is itself a rounded quotient) and
             the fma's result rounding: 16 u.
             (attention.h rounds mc = mx * c2 on its own: that error is common to the row, it cancels in P and shows in lse.)
  lse        |lse - ref| <= max_j e_s(i,.) + (F + 8) u + u |m_i| + b_log;  u |m_i|: the row-common shift just named
             (attention.h, attn_fwd_mfma_body: `const float mc = mx * c2`, two roundings of 2^-24 |m_i| log2 e each, in natural
             units 2^-23 |m_i|);  b_log = 4 u max(1, log sum) + u |lse|: __logf within a few ulp of max(1, log sum), the final
             mx scale + log one product and one sum.  (b_lse of tests/test_gpu_loss_kernels.py has the same two terms with
             U = 2^-24: 8 U max(1, log sum) is this 4 u; its U |lse| stands for one rounding of a sum, here there are a product
             and a sum, so u |lse| is twice that term.)
  o          |o - ref|_ic <= sum_j P~_ij |v_jc| (eps_ij + hP_j + (F + 2) u) + fl sum_{j<F} |v_jc| + h |ref_ic| (+ 2^-24, fp16);
             hP_j = h on the feature columns of the 16-bit matrix-core forward (attention.h: pack8<HT> of the probabilities
             before P V; the self term stays fp32), 0 in every other family;  fl = 2^-24 there for fp16 (the packed
             probability has a smallest step: gradual underflow below 2^-14), 0 otherwise;  (F + 2) u: the P V sum.
  backward   tested IN ISOLATION: it is given o = T(reference o) and lse = fp32(reference lse).
    delta    |D delta_i| <= sum_c |dO_ic| (h |o_ic| + fo) + (Dh + 2) u sum_c |dO_ic o_ic|     (the stored o, then the dot product;
             fo = 2^-25 for fp16: an o element below 2^-14 is stored with the subnormal step, not with relative h - a row
             whose dominant self term is dropped has such an o)
    dP       |D dP_ij|   <= (Dh + 2) u sum_c |dO_ic| |v_jc|
    p        the probability is recomputed as exp(s - lse): relative error
             eps'_ij = e_s(i,j) + (16 + 2 |s_ij - lse_i| + |lse_i| + |s_ij|) u
             |lse_i| u: the stored lse's rounding (2^-24 |lse|) and the key-split form's own product l2 = lse * log2 e
             (attention_bwd2.hip, item_a: `l2 = sL[row] * 1.44...f`); |s_ij| u: there the exponent is fmaf(sc, c2, -l2) with the
             rounded c2 - its error multiplies s, not s - lse (same line); the other forms round s scale first: also |s| 2^-24.
    dS       E_ij = |D dS_ij| <= P_ij scale (|D delta_i| + |D dP_ij| k_ij + eps'_ij |k dP_ij - delta_i|) + hS |dS_ij| + fl
    P~       |D P~_ij| <= (eps'_ij + hS) P~_ij + fl
             hS = h on the feature columns of the 16-bit matrix-core backward (the scratch of attn_bwd_rows / attn_bwd_keys and
             the LDS tiles of the fused forms hold dS / P~ in the operand type: store8_h<HT>, pack8<HT>), 0 in attn_bwd_simple
             and the f32 kernels (fp32 scratch); the self column stays fp32 everywhere.  fl = 2^-24 for fp16 where hS = h.
    dQ       |D dQ_ic| <= sum_j E_ij |k_jc| + (F + 2) u sum_j |dS_ij k_jc| + h |dQ_ic|
    dK       |D dK_jc| <= sum_i E_ij |q_ic| + (S + 2) u sum_i |dS_ij q_ic| + h |dK_jc|;   dV likewise with D P~ and dO
    self     dK_i = dS_iF q_i, dV_i = P~_iF dO_i: E_iF |q_ic| (D P~_iF |dO_ic|) + 2 u |result| + h |result|
    fp16 outputs get an absolute floor of 2^-24 (subnormal results), as _ln_edge of tests/test_gpu_kernels.py has.
  underflow  (`peaked` cases: exponents down to -300.)  A probability below 2^-126 is flushed to zero by the exp2 unit, and an
             fp32 product below it may be: TINY = 2^-126 absolute on every unnormalised probability (the row sum is >= 1, so
             TINY k_ij on P~; in the backward TINY on p, i.e. TINY scale |k dP - delta| on dS), on dS itself and on every output.

A case (`make_case`) owns every buffer of one forward and one backward call: qkv, dO and the backward's o / lse inputs between
guard rows of one NaN bit pattern, the outputs o, lse, dqkv PREFILLED with that pattern between guard rows (an element a kernel
does not write, or an over-read that reaches arithmetic, shows as NaN), and (GPU) a NaN-filled workspace with a guard behind it.
`family_of` restates the dispatch rule of tim_attention_fwd / _bwd so that a GPU case can assert the kernel family and row split
it is meant for; the tests see results, not kernel names.
"""
from types import SimpleNamespace

import torch

from tests.gemm_ref import F64, OP_DTYPE, U, guarded, nan_filled, share_of_bound
from tests.test_gpu_kernels import HALF_ULP, _bits_equal

SEED, LAYER = 99, 1
SITE = 16 + 8 * LAYER            # csrc/common.h: layer_site(layer, SITE_L_ATTN)
TABLE = {(128, 1), (128, 2), (128, 3), (128, 4), (128, 5), (64, 1), (64, 2), (64, 4), (32, 1), (32, 2)}   # attention.h: attn_for_shape
H16_BWD = ("fused_ks", "fused", "rows_keys")     # the 16-bit matrix-core backward forms: dS / P~ travel in the operand type
KNOBS = dict(ATTN_WAVES=0, ATTN_SPLIT_MIN=4, ATTN_FUSED=1, ATTN_KS=1)      # tim_knobs.h defaults
LSE_GUARD, WS_GUARD = 64, 256


def _ru(x, m):
    return (x + m - 1) // m * m


# ---- the dispatch rule ---------------------------------------------------------------------------------------------------------
def _row_split(B, H, S, waves_min):
    """attention.h: attn_row_split with s0 = 0 -> (rsplit, rper)"""
    nrb, bh = (S + 31) // 32, B * H
    want = 1 if bh >= 512 else (512 + bh - 1) // bh
    want = max(1, min(want, nrb // max(1, waves_min)))
    rper = (nrb + want - 1) // want
    return (nrb + rper - 1) // rper, rper


def _waves(S, cap, knob):
    """attention.h: attn_waves; knob: TIMHIP_ATTN_WAVES where the launcher takes it, else 0"""
    n = max(1, min(cap, (S + 31) // 32))
    return knob if 1 <= knob <= 8 else n


def _fused_fits(S, F, Dh, ks, kn):
    SP = _ru(S, 32)
    return kn["ATTN_FUSED"] != 0 and Dh == 128 and (F + 31) // 32 == 4 and 2 * 128 * 128 * 2 + 2 * SP * 128 * 2 + (SP * 12 if ks else 0) <= 160 * 1024


def family_of(prec, desc, knobs=None):
    """the dispatch rule of tim_attention_fwd / _bwd (include/timhip.h, attention.hip) restated: which kernel family a call
    gets, its row split (rsplit, rper) and its waves per block.  desc: B, S, F, H, Dh and fp32 (TIMHIP_DESC_ATTN_FP32).
    forward: mfma | f32 | simple;  backward: fused_ks | fused | rows_keys | f32 | simple;  `unsupported` for F > 192."""
    kn = dict(KNOBS)
    kn.update(knobs or {})
    B, S, F, H, Dh = (desc[k] for k in "B S F H Dh".split())
    E, bh = H * Dh, B * H
    out = SimpleNamespace(fwd="simple", bwd="simple", fwd_split=(1, (S + 31) // 32), bwd_split=(1, (S + 31) // 32), fwd_waves=4, bwd_waves=4)
    if F > 192:
        out.fwd = out.bwd = "unsupported"
        return out
    h16, table = prec in HALF_ULP, (Dh, (F + 31) // 32) in TABLE
    if desc.get("fp32"):
        return out
    if h16 and E % 8 == 0:
        if table:     # (the forward's grid is one-dimensional: no limit on B * H)
            out.fwd = "mfma"
            out.fwd_split = _row_split(B, H, S, kn["ATTN_SPLIT_MIN"] if bh < 128 else 4)
            out.fwd_waves = _waves(32 * out.fwd_split[1], 4, kn["ATTN_WAVES"])
        if bh <= 65535:
            if kn["ATTN_KS"] != 0 and _fused_fits(S, F, Dh, True, kn):
                out.bwd, out.bwd_waves = "fused_ks", 8
            elif _fused_fits(S, F, Dh, False, kn):
                out.bwd, out.bwd_waves = "fused", 8
            elif table:
                out.bwd = "rows_keys"
                out.bwd_split = _row_split(B, H, S, 4)
                out.bwd_waves = _waves(32 * min(out.bwd_split[1], 4) if out.bwd_split[0] > 1 else S, 8, kn["ATTN_WAVES"])
    if not h16 and E % 4 == 0 and bh <= 65535 and table:
        out.fwd = out.bwd = "f32"
        out.fwd_waves = out.bwd_waves = _waves(S, 8, 0)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _heads(x, B, S, H, Dh, n):
    """[B * S, n * E] -> n tensors [B, H, S, Dh]"""
    v = x.reshape(B, S, n, H, Dh)
    return [v[:, :, i].transpose(1, 2) for i in range(n)]


def _rows(ts, B, S, H, Dh):
    """n tensors [B, H, S, Dh] -> [B * S, n * E]"""
    return torch.stack([t.transpose(1, 2) for t in ts], 2).reshape(B * S, len(ts) * H * Dh)


def planted(S, F):
    """the query row whose self score dominates; the one behind it has its self score far below the rest"""
    return F + 1 if S >= F + 3 else F


def make_case(prec, B, S, F, H, Dh, p=0.0, seed=0, peaked=False, device="cpu", keep=None, plain=False, fp32=False):
    """every buffer of one timhip_attention_fwd and one timhip_attention_bwd call.
    q rows are scaled by 2^randint(-2, 2), k rows by 2^randint(-1, 1), v rows by 2^randint(-4, 4), dO rows by 2^randint(-6, 6);
    three planted rows: a query row with k_i = 4 q_i (its self score dominates), the next one with k_i = -4 q_i (its self score
    is far below the rest) - rows F + 1 and F + 2, or F and F + 1 where there are fewer than three query rows (`planted`) - and
    feature key F / 2, which every row prefers (all q rows share a positive first component, the key is 2 sqrt(Dh) e_0: score
    4 x the row's scale); with three or more query rows, row F gets a self score equal to that key's, so that its self term
    carries weight without saturating the row, and the last feature row F - 1 gets q . k of the same size, so that a self term
    it is given by mistake carries weight too; `peaked` multiplies q by 8.  Everything is rounded to the operand
    type and kept as fp64.  keep: [B * H * S, LP] 0/1, the site's keep set (timhip_dropout_mask on the GPU); without one and
    p > 0 a Bernoulli draw (CPU tests).  plain: unscaled randn and no planted rows - the inputs of _attn_case."""
    T, E, LP = OP_DTYPE[prec], H * Dh, _ru(F + 1, 8)
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda: torch.randn(B, H, S, Dh, generator=g, device=device, dtype=torch.float32)
    p2 = lambda lo, hi: torch.exp2(torch.randint(lo, hi + 1, (B, H, S, 1), generator=g, device=device).float())
    q, k, v, dO = rn(), rn(), rn(), rn()
    if not plain:
        sq = p2(-2, 2)
        i1 = planted(S, F)
        if S > F:
            sq[:, :, i1:i1 + 2] = 1.0
        q, k, v, dO = q * sq, k * p2(-1, 1), v * p2(-4, 4), dO * p2(-6, 6)
        q[..., 0] = 2 * sq[..., 0]
        k[:, :, F // 2] = 0.0
        k[:, :, F // 2, 0] = 2 * Dh ** 0.5
        # rows F - 1 and F: q_i . k_i scale equal to the preferred key's score (4 x the row's scale).  Row F's self term then
        # matters without saturating the row, and a self term that a kernel gives row F - 1 by mistake matters as much.  (As a
        # feature key, row F - 1 gets a random score from every other row: the shared first component adds 16 / Dh of their scale.
        # F - 1 = F / 2 is the preferred key itself: its own q . k is that score already)
        for i in ([F - 1] if F - 1 != F // 2 else []) + ([F] if i1 > F else []):
            k[:, :, i] = q[:, :, i] * (4 * sq[:, :, i] * Dh ** 0.5 / q[:, :, i].square().sum(-1, keepdim=True))
        if S > i1:
            k[:, :, i1] = 4 * q[:, :, i1]
        if S > i1 + 1:
            k[:, :, i1 + 1] = -4 * q[:, :, i1 + 1]
        if peaked:
            q = q * 8
    rd = lambda t: t.to(T).to(F64)
    c = SimpleNamespace(prec=prec, T=T, B=B, S=S, F=F, H=H, Dh=Dh, E=E, LP=LP, p=float(p), device=device, peaked=peaked,
                        h=HALF_ULP.get(prec, 0.0), fp32=fp32, q=rd(q), k=rd(k), v=rd(v), dO=rd(dO), ref=None, ws=None, ws_whole=None)
    if p > 0:
        if keep is None:
            keep = (torch.rand(B * H * S, LP, generator=g, device=device) >= p).to(torch.uint8)
        c.keep = keep.reshape(B, H, S, LP)
    else:
        c.keep = None
    M = B * S
    c.qkv_whole, c.qkv = guarded(M, 3 * E, 3 * E, T, device, _rows([c.q, c.k, c.v], B, S, H, Dh))
    c.dO_whole, c.dO_buf = guarded(M, E, E, T, device, _rows([c.dO], B, S, H, Dh))
    r = reference(c)
    c.o_in_whole, c.o_in = guarded(M, E, E, T, device, _rows([r.o], B, S, H, Dh))
    c.lse_in_whole = nan_filled((B * H * S + 2 * LSE_GUARD,), torch.float32, device)
    c.lse_in = c.lse_in_whole[LSE_GUARD:LSE_GUARD + B * H * S]
    c.lse_in[:] = r.lse.reshape(-1).float()
    c.o_whole, c.o = guarded(M, E, E, T, device)
    c.dqkv_whole, c.dqkv = guarded(M, 3 * E, 3 * E, T, device)
    c.lse_whole = nan_filled((B * H * S + 2 * LSE_GUARD,), torch.float32, device)
    c.lse = c.lse_whole[LSE_GUARD:LSE_GUARD + B * H * S]
    c.inputs = {n: getattr(c, n).clone() for n in ("qkv_whole", "dO_whole", "o_in_whole", "lse_in_whole")}
    c.poison = {n: getattr(c, n).clone() for n in ("o_whole", "lse_whole", "dqkv_whole")}
    return c


def attach_workspace(c, nbytes):
    """a NaN-filled workspace (every byte 0xFF: a NaN in each of the three element types) of nbytes with a guard behind it"""
    c.ws_whole = torch.full((nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=c.device)
    c.ws = c.ws_whole[:nbytes]


def repoison(c, names=("o_whole", "lse_whole", "dqkv_whole")):
    for n in names:
        getattr(c, n).copy_(c.poison[n])
    if c.ws_whole is not None:
        c.ws_whole.fill_(0xFF)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def reference(c):
    """every intermediate of the module docstring in float64, [B, H, S, F + 1] with column F the self column"""
    if c.ref is not None:
        return c.ref
    q, k, v, dO, F, S = c.q, c.k, c.v, c.dO, c.F, c.S
    sc = c.Dh ** -0.5
    kf, vf = k[:, :, :F], v[:, :, :F]
    live = torch.ones(S, F + 1, dtype=torch.bool, device=q.device)
    live[:F, F] = False
    dot = lambda a, bf, b: torch.cat([a @ bf.transpose(-1, -2), (a * b).sum(-1, keepdim=True)], -1)
    s = (sc * dot(q, kf, k)).masked_fill(~live, float("-inf"))
    A = dot(q.abs(), kf.abs(), k.abs()) * live
    m = s.max(-1, keepdim=True).values
    e = (s - m).exp()
    se = e.sum(-1, keepdim=True)
    P = e / se
    lse = (m + se.log()).squeeze(-1)
    kfac = torch.ones_like(P) if c.keep is None else c.keep[..., :F + 1].to(F64) / (1.0 - c.p)
    Pt = P * kfac
    mix = lambda w, xf, x: w[..., :F] @ xf + w[..., F:] * x
    o = mix(Pt, vf, v)
    dP = dot(dO, vf, v)
    delta = (Pt * dP).sum(-1, keepdim=True)
    dS = P * (kfac * dP - delta) * sc
    dQ = mix(dS, kf, k)
    keys = lambda w, x: torch.cat([w[..., :F].transpose(-1, -2) @ x, w[:, :, F:, F:] * x[:, :, F:]], 2)
    c.ref = SimpleNamespace(s=s, A=A, live=live, m=m, se=se, P=P, lse=lse, kfac=kfac, Pt=Pt, o=o, dP=dP, delta=delta, dS=dS, dQ=dQ,
                            dK=keys(dS, q), dV=keys(Pt, dO), scale=sc, dot=dot, mix=mix, keys=keys)
    return c.ref


def _es(c, r):
    es = (c.Dh + 2) * U * r.scale * r.A
    return es, es.max(-1, keepdim=True).values


TINY = 2.0 ** -126     # the smallest normal fp32: below it the exp2 unit and fp32 products may flush to zero


def _floor(c):
    return 2.0 ** -24 if c.prec == "fp16" else 0.0


def _cols(c, x):
    """x on the feature columns, 0 on the self column"""
    w = torch.zeros(c.F + 1, dtype=F64, device=c.q.device)
    w[:c.F] = x
    return w


def fwd_bounds(c, family):
    """{name: (want, bound, arithmetic part)} of o [B, H, S, Dh] and lse [B, H, S]"""
    r, u, F = reference(c), U, c.F
    es, er = _es(c, r)
    sd = torch.where(r.live, (r.s - r.m).abs(), torch.zeros_like(r.P))
    eps = es + er + (F + 16 + 2 * sd) * u
    b_lse = (er + (F + 8) * u + u * r.m.abs() + 4 * u * r.se.log().clamp(min=1.0)).squeeze(-1) + u * r.lse.abs()
    packs = family == "mfma"
    w = r.Pt * (eps + _cols(c, c.h if packs else 0.0) + (F + 2) * u) + _cols(c, _floor(c) if packs else 0.0) + TINY * r.kfac * r.live
    a_o = r.mix(w, c.v[:, :, :F].abs(), c.v.abs()) + TINY
    return {"o": (r.o, a_o + c.h * r.o.abs() + _floor(c), a_o), "lse": (r.lse, b_lse, b_lse)}


def bwd_bounds(c, family):
    """{name: (want, bound, arithmetic part)} of dQ, dK, dV [B, H, S, Dh] for a backward that is GIVEN o = T(ref) and lse = fp32(ref)"""
    r, u, F, S, h = reference(c), U, c.F, c.S, c.h
    es, _ = _es(c, r)
    q, k, v, dO = c.q.abs(), c.k.abs(), c.v.abs(), c.dO.abs()
    d_delta = (dO * (h * r.o.abs() + _floor(c) / 2)).sum(-1, keepdim=True) + (c.Dh + 2) * u * (c.dO * r.o).abs().sum(-1, keepdim=True)
    d_dP = (c.Dh + 2) * u * r.dot(dO, v[:, :, :F], v)
    zero = torch.zeros_like(r.P)
    lse = r.lse.unsqueeze(-1)
    epsb = es + (16 + 2 * torch.where(r.live, (r.s - lse).abs(), zero) + lse.abs() + torch.where(r.live, r.s.abs(), zero)) * u
    hs = h if family in H16_BWD else 0.0
    hS, fl = _cols(c, hs), _cols(c, _floor(c) if hs else 0.0)
    E = r.P * r.scale * (d_delta + d_dP * r.kfac + epsb * (r.kfac * r.dP - r.delta).abs()) + hS * r.dS.abs() + fl
    E = E + TINY * (1 + r.scale * (r.kfac * r.dP - r.delta).abs()) * r.live
    dPt = (epsb + hS) * r.Pt + fl + TINY * r.kfac * r.live
    out = {}
    a = r.mix(E, k[:, :, :F], k) + (F + 2) * u * r.mix(r.dS.abs(), k[:, :, :F], k)
    a = a + TINY
    out["dQ"] = (r.dQ, a + h * r.dQ.abs() + _floor(c), a)
    for name, want, err, w, x in (("dK", r.dK, E, r.dS, q), ("dV", r.dV, dPt, r.Pt, dO)):
        a = r.keys(err, x) + torch.cat([(S + 2) * u * (w[..., :F].abs().transpose(-1, -2) @ x), 2 * u * want[:, :, F:].abs()], 2)
        a = a + TINY
        out[name] = (want, a + h * want.abs() + _floor(c), a)
    return out


# ---- verification --------------------------------------------------------------------------------------------------------------
def _guards_ok(whole, before, rows):
    return _bits_equal(whole[:2], before[:2]) and _bits_equal(whole[2 + rows:], before[2 + rows:])


def _lse_guards_ok(whole, before):
    return _bits_equal(whole[:LSE_GUARD], before[:LSE_GUARD]) and _bits_equal(whole[-LSE_GUARD:], before[-LSE_GUARD:])


def _inputs_ok(c):
    return all(_bits_equal(getattr(c, n), t) for n, t in c.inputs.items())


def _check(name, got, want, bound, arith, family):
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite (never written, or computed from a guard / unwritten scratch)" % name
    sh = share_of_bound(got, want, bound)
    assert sh <= 1.0, "%s: the %s family uses %.3g of its elementwise bound" % (name, family, sh)
    return share_of_bound(got, want, bound, arith)


def verify_fwd(c, family):
    """the forward's outputs in c.o / c.lse: guards bit for bit, every element finite and within its own bound.  Returns the
    largest used share of the (arithmetic part of the) bound"""
    M = c.B * c.S
    assert _guards_ok(c.o_whole, c.poison["o_whole"], M), "o: a guard row was written"
    assert _lse_guards_ok(c.lse_whole, c.poison["lse_whole"]), "lse: a guard element was written"
    assert _inputs_ok(c), "an input buffer or its guard rows changed"
    b = fwd_bounds(c, family)
    got = {"o": _heads(c.o.to(F64), c.B, c.S, c.H, c.Dh, 1)[0], "lse": c.lse.to(F64).reshape(c.B, c.H, c.S)}
    return max(_check(n, got[n], *b[n], family) for n in ("lse", "o"))


def got_grads(c):
    return dict(zip(("dQ", "dK", "dV"), _heads(c.dqkv.to(F64), c.B, c.S, c.H, c.Dh, 3)))


def verify_bwd(c, family):
    """the backward's output in c.dqkv, likewise; with a workspace attached, the guard behind it as well"""
    assert _guards_ok(c.dqkv_whole, c.poison["dqkv_whole"], c.B * c.S), "dqkv: a guard row was written"
    assert _inputs_ok(c), "an input buffer or its guard rows changed"
    if c.ws_whole is not None:
        assert bool((c.ws_whole[c.ws.numel():] == 0xFF).all()), "a byte behind the workspace was written"
    b, got = bwd_bounds(c, family), got_grads(c)
    return max(_check(n, got[n], *b[n], family) for n in ("dQ", "dK", "dV"))


def max_norm_accepts_bwd(c, tol_rel):
    """the criterion of _attn_case (tests/test_gpu_kernels.py) for the backward: one number for the whole dqkv matrix,
    max|err| <= 5 tol(prec) max(1, max|ref|) + 2 HALF_ULP max|ref| - what the elementwise bound replaces"""
    r, got = reference(c), got_grads(c)
    gmax = max(float(t.abs().max()) for t in (r.dQ, r.dK, r.dV))
    err = max(float((got[n] - w).abs().max()) for n, w in (("dQ", r.dQ), ("dK", r.dK), ("dV", r.dV)))
    return err <= 5 * tol_rel * max(1.0, gmax) + 2 * c.h * gmax


# ---- the fp32 emulation of a correct kernel, and eleven subtly wrong ones (the second of the issue's ten, in both directions) ------------------------------------------------------------
MUTATIONS = {   # name: (pass, what the wrong kernel does)
    "pad_key_unmasked": ("fwd", "1: the first padded key (index F, score 0, value 0) is not masked"),
    "self_missing_row_f": ("both", "2: row F is taken for a feature row (no self term)"),
    "self_present_row_f_minus_1": ("fwd", "2: row F - 1 is taken for a query row (a self term)"),
    "self_keep_pitch": ("both", "3: the self column's keep factor is taken at pitch F + 1 instead of LP"),
    "lse_without_self": ("fwd", "4: the self term is missing in lse's sum"),
    "dq_without_self": ("bwd", "5: dQ is missing dS_self k_i"),
    "own_kv_zero": ("bwd", "6: the own-key / own-value gradients of the query rows are stored as zero"),
    "last_row_clamped": ("both", "7: row S - 1 is computed from row S - 2"),
    "dq_scaled": ("bwd", "8: dQ is scaled by 1 + 2^-5"),
    "split_reads_previous_window": ("both", "9: the second part of a row split reads the keys / values of window b - 1"),
    "delta_without_keep": ("bwd", "10: delta is taken without the keep factors"),
}


def _split_row0(c, fam):
    """first row of the second part of a row split: the family's own split, or two halves where it takes none"""
    part = fam.fwd_split if fam.fwd_split[0] > 1 else (fam.bwd_split if fam.bwd_split[0] > 1 else (2, ((c.S + 31) // 32 + 1) // 2))
    return 32 * part[1]


def applies(c, mut, fam):
    """whether the mutation changes a result at this case's shape beyond the arithmetic's own uncertainty:
    pad_key_unmasked, self_missing_row_f, self_present_row_f_minus_1 - not `peaked` (there every row's maximum is at least 8 and the rows are
    saturated: exp(0 - m) and a stray self term are below the score error e_s);  dq_without_self - a query row besides the
    planted ones (the first: P_self = 1, so dS_self = P (k dP - delta) cancels; the second: P_self = 0);  dq_scaled - F > 1
    (one key: P = 1 and dS = 0 exactly);  split_reads_previous_window - a row in the second part that is not the planted row
    whose self term has all the weight (the feature keys it reads do not matter)"""
    F, S = c.F, c.S
    return {"pad_key_unmasked": F % 32 != 0 and not c.peaked, "self_missing_row_f": S > F and not c.peaked, "self_present_row_f_minus_1": not c.peaked,
            "self_keep_pitch": c.p > 0 and c.LP != F + 1 and S > F, "lse_without_self": S > F, "dq_without_self": S > F + 2,
            "own_kv_zero": S > F, "last_row_clamped": S >= 2, "dq_scaled": F > 1,
            "split_reads_previous_window": c.B > 1 and len(set(range(_split_row0(c, fam), S)) - {planted(S, F)}) > 0,
            "delta_without_keep": c.p > 0}[mut]


def emulate(c, fam, mut=None, rows=None):
    """what a correct kernel of family `fam` (family_of's answer) computes, in float32 torch, rounding exactly where that family
    rounds: P (the 16-bit matrix-core forward), o, dS / P~ (the 16-bit matrix-core backward) and the outputs.  The backward is
    given c.o_in and c.lse_in.  `mut` names one deliberate mistake (MUTATIONS); rows: a [B, H, S] bool mask of the rows own_kv_zero / dq_scaled hit (all).
    Returns o, lse [B, H, S], dQ, dK, dV."""
    f32, T, F, S, B = torch.float32, c.T, c.F, c.S, c.B
    dev = c.q.device
    q, k, v, dO = (t.to(f32) for t in (c.q, c.k, c.v, c.dO))
    sc = torch.tensor(c.Dh ** -0.5, dtype=f32)
    row = torch.arange(S, device=dev)
    isq = row >= F
    if mut == "self_missing_row_f":
        isq = row > F
    if mut == "self_present_row_f_minus_1":
        isq = row >= F - 1
    kfac = torch.ones(B, c.H, S, F + 1, dtype=f32, device=dev)
    if c.keep is not None:
        ds = torch.tensor(1.0, dtype=f32) / (torch.tensor(1.0, dtype=f32) - torch.tensor(c.p, dtype=f32))
        keep = c.keep[..., :F + 1].clone()
        if mut == "self_keep_pitch":
            flat = c.keep.reshape(-1)
            idx = torch.arange(B * c.H * S, device=dev) * (F + 1) + F
            keep[..., F] = flat[idx].reshape(B, c.H, S)
        kfac = keep.to(f32) * ds
    rt = lambda t: t.to(T).to(f32)
    dot = lambda a, bf, b: torch.cat([a @ bf.transpose(-1, -2), (a * b).sum(-1, keepdim=True)], -1)
    mix = lambda w, xf, x: w[..., :F] @ xf + w[..., F:] * x

    def run(kk, vv):
        """kk, vv: where the feature keys / values are read from (k, v themselves in a correct kernel)"""
        kf, vf = kk[:, :, :F], vv[:, :, :F]
        s = dot(q, kf, k) * sc
        s[..., F] = torch.where(isq, s[..., F], torch.full_like(s[..., F], float("-inf")))
        m = s.max(-1, keepdim=True).values
        if mut == "pad_key_unmasked":
            m = m.clamp(min=0.0)
        e = (s - m).exp()
        se = e.sum(-1, keepdim=True)
        if mut == "pad_key_unmasked":
            se = se + (-m).exp()
        lse = (m + se.log()).squeeze(-1)
        if mut == "lse_without_self":
            lse = torch.where(isq, (m + (se - e[..., F:]).log()).squeeze(-1), lse)
        Pt = e / se * kfac
        if fam.fwd == "mfma":
            Pt = torch.cat([rt(Pt[..., :F]), Pt[..., F:]], -1)
        o = rt(mix(Pt, vf, v))
        # the backward, from the o and lse it is handed
        p = (s - c.lse_in.reshape(B, c.H, S, 1)).exp()
        dP = dot(dO, vf, v)
        o_in = _heads(c.o_in.to(f32), B, S, c.H, c.Dh, 1)[0]
        delta = (dO * o_in).sum(-1, keepdim=True)
        if mut == "delta_without_keep":
            delta = (p * dP).sum(-1, keepdim=True)
        dS, Pb = p * (dP * kfac - delta) * sc, p * kfac
        if fam.bwd in H16_BWD:
            dS, Pb = torch.cat([rt(dS[..., :F]), dS[..., F:]], -1), torch.cat([rt(Pb[..., :F]), Pb[..., F:]], -1)
        dQ = dS[..., :F] @ kf if mut == "dq_without_self" else mix(dS, kf, k)
        hit = torch.ones(B, c.H, S, 1, dtype=f32, device=dev) if rows is None else rows.to(f32).unsqueeze(-1)
        if mut == "dq_scaled":
            dQ = dQ * (1 + 2.0 ** -5 * hit)
        own = 1.0 - hit[:, :, F:] if mut == "own_kv_zero" else 1.0
        keys = lambda w, x: torch.cat([w[..., :F].transpose(-1, -2) @ x, own * w[:, :, F:, F:] * x[:, :, F:]], 2)
        return [o, lse, rt(dQ), rt(keys(dS, q)), rt(keys(Pb, dO))]

    out = run(k, v)
    if mut == "split_reads_previous_window":
        r0 = _split_row0(c, fam)
        wrong = run(k.roll(1, 0), v.roll(1, 0))
        for t, w in zip(out, wrong):
            t[1:, :, r0:] = w[1:, :, r0:]
    if mut == "last_row_clamped":
        for t in out:
            t[:, :, S - 1] = t[:, :, S - 2]
    return SimpleNamespace(o=out[0], lse=out[1], dQ=out[2], dK=out[3], dV=out[4])


def store(c, em):
    """write an emulation's results into the case's output buffers, as a kernel would"""
    c.o[:] = _rows([em.o], c.B, c.S, c.H, c.Dh).to(c.T)
    c.lse[:] = em.lse.reshape(-1)
    c.dqkv[:] = _rows([em.dQ, em.dK, em.dV], c.B, c.S, c.H, c.Dh).to(c.T)


def mutate(c, name, fam, rows=None):
    """the emulation with one realistic kernel error (MUTATIONS), stored in the case's output buffers"""
    assert name in MUTATIONS and applies(c, name, fam)
    repoison(c)
    store(c, emulate(c, fam, name, rows))


# ---- the cases of tests/test_gpu_attention_edges.py (tests/test_attn_ref.py runs the emulation over the same list) ----------------
PRECS = ["fp32", "bf16x3", "bf16", "fp16"]


def _case(name, B, S, F, H, Dh, p=0.0, precs=PRECS, knobs=None, fp32=False, peaked=False, want16=None, want32=None):
    return SimpleNamespace(name=name, B=B, S=S, F=F, H=H, Dh=Dh, p=p, precs=list(precs), knobs=knobs or {}, fp32=fp32, peaked=peaked,
                           want={"h16": want16 or {}, "f32": want32 or {}})


def _table_cases():
    out = []
    for Dh, njb in sorted(TABLE):
        for F in (32 * njb - 31, 32 * njb - 1, 32 * njb):
            S = F + 37
            for p in (0.0, 0.3):
                bwd = "rows_keys"
                if (Dh, njb) == (128, 4):   # the fused backward: the key-split form at S <= 160, the plain fused form above
                    bwd = "fused_ks" if S <= 160 else "fused"
                out.append(_case("table %dx%d F=%d p=%g" % (Dh, njb, F, p), 2, S, F, 2, Dh, p, want16=dict(fwd="mfma", bwd=bwd),
                                 want32=dict(fwd="f32", bwd="f32")))
    for F in (97, 127, 128):
        for p in (0.0, 0.3):
            out.append(_case("table 128x4 F=%d p=%g two-kernel" % (F, p), 2, F + 37, F, 2, 128, p, precs=["bf16", "fp16"],
                             knobs=dict(ATTN_FUSED=0), want16=dict(fwd="mfma", bwd="rows_keys")))
            out.append(_case("table 128x4 F=%d p=%g one wave per row block" % (F, p), 2, F + 37, F, 2, 128, p, precs=["bf16", "fp16"],
                             knobs=dict(ATTN_KS=0), want16=dict(fwd="mfma", bwd="fused")))
    # one peaked case per family: (128, 4) at S = 134 / 165 and with the two-kernel backward; (64, 2); head width 16 below
    out.append(_case("peaked 128x4 S=134", 2, 134, 97, 2, 128, 0.3, peaked=True, want16=dict(fwd="mfma", bwd="fused_ks"), want32=dict(fwd="f32", bwd="f32")))
    out.append(_case("peaked 128x4 S=165", 2, 165, 128, 2, 128, 0.3, peaked=True, precs=["bf16", "fp16"], want16=dict(fwd="mfma", bwd="fused")))
    out.append(_case("peaked 64x2", 2, 100, 63, 2, 64, 0.3, peaked=True, want16=dict(fwd="mfma", bwd="rows_keys"), want32=dict(fwd="f32", bwd="f32")))
    return out


def _split_cases():
    mk, f32 = dict(fwd="mfma", bwd="rows_keys"), dict(fwd="f32", bwd="f32")
    h16 = ["bf16", "fp16"]
    return [
        _case("split 260: 5 + 4 row blocks", 1, 260, 50, 2, 64, 0.3, precs=h16, want16=dict(mk, fwd_split=(2, 5), bwd_split=(2, 5))),
        _case("split 260, two windows", 2, 260, 50, 2, 64, 0.3, precs=h16, want16=dict(mk, fwd_split=(2, 5), bwd_split=(2, 5))),   # (a window stride in a second part)
        _case("split 499: four parts of four", 1, 499, 100, 1, 128, 0.3, precs=h16, want16=dict(mk, fwd_split=(4, 4), bwd_split=(4, 4))),
        _case("split 70, SPLIT_MIN=1: three parts of one", 1, 70, 40, 1, 32, 0.3, precs=h16, knobs=dict(ATTN_SPLIT_MIN=1),
              want16=dict(mk, fwd_split=(3, 1), bwd_split=(1, 3))),
        _case("155, WAVES=1", 2, 155, 100, 2, 128, 0.3, precs=h16, knobs=dict(ATTN_WAVES=1, ATTN_FUSED=0), want16=dict(mk, fwd_waves=1, bwd_waves=1)),
        _case("155, WAVES=2", 2, 155, 100, 2, 128, 0.3, precs=h16, knobs=dict(ATTN_WAVES=2, ATTN_FUSED=0), want16=dict(mk, fwd_waves=2, bwd_waves=2)),
        _case("155, WAVES=1, fused backward", 2, 155, 100, 2, 128, 0.3, precs=h16, knobs=dict(ATTN_WAVES=1), want16=dict(fwd="mfma", bwd="fused_ks", fwd_waves=1)),
        _case("300 in fp32: ten row blocks on eight waves", 1, 300, 100, 2, 128, 0.3, precs=["fp32"], want32=dict(f32, fwd_waves=8, bwd_waves=8)),
    ]


def _row_edge_cases():
    mk, f32 = dict(fwd="mfma", bwd="rows_keys"), dict(fwd="f32", bwd="f32")
    return [
        _case("S = F: no query row", 2, 40, 40, 2, 64, 0.3, want16=mk, want32=f32),
        _case("F = 32, S = 33: the query row opens a block", 2, 33, 32, 2, 64, 0.3, want16=mk, want32=f32),
        _case("S = F = 1", 2, 1, 1, 2, 32, 0.3, want16=mk, want32=f32),
    ]


def _simple_cases():
    sm = dict(fwd="simple", bwd="simple")
    out = [_case("simple Dh=16 H=3", 2, 31, 12, 3, 16, 0.3, want16=sm, want32=sm),
           _case("simple 64 x three key blocks F=66", 2, 70, 66, 2, 64, 0.3, want16=sm, want32=sm),
           _case("simple Dh=80 F=20", 2, 27, 20, 2, 80, 0.3, want16=sm, want32=sm),
           _case("simple 128x4 under ATTN_FP32", 2, 134, 97, 2, 128, 0.3, fp32=True, want16=sm, want32=sm),
           _case("simple peaked Dh=16", 2, 31, 12, 3, 16, 0.3, peaked=True, want16=sm, want32=sm)]
    for F in (64, 65, 129, 192):      # the keys-per-lane edges and the KPL limit (head width 16 is in no table entry)
        out.append(_case("simple F=%d" % F, 2, F + 5, F, 2, 16, 0.3, want16=sm, want32=sm))
    return out


GPU_CASES = {"table": _table_cases(), "split": _split_cases(), "rows": _row_edge_cases(), "simple": _simple_cases()}


def expected_family(cs, prec):
    """assert that the dispatch rule gives the case what it is meant for; returns family_of's answer"""
    fam = family_of(prec, dict(B=cs.B, S=cs.S, F=cs.F, H=cs.H, Dh=cs.Dh, fp32=cs.fp32), cs.knobs)
    for key, val in cs.want["h16" if prec in HALF_ULP else "f32"].items():
        assert getattr(fam, key) == val, (cs.name, prec, key, getattr(fam, key), val)
    return fam
