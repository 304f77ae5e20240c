"""Plain restatements of the eight C entry points of tim_amd/csrc/losses.hip, one function each, written as closed forms (no
autograd) so that they stand apart from the oracle they are pinned to (tests/test_losses_ref.py) and from the kernels they check
(tests/test_gpu_loss_kernels.py).  Every function computes in the dtype of its first argument: float64 is the reference; the
same call on float32 tensors is the "torch-CPU float32 evaluation of the same formulas" whose error against float64 calibrates
the fast-intrinsic allowance of the GPU tests.
"""
import torch

EPS32 = 2.0 ** -24          # unit roundoff of fp32
TINY32 = 2.0 ** -126        # smallest normal fp32: a result below it may be flushed to zero


# ================================================================================================ cross entropy under mixup
def ce_mixup(x, ya, yb, lam, eps, g=1.0):
    """timhip_ce_mixup_fwd / _bwd.  x [rows, C]; ya, yb int64 [rows] (yb may be None); a target outside [0, C) is ignored.
    Returns a dict: loss, stats [rows, 4] = (lse, mean, ce_a | -1, ce_b | -1), accum = (sum_a, n_a, sum_b, n_b) and
    dlogits = g * d loss / d x by the closed formula
        (wa + wb) softmax - wa ((1-eps) 1[c = ya] + eps / C) - wb ((1-eps) 1[c = yb] + eps / C),
        wa = lam / n_a on the rows of side a, wb = (1 - lam) / n_b on the rows of side b."""
    rows, C = x.shape
    mx = x.max(dim=1, keepdim=True).values
    lse = (mx + (x - mx).exp().sum(1, keepdim=True).log()).squeeze(1)
    mean = x.sum(1) / C
    stats = torch.full((rows, 4), -1.0, dtype=x.dtype)
    stats[:, 0], stats[:, 1] = lse, mean
    accum = torch.zeros(4, dtype=x.dtype)
    w = []
    for k, (y, coef) in enumerate(((ya, lam), (yb, 1.0 - lam))):
        v = torch.zeros(rows, dtype=torch.bool) if y is None else (y >= 0) & (y < C)
        idx = torch.nonzero(v).flatten()
        if idx.numel():
            ce = (1.0 - eps) * (lse[idx] - x[idx, y[idx]]) + eps * (lse[idx] - mean[idx])
            stats[idx, 2 + k] = ce
            accum[2 * k], accum[2 * k + 1] = ce.sum(), float(idx.numel())
        wk = torch.zeros(rows, dtype=x.dtype)
        if idx.numel():
            wk[idx] = g * coef / idx.numel()
        w.append((wk, v, idx, y))
    la = accum[0] / accum[1] if accum[1] > 0 else accum[0] * 0
    lb = accum[2] / accum[3] if accum[3] > 0 else accum[2] * 0
    loss = lam * la + (1.0 - lam) * lb
    wsum = (w[0][0] + w[1][0])[:, None]
    d = wsum * (x - lse[:, None]).exp() - wsum * eps / C
    for wk, v, idx, y in w:
        if idx.numel():
            d[idx, y[idx]] -= wk[idx] * (1.0 - eps)
    return {"loss": loss, "stats": stats, "accum": accum, "dlogits": d}


# ================================================================================================ sigmoid focal loss
def focal_terms(x, t, alpha, gamma, stable=None):
    """per-element focal loss and its derivative in x, no weights.
        loss = a_t ce (1 - p_t)^gamma,  ce = max(x, 0) - x t + log1p(exp(-|x|)),  p_t = p t + (1 - p)(1 - t)
        d loss / d x = a_t [ (p - t) q^gamma - ce gamma q^(gamma-1) (2t - 1) p (1 - p) ],  q = 1 - p_t
    The second term is 0 where p (1 - p) q^(gamma-1) has the limit 0 and its factors read 0 * inf (q = 0 needs t in {0, 1} and
    p = t, where p (1 - p) = q (1 - q)): autograd of the reference's expression gives NaN there for gamma < 1, the limit is 0.
    stable (default: for float64): 1 - p as sigmoid(-x) and q as p (1 - t) + (1 - p) t, so that the reference keeps its digits
    where p rounds to 1; otherwise the kernel's own order of operations (1 / (1 + exp(-x)), 1 - p, 1 - p_t)."""
    if stable is None:
        stable = x.dtype == torch.float64
    if stable:
        p, np_ = torch.sigmoid(x), torch.sigmoid(-x)
        q = p * (1.0 - t) + np_ * t
    else:
        p = 1.0 / (1.0 + (-x).exp())
        np_ = 1.0 - p
        q = 1.0 - (p * t + np_ * (1.0 - t))
    ce = x.clamp(min=0) - x * t + torch.log1p((-x.abs()).exp())
    mod = q * q if gamma == 2.0 else q.pow(gamma)
    if gamma == 2.0:
        dmod = 2.0 * q
    else:
        dmod = torch.where(q > 0, gamma * q.pow(gamma - 1.0), torch.zeros_like(q))
    at = alpha * t + (1.0 - alpha) * (1.0 - t) if alpha >= 0 else torch.ones_like(t)
    loss = at * ce * mod
    dx = at * ((p - t) * mod - ce * dmod * (2.0 * t - 1.0) * p * np_)
    return loss, dx, {"p": p, "q": q, "ce": ce, "mod": mod, "dmod": dmod, "at": at, "pp": p * np_}


def _row_factor(rows, w, valid, dtype):
    f = torch.ones(rows, dtype=dtype) if w is None else w.to(dtype).clone()
    if valid is not None:
        f = torch.where(valid.bool(), f, torch.zeros_like(f))
    return f


def focal(x, t, w=None, valid=None, alpha=0.25, gamma=2.0, g=1.0, stable=None):
    """timhip_focal_loss_fwd / _bwd: elementwise loss (rows with valid == 0 give 0), its sum, and dx = g * d sum / d x"""
    loss, dx, _ = focal_terms(x, t, alpha, gamma, stable)
    f = _row_factor(x.shape[0], w, valid, x.dtype)[:, None]
    keep = torch.ones_like(f, dtype=torch.bool) if valid is None else valid.bool()[:, None]
    elem = torch.where(keep, f * loss, torch.zeros_like(loss))          # (an excluded row is 0 whatever its logits hold)
    return elem, elem.sum(), torch.where(keep, g * f * dx, torch.zeros_like(dx))


def focal_bound(x64, t64, alpha, gamma, u=EPS32):
    """first-order fp32 rounding bound of focal_terms per element, (bound_loss, bound_dx), from the float64 intermediates:
    p, 1 - p, p_t and q are values in [0, 1] produced by a handful of roundings each: absolute error dq = 8u (one fast exp, a
    reciprocal, two products, two sums, one difference; the fast exp's relative error of a few u enters p as p (1 - p) times it);
    ce sums three terms of size <= |x| + 1: dce = 4u (|x| + 1) + 4u ce; q^gamma moves by gamma (q + dq)^(gamma-1) dq for
    gamma >= 1 and by at most dq^gamma for gamma < 1 (Hoelder), plus 8u relative for powf itself."""
    _, _, m = focal_terms(x64, t64, alpha, gamma, True)
    q, ce, mod, dmod, at, pp, p = m["q"], m["ce"], m["mod"], m["dmod"], m["at"], m["pp"], m["p"]
    dq = 8 * u
    dce = 4 * u * (x64.abs() + 1.0) + 4 * u * ce
    if gamma >= 1.0:
        dmodv = gamma * (q + dq).pow(gamma - 1.0) * dq + 8 * u * mod
    else:
        dmodv = torch.minimum(torch.full_like(q, dq ** gamma), gamma * q.clamp(min=1e-300).pow(gamma - 1.0) * dq) + 8 * u * mod
    b_loss = at * (dce * mod + ce * dmodv + 4 * u * ce * mod)
    # second term T = ce * [gamma q^(gamma-1) pp] * (2t - 1), pp = p (1 - p) <= q; the bracket's error:
    e = gamma - 1.0
    base = torch.clamp(q, min=dq) if e < 0 else q + dq
    dbr = gamma * (abs(e) * base.pow(e) * dq + base.pow(e) * 4 * u) + 8 * u * dmod * pp
    br = dmod * pp
    s = (2.0 * t64 - 1.0).abs()
    b_dx = at * (dq * mod + (p - t64).abs() * dmodv + s * (dce * br + ce * dbr) + 4 * u * ((p - t64).abs() * mod + s * ce * br))
    return b_loss, b_dx


# ================================================================================================ 1-D DIoU
def diou_1d(pred, off, valid=None, eps=1e-8, g=1.0):
    """timhip_diou_1d: per-row loss 1 - I / max(U, eps) + (rho / max(Lc, eps))^2 and dpred = g * d loss / d pred, rows with
    valid == 0 give 0.  The gradient follows the compiled TorchScript form of the reference:
      * min(a, b) passes a gradient to a only where a < b, max(a, b) only where a > b (strict: nothing at an exact tie);
      * clamp(v, min=eps) passes a gradient only where v >= eps.
    Returns (loss [n], dpred [n, 2], branches [n, 6] = (lp < lg, rp < rg, lp > lg, rp > rg, U >= eps, Lc >= eps), scale [n]) with
    scale = 2 / Uc + 1 / Lcc, the sum of the magnitudes of the gradient's terms (I <= U and |rho| <= Lc / 2)."""
    ok = torch.ones(pred.shape[0], dtype=torch.bool) if valid is None else valid.bool()
    one = torch.ones((), dtype=pred.dtype)
    lp, rp = torch.where(ok, pred[:, 0], one), torch.where(ok, pred[:, 1], one)
    lg, rg = torch.where(ok, off[:, 0], one), torch.where(ok, off[:, 1], one)
    I = torch.minimum(rp, rg) + torch.minimum(lp, lg)
    U = (lp + rp) + (lg + rg) - I
    Lc = torch.maximum(lp, lg) + torch.maximum(rp, rg)
    Uc, Lcc = U.clamp(min=eps), Lc.clamp(min=eps)
    rho = 0.5 * (rp - lp - rg + lg)
    z = rho / Lcc
    loss = 1.0 - I / Uc + z * z
    br = torch.stack([lp < lg, rp < rg, lp > lg, rp > rg, U >= eps, Lc >= eps], dim=1)
    f = br.to(pred.dtype)
    a, b = 1.0 / Uc, I / (Uc * Uc)
    dl = -(f[:, 0] * a - b * f[:, 4] * (1.0 - f[:, 0])) + 2.0 * z * (-0.5 / Lcc - rho / (Lcc * Lcc) * f[:, 5] * f[:, 2])
    dr = -(f[:, 1] * a - b * f[:, 4] * (1.0 - f[:, 1])) + 2.0 * z * (0.5 / Lcc - rho / (Lcc * Lcc) * f[:, 5] * f[:, 3])
    zero = torch.zeros_like(loss)
    d = torch.stack([torch.where(ok, g * dl, zero), torch.where(ok, g * dr, zero)], dim=1)
    return torch.where(ok, loss, zero), d, br, torch.where(ok, 2.0 / Uc + 1.0 / Lcc, zero)


# ================================================================================================ detection side loss
def det_side(logits, targets, iou, off, reg, thr, alpha, gamma, eps, lambda_reg, momentum, norm_in, g=1.0):
    """timhip_det_side_loss_fwd / _bwd.  logits / targets: lists of [rows, C_k].  Returns (block [8], new normaliser,
    [dlogits_k], dreg): block = (loss, focal sum, DIoU sum, positives, normaliser used, 0, 0, 0)."""
    K = len(logits)
    dt = reg.dtype
    valid = iou >= 0
    w = torch.where(iou < thr, torch.ones_like(iou), iou)
    pos = off[:, 0] != float("inf")
    fs, dxs = torch.zeros((), dtype=dt), []
    for x, t in zip(logits, targets):
        _, s, dx = focal(x, t, w, valid, alpha, gamma)
        fs = fs + s
        dxs.append(dx)
    dl, dd, _, _ = diou_1d(reg, off, pos, eps)
    npos = float(pos.sum())
    nm = momentum * norm_in + (1.0 - momentum) * max(npos, 1.0)
    loss = fs / (K * nm) + (lambda_reg * dl.sum() / nm if npos > 0 else 0.0)
    block = torch.zeros(8, dtype=dt)
    block[0], block[1], block[2], block[3], block[4] = loss, fs, dl.sum(), npos, nm
    return block, nm, [dx * (g / (K * nm)) for dx in dxs], dd * (g * lambda_reg / nm)


# ================================================================================================ DRLoc
def drloc_gather(base, o1, o2, sb, sl, D, pos1, pos2, m):
    """timhip_drloc_gather.  x1 / x2 are the [n, l, D] views of the flat buffer `base` that start at elements o1 / o2 with element
    strides (sb, sl, 1): out[(b*m + i), 0:D] = x1[b, pos1[b, i], :], out[.., D:2D] = x2[b, pos2[b, i], :]  (values unchanged)"""
    p1, p2 = pos1.reshape(-1), pos2.reshape(-1)
    b = torch.arange(p1.numel()) // m
    c = torch.arange(D)
    i1 = (o1 + b * sb + p1 * sl)[:, None] + c
    i2 = (o2 + b * sb + p2 * sl)[:, None] + c
    return torch.cat([base[i1], base[i2]], dim=1)


def drloc_scatter_add(gr, base, o1, o2, sb, sl, D, pos1, pos2, m):
    """timhip_drloc_scatter_add onto the flat buffer `base` (dx1 / dx2 start at elements o1 / o2; they may overlap or coincide):
    returns (base + scattered terms, sum of |terms| per element, number of terms per element)."""
    p1, p2 = pos1.reshape(-1), pos2.reshape(-1)
    b = torch.arange(p1.numel()) // m
    c = torch.arange(D)
    idx = torch.cat([((o1 + b * sb + p1 * sl)[:, None] + c).reshape(-1), ((o2 + b * sb + p2 * sl)[:, None] + c).reshape(-1)])
    val = torch.cat([gr[:, :D].reshape(-1), gr[:, D:2 * D].reshape(-1)]).to(base.dtype)
    out = base.clone().index_add_(0, idx, val)
    mag = torch.zeros_like(base).index_add_(0, idx, val.abs())
    cnt = torch.zeros_like(base).index_add_(0, idx, torch.ones_like(val))
    return out, mag, cnt
