"""tests/losses_ref.py (the float64 closed forms the GPU loss-kernel tests check against) pinned to the oracle under float64 autograd
and to the reference-generated vectors tests/golden/loss_*.npz.  CPU only."""
import os

import numpy as np
import pytest
import torch

from oracle import tim_oracle as O
from tests import losses_ref as R
from tests.helpers import GOLDEN
from tests.test_loss_oracle import CE_CASES, DET_CASES, DIOU_TIE_CASES, ce_inputs, det_inputs

F64 = torch.float64


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ cross entropy
def _oracle_ce(x, ya, yb, lam, eps):
    """O.mixup_ce with the kernel's meaning of a target outside [0, C) (ignored) and of a side without a valid row (term 0)"""
    C = x.shape[1]
    fix = lambda y: None if y is None else torch.where((y >= 0) & (y < C), y, torch.full_like(y, -1))
    ya, yb = fix(ya), fix(yb)
    xr = x.clone().requires_grad_(True)
    crit = torch.nn.CrossEntropyLoss(label_smoothing=eps, ignore_index=-1)
    loss = xr.sum() * 0.0
    if bool((ya != -1).any()):
        loss = loss + lam * crit(xr[ya != -1], ya[ya != -1])
    if yb is not None and bool((yb != -1).any()):
        loss = loss + (1.0 - lam) * crit(xr[yb != -1], yb[yb != -1])
    loss.backward()
    return loss.detach(), xr.grad


@pytest.mark.parametrize("case", CE_CASES)
def test_ce_ref_matches_golden_and_oracle(case):
    g = np.load(os.path.join(GOLDEN, case))
    x, ya, yb, lam = ce_inputs(g)
    r = R.ce_mixup(x, ya, yb, lam, 0.2)
    assert abs(r["loss"].item() - float(g["loss"])) < 1e-12
    d = r["dlogits"].numpy()
    assert np.abs(d[:, :128] - g["dlogits"]).max() < 1e-7            # (the fixture stores these columns in fp32)
    assert np.abs(np.abs(d).sum(1) - g["row_abs"]).max() < 1e-10
    assert np.abs(d.sum(1) - g["row_sum"]).max() < 1e-10
    xo = x.clone().requires_grad_(True)
    lo = O.mixup_ce(xo, ya, yb, lam, 0.2)
    lo.backward()
    assert abs(lo.item() - r["loss"].item()) < 1e-12 and (xo.grad - r["dlogits"]).abs().max().item() < 1e-12


@pytest.mark.parametrize("eps", [0.0, 0.2])
@pytest.mark.parametrize("rows,C", [(1, 5), (7, 13), (6, 1024)])
def test_ce_ref_edges(rows, C, eps):
    """targets -1, C - 1, C and C + 7; yb None; one side with no valid row while lam = 0.3; an upstream gradient"""
    x = torch.randn(rows, C, generator=gen(rows), dtype=F64) * 3.0
    ya = torch.tensor([C - 1, -1, C, C + 7, 0, 3, 2][:rows])
    for yb, lam in ((None, 1.0), (torch.tensor([2, C - 1, -1, 1, C + 7, C, 0][:rows]), 0.3), (torch.full((rows,), -1), 0.3),
                    (torch.full((rows,), C), 0.3)):
        r = R.ce_mixup(x, ya, yb, lam, eps, g=1.7)
        lo, go = _oracle_ce(x, ya, yb, lam, eps)
        assert abs(r["loss"].item() - lo.item()) < 1e-12
        assert (r["dlogits"] - 1.7 * go).abs().max().item() < 1e-12
        va = (ya >= 0) & (ya < C)
        assert r["accum"][1].item() == float(va.sum()) and bool((r["stats"][~va, 2] == -1).all())
        assert bool((r["stats"][va, 2] >= 0).all())
        assert (r["stats"][:, 0] - torch.logsumexp(x, 1)).abs().max().item() < 1e-12


# ------------------------------------------------------------------------------------------------ focal
def _focal_inputs(rows, C, seed):
    x = torch.randn(rows, C, generator=gen(seed), dtype=F64) * 3.0
    t = torch.rand(rows, C, generator=gen(seed + 1), dtype=F64).pow(6.0)
    t[0, :] = 0.0
    t[1 % rows, ::2] = 1.0
    w = torch.rand(rows, generator=gen(seed + 2), dtype=F64) + 0.5
    valid = torch.rand(rows, generator=gen(seed + 3)) > 0.3
    return x, t, w, valid


@pytest.mark.parametrize("alpha", [-1.0, 0.25])
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 3.0])
def test_focal_ref_matches_oracle(gamma, alpha):
    x, t, w, valid = _focal_inputs(23, 11, 5)
    for ww, vv in ((None, None), (w, None), (None, valid), (w, valid)):
        elem, tot, dx = R.focal(x, t, ww, vv, alpha, gamma, g=0.6)
        keep = torch.ones(23, dtype=torch.bool) if vv is None else vv
        xo = x.clone().requires_grad_(True)
        lo = O.focal_loss(xo[keep], t[keep], None if ww is None else ww[keep], alpha, gamma)
        lo.backward()
        assert abs(tot.item() - lo.item()) < 1e-10 * max(1.0, abs(lo.item()))
        assert (dx - 0.6 * xo.grad).abs().max().item() < 1e-10
        eo = O.focal_loss(x[keep], t[keep], None if ww is None else ww[keep], alpha, gamma, reduction="none")
        assert (elem[keep] - eo).abs().max().item() < 1e-12 and bool((elem[~keep] == 0).all()) and bool((dx[~keep] == 0).all())


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 3.0])
def test_focal_ref_saturated_logits(gamma):
    """logits of +-20, +-90, +-200 against hard and smoothed targets: the closed form is finite everywhere, equals autograd of the
    oracle where that is finite, and is 0 where the oracle's autograd reads 0 * inf (q == 0 under gamma < 1: the limit is 0)"""
    xs = torch.tensor([20.0, -20.0, 90.0, -90.0, 200.0, -200.0], dtype=F64)
    ts = torch.tensor([0.0, 1.0, 0.9, 0.001], dtype=F64)
    x, t = xs[:, None].expand(6, 4).contiguous(), ts[None, :].expand(6, 4).contiguous()
    elem, tot, dx = R.focal(x, t, None, None, 0.25, gamma)
    assert bool(torch.isfinite(elem).all() and torch.isfinite(dx).all())
    xo = x.clone().requires_grad_(True)
    O.focal_loss(xo, t, None, 0.25, gamma).backward()
    fin = torch.isfinite(xo.grad)
    # the oracle computes 1 - p where the closed form uses sigmoid(-x): they differ by the rounding of p near 1, 2^-53 in q
    sc = dx.abs() + 1e-12
    assert bool(((dx - xo.grad).abs()[fin] <= 1e-6 * sc[fin] + 1e-14).all())
    assert bool((dx[~fin].abs() < 1e-30).all())
    if gamma >= 1.0:
        assert bool(fin.all())
    # float32 evaluation of the kernel's own order of operations: finite on the same inputs
    e32, _, d32 = R.focal(x.float(), t.float(), None, None, 0.25, gamma)
    assert bool(torch.isfinite(e32).all() and torch.isfinite(d32).all())


@pytest.mark.parametrize("case", DET_CASES)
def test_focal_and_diou_ref_match_golden(case):
    g = np.load(os.path.join(GOLDEN, case))
    logits, targets, w, valid = det_inputs(g)
    elem, tot, dx = R.focal(logits.double(), targets.double(), w.double(), valid, 0.25, 2.0)
    # the vectors are the reference's fp32 run: the float64 closed form is held to them at fp32 resolution (32 roundings of
    # u = 2^-24 along the chain sigmoid - BCE - power - weight and its autograd), and to the float64 oracle at 1e-10
    assert abs(tot.item() - float(g["focal"])) <= 1e-6 * abs(float(g["focal"]))
    assert np.abs(dx.numpy() - g["dlogits"]).max() <= 32 * R.EPS32 * np.abs(g["dlogits"]).max()
    xo = logits.double().requires_grad_(True)
    lo = O.focal_loss(xo[valid], targets.double()[valid], w.double()[valid])
    lo.backward()
    assert abs(tot.item() - lo.item()) <= 1e-10 * lo.item() and (dx - xo.grad).abs().max().item() <= 1e-10
    assert np.abs(elem[valid].sum(1).numpy() - g["elem_rowsum"]).max() <= 1e-5 * np.abs(g["elem_rowsum"]).max()
    loss, d, _, _ = R.diou_1d(torch.from_numpy(g["pred"]).double(), torch.from_numpy(g["off"]).double())
    assert abs(loss.sum().item() - float(g["diou"])) <= 1e-6 * abs(float(g["diou"]))
    assert np.abs(d.numpy() - g["dpred"]).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ DIoU
@pytest.mark.parametrize("case", DIOU_TIE_CASES + DET_CASES)
def test_diou_ref_matches_oracle_and_takes_one_branch(case):
    g = np.load(os.path.join(GOLDEN, case))
    p32, o32 = torch.from_numpy(g["pred"]), torch.from_numpy(g["off"])
    valid = torch.arange(p32.shape[0]) % 5 != 2
    for vv in (None, valid):
        loss, d, br, scale = R.diou_1d(p32.double(), o32.double(), vv, 1e-8, g=1.3)
        keep = torch.ones(p32.shape[0], dtype=torch.bool) if vv is None else vv
        po = p32.double().requires_grad_(True)
        lo = O.diou_1d(po[keep], o32.double()[keep])
        lo.backward()
        assert abs(loss.sum().item() - lo.item()) <= 1e-12 * abs(lo.item())
        assert bool(((d - 1.3 * po.grad).abs() <= 1e-12 * scale[:, None]).all())
        assert bool((d[~keep] == 0).all() and (loss[~keep] == 0).all())
    # a float32 and a float64 evaluation take the same branch in every row (ties are exact, clamps are a factor 4 from eps)
    loss, d, br, scale = R.diou_1d(p32.double(), o32.double())
    l32, d32, br32, _ = R.diou_1d(p32, o32)
    assert torch.equal(br, br32)
    lp, rp, lg, rg = (t.double() for t in (p32[:, 0], p32[:, 1], o32[:, 0], o32[:, 1]))
    U = (lp + rp) + (lg + rg) - torch.minimum(lp, lg) - torch.minimum(rp, rg)
    Lc = torch.maximum(lp, lg) + torch.maximum(rp, rg)
    for v in (U, Lc):
        assert bool(((v == 0) | (v <= 1e-8 / 4) | (v >= 4e-8)).all())
    assert bool(((d32.double() - d).abs() <= 8 * R.EPS32 * scale[:, None]).all())
    if case in DIOU_TIE_CASES:     # the reference's own compiled-call gradient and per-row loss, computed in fp32
        assert bool(((d - torch.from_numpy(g["dpred"]).double()).abs() <= 8 * R.EPS32 * scale[:, None]).all())
        assert np.abs(loss.numpy() - g["rowloss"]).max() <= 8 * R.EPS32 * 2.0
        assert abs(loss.sum().item() - float(g["diou"])) <= 1e-6 * float(g["diou"])


# ------------------------------------------------------------------------------------------------ detection side
@pytest.mark.parametrize("heads,npos,gamma,alpha", [(1, 9, 2.0, 0.25), (3, 9, 0.5, -1.0), (4, 0, 3.0, 0.25), (2, 9, 1.0, 0.25)])
def test_det_side_ref_matches_composition(heads, npos, gamma, alpha):
    rows, thr, lam, mom, norm0 = 40, 0.6, 0.5, 0.9, 17.0
    gg = gen(heads)
    Cs = [5, 1, 9, 3][:heads]
    xs = [torch.randn(rows, c, generator=gg, dtype=F64) * 2 for c in Cs]
    ts = [torch.rand(rows, c, generator=gg, dtype=F64).pow(4.0) for c in Cs]
    iou = torch.rand(rows, generator=gg, dtype=F64)
    iou[::7] = -1.0
    off = torch.full((rows, 2), float("inf"), dtype=F64)
    pos = torch.zeros(rows, dtype=torch.bool)
    pos[torch.nonzero(iou >= thr).flatten()[:npos]] = True
    off[pos] = torch.rand(int(pos.sum()), 2, generator=gg, dtype=F64)
    reg = torch.rand(rows, 2, generator=gg, dtype=F64)
    block, nm, dxs, dreg = R.det_side(xs, ts, iou, off, reg, thr, alpha, gamma, 1e-8, lam, mom, norm0, g=0.7)
    xo = [x.clone().requires_grad_(True) for x in xs]
    ro = reg.clone().requires_grad_(True)
    valid, w = iou >= 0, torch.where(iou < thr, torch.ones_like(iou), iou)
    n = int(pos.sum())
    want_nm = mom * norm0 + (1 - mom) * max(n, 1)
    tot = sum(O.focal_loss(x[valid], t[valid], w[valid], alpha, gamma) for x, t in zip(xo, ts)) / (heads * want_nm)
    if n > 0:
        tot = tot + lam * O.diou_1d(ro[pos], off[pos]) / want_nm
    (tot * 0.7).backward()
    assert abs(nm - want_nm) < 1e-12 and abs(block[0].item() - tot.item()) < 1e-12 and block[3].item() == n and block[4].item() == nm
    assert bool((block[5:] == 0).all())
    for d, x in zip(dxs, xo):
        assert (d - x.grad).abs().max().item() < 1e-12 and bool((d[~valid] == 0).all())
    want_r = ro.grad if ro.grad is not None else torch.zeros_like(reg)
    assert (dreg - want_r).abs().max().item() < 1e-12 and bool((dreg[~pos] == 0).all())


# ------------------------------------------------------------------------------------------------ DRLoc
def test_drloc_ref_matches_oracle_gather_and_its_adjoint():
    n, l, D, m = 3, 5, 4, 6
    feats = torch.randn(n, 2 * l, D, generator=gen(1), dtype=F64)
    p1, p2 = torch.randint(l, (n, m), generator=gen(2)), torch.randint(l, (n, m), generator=gen(3))
    base = feats.reshape(-1)
    idx = lambda x, pos: torch.gather(x, 1, pos.unsqueeze(-1).expand(-1, -1, D))          # collect_samples (oracle/tim_oracle.py)
    for (x1, x2, o2, sb) in ((feats[:, :l], feats[:, l:], l * D, 2 * l * D), (feats[:, :l], feats[:, :l], 0, 2 * l * D)):
        out = R.drloc_gather(base, 0, o2, sb, D, D, p1, p2, m)
        assert torch.equal(out, torch.cat([idx(x1, p1), idx(x2, p2)], dim=2).reshape(n * m, 2 * D))
        gr = torch.randn(n * m, 2 * D + 3, generator=gen(4), dtype=F64)
        pre = torch.randn(base.numel(), generator=gen(5), dtype=F64)
        got, mag, cnt = R.drloc_scatter_add(gr, pre, 0, o2, sb, D, D, p1, p2, m)
        xb = base.clone().requires_grad_(True)
        (R.drloc_gather(xb, 0, o2, sb, D, D, p1, p2, m) * gr[:, :2 * D]).sum().backward()     # the scatter is the gather's adjoint
        assert (got - (pre + xb.grad)).abs().max().item() < 1e-12
        assert cnt.sum().item() == 2 * n * m * D and bool((mag >= (got - pre).abs() - 1e-12).all())
