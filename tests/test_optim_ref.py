"""tests/optim_ref.py on the CPU: the float64 restatement against torch's own clip + AdamW, and the bounds against an fp32
emulation of the kernel's formula on every input family the GPU tests draw from (tests/test_gpu_optim_edges.py imports the same
generators): the check that the inputs, and not the kernel, keep the bounds honest."""
import math

import pytest
import torch

from tests import optim_ref as R

F64 = torch.float64


def test_float64_step_is_clip_grad_norm_then_adamw():
    """3 steps over two groups with different betas, learning rates and decays, one shared clip: per element within 1e-12
    relative of torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW on float64 tensors (step 1 is clipped, step 2 is not)."""
    gn = torch.Generator().manual_seed(0)
    shapes = [[(5, 7), (33,)], [(64,), (3, 3), (1,)]]
    hyper = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
    mine = [[torch.randn(s, generator=gn, dtype=F64) for s in grp] for grp in shapes]
    theirs = [[p.clone().requires_grad_(True) for p in grp] for grp in mine]
    opt = torch.optim.AdamW([dict(params=ps, **h) for ps, h in zip(theirs, hyper)])
    mom = [[(torch.zeros_like(p), torch.zeros_like(p)) for p in grp] for grp in mine]
    steps = [0, 0]
    max_norm = 1.0
    for it in range(3):
        grads = [[torch.randn(p.shape, generator=gn, dtype=F64) * (0.01 if it == 1 else 1.0) for p in grp] for grp in mine]
        for grp, gs in zip(theirs, grads):
            for p, g in zip(grp, gs):
                p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([p for grp in theirs for p in grp], max_norm)
        opt.step()
        n64 = R.norm([g for gs in grads for g in gs])
        assert abs(n64 - total.item()) <= 1e-12 * total.item()
        for gi, h in enumerate(hyper):
            _, coef, bad, steps[gi], bc1, bc2s = R.finish(n64, max_norm, [], steps[gi], *h["betas"], exact=True)
            assert not bad and (coef < 1.0) == (it != 1)
            for i, p in enumerate(mine[gi]):
                m, v = mom[gi][i]
                p1, m1, v1 = R.update(p, grads[gi][i], m, v, coef, h["lr"], bc1, bc2s, *h["betas"], h["eps"], h["weight_decay"],
                                      exact=True)
                mine[gi][i], mom[gi][i] = p1, (m1, v1)
    for gi in range(2):
        for i, q in enumerate(theirs[gi]):
            st = opt.state[q]
            for a, b in ((mine[gi][i], q.detach()), (mom[gi][i][0], st["exp_avg"]), (mom[gi][i][1], st["exp_avg_sq"])):
                assert bool(((a - b).abs() <= 1e-12 * b.abs()).all()), (gi, i, ((a - b).abs() / b.abs()).max().item())
            assert float(st["step"]) == 3.0 == steps[gi]


def test_finish_follows_the_header():
    n32, coef, bad, t, bc1, bc2s = R.finish(4.0, 1.0, [0, 0], 9, 0.9, 0.999)
    assert (n32, bad, t) == (4.0, False, 10) and coef == R.f32(1.0 / (4.0 + R.CLIP_EPS))
    assert bc1 == R.f32(1.0 - 0.9 ** 10) and bc2s == R.f32(math.sqrt(1.0 - 0.999 ** 10))
    assert R.finish(0.5, 1.0, [], 0, 0.9, 0.999)[1] == 1.0 and R.finish(1e30, 0.0, [], 0, 0.9, 0.999)[1] == 1.0
    assert R.finish(4.0, 1.0, [0, 5], 9, 0.9, 0.999)[2:4] == (True, 9)
    assert R.finish(1e39, 1.0, [], 9, 0.9, 0.999)[2:4] == (True, 9)            # finite in fp64, inf as fp32
    assert R.finish(float("nan"), 1.0, [], 9, 0.9, 0.999)[2:4] == (True, 9)
    assert R.finish(0.0, 1.0, [], 0, 0.0, 0.5)[3:] == (1, 1.0, R.f32(math.sqrt(0.5)))


# (family, max_norm) as the GPU tests use them; the settings span t = 1 .. 100000, the three beta pairs and coef 1e-17 .. 1
SETTINGS = [(fam, mn, step, betas, lr, wd)
            for fam, mn in (("normal", 1.0), ("normal", 0.0), ("small_grad", 1.0), ("wide", 1.0), ("zero_grad", 1.0), ("huge", 1.0))
            for step, betas, lr, wd in ((0, R.BETAS[0], 1e-2, 0.05), (9, R.BETAS[1], 1e-3, 0.0), (999, R.BETAS[2], 0.0, 0.01),
                                        (99999, R.BETAS[0], 3e-2, 0.5))]


@pytest.mark.parametrize("fam,max_norm,step,betas,lr,wd", SETTINGS)
def test_fp32_emulation_stays_inside_the_bounds(fam, max_norm, step, betas, lr, wd):
    """The kernel's formula in torch's fp32 (no fused multiply-adds) against the float64 reference: below 1.0 of every bound.
    The norm and the clip coefficient, emulated as 16-term fp32 lane sums under a float64 total, stay inside theirs."""
    n = 200000
    p, g, m, v = R.FAMILIES[fam](n, 11 + step)
    n64 = R.norm([g])
    n32, coef, bad, t, bc1, bc2s = R.finish(n64, max_norm, [], step, *betas)
    assert not bad and t == step + 1
    lanes = g[:n - n % 16].reshape(-1, 16)
    acc = torch.zeros(lanes.shape[0])
    for j in range(16):
        acc = acc + lanes[:, j] * lanes[:, j]
    emu = R.f32(math.sqrt(float(acc.double().sum()) + float(g[n - n % 16:].double().square().sum())))
    assert abs(emu - n64) <= R.NORM_LIMIT * n64
    if max_norm > 0:
        import numpy as np
        c = float(min(np.float32(1.0), np.float32(max_norm) / (np.float32(emu) + np.float32(1e-6))))
        assert abs(c - coef) <= R.COEF_LIMIT * coef
    args = (p, g, m, v, coef, R.f32(lr), bc1, bc2s, betas[0], betas[1], 1e-8, wd)
    ref, lim, out = R.update(*args), R.bounds(*args), R.emulate_fp32(*args)
    ratios = [R.ratio(o, r, l) for o, r, l in zip(out, ref, lim)]
    print("fp32 emulation / bound (p, m, v): %.3f %.3f %.3f  %s t=%d betas=%s coef=%.3g" % (tuple(ratios) + (fam, t, betas, coef)))
    assert all(r < 1.0 for r in ratios), ratios
    if lr == 0.0:
        assert torch.equal(out[0], p)                      # lr = 0: no decay, no update


def test_ratio_rejects_what_it_should():
    ref, lim = torch.tensor([1.0, 0.0], dtype=F64), torch.tensor([1e-7, 0.0], dtype=F64)
    assert R.ratio(torch.tensor([1.0, 0.0]), ref, lim) == 0.0
    assert R.ratio(torch.tensor([1.0 + 2.0 ** -22, 0.0]), ref, lim) > 1.0
    assert R.ratio(torch.tensor([1.0, 1e-40]), ref, lim) == float("inf")       # a zero limit asks for the exact value
    assert R.ratio(torch.tensor([float("nan"), 0.0]), ref, lim) == float("inf")
    # swapped moments are far outside the bounds
    p, g, m, v = R.family_normal(1000, 3)
    args = (p, g, m, v, 1.0, 1e-2, 0.1, 0.1, 0.9, 0.999, 1e-8, 0.01)
    (_, m1, v1), (_, lim_m, lim_v) = R.update(*args), R.bounds(*args)
    assert R.ratio(v1.float(), m1, lim_m) > 1e3 and R.ratio(m1.float(), v1, lim_v) > 1e3
