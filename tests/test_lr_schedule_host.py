"""The learning-rate schedule of tim_amd/schedule.py without a GPU: `lr_at` - the float64 definition rounded once to fp32 -
against torch's own CosineAnnealingLR and a restatement of pytorch_warmup's LinearWarmup written here; `FusedAdamW` plus schedule
on CPU tensors against clip_grad_norm_ + torch.optim.AdamW fed the same rates; the attachment rules and the state.  On the GPU:
tests/test_gpu_lr_schedule.py."""
import math

import numpy as np
import pytest
import torch

import tim_amd
from tim_amd import _lib
from tim_amd.optim import FusedAdamW
from tim_amd.schedule import CosineWarmupSchedule


def _f32(x):
    return float(np.float32(x))


def _sched(base=1e-4, T_max=10, eta_min=1e-6, warmup_period=0, groups=None):
    groups = groups or [{"params": [torch.zeros(3, requires_grad=True)], "lr": base}]
    opt = FusedAdamW(groups, lr=base)
    return opt, CosineWarmupSchedule(opt, T_max, eta_min=eta_min, warmup_period=warmup_period)


def _torch_cosine(base, eta_min, T_max):
    opt = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=base)
    return opt, torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=T_max, eta_min=eta_min)


@pytest.mark.parametrize("base,eta_min,T_max,steps", [(1e-4, 1e-6, 1000, 1000), (1e-4, 1e-6, 37, 37), (1e-3, 0.0, 1, 5),
                                                      (1e-4, 1e-6, 7, 30)])
def test_cosine_part_equals_torch_after_rounding_to_fp32(base, eta_min, T_max, steps):
    """torch's scheduler driven step by step (its recursive form, a Python double carried along; past T_max it simply goes on)
    against the closed form evaluated afresh: equal once both are rounded to fp32 - a condition, not a tolerance"""
    _, sched = _sched(base, T_max, eta_min)
    opt, cos = _torch_cosine(base, eta_min, T_max)
    worst = 0.0
    for t in range(steps + 1):
        want = opt.param_groups[0]["lr"]
        got = sched.lr_at(t)
        unrounded = eta_min + (base - eta_min) * (1 + math.cos(math.pi * t / T_max)) / 2
        worst = max(worst, abs(unrounded - want) / max(abs(want), 1e-300))
        assert got == _f32(got) and got == _f32(want), (t, got, want)
        opt.step()
        cos.step()
    print("largest relative distance of the closed form from torch's double over %d steps: %.3g" % (steps, worst))


@pytest.mark.parametrize("T_max", [9, 40])
@pytest.mark.parametrize("P_of", ["1", "2", "5", "T_max", "T_max + 3"])
def test_warmup_equals_a_restatement_of_linear_warmup(T_max, P_of):
    """pytorch_warmup.LinearWarmup restated: it keeps the undampened rates, dampens once when constructed, and `dampening()`
    restores the kept rates around `lr_scheduler.step()`, keeps the new ones and multiplies by min(1, (step + 1) / P)"""
    P = eval(P_of, {"T_max": T_max})
    base, eta_min = 1e-4, 1e-6
    _, sched = _sched(base, T_max, eta_min, warmup_period=P)
    opt, cos = _torch_cosine(base, eta_min, T_max)
    grp = opt.param_groups[0]
    kept, step = grp["lr"], 0
    grp["lr"] = kept * min(1.0, (step + 1) / P)                    # LinearWarmup.__init__ -> dampen()
    for t in range(T_max + 8):
        assert sched.lr_at(t) == _f32(grp["lr"]), (t, sched.lr_at(t), grp["lr"])
        if t == 0:
            assert sched.lr_at(0) == _f32(base / P)
        opt.step()
        grp["lr"] = kept                                           # with warmup_scheduler.dampening():
        cos.step()                                                 #     lr_scheduler.step()
        kept, step = grp["lr"], step + 1
        grp["lr"] = kept * min(1.0, (step + 1) / P)


def test_two_groups_keep_their_ratio():
    ps = [torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)]
    opt, sched = _sched(T_max=20, eta_min=0.0, warmup_period=4, groups=[{"params": [ps[0]], "lr": 1e-3}, {"params": [ps[1]], "lr": 2.5e-4}])
    assert sched.base_lrs == [1e-3, 2.5e-4]
    for t in range(30):
        a, b = sched.lr_at(t, 0), sched.lr_at(t, 1)
        assert abs(a - 4.0 * b) <= 2.0 ** -23 * a, (t, a, b)      # (eta_min = 0: the curve is base_lr times one factor)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    assert sched.last_lr() == [sched.lr_at(0, 0), sched.lr_at(0, 1)] and sched.t == 1


def _three(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=dtype).requires_grad_(True) for s in [(5, 7), (9,), (3,)]]


def _rel(a, b):
    return ((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-12)])    # tests/test_optim_host.py's tolerances
def test_cpu_training_follows_torch_adamw_fed_the_same_rates(dtype, tol):
    ps, qs = _three(dtype), _three(dtype)
    ours = FusedAdamW(ps, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.05, max_grad_norm=0.5)
    sched = CosineWarmupSchedule(ours, T_max=10, eta_min=1e-4, warmup_period=3)
    ref = torch.optim.AdamW(qs, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.05)
    for t in range(12):
        g = torch.Generator().manual_seed(10 + t)
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, generator=g, dtype=dtype)
            p.grad, q.grad = gr.clone(), gr.clone()
        ref.param_groups[0]["lr"] = sched.lr_at(t)
        torch.nn.utils.clip_grad_norm_(qs, 0.5)
        ours.step()
        ref.step()
        assert sched.last_lr() == [sched.lr_at(t)] and sched.t == t + 1
    rates = [sched.lr_at(t) for t in range(12)]
    assert rates[0] == _f32(1e-2 / 3) and rates[2] == max(rates) and rates[10] == _f32(1e-4) and rates[11] > rates[10]
    for p, q in zip(ps, qs):
        assert _rel(p, q) <= tol
    assert ours.param_groups[0]["lr"] == 1e-2                      # the host number is neither read nor written


def test_skipped_step_advances_the_schedule_and_moves_nothing():
    ps = _three(torch.float64)
    opt = FusedAdamW(ps, lr=1e-2, max_grad_norm=1.0)
    sched = CosineWarmupSchedule(opt, T_max=10, warmup_period=2)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    snap = [p.detach().clone() for p in ps]
    ps[1].grad[3] = float("inf")
    opt.step()
    assert int(opt.skipped_steps) == 1 and sched.t == 2 and sched.last_lr() == [sched.lr_at(1)]
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, snap))
    assert float(opt.state_dict()["state"][0]["step"]) == 1.0
    ps[1].grad[3] = 1.0
    opt.step()
    assert sched.last_lr() == [sched.lr_at(2)] and float(opt.state_dict()["state"][0]["step"]) == 2.0


def test_state_round_trip_set_step_and_the_attachment_rules():
    opt, sched = _sched(3e-3, T_max=50, eta_min=1e-5, warmup_period=7)
    assert tim_amd.CosineWarmupSchedule is CosineWarmupSchedule
    p = opt.param_groups[0]["params"][0]
    p.grad = torch.ones_like(p)
    for _ in range(4):
        opt.step()
    sd = sched.state_dict()
    assert sd == {"t": 4, "base_lrs": [3e-3], "T_max": 50, "eta_min": 1e-5, "warmup_period": 7}
    assert all(type(v) in (int, float, list) for v in sd.values()) and type(sd["base_lrs"][0]) is float
    opt2, sched2 = _sched(1.0, T_max=3)
    sched2.load_state_dict(sd)
    assert sched2.state_dict() == sd and [sched2.lr_at(t) for t in range(60)] == [sched.lr_at(t) for t in range(60)]
    sched.set_step(20)
    assert sched.t == 20
    opt.step()
    assert sched.last_lr() == [sched.lr_at(20)] and sched.state_dict()["t"] == 21
    with pytest.raises(RuntimeError, match="already has a schedule"):
        CosineWarmupSchedule(opt, 10)
    with pytest.raises(RuntimeError, match="the optimizer advances the schedule"):
        sched.step()
    with pytest.raises(TypeError):
        CosineWarmupSchedule(torch.optim.AdamW([torch.zeros(1, requires_grad=True)]), 10)
    for bad in [dict(T_max=0), dict(T_max=2.0), dict(T_max=True), dict(T_max=5, warmup_period=-1), dict(T_max=5, warmup_period=1.5),
                dict(T_max=5, eta_min=-1e-6), dict(T_max=5, eta_min=float("nan")), dict(T_max=5, eta_min=float("inf"))]:
        with pytest.raises(ValueError):
            CosineWarmupSchedule(FusedAdamW([torch.zeros(1, requires_grad=True)]), **bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            sched.set_step(bad)
    with pytest.raises(ValueError):
        sched2.load_state_dict(dict(sd, base_lrs=[1e-3, 1e-3]))
    many = [{"params": [torch.zeros(1, requires_grad=True)]} for _ in range(_lib.OPT_MAX_STATES + 1)]
    with pytest.raises(ValueError):
        FusedAdamW(many)                                           # (the optimizer's own limit: a schedule never sees more groups)


def test_detach_hands_the_rate_back_to_the_host():
    ps, qs = _three(torch.float64), _three(torch.float64)
    opt = FusedAdamW(ps, lr=1e-2)
    sched = CosineWarmupSchedule(opt, T_max=10, warmup_period=4)
    ref = torch.optim.AdamW(qs, lr=1e-2)

    def both(lr_ref):
        for p, q in zip(ps, qs):
            p.grad, q.grad = torch.ones_like(p), torch.ones_like(q)
        ref.param_groups[0]["lr"] = lr_ref
        opt.step()
        ref.step()

    opt.param_groups[0]["lr"] = 0.5                                # attached: a host write has no effect
    both(sched.lr_at(0))
    sched.detach()
    assert opt._schedule is None
    both(0.5)                                                      # detached: it takes effect again
    opt.param_groups[0]["lr"] = 3e-3
    both(3e-3)
    for p, q in zip(ps, qs):
        assert _rel(p, q) <= 1e-12
    assert sched.state_dict()["t"] == 1
    CosineWarmupSchedule(opt, T_max=10)                            # and the optimizer takes a new schedule


def test_a_step_without_gradients_is_not_counted_and_the_counter_is_read_only():
    opt, sched = _sched(1e-3, T_max=10, warmup_period=2)
    opt.step()                                                     # no parameter has a gradient: FusedAdamW returns before it is a step
    assert sched.t == 0 and sched.last_lr() == [0.0]
    with pytest.raises(AttributeError):
        sched.t = 3                                                # (set_step is the way: one counter, shared by the groups)
    assert _lib.ABI_VERSION == 6 and not [n for n in _lib.exported_symbols() if "schedule" in n]   # the library is untouched
