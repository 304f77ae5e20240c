"""The learning-rate schedule of tim_amd/schedule.py on the GPU: `FusedAdamW` plus schedule, eagerly, against `reference_step` fed
`lr_at(t)` and inside the per-element bounds of tests/optim_ref.py; the step replayed by `GraphedStep` (the rate of every replay is
the definition's, a host write to `group["lr"]` has no effect, replay == eager); a bare capture is refused; the skipped step;
resume from the two state_dicts; the example.

The LR word of a state block must hold `lr_at(t)` bit for bit: the rate is computed on the host and is an fp32 value already."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import optim_ref as R  # noqa: E402
from tests.test_gpu_graph import _model, _step  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tim_amd.optim import FusedAdamW, reference_step  # noqa: E402
from tim_amd.schedule import CosineWarmupSchedule  # noqa: E402

DEV = "cuda:0"


def _definition(t, base, eta_min, T_max, P):
    cos_lr = eta_min + (base - eta_min) * (1 + math.cos(math.pi * t / T_max)) / 2
    omega = min(1.0, (t + 1) / P) if P >= 1 else 1.0
    return float(np.float32(cos_lr * omega))


def _lr_word(opt, group=0):
    return opt._blocks[group, L.OPT_LR].item()


def _bits(t):
    return t.view(torch.int32)


def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in shapes]


def _set_grads(ps, seed):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)


def test_eager_steps_follow_reference_step_at_the_scheduled_rates():
    """8 steps over T_max = 6 with 3 warm-up steps, two groups.  Per step: the LR words are lr_at(t) bit for bit; p, m, v of every
    tensor element by element inside tests/optim_ref.py's bounds, computed from the state the step started from; at the end the
    trajectory against `reference_step` fed lr_at(t): tests/test_gpu_optim.py holds the kernels to 1e-6 of a tensor's largest entry
    after 5 steps (fp32 arithmetic in another association than torch's); the distance grows with the steps, so 8 / 5 of it."""
    shapes = [(1,), (7,), (65, 33)]
    hyper = dict(betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    ps = _params(shapes, 0)
    opt = FusedAdamW([{"params": ps[:2], "lr": 1e-2}, {"params": ps[2:], "lr": 3e-3}], max_grad_norm=1.0, **hyper)
    sched = CosineWarmupSchedule(opt, T_max=6, eta_min=1e-5, warmup_period=3)
    owner = [0, 0, 1]
    mk = lambda sl: {"params": [p.detach().clone() for p in sl], "grads": None, "exp_avg": [torch.zeros_like(p) for p in sl],   # noqa: E731
                     "exp_avg_sq": [torch.zeros_like(p) for p in sl], "lr": None, "betas": hyper["betas"], "eps": hyper["eps"],
                     "weight_decay": hyper["weight_decay"], "state": {"step": 0, "skipped": 0}}
    ref = [mk(ps[:2]), mk(ps[2:])]
    worst = 0.0
    for t in range(8):
        _set_grads(ps, 100 + t)
        lrs = [sched.lr_at(t, 0), sched.lr_at(t, 1)]
        assert lrs == [_definition(t, 1e-2, 1e-5, 6, 3), _definition(t, 3e-3, 1e-5, 6, 3)]
        before = [(p.detach().cpu(), p.grad.cpu(), opt.state[p]["exp_avg"].cpu() if p in opt.state else torch.zeros(p.shape),
                   opt.state[p]["exp_avg_sq"].cpu() if p in opt.state else torch.zeros(p.shape)) for p in ps]
        for gi, sl in enumerate((ps[:2], ps[2:])):
            ref[gi]["grads"], ref[gi]["lr"] = [p.grad.clone() for p in sl], lrs[gi]
        reference_step(ref, 1.0)
        opt.step()
        assert [R.bits32(_lr_word(opt, gi)) for gi in (0, 1)] == [R.bits32(x) for x in lrs], (t, lrs)
        assert sched.last_lr() == lrs and sched.t == t + 1
        n64 = R.norm([b[1] for b in before])
        _, coef, bad, step1, bc1, bc2s = R.finish(n64, 1.0, [], t, *hyper["betas"])
        k_coef = opt.last_clip_coef.item()
        assert not bad and step1 == t + 1 and abs(k_coef - coef) <= R.COEF_LIMIT * coef
        for p, b, gi in zip(ps, before, owner):
            args = b + (k_coef, lrs[gi], bc1, bc2s, hyper["betas"][0], hyper["betas"][1], hyper["eps"], hyper["weight_decay"])
            outs = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
            for k, out, rf, lm in zip("pmv", outs, R.update(*args), R.bounds(*args)):
                r = R.ratio(out, rf, lm)
                worst = max(worst, r)
                assert r <= 1.0, (t, tuple(p.shape), k, r)
    print("largest |kernel - float64| / bound %.3f" % worst)
    want = [(ref[gi]["params"][i], ref[gi]["exp_avg"][i], ref[gi]["exp_avg_sq"][i]) for gi, i in ((0, 0), (0, 1), (1, 0))]
    for p, (wp, wm, wv) in zip(ps, want):
        for a, b in ((p.detach(), wp), (opt.state[p]["exp_avg"], wm), (opt.state[p]["exp_avg_sq"], wv)):
            assert (a - b).abs().max().item() <= 1e-6 * 8 / 5 * max(b.abs().max().item(), 1e-30), tuple(p.shape)
    assert float(opt.state_dict()["state"][0]["step"]) == 8.0 and int(opt.skipped_steps) == 0
    assert [g["lr"] for g in opt.param_groups] == [1e-2, 3e-3]    # the host numbers are neither read nor written


def _fixed(seed=5):
    ps = _params([(64, 64), (100, 52), (4097,), (3,)], seed)
    opt = FusedAdamW(ps, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0)
    sched = CosineWarmupSchedule(opt, T_max=7, eta_min=1e-5, warmup_period=2)
    _set_grads(ps, 11)
    return ps, opt, sched


def test_a_bare_capture_is_refused_and_detach_hands_the_rate_back(monkeypatch):
    """a step captured outside GraphedStep would replay the rate it was captured with: refused before anything is launched, with
    nothing counted (the capture is simulated: the refusal is host logic in front of the first launch)"""
    ps, opt, sched = _fixed()
    opt.step()
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="GraphedStep"):
            opt.step()
    assert sched.t == 1
    sched.detach()
    opt.param_groups[0]["lr"] = 4e-3
    opt.step()                                                     # host-driven again
    assert R.bits32(_lr_word(opt)) == R.bits32(R.f32(4e-3)) and sched.t == 1


def _near(a, b, moved, what):
    """tests/test_gpu_optim.py's replay == eager criterion at model level: the backward's column sums use fp32 atomics, so two runs
    differ in the last bits of a few gradients, and Adam turns a rounding-level gradient into a full lr-sized move - the distance
    of two runs is bounded by what the steps could move at all (the key third of an in-projection bias, whose exact gradient
    is zero, walks by lr per step in either run: only its maximum is bounded)"""
    d = (a.float() - b.float()).abs()
    mean_ok = what.endswith("in_proj_bias") or d.mean().item() <= 0.1 * moved
    assert d.max().item() <= 2 * moved and mean_ok, (what, d.max().item(), d.mean().item())


def test_graphed_step_walks_the_schedule():
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na, N, W = 2, 4, 2, 4, 3
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    static = {k: v.to(DEV).clone() for k, v in inp.items()}

    def run(graphed):
        model = _model(cfg, sd, "fp16", 0.0)
        opt = FusedAdamW.for_model(model, lr=2e-3, weight_decay=0.01, max_grad_norm=1.0)
        sched = CosineWarmupSchedule(opt, T_max=6, eta_min=1e-5, warmup_period=4)
        cot = []
        inner = _step(model, static, nv, na, cot)

        def fn():
            outs = inner()
            opt.step()
            prods = [o.detach().float() * r for o, r in zip(outs, cot)]
            # [the scalar whose gradient the step took, the sum of the magnitudes of its terms]
            return torch.stack([torch.stack([x.sum() for x in prods]).sum(), torch.stack([x.abs().sum() for x in prods]).sum()])
        if graphed:
            step = GraphedStep(model, fn, warmup=W, optimizer=opt)
        else:
            step = fn
            for _ in range(W):                                     # the wrapper's warm-up steps are real steps
                fn()
        t0 = sched.t
        losses, mags, rates, before, gl1 = [], [], [], [], []
        for k in range(N):
            before.append({n: p.detach().clone() for n, p in model.named_parameters()})
            if graphed:
                opt.param_groups[0]["lr"] = 0.5                    # not read while the schedule is attached
            scalar, mag = step().tolist()
            losses.append(scalar)
            mags.append(mag)
            rates.append(_lr_word(opt))
            assert sched.last_lr() == [rates[-1]]
            gl1.append({n: p.grad.abs().sum().item() for n, p in model.named_parameters() if p.grad is not None})
        torch.cuda.synchronize()
        F.graph_safe_dropout(DEV, enable=False)
        return t0, losses, mags, rates, sched, opt, before, gl1, {n: p.detach().clone() for n, p in model.named_parameters()}

    t0e, loss_e, mag_e, rate_e, sched_e, _, bef_e, gl1_e, par_e = run(False)
    t0g, loss_g, _, rate_g, sched_g, opt_g, bef_g, _, par_g = run(True)
    assert t0e == t0g == W                                         # the counter value read before the first replay
    want = [sched_g.lr_at(t0g + k) for k in range(N)]
    assert [R.bits32(x) for x in rate_g] == [R.bits32(x) for x in want] == [R.bits32(x) for x in rate_e], (rate_g, rate_e, want)
    assert want == [_definition(W + k, 2e-3, 1e-5, 6, 4) for k in range(N)] and len(set(want)) == N
    assert sched_g.t == W + N and float(opt_g.state_dict()["state"][0]["step"]) == W + N and int(opt_g.skipped_steps) == 0
    # replay == eager.  Parameters: within what the W + N steps could move (above).
    moved = sum(sched_g.lr_at(t) for t in range(W + N))
    for n in par_g:
        _near(par_e[n], par_g[n], moved, n)
    # The scalar of step k is a deterministic function of the parameters step k started from, the same function in both runs, with
    # gradient p.grad.  Where every parameter agrees to the bit the scalars must be EQUAL.  Where some differ (atomics in an
    # earlier backward, amplified by Adam): to first order the scalars differ by sum_n ||grad_n||_1 * D_n, twice that for the
    # curvature, with D_n the distance of the OPERANDS - a master that moved at all can move its fp16 copy by one fp16 ulp, so
    # D_n = max(max |delta theta_n|, 2^-10 max |theta_n|) for a tensor that differs and 0 for one that does not; and the fp16
    # roundings of the activations may then fall differently too, one fp16 ulp (2^-10) of every term of the scalar.
    U16 = 2.0 ** -10
    for k in range(N):
        first, differ = 0.0, False
        for n, g in gl1_e[k].items():
            a, b = bef_e[k][n].float(), bef_g[k][n].float()
            if not torch.equal(a, b):
                differ = True
                first += g * max((a - b).abs().max().item(), U16 * a.abs().max().item())
        bound = 2.0 * first + (U16 * mag_e[k] if differ else 0.0)
        print("replay %d: scalar %.9g, eager %.9g, parameters %s, bound on the distance %.3g"
              % (k, loss_g[k], loss_e[k], "differ" if differ else "bit-equal", bound))
        assert abs(loss_g[k] - loss_e[k]) <= bound, (k, loss_g, loss_e, bound)


def test_skipped_step_advances_the_schedule_on_the_device_path():
    ps, opt, sched = _fixed()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt.extra_flags.append(flag)
    opt.step()
    snap = [p.detach().clone() for p in ps] + [opt.state[p]["exp_avg"].clone() for p in ps]
    flag.fill_(1)
    opt.step()
    words = opt._blocks.view(torch.int32)[0].cpu()
    assert int(words[L.OPT_FOUND_INF]) == 1 and int(words[L.OPT_STEP]) == 1 and int(words[L.OPT_SKIPPED]) == 1
    assert sched.t == 2 and R.bits32(_lr_word(opt)) == R.bits32(sched.lr_at(1)) and sched.last_lr() == [sched.lr_at(1)]
    assert all(torch.equal(a, b) for a, b in zip([p.detach() for p in ps] + [opt.state[p]["exp_avg"] for p in ps], snap))
    flag.zero_()
    opt.step()
    assert int(opt.found_inf) == 0 and sched.t == 3 and float(opt.state_dict()["state"][0]["step"]) == 2.0
    assert not torch.equal(ps[0].detach(), snap[0])


def test_resume_continues_bit_for_bit():
    ps, opt, sched = _fixed()
    for _ in range(6):
        opt.step()
    want = [p.detach().clone() for p in ps] + [opt._blocks.clone()]
    ps2, opt2, sched2 = _fixed()
    for _ in range(3):
        opt2.step()
    sd_opt, sd_sched = opt2.state_dict(), sched2.state_dict()
    assert sd_sched["t"] == 3
    ps3 = [p.detach().clone().requires_grad_(True) for p in ps2]
    opt3 = FusedAdamW(ps3, lr=1.0, max_grad_norm=1.0)
    sched3 = CosineWarmupSchedule(opt3, T_max=99)
    opt3.load_state_dict(sd_opt)
    sched3.load_state_dict(sd_sched)
    for p3, p2 in zip(ps3, ps2):
        p3.grad = p2.grad.clone()
    for _ in range(3):
        opt3.step()
    got = [p.detach().clone() for p in ps3]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want[:-1]))
    assert R.bits32(_lr_word(opt3)) == R.bits32(want[-1][0, L.OPT_LR].item()) == R.bits32(sched.lr_at(5))
    assert sched3.state_dict() == dict(sd_sched, t=6)


def test_example_prints_a_rate_that_follows_the_definition():
    """examples/train_graphed_scheduled_synthetic.py: the captured device-data iteration with the schedule attached; replay k
    trains at iteration k of the curve (the example sets the counter to 0 after the capture)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_graphed_scheduled_synthetic as ex
    hist = ex.main(["--steps", "12", "--warmup-steps", "4"])
    assert len(hist) == 12 and all(math.isfinite(loss) for loss, *_ in hist)
    for k, (_, rate, want, _) in enumerate(hist):
        assert R.bits32(rate) == R.bits32(want) and want == _definition(k, 1e-3, 1e-6, 12, 4), (k, rate, want)
    rates = [h[1] for h in hist]
    assert rates[0] == float(np.float32(1e-3 / 4)) and rates[3] == max(rates) and len(set(rates)) == 12
    assert len({h[3] for h in hist}) == 12                         # lam still redrawn on every replay
