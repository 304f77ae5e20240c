"""Semantics of the fused optimizer step (tim_amd/optim.py) on CPU tensors: `FusedAdamW` runs `reference_step` there, the
plain-torch statement of what the HIP kernels compute.  Checked against `clip_grad_norm_` + `torch.optim.AdamW`; the GPU tests
(tests/test_gpu_optim.py) then check the kernels against `reference_step`."""
import re

import pytest
import torch

from tim_amd import _lib
from tim_amd.optim import FusedAdamW, reference_step


def _params(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(5, 7), (9,), (3,), (4, 2, 3)]
    return [torch.randn(s, generator=g, dtype=dtype).requires_grad_(True) for s in shapes]


def _set_grads(ps, qs, seed, skip=(2,), scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for i, (p, q) in enumerate(zip(ps, qs)):
        if i in skip:
            continue
        gr = torch.randn(p.shape, generator=g, dtype=p.dtype) * scale
        p.grad, q.grad = gr.clone(), gr.clone()


def _rel(a, b):
    return ((a.detach() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.float64, 1e-12)])
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e3])          # no clip / clipping active / clip configured but inactive
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_cpu_step_is_clip_plus_torch_adamw(dtype, tol, max_norm, wd):
    ps, qs = _params(dtype), _params(dtype)
    ours = FusedAdamW(ps, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, max_grad_norm=max_norm)
    ref = torch.optim.AdamW(qs, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    for it in range(6):
        _set_grads(ps, qs, 10 + it)                             # parameter 2 never gets a gradient
        before = [q.grad.clone() for q in qs if q.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(qs, max_norm if max_norm is not None else float("inf"))
        ours.step()
        ref.step()
        assert _rel(ours.last_grad_norm.to(dtype), norm) <= max(tol, 1e-6)
        # the clip lives in the coefficient: our gradients are not rescaled in memory
        for p, g0 in zip([p for p in ps if p.grad is not None], before):
            assert torch.equal(p.grad, g0)
    for p, q in zip(ps, qs):
        assert _rel(p, q) <= tol
    assert torch.equal(ps[2], _params(dtype)[2]) and ps[2] not in ours.state
    assert int(ours.skipped_steps) == 0


def test_state_dict_round_trips_with_torch_adamw():
    ps, qs = _params(torch.float64), _params(torch.float64)
    ours = FusedAdamW(ps, lr=3e-3, weight_decay=0.01)
    ref = torch.optim.AdamW(qs, lr=3e-3, weight_decay=0.01)
    for it in range(3):
        _set_grads(ps, qs, it, skip=())
        ours.step()
        ref.step()
    sd_ours, sd_ref = ours.state_dict(), ref.state_dict()
    assert set(sd_ref["param_groups"][0]) <= set(sd_ours["param_groups"][0])
    assert set(sd_ours["state"][0]) == set(sd_ref["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert float(sd_ours["state"][0]["step"]) == 3.0
    # ours -> torch and torch -> ours, on fresh optimizers over the swapped parameter sets, then three more steps each way
    to_torch = torch.optim.AdamW(ps, lr=1.0)
    to_torch.load_state_dict(sd_ours)
    to_ours = FusedAdamW(qs, lr=1.0)
    to_ours.load_state_dict(sd_ref)
    assert to_ours.param_groups[0]["lr"] == 3e-3 and to_ours.param_groups[0]["max_grad_norm"] is None
    for it in range(3):
        _set_grads(ps, qs, 20 + it, skip=())
        to_torch.step()
        to_ours.step()
    for p, q in zip(ps, qs):
        assert _rel(p, q) <= 1e-12
    assert float(to_ours.state_dict()["state"][0]["step"]) == 6.0


@pytest.mark.parametrize("how", ["inf_gradient", "nan_gradient", "external_flag"])
def test_nonfinite_step_is_skipped_and_does_not_advance_the_count(how):
    ps, qs = _params(torch.float64), _params(torch.float64)
    ours = FusedAdamW(ps, lr=1e-2, max_grad_norm=1.0)
    ref = torch.optim.AdamW(qs, lr=1e-2)
    flag = torch.zeros(1, dtype=torch.int32)
    ours.extra_flags.append(flag)

    def both(seed):
        _set_grads(ps, qs, seed, skip=())
        torch.nn.utils.clip_grad_norm_(qs, 1.0)
        ours.step()
        ref.step()

    both(1)
    snap = [p.detach().clone() for p in ps]
    moments = [ours.state[p]["exp_avg"].clone() for p in ps]
    _set_grads(ps, ps, 2, skip=())
    if how == "external_flag":
        flag.fill_(1)
    else:
        ps[1].grad[3] = float("inf") if how == "inf_gradient" else float("nan")
    ours.step()                                                   # the bad step: ours only
    flag.zero_()
    assert int(ours.skipped_steps) == 1 and int(ours.found_inf) == 1
    for p, s, m in zip(ps, snap, moments):
        assert torch.equal(p.detach(), s) and torch.equal(ours.state[p]["exp_avg"], m)
    assert float(ours.state_dict()["state"][0]["step"]) == 1.0
    both(3)                                                       # bias correction as if the bad step never happened
    assert int(ours.skipped_steps) == 1 and int(ours.found_inf) == 0
    for p, q in zip(ps, qs):
        assert _rel(p, q) <= 1e-12


def test_reference_step_shares_one_norm_over_groups():
    a, b = torch.full((4,), 1.0, dtype=torch.float64), torch.full((3,), 2.0, dtype=torch.float64)
    mk = lambda p, g, lr: {"params": [p], "grads": [g], "exp_avg": [torch.zeros_like(p)], "exp_avg_sq": [torch.zeros_like(p)],
                           "lr": lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "state": {"step": 0, "skipped": 0}}
    ga, gb = torch.full((4,), 3.0, dtype=torch.float64), torch.full((3,), 4.0, dtype=torch.float64)
    groups = [mk(a, ga, 0.1), mk(b, gb, 0.2)]
    norm, coef, bad = reference_step(groups, max_grad_norm=1.0)
    assert not bad and abs(float(norm) - (4 * 9 + 3 * 16) ** 0.5) < 1e-12 and abs(float(coef) - 1.0 / (float(norm) + 1e-6)) < 1e-15
    assert groups[0]["state"]["step"] == groups[1]["state"]["step"] == 1
    # the first Adam step moves every entry by lr against the gradient's sign, whatever the clip did to its size
    assert torch.allclose(a, torch.full_like(a, 0.9), atol=1e-6) and torch.allclose(b, torch.full_like(b, 1.8), atol=1e-6)


def test_unsupported_modes_raise():
    p = [torch.zeros(3, requires_grad=True)]
    with pytest.raises(ValueError):
        FusedAdamW(p, amsgrad=True)
    with pytest.raises(ValueError):
        FusedAdamW(p, maximize=True)
    with pytest.raises(ValueError):
        FusedAdamW(p, lr=-1.0)
    sd = torch.optim.AdamW(p, amsgrad=True).state_dict()
    with pytest.raises(ValueError):
        FusedAdamW(p).load_state_dict(sd)


def test_optimizer_entry_points_are_declared_exported_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "timhip.h")).read()
    declared = {n for n in re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", hdr) if n.startswith("timhip_optim_")}
    assert declared == {"timhip_optim_norm_partials", "timhip_optim_norm", "timhip_optim_finish", "timhip_optim_update"}
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in declared) and declared <= set(_lib.exported_symbols())
    assert lib.timhip_version() == _lib.ABI_VERSION == 6          # no existing struct changed layout
    # the table walk is host arithmetic: bad items are refused before anything is launched
    import ctypes as C
    bad = (_lib.TimOptItem * 1)(_lib.TimOptItem(16, 16, 16, 16, 16, None, 4, 4, 64, 64))      # plain without tr
    assert lib.timhip_optim_norm_partials(C.cast(bad, C.c_void_p), 1) == -1
    ok = (_lib.TimOptItem * 2)(_lib.TimOptItem(16, 16, 16, 16, None, None, 1, 4097, 0, 0),
                               _lib.TimOptItem(16, 20, 16, 16, None, None, 64, 64, 0, 0))       # 4-byte aligned gradient
    assert lib.timhip_optim_norm_partials(C.cast(ok, C.c_void_p), 2) == 2 + 2
