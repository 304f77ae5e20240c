"""CPU test of the attention checker itself (tests/attn_ref.py): the float64 reference equals oracle.attention_structured plus
autograd; an fp32 emulation of a correct kernel of each family stays inside the elementwise bounds for every case of
tests/test_gpu_attention_edges.py at every precision (the largest used shares are printed); each of a list of subtly wrong
kernels is rejected in every case it applies to; and two of them are shown to pass the max-norm criterion of _attn_case
(tests/test_gpu_kernels.py), which is what the elementwise bound adds."""
import pytest
import torch

from oracle import tim_oracle as O
from tests import attn_ref as A

ALL_CASES = [(grp, cs) for grp in sorted(A.GPU_CASES) for cs in A.GPU_CASES[grp]]
TOL = {"fp32": 1e-5, "bf16x3": 5e-5, "bf16": 1e-3, "fp16": 1.5e-4}        # tests/test_gpu_kernels.py: tol()


def _make(cs, prec, seed=3, **kw):
    return A.make_case(prec, cs.B, cs.S, cs.F, cs.H, cs.Dh, p=cs.p, seed=seed, peaked=cs.peaked, fp32=cs.fp32, **kw)


def _rejected(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("B,S,F,H,Dh", [(2, 45, 20, 2, 16), (1, 33, 32, 3, 32), (2, 12, 12, 1, 64)])
def test_reference_equals_the_oracle_and_autograd(B, S, F, H, Dh, p):
    c = A.make_case("bf16", B, S, F, H, Dh, p=p, seed=5)
    r = A.reference(c)
    x = torch.stack([c.q, c.k, c.v]).clone().requires_grad_(True)
    mask = None if p == 0 else c.keep[..., :F + 1].double()
    o = O.attention_structured(x[0], x[1], x[2], F, mask, p)
    (o * c.dO).sum().backward()
    rel = lambda got, want: float((got - want).abs().max() / want.abs().max().clamp(min=1e-300))
    assert rel(r.o, o.detach()) <= 1e-12
    for got, want in zip((r.dQ, r.dK, r.dV), x.grad):
        assert rel(got, want) <= 1e-12
    # lse against a dense statement: log sum exp over the live columns
    s = r.s.masked_fill(~r.live, float("-inf"))
    assert rel(r.lse, torch.logsumexp(s, -1)) <= 1e-12
    # delta as the kernels take it: the row sum of dO * o
    assert rel(r.delta.squeeze(-1), (c.dO * r.o).sum(-1)) <= 1e-10


@pytest.mark.parametrize("group", sorted(A.GPU_CASES))
def test_emulation_stays_inside_the_bounds_for_every_gpu_case(group):
    """every case of the GPU module, every precision it runs in: the family it is meant for (the dispatch rule, restated), then an
    fp32 emulation of that family within the bound.  Largest shares are printed per family and pass"""
    worst = {}
    for cs in A.GPU_CASES[group]:
        for prec in cs.precs:
            fam = A.expected_family(cs, prec)
            c = _make(cs, prec)
            A.store(c, A.emulate(c, fam))
            for key, sh in (("fwd " + fam.fwd + " " + prec, A.verify_fwd(c, fam.fwd)), ("bwd " + fam.bwd + " " + prec, A.verify_bwd(c, fam.bwd))):
                worst[key] = max(worst.get(key, 0.0), sh)
    for key in sorted(worst):
        print("largest used share of the elementwise bound, %s, %-24s %.3f" % (group, key, worst[key]))
        assert worst[key] < 1.0


MUT_CASES = [cs for _, cs in ALL_CASES]      # every case of the GPU list: what a mutation does not apply to is attn_ref.applies' to say


@pytest.mark.parametrize("mut", sorted(A.MUTATIONS))
def test_every_mutation_is_rejected_in_every_case_it_applies_to(mut):
    which, n = A.MUTATIONS[mut][0], 0
    for cs in MUT_CASES:
        for prec in cs.precs:
            if prec == "bf16x3":      # (fp32 storage and the same kernels as fp32: the emulation is the same)
                continue
            fam = A.expected_family(cs, prec)
            c = _make(cs, prec)
            if not A.applies(c, mut, fam):
                continue
            A.mutate(c, mut, fam)
            rf, rb = _rejected(A.verify_fwd, c, fam.fwd), _rejected(A.verify_bwd, c, fam.bwd)
            if which in ("fwd", "both"):
                assert rf, (mut, cs.name, prec, "forward")
            if which in ("bwd", "both"):
                assert rb, (mut, cs.name, prec, "backward")
            n += 1
    assert n > 0
    print("%s: rejected in %d cases" % (mut, n))


def test_an_unwritten_element_and_a_written_guard_are_rejected():
    cs = A.GPU_CASES["rows"][1]
    fam = A.expected_family(cs, "fp16")
    for spoil, fn in ((lambda c: c.dqkv_whole.__setitem__((1, 3), 1.0), A.verify_bwd), (lambda c: c.o_whole.__setitem__((-1, 0), 0.5), A.verify_fwd),
                      (lambda c: c.lse_whole.__setitem__(A.LSE_GUARD - 1, 0.0), A.verify_fwd),
                      (lambda c: c.dqkv.__setitem__((5, 7), float("nan")), A.verify_bwd), (lambda c: c.qkv_whole.__setitem__((0, 0), 0.0), A.verify_fwd)):
        c = _make(cs, "fp16")
        A.store(c, A.emulate(c, fam))
        assert A.verify_fwd(c, fam.fwd) < 1.0 and A.verify_bwd(c, fam.bwd) < 1.0
        spoil(c)
        assert _rejected(fn, c, fam.fwd if fn is A.verify_fwd else fam.bwd)


@pytest.mark.parametrize("mut", ["own_kv_zero", "dq_scaled"])
def test_the_max_norm_criterion_accepts_what_the_elementwise_bound_rejects(mut):
    """bf16 at 3 x 155 x 100 x 2 x 128 on inputs like _attn_case's (unscaled randn): its criterion for the backward is ONE number
    for the whole dqkv matrix, lim = 5 tol + 2 HALF_ULP max|ref| = 0.018 here, set by the largest dQ element (1.39).
      * own_kv_zero: 91 % of the own-key / own-value gradient elements of the query rows are smaller than lim.  A kernel that
        stores zeros there in every query row whose own gradients all stay below lim (more than a third of the query rows) passes
        the max-norm criterion; the elementwise bound rejects it.
      * dq_scaled: dQ 3 % too large in every row whose largest |dQ| is below 0.8 x 32 lim = 0.46 (73 % of the rows) passes
        the max-norm criterion; the elementwise bound rejects it.
    Applied to EVERY row both mistakes are caught by the max-norm criterion as well, through their few largest elements only
    (the largest own gradient is above lim, 3 % of the largest dQ element is 0.044): that is asserted too."""
    fam = A.family_of("bf16", dict(B=3, S=155, F=100, H=2, Dh=128))
    c = A.make_case("bf16", 3, 155, 100, 2, 128, p=0.0, seed=11, plain=True)
    A.store(c, A.emulate(c, fam))
    assert A.verify_bwd(c, fam.bwd) < 1.0 and A.max_norm_accepts_bwd(c, TOL["bf16"])
    r = A.reference(c)
    gmax = max(float(t.abs().max()) for t in (r.dQ, r.dK, r.dV))
    lim = 5 * TOL["bf16"] * max(1.0, gmax) + 2 * c.h * gmax
    rows = torch.zeros(c.B, c.H, c.S, dtype=torch.bool)
    if mut == "own_kv_zero":
        rows[:, :, c.F:] = torch.maximum(r.dK[:, :, c.F:].abs().amax(-1), r.dV[:, :, c.F:].abs().amax(-1)) < 0.9 * lim
        assert float(rows[:, :, c.F:].float().mean()) > 1 / 3
        assert float((r.dK[:, :, c.F:].abs() < lim).float().mean()) >= 0.85
    else:
        rows[:] = r.dQ.abs().amax(-1) * 2.0 ** -5 < 0.8 * lim        # (0.8: the 16-bit store's own rounding takes the rest)
        print("dq_scaled hits %.2f of the rows" % float(rows.float().mean()))
        assert float(rows.float().mean()) > 0.5
    A.mutate(c, mut, fam, rows)
    assert A.max_norm_accepts_bwd(c, TOL["bf16"]), "the max-norm criterion was expected to let this one through"
    assert _rejected(A.verify_bwd, c, fam.bwd)
    A.mutate(c, mut, fam)
    assert not A.max_norm_accepts_bwd(c, TOL["bf16"]) and _rejected(A.verify_bwd, c, fam.bwd)
