"""The float64 restatements of tests/rowops_ref.py against the oracle (oracle/tim_oracle.py), on the CPU: what the GPU tests
of tests/test_gpu_rowops.py compare the row kernels with must not be wrong in the same way as a kernel."""
import numpy as np
import pytest
import torch

from oracle import tim_oracle as O
from tests import helpers as H
from tests import rowops_ref as R
from tim_amd.functional import EncoderPlan

F64 = torch.float64


def _rn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def test_time_l1_is_the_oracles_first_layer():
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, inp = H.synth_torch(cfg, 3, 4, 2, seed=1, dtype=F64)
    times = inp["times"].reshape(-1, 2).clone().requires_grad_(True)
    w = sd["time_mlp.0.weight"].clone().requires_grad_(True)
    b = sd["time_mlp.0.bias"].clone().requires_grad_(True)
    want = torch.relu(O._lin(times, w, b))
    got = R.time_l1(times.detach(), w.detach(), b.detach())
    np.testing.assert_allclose(got.numpy(), want.detach().numpy(), atol=1e-14)
    assert (got == 0).any() and (got > 0).any()          # both sides of the relu
    dh = _rn(*want.shape, seed=2)
    (want * dh).sum().backward()
    # the kernel's contract: the relu mask is folded into dh by the caller
    dw, db, dt = R.time_l1_bwd(times.detach(), w.detach(), dh * (want.detach() > 0))
    np.testing.assert_allclose(dw.numpy(), w.grad.numpy(), atol=1e-13)
    np.testing.assert_allclose(db.numpy(), b.grad.numpy(), atol=1e-13)
    np.testing.assert_allclose(dt.numpy(), times.grad.numpy(), atol=1e-13)
    terms = R.time_l1_abs_terms(times.detach(), w.detach(), b.detach())
    assert (terms + 1e-15 >= got).all()


LAYOUTS = [("recognition", "audio_visual", "audio_visual", True, 4, 2),
           ("recognition", "visual", "visual", True, 5, 0),
           ("recognition", "audio", "audio", False, 0, 3),
           ("detection", "audio_visual", "audio_visual", True, 6, 3),
           ("detection", "visual", "visual", False, 7, 0)]


@pytest.mark.parametrize("variant,im,dm,vn,nv,na", LAYOUTS)
def test_assembly_over_the_hosts_table_is_the_oracles_feature_encoding(variant, im, dm, vn, nv, na):
    nc = None
    if variant == "detection":
        nc = [[7, 11, 13], 5] if vn else (13, 5)
    cfg = H.tiny_cfg(variant, im, dm, vn, num_class=nc)
    cfg.feat_drop = cfg.seq_drop = 0.0                  # eval mode
    B, d = 3, cfg.d_model
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=1, dtype=F64)
    te = O.time_mlp(sd, inp["times"]).detach().requires_grad_(True)
    plan = EncoderPlan(cfg, te.shape[1], nv, na)
    table = [tuple(int(v) for v in r) for r in plan.table("cpu").tolist()]      # the int32 table the kernels read
    assert table == [tuple(r) for r in plan.rows]
    e = [None, None]
    for name, slot in plan.embedders:
        e[slot] = O._embed(sd, name, inp[name], None, cfg, None).detach().requires_grad_(True)
    cls = [sd["feature_encoding." + n].reshape(d).clone().requires_grad_(True) for n in plan.cls_names]
    mod = [sd["feature_encoding." + n].reshape(2 * d).clone().requires_grad_(True) for n in plan.mod_names]
    got = R.assemble(table, B, d, e[0], e[1], cls, te, mod)
    want = O.feature_encoding(sd, cfg, inp["visual"], inp["audio"], te.detach(), nv, na)
    assert got.shape == want.shape == (B, plan.S, 2 * d)
    np.testing.assert_allclose(got.detach().numpy(), want.detach().numpy(), atol=1e-12)
    # backward: the explicit sums == autograd through the restated forward
    dx = _rn(B, plan.S, 2 * d, seed=3)
    (got * dx).sum().backward()
    g = R.assemble_bwd(table, B, d, dx, cfg.num_feats, te.shape[1], len(cls), len(mod))
    for slot in (0, 1):
        if e[slot] is not None:
            np.testing.assert_allclose(g["d_e%d" % slot].numpy(), e[slot].grad.numpy(), atol=1e-12)
            assert bool(g["wrote%d" % slot].all())
    for a, p in zip(g["d_cls"] + g["d_mod"], cls + mod):
        np.testing.assert_allclose(a.numpy(), p.grad.numpy(), atol=1e-11)
    np.testing.assert_allclose(g["d_te"].numpy(), te.grad.numpy(), atol=1e-12)


@pytest.mark.parametrize("a", [0, 1, 2])
def test_layernorm_is_the_oracles(a):
    y = _rn(9, 40, seed=4) * 2 + 0.5
    w, b, dx = 1 + 0.1 * _rn(40, seed=5), 0.1 * _rn(40, seed=6), _rn(9, 40, seed=7)
    yy, ww, bb = [t.clone().requires_grad_(True) for t in (y, w, b)]
    want = O._ln({0: lambda t: t, 1: torch.relu, 2: O._gelu}[a](yy), ww, bb)
    got, mean, rstd = R.layernorm(y, w, b, a)
    np.testing.assert_allclose(got.numpy(), want.detach().numpy(), atol=1e-13)
    x = R.act(a, y)
    np.testing.assert_allclose(mean.numpy(), x.mean(-1).numpy(), atol=1e-14)
    np.testing.assert_allclose(rstd.numpy(), (x.var(-1, unbiased=False) + 1e-5).rsqrt().numpy(), rtol=1e-12)
    (want * dx).sum().backward()
    dy, dg, db = R.layernorm_bwd(y, w, dx, a)
    np.testing.assert_allclose(dy.numpy(), yy.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(dg.numpy(), ww.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(db.numpy(), bb.grad.numpy(), atol=1e-12)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_split_operands_keep_22_bits(dtype):
    """[hi | lo | hi]: hi + lo reproduces the fp32 value to 2^-22 relative (fp16: for values whose lo half stays normal)"""
    g = torch.Generator().manual_seed(8)
    v = (torch.randn(4096, generator=g) * torch.exp2(torch.randint(-6, 7, (4096,), generator=g).float())).float()
    hi, lo = R.split3(v, dtype)
    err = (hi.double() + lo.double() - v.double()).abs()
    if dtype == torch.bfloat16:
        # two 8-bit halves: 2^-8 * 2^-8 = 2^-16 relative - the bf16 pair is NOT a 22-bit value
        assert (err <= 2.0 ** -16 * v.double().abs()).all()
    else:
        # hi within 2^-11 |v|, lo = T(v - hi) within 2^-11 |v - hi| (or half the subnormal step 2^-25)
        assert (err <= torch.maximum(2.0 ** -22 * v.double().abs(), torch.tensor(2.0 ** -25, dtype=F64))).all()
    assert torch.equal(hi, v.to(dtype))


def test_row_moves_are_inverse_on_covered_rows():
    x = _rn(3, 12, 8, seed=9)
    ranges = [(7, 2), (2, 1), (9, 3)]
    rows = R.gather_ranges(x, ranges)
    back = R.scatter_ranges_add(torch.zeros_like(x), ranges, rows)
    covered = torch.zeros(12, dtype=torch.bool)
    for s0, n in ranges:
        covered[s0:s0 + n] = True
    assert torch.equal(back[:, covered], x[:, covered]) and bool((back[:, ~covered] == 0).all())
    y = torch.sigmoid(_rn(5, 2, seed=10)).requires_grad_(True)
    z = _rn(5, 2, seed=11).requires_grad_(True)
    s = torch.sigmoid(z)
    gz, = torch.autograd.grad((s * 3.0).sum(), z)
    np.testing.assert_allclose(R.sigmoid_bwd(torch.full((5, 2), 3.0, dtype=F64), s.detach()).numpy(), gz.numpy(), atol=1e-14)
