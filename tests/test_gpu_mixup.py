"""Device-side mixup (tim_amd/mixup.py, csrc/mixup.hip, the device-lam cross entropy of csrc/losses.hip) against the CPU
restatement tests/mixup_ref.py, the reference's own mixup_data (tests/golden/mixup_small.npz) and under graph replay."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import mixup_ref as R  # noqa: E402
from tests.test_mixup_ref import GOLDEN, GPU_DRAW_RUNS, N_DRAWS, draws  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd import losses  # noqa: E402
from tim_amd.mixup import Mixup, mixup_data  # noqa: E402

DEV = "cuda:0"
TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PREC = {"fp32": L.PREC_FP32, "fp16": L.PREC_F16, "bf16": L.PREC_BF16}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def draw_raw(seed, counter, alpha, B, n):
    lam = torch.full((n,), -1.0, dtype=torch.float32, device=DEV)
    perm = torch.full((n, B), -1, dtype=torch.int32, device=DEV)
    inv = torch.full((n, B), -1, dtype=torch.int32, device=DEV)
    L.call("timhip_mixup_draw", seed, L.ptr(counter), alpha, B, n, L.ptr(lam), L.ptr(perm), L.ptr(inv), _stream())
    return lam.cpu().numpy(), perm.cpu().numpy(), inv.cpu().numpy()


def check_lam(dev_lam, ref_lam, margin):
    """device lam within 1e-5 relative of the restatement wherever the restatement is clear of its accept boundary"""
    clear = margin >= R.NEAR
    rel = np.abs(dev_lam.astype(np.float64) - ref_lam) / np.maximum(np.abs(ref_lam), 1e-300)
    print("lam: %d of %d draws clear of the boundary, max relative deviation there %.2e" % (clear.sum(), clear.size, rel[clear].max(initial=0.0)))
    assert (rel[clear] <= 1e-5).all()
    return 1.0 - clear.mean()


# ---- 1. draw ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("B", [1, 2, 5, 64, 257])
def test_draw_is_the_restatement(B, n):
    seed, alpha = 17 + B, 0.2
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    for launch in range(2):       # the second launch continues the sequence
        lam, perm, inv = draw_raw(seed, counter, alpha, B, n)
        rl, rp, ri, margin = R.draw(seed, launch * n, alpha, B, n)
        assert int(counter.item()) == (launch + 1) * n
        assert np.array_equal(perm, rp) and np.array_equal(inv, ri)
        assert all(np.array_equal(i[p], np.arange(B)) for p, i in zip(perm, inv))
        check_lam(lam, rl, margin)


@pytest.mark.parametrize("seed,alpha", GPU_DRAW_RUNS)
def test_draw_distribution(seed, alpha):
    ref_lam, margin = draws(seed, alpha)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    lam, perm, _ = draw_raw(seed, counter, alpha, 2, N_DRAWS)
    assert int(counter.item()) == N_DRAWS
    flagged = check_lam(lam, ref_lam, margin)
    assert flagged <= 0.01
    assert ((lam >= 0) & (lam <= 1)).all()
    m, v = R.moments(lam)
    em, dm, ev, dv = R.beta_moment_bounds(alpha, N_DRAWS)
    print("alpha %g on the device: mean %.5f (0.5 +- %.4f), variance %.5f (%.5f +- %.4f)" % (alpha, m, dm, v, ev, dv))
    assert abs(m - em) <= dm and abs(v - ev) <= dv
    assert 0.4 < (perm[:, 0] == 1).mean() < 0.6


@pytest.mark.parametrize("alpha", [0.0, -1.0])
def test_draw_alpha_off(alpha):
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    lam, perm, inv = draw_raw(3, counter, alpha, 7, 4)
    _, rp, ri, _ = R.draw(3, 0, alpha, 7, 4)
    assert (lam == 1.0).all() and np.array_equal(perm, rp) and np.array_equal(inv, ri)


@pytest.mark.parametrize("alpha", [0.01, 0.049, 16.5, float("nan"), float("inf")])
def test_draw_refuses_alpha_outside_the_range(alpha):
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(L.TimHipError):
        draw_raw(3, counter, alpha, 4, 1)
    assert int(counter.item()) == 0
    with pytest.raises(ValueError):
        Mixup(4, alpha=alpha, device=DEV)


@pytest.mark.parametrize("alpha", [0.05, 0.1, 4.0, 16.0])
def test_draw_accepts_the_declared_range(alpha):
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    lam, _, _ = draw_raw(5, counter, alpha, 3, 64)
    rl, _, _, margin = R.draw(5, 0, alpha, 3, 64)
    check_lam(lam, rl, margin)


# ---- 2. apply ---------------------------------------------------------------------------------------------------------
GUARD = 16   # elements of NaN on either side of every output (a multiple of 16 bytes in every dtype)


def _embedded(n, dtype, off, fill):
    """n elements inside a larger buffer, `off` elements past 16-byte alignment, NaN around them"""
    buf = torch.full((n + 2 * GUARD + off,), float("nan"), dtype=TORCH[dtype], device=DEV)
    view = buf[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == (off * buf.element_size()) % 16
    if fill is not None:
        view.copy_(fill)
    return buf, view


def run_apply(specs, B, lam, index, seed=0):
    """specs: [(dtype, elems, misalignment in elements)] -> one launch; every output checked against the float64 restatement"""
    g = torch.Generator().manual_seed(seed)
    lam_t = torch.tensor([lam], dtype=torch.float32, device=DEV)
    idx_t = torch.tensor(index, dtype=torch.int32, device=DEV)
    srcs, dsts, xs = [], [], []
    for dtype, elems, off in specs:
        x = torch.randn(B * elems, generator=g).to(TORCH[dtype])
        xs.append(x.double().numpy().reshape(B, elems))
        srcs.append(_embedded(B * elems, dtype, off, x.to(DEV)))
        dsts.append(_embedded(B * elems, dtype, off, None))
    n = len(specs)
    L.call("timhip_mixup_apply", n, (C.c_void_p * n)(*[s[1].data_ptr() for s in srcs]), (C.c_void_p * n)(*[d[1].data_ptr() for d in dsts]),
           (C.c_int64 * n)(*[e for _, e, _ in specs]), (C.c_int32 * n)(*[PREC[d] for d, _, _ in specs]), B, L.ptr(lam_t), L.ptr(idx_t),
           _stream())
    torch.cuda.synchronize()
    lam64 = float(np.float32(lam))
    outs = []
    for (dtype, elems, off), (buf, view), x in zip(specs, dsts, xs):
        full = buf.double().cpu().numpy()
        lo, hi = GUARD + off, GUARD + off + B * elems
        assert np.isnan(full[:lo]).all() and np.isnan(full[hi:]).all(), "guard rows written"
        out = full[lo:hi].reshape(B, elems)
        ref, bound = R.mix(x, lam64, index), R.mix_bound(x, lam64, index, dtype)
        err = np.abs(out - ref)
        print("%s elems %d off %d B %d: max err / bound %.3f" % (dtype, elems, off, B, (err / bound).max()))
        assert (err <= bound).all()
        outs.append((out, x))
    return outs


@pytest.mark.parametrize("elems", [1, 3, 4, 7, 1025])
@pytest.mark.parametrize("dtype", ["fp32", "fp16", "bf16"])
def test_apply_widths(dtype, elems):
    run_apply([(dtype, elems, 0)], 3, 0.3, [2, 0, 1])


def test_apply_grid_stride_wraps():
    """2^20 + 3 elements per item at B = 3: 786435 chunks for a grid of 2048 x 256 threads, an item tail, items off alignment"""
    run_apply([("fp32", 2 ** 20 + 3, 0)], 3, 0.71, [1, 2, 0])


@pytest.mark.parametrize("dtype,elems", [("fp32", 8), ("fp32", 1025), ("fp16", 24), ("bf16", 7)])
def test_apply_base_off_alignment(dtype, elems):
    run_apply([(dtype, elems, 1)], 3, 0.4, [1, 2, 0])


@pytest.mark.parametrize("B,index", [(1, [0]), (2, [1, 0]), (2, [0, 1])])
def test_apply_small_batches(B, index):
    run_apply([("fp32", 7, 0), ("fp32", 64, 0)], B, 0.25, index)


def test_apply_three_tensors_of_different_widths_and_dtypes():
    run_apply([("fp32", 1025, 0), ("fp16", 24, 0), ("bf16", 13, 0), ("fp32", 4, 1)], 5, 0.6, [3, 0, 4, 1, 2])


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_apply_lam_at_the_ends(lam):
    index = [2, 0, 1]
    for out, x in run_apply([("fp32", 37, 0), ("fp16", 40, 0), ("bf16", 9, 0)], 3, lam, index):
        assert np.array_equal(out, x if lam == 1.0 else x[index])


def test_apply_refuses_bad_arguments():
    x = torch.zeros(8, device=DEV)
    lam, idx = torch.ones(1, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    one = lambda a, T: (T * 1)(a)   # noqa: E731
    args = lambda nt, elems, prec: (nt, one(x.data_ptr(), C.c_void_p), one(x.data_ptr(), C.c_void_p), one(elems, C.c_int64),   # noqa: E731
                                    one(prec, C.c_int32), 2, L.ptr(lam), L.ptr(idx), _stream())
    for bad in (args(0, 4, L.PREC_FP32), args(5, 4, L.PREC_FP32), args(1, 0, L.PREC_FP32), args(1, 4, L.PREC_BF16X3)):
        with pytest.raises(L.TimHipError):
            L.call("timhip_mixup_apply", *bad)
    with pytest.raises(L.TimHipError):
        Mixup(2, device=DEV).mix([torch.zeros(2, 3)])          # a CPU tensor: no fallback
    with pytest.raises(L.TimHipError):
        Mixup(2, device="cpu")


# ---- 3. golden --------------------------------------------------------------------------------------------------------
def test_mix_and_targets_are_the_reference():
    g = np.load(GOLDEN)
    lam, index = float(g["lam"]), g["index"]
    mix = Mixup(5, alpha=0.2, device=DEV).set(lam, index)
    xs = [g["x%d" % i] for i in range(3)]
    outs = mix.mix([torch.from_numpy(x).to(DEV) for x in xs])
    for i, (x, o) in enumerate(zip(xs, outs)):
        assert o.dtype == torch.float32 and tuple(o.shape) == x.shape
        err = np.abs(o.double().cpu().numpy() - g["mixed%d" % i].astype(np.float64))
        bound = R.mix_bound(x, lam, index)
        print("golden tensor %d: max err / bound %.3f" % (i, (err / bound).max()))
        assert (err <= bound).all()
    y = {k: torch.from_numpy(g["y_" + k]).to(DEV) for k in ("verb", "noun", "action", "class_id")}
    y_a, y_b = mix.targets(y)
    assert y_a is y
    for k in y:
        assert y_b[k].dtype == torch.int64 and np.array_equal(y_b[k].cpu().numpy(), g["yb_" + k])
    assert np.array_equal(mix.targets(y["verb"])[1].cpu().numpy(), g["yb_verb"])
    # a view that is not contiguous mixes like its contiguous copy
    xt = torch.from_numpy(xs[0]).to(DEV).transpose(1, 2)
    assert torch.equal(mix.mix([xt])[0], mix.mix([xt.contiguous()])[0])


def test_set_validates():
    mix = Mixup(4, device=DEV)
    for lam, index in ((1.5, [0, 1, 2, 3]), (-0.1, [0, 1, 2, 3]), (0.5, [0, 1, 2]), (0.5, [0, 1, 2, 2]), (0.5, [0, 1, 2, 4]),
                       (float("nan"), [0, 1, 2, 3])):
        with pytest.raises(ValueError):
            mix.set(lam, index)
    mix.set(0.25, torch.tensor([3, 2, 0, 1]))
    assert mix.inverse.tolist() == [2, 3, 1, 0] and mix.lam.item() == 0.25


def test_state_dict_continues_the_sequence():
    a = Mixup(6, alpha=0.2, device=DEV, seed=5)
    for _ in range(3):
        a.draw()
    sd = a.state_dict()
    assert sd["counter"] == 3 and sd["seed"] == 5 and sd["alpha"] == 0.2
    b = Mixup(6, alpha=1.0, device=DEV, seed=0)
    b.load_state_dict(sd)
    a.draw()
    b.draw()
    assert torch.equal(a.lam, b.lam) and torch.equal(a.index, b.index) and torch.equal(a.inverse, b.inverse)
    rl, rp, _, margin = R.draw(5, 3, 0.2, 6, 1)
    assert np.array_equal(a.index.cpu().numpy(), rp[0])


def test_mixup_data_has_the_reference_signature():
    g = np.load(GOLDEN)
    x = [torch.from_numpy(g["x%d" % i]).to(DEV) for i in range(3)]
    y = {k: torch.from_numpy(g["y_" + k]).to(DEV) for k in ("verb", "noun", "action", "class_id")}
    state = Mixup(5, alpha=0.2, device=DEV, seed=2)
    mixed, y_a, y_b, lam = mixup_data(x, y, alpha=0.2, state=state)
    assert lam is state.lam and lam.is_cuda and y_a is y and len(mixed) == 3
    idx = state.index.long()
    l64 = float(lam.item())
    for a, m in zip(x, mixed):
        xn = a.double().cpu().numpy()
        assert (np.abs(m.double().cpu().numpy() - R.mix(xn, l64, idx.cpu().numpy())) <= R.mix_bound(xn, l64, idx.cpu().numpy())).all()
    assert all(torch.equal(y_b[k], y[k][idx]) for k in y)
    mixed2, _, _, lam2 = mixup_data(x, y, alpha=0.2)          # the module's own state for (device, batch size)
    assert lam2.is_cuda and lam2.numel() == 1 and mixup_data(x, y, alpha=0.2)[3] is lam2


# ---- 4. backward ------------------------------------------------------------------------------------------------------
def test_mix_backward():
    mix = Mixup(5, alpha=0.2, device=DEV, seed=4).draw()
    g = torch.Generator().manual_seed(2)
    a = torch.randn(5, 3, 7, generator=g).to(DEV)
    te = torch.randn(5, 11, 6, generator=g).to(DEV).requires_grad_(True)
    h = torch.randn(5, 8, generator=g).to(DEV).half().requires_grad_(True)
    dte, dh = torch.randn(5, 11, 6, generator=g).to(DEV), torch.randn(5, 8, generator=g).to(DEV).half()
    oa, ote, oh = mix.mix([a, te, h])
    assert not oa.requires_grad and ote.requires_grad and oh.requires_grad
    torch.autograd.backward([ote, oh], [dte, dh])
    lam, inv = float(mix.lam.item()), mix.inverse.cpu().numpy()
    for x, dy, dtype in ((te, dte, "fp32"), (h, dh, "fp16")):
        dyn = dy.double().cpu().numpy()
        err = np.abs(x.grad.double().cpu().numpy() - R.mix_backward(dyn, lam, inv))
        assert x.grad.dtype == x.dtype and (err <= R.mix_bound(dyn, lam, inv, dtype)).all()
    assert a.grad is None
    # the backward launch covers the tensors that need a gradient only: alone, te gets the bits it got next to h
    te2 = te.detach().requires_grad_(True)
    oa, ote = mix.mix([a, te2])
    gte, = torch.autograd.grad([ote], [te2], [dte])
    assert not oa.requires_grad and torch.equal(gte, te.grad)


def test_backward_after_a_redraw_is_refused():
    mix = Mixup(4, alpha=0.2, device=DEV, seed=1).draw()
    x = torch.randn(4, 6, device=DEV, requires_grad=True)
    out, = mix.mix([x])
    mix.draw()
    with pytest.raises(RuntimeError, match="redrawn"):
        out.sum().backward()
    assert x.grad is None
    out, = mix.mix([x])
    out.sum().backward()           # in order it goes through
    assert x.grad is not None


# ---- 5. cross entropy with lam in device memory --------------------------------------------------------------------------
@pytest.mark.parametrize("b_valid", [True, False])
@pytest.mark.parametrize("lam", [0.3, 0.0, 1.0, 0.8611])
def test_cross_entropy_with_device_lam_is_the_float_path(lam, b_valid):
    g = torch.Generator().manual_seed(3)
    rows, Cn = 7, 13
    x = (torch.randn(rows, Cn, generator=g) * 2).to(DEV)
    ta = torch.randint(0, Cn, (rows,), generator=g).to(DEV)
    tb = torch.randint(0, Cn, (rows,), generator=g).to(DEV)
    ta[2] = -1
    tb[5] = -1
    if not b_valid:
        tb.fill_(-1)
    lam_t = torch.tensor([lam], dtype=torch.float32, device=DEV)
    gout = torch.tensor(0.7, device=DEV)

    def run(l, poke=None):
        xx = x.clone().requires_grad_(True)
        loss = losses.mixup_cross_entropy(xx, ta, tb, l, 0.2)
        if poke is not None:
            lam_t.fill_(poke)          # the state is redrawn between forward and backward
        loss.backward(gout)
        return loss.detach().clone(), xx.grad.clone()

    want = run(float(lam_t.item()))
    got = run(lam_t)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.isfinite(got[0]) and torch.isfinite(got[1]).all()
    poked = run(lam_t, poke=0.123)
    assert torch.equal(poked[0], want[0]) and torch.equal(poked[1], want[1])
    lam_t.fill_(lam)
    # mixup_criterion with this module's criterion takes the same route
    crit = losses.CrossEntropyLoss(label_smoothing=0.2)
    xx = x.clone().requires_grad_(True)
    assert torch.equal(losses.mixup_criterion(crit, xx, xx, ta, tb, lam_t).detach(), want[0])


# ---- 6. replay --------------------------------------------------------------------------------------------------------
def test_captured_draw_mix_loss_redraws_on_every_replay():
    g = np.load(GOLDEN)
    xs = [g["x%d" % i] for i in range(3)]
    x = [torch.from_numpy(a).to(DEV) for a in xs]
    gen = torch.Generator().manual_seed(5)
    ya = torch.randint(0, 7, (5, 3), generator=gen).to(DEV)
    ya[1, 2] = -1
    mix, eager = Mixup(5, alpha=0.2, device=DEV, seed=23), Mixup(5, alpha=0.2, device=DEV, seed=23)

    def step():
        mix.draw()
        mixed = mix.mix(x)
        y_a, y_b = mix.targets(ya)
        return mixed, losses.mixup_cross_entropy(mixed[0].view(15, 7), y_a.view(-1), y_b.view(-1), mix.lam, 0.2), y_b

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                         # warm-up (allocator, library); then the sequence starts over
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    mix.counter.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mixed, loss, y_b = step()
    torch.cuda.synchronize()
    assert int(mix.counter.item()) == 0          # capture launches nothing
    lams = []
    for k in range(4):
        graph.replay()
        torch.cuda.synchronize()
        eager.draw()
        assert torch.equal(mix.lam, eager.lam) and torch.equal(mix.index, eager.index) and torch.equal(mix.inverse, eager.inverse)
        lam, index = float(mix.lam.item()), mix.index.cpu().numpy()
        rl, rp, _, margin = R.draw(23, k, 0.2, 5, 1)
        assert np.array_equal(index, rp[0])
        lams.append(lam)
        for a, m in zip(xs, mixed):
            assert (np.abs(m.double().cpu().numpy() - R.mix(a, lam, index)) <= R.mix_bound(a, lam, index)).all()
        assert torch.equal(y_b, ya[torch.from_numpy(index).long().to(DEV)])
        want = losses.mixup_cross_entropy(mixed[0].view(15, 7), ya.view(-1), y_b.view(-1), lam, 0.2)
        assert torch.equal(loss, want) and torch.isfinite(loss)
    assert len(set(lams)) == 4 and int(mix.counter.item()) == 4


def test_graphed_training_iteration_redraws():
    """time MLP -> draw -> mix -> encoder -> four cross entropies with the device lam + DRLoc -> backward -> FusedAdamW, one capture"""
    import bench
    from tim_amd.graph import GraphedStep
    from tim_amd.optim import FusedAdamW
    from tim_amd.tim import TIM
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na, nf = 4, 4, 2, cfg.num_feats
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, feat_drop=0.1, seq_drop=0.1,
                d_model=cfg.d_model, nhead=cfg.nhead, num_layers=cfg.num_layers, enc_dropout=0.1, num_feats=nf, precision="fp16")
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    static = {k: v.to(DEV).clone() for k, v in inp.items()}
    tgt = bench.make_rec_targets(cfg, B, nv, na, 7, DEV)
    gen = torch.Generator().manual_seed(0)
    pos = (torch.randint(nf, (B, 8), generator=gen).to(DEV), torch.randint(nf, (B, 8), generator=gen).to(DEV))
    opt = FusedAdamW.for_model(model, lr=1e-3, weight_decay=1e-4, max_grad_norm=1.0)
    mix = Mixup(B, alpha=0.2, device=DEV, seed=9)

    def fn():
        for p in model.parameters():
            p.grad = None
        mix.draw()
        te = model(static["times"], "time_mlp")
        vis, aud, te = mix.mix([static["visual"], static["audio"], te])
        y_a, y_b = mix.targets(tgt)
        (verb, noun, action, audio), feats = model([vis, aud], "encoder", te, nv, na)
        ce = lambda x, k: losses.mixup_cross_entropy(x, y_a[k].reshape(-1), y_b[k].reshape(-1), mix.lam, 0.2)   # noqa: E731
        loss = (ce(verb, "verb") + ce(noun, "noun") + ce(action, "action")) / 3.0 + ce(audio, "class_id")
        loss = loss + 0.3 * losses.dense_relative_localization_loss_crossmodal(feats[:, :nf], feats[:, nf:], model, 8, positions=pos)
        loss.backward()
        opt.step()
        return loss.detach()

    try:
        gs = GraphedStep(model, fn, warmup=2, optimizer=opt)
        mix.counter.zero_()
        lams, seen = [], []
        for k in range(3):
            loss = gs()
            torch.cuda.synchronize()
            lams.append(float(mix.lam.item()))
            seen.append(mix.index.cpu().numpy().copy())
            assert np.array_equal(seen[-1], R.permutation(9, k, B)[0])
            assert torch.isfinite(loss).item()
            grads = [p.grad for p in model.parameters() if p.grad is not None]
            assert grads and all(torch.isfinite(gr).all().item() for gr in grads)
        assert len(set(lams)) == 3, lams
        assert int(opt.skipped_steps) == 0
    finally:
        F.graph_safe_dropout(DEV, enable=False)
