"""Device-side batch sampler (tim_amd/csrc/sampler.hip, tim_amd/data.py: WindowSampler, tim_amd/losses.py: DrlocPositions)
against the integer restatement tests/sampler_ref.py and the oracle's batch assembly.  Everything bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import data_oracle as D  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import losses  # noqa: E402
from tim_amd._lib import ptr  # noqa: E402
from tim_amd.data import DeviceWindowDataset, WindowSampler  # noqa: E402
from tim_amd.losses import DrlocPositions  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import sampler_ref as R  # noqa: E402
from tests.golden.batch_inputs import make_tables  # noqa: E402

DEV = "cuda:0"
NF, V_AUG, A_AUG = 6, 3, 2
_TABLES = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def tables(modality, Cv=8, Ca=12):
    key = (modality, Cv, Ca)
    if key not in _TABLES:
        tb = make_tables(4, modality, nf=NF, num_aug=V_AUG, Cv=Cv, Ca=Ca)
        _TABLES[key] = (tb, DeviceWindowDataset(tb["windows"], tb["num_feats"], tb["window_size"], tb["max_visual_actions"],
                                                tb["max_audio_actions"], tb["model_modality"], tb["v_feats"], tb["v_feat_times"],
                                                tb["a_feats"], tb["a_feat_times"], device=DEV))
    return _TABLES[key]


def guarded(n, dtype, pattern):
    """a buffer of n elements between two guard runs of 8 pattern elements -> (whole, view)"""
    full = torch.full((n + 16,), pattern, dtype=dtype, device=DEV)
    return full, full[8:8 + n]


def guards_intact(full, n, pattern):
    return bool((full[:8] == pattern).all().item() and (full[8 + n:] == pattern).all().item())


# ---- 1. the draw ------------------------------------------------------------------------------------------------------
# (N, world, rank, batch, shuffle, last)
DRAWS = [(7, 1, 0, 3, True, "wrap"), (7, 1, 0, 3, True, "drop"), (7, 1, 0, 3, False, "wrap"), (7, 3, 2, 2, True, "wrap"), (7, 3, 2, 2, True, "drop"),
         (7, 3, 0, 2, False, "drop"), (7, 8, 1, 1, True, "wrap"), (7, 8, 7, 1, True, "drop"), (7, 1, 0, 8, True, "wrap"), (7, 1, 0, 7, True, "drop"),
         (64, 2, 1, 8, True, "wrap"), (65, 4, 3, 8, True, "wrap"), (65, 4, 0, 8, True, "drop"), (1, 1, 0, 2, True, "wrap"), (4097, 1, 0, 300, True, "wrap")]


@pytest.mark.parametrize("N,W,r,B,shuffle,last", DRAWS)
def test_draw_is_the_restatement(N, W, r, B, shuffle, last):
    L.load()
    seed = 0x1234567890ABCDEF
    _, I = R.geometry(N, W, B, last)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    wf, window = guarded(B, torch.int32, 0x5A5A5A5A)
    vf, valid = guarded(B, torch.uint8, 0xA5)
    af, v_aug = guarded(B * NF, torch.int32, 0x5A5A5A5A)
    bf, a_aug = guarded(B * NF, torch.int32, 0x5A5A5A5A)
    ef, words = guarded(2, torch.int64, 0x5A5A5A5A5A5A5A5A)
    calls = 3 * I + 1 if N < 1000 else 2                     # 3 epochs + 1 iteration
    for t in range(calls):
        L.call("timhip_sampler_draw", seed, ptr(counter), N, W, r, B, int(shuffle), L.SAMPLER_WRAP if last == "wrap" else L.SAMPLER_DROP,
               NF, V_AUG, A_AUG, ptr(window), ptr(valid), ptr(v_aug), ptr(a_aug), ptr(words), words.data_ptr() + 8, _stream())
        torch.cuda.synchronize()
        want = R.draw(seed, t, N, W, r, B, shuffle, last, NF, V_AUG, A_AUG)
        assert np.array_equal(window.cpu().numpy(), want["window"]), t
        assert np.array_equal(valid.cpu().numpy(), want["valid"]), t
        assert np.array_equal(v_aug.cpu().numpy().reshape(B, NF), want["v_aug"]) and np.array_equal(a_aug.cpu().numpy().reshape(B, NF), want["a_aug"])
        assert words.tolist() == [want["epoch"], want["iteration"]] == [t // I, t % I]
        assert int(counter.item()) == t + 1
        assert guards_intact(wf, B, 0x5A5A5A5A) and guards_intact(vf, B, 0xA5) and guards_intact(af, B * NF, 0x5A5A5A5A)
        assert guards_intact(bf, B * NF, 0x5A5A5A5A) and guards_intact(ef, 2, 0x5A5A5A5A5A5A5A5A)


def test_draw_without_aug_and_word_outputs_from_a_later_counter():
    L.load()
    counter = torch.tensor([(5 << 33) + 2], dtype=torch.int64, device=DEV)      # an iteration number beyond 32 bits
    wf, window = guarded(3, torch.int32, 0x5A5A5A5A)
    vf, valid = guarded(3, torch.uint8, 0xA5)
    L.call("timhip_sampler_draw", 7, ptr(counter), 7, 1, 0, 3, 1, L.SAMPLER_WRAP, 0, 0, 0, ptr(window), ptr(valid), None, None, None, None, _stream())
    torch.cuda.synchronize()
    want = R.draw(7, (5 << 33) + 2, 7, 1, 0, 3, True, "wrap")
    assert np.array_equal(window.cpu().numpy(), want["window"]) and np.array_equal(valid.cpu().numpy(), want["valid"])
    assert int(counter.item()) == (5 << 33) + 3 and guards_intact(wf, 3, 0x5A5A5A5A) and guards_intact(vf, 3, 0xA5)


# ---- 2. the batch -----------------------------------------------------------------------------------------------------
def expected_batch(tb, d):
    """the oracle's collate of the restated draw; the labels and ids of absent rows are -1"""
    B = len(d["window"])
    zeros = np.zeros((B, NF), np.int64)
    va, aa = (d["v_aug"] if d["v_aug"] is not None else zeros), (d["a_aug"] if d["a_aug"] is not None else zeros)
    v, a, t, label, meta = D.collate([D.getitem(tb, int(w), va[b], aa[b]) for b, w in enumerate(d["window"])])
    gone = d["valid"] == 0
    for x in list(label.values()) + list(meta.values()):
        x[gone] = -1
    return v, a, t, label, meta


def prefill(out):
    v, a, t, label, meta = out
    for x in (v, a, t):
        x.fill_(float("nan"))
    for x in list(label.values()) + [meta["v_action_ids"], meta["a_action_ids"]]:
        x.fill_(-7777)


def assert_batch(out, want, smp):
    v, a, t, label, meta = out
    wv, wa, wt, wl, wm = want
    for got, ref in ((v, wv), (a, wa), (t, wt)):
        assert tuple(got.shape) == ref.shape and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), ref.astype(np.float32))
    assert sorted(label) == sorted(wl) == ["action", "class_id", "noun", "verb"]
    for k in wl:
        assert label[k].dtype == torch.int64 and np.array_equal(label[k].cpu().numpy(), wl[k]), k
    for k in wm:
        assert meta[k].dtype == torch.int64 and np.array_equal(meta[k].cpu().numpy(), wm[k]), k
    B, ds = smp.batch_size, smp.dataset
    assert meta["num_v_queries"].tolist() == [ds.max_visual_actions] * B and meta["num_a_queries"].tolist() == [ds.max_audio_actions] * B
    assert meta["window"] is smp.window and meta["valid"] is smp.valid


@pytest.mark.parametrize("modality,Cv,Ca,B", [("audio_visual", 8, 12, 3), ("visual", 8, 12, 3), ("audio", 8, 12, 3), ("audio_visual", 10, 7, 3),
                                              ("visual", 10, 7, 8), ("audio", 10, 7, 3), ("audio_visual", 1024, 2304, 2)])
def test_next_batch_is_the_oracles_collate_of_the_restated_draw(modality, Cv, Ca, B):
    tb, ds = tables(modality, Cv, Ca)
    seed = 17
    smp = ds.sampler(B, seed=seed, shuffle=True, last="wrap")
    assert isinstance(smp, WindowSampler) and smp.iterations_per_epoch == -(-7 // B)
    ptrs, absent = None, 0
    for t in range(smp.iterations_per_epoch + 1):
        prefill((smp.visual, smp.audio, smp.times, smp.label, smp.metadata))
        out = smp.next_batch()
        torch.cuda.synchronize()
        d = R.draw(seed, t, 7, 1, 0, B, True, "wrap", NF, V_AUG if ds.has_v else 0, V_AUG if ds.has_a else 0)
        assert np.array_equal(smp.window.cpu().numpy(), d["window"]) and np.array_equal(smp.valid.cpu().numpy(), d["valid"])
        assert_batch(out, expected_batch(tb, d), smp)
        absent += int((d["valid"] == 0).sum())
        assert (int(smp.epoch.item()), int(smp.iteration.item())) == (d["epoch"], d["iteration"])
        flat = [out[0], out[1], out[2]] + [out[3][k] for k in sorted(out[3])] + [out[4][k] for k in sorted(out[4])]
        assert ptrs is None or (ptrs == [x.data_ptr() for x in flat] and all(x is y for x, y in zip(flat, keep)))
        ptrs, keep = [x.data_ptr() for x in flat], flat
        # the present rows are what batch() assembles from the same host indices
        bv, ba, bt, bl, bm = ds.batch(d["window"], d["v_aug"], d["a_aug"])
        ok = torch.from_numpy(d["valid"] != 0).to(DEV)
        assert torch.equal(out[0], bv) and torch.equal(out[1], ba) and torch.equal(out[2], bt)
        assert all(torch.equal(out[3][k][ok], bl[k][ok]) for k in bl) and torch.equal(out[4]["v_action_ids"][ok], bm["v_action_ids"][ok])
        names = ds.narration_ids(smp.window.cpu())
        assert names["v_narration_ids"] == bm["v_narration_ids"] and names["a_narration_ids"] == bm["a_narration_ids"]
    assert absent > 0 or 7 % B == 0
    assert out[1].shape == ((B, 0) if not ds.has_a else (B, NF, Ca)) and out[0].shape == ((B, 0) if not ds.has_v else (B, NF, Cv))


def test_window_batch_on_views_off_16_byte_alignment_and_hostile_words():
    """Cv = 8 rows move as 16-byte accesses only where source and destination are aligned: an output one float off takes the
    element path; a window or an augmentation index outside its table reads entry 0"""
    tb, ds = tables("audio_visual")
    smp = ds.sampler(3, seed=2)
    smp.next_batch()
    torch.cuda.synchronize()
    want_v, want_a = smp.visual.clone(), smp.audio.clone()
    vf, v_out = guarded(3 * NF * 8 + 1, torch.float32, -123.0)
    af, a_out = guarded(3 * NF * 12 + 3, torch.float32, -123.0)
    d = smp._descriptor()
    d.visual, d.audio = v_out.data_ptr() + 4, a_out.data_ptr() + 12
    L.call("timhip_window_batch", C.byref(d), _stream())
    torch.cuda.synchronize()
    assert torch.equal(v_out[1:].view(3, NF, 8), want_v) and torch.equal(a_out[3:].view(3, NF, 12), want_a)
    assert guards_intact(vf, 3 * NF * 8 + 1, -123.0) and guards_intact(af, 3 * NF * 12 + 3, -123.0)
    assert float(v_out[0]) == -123.0 and bool((a_out[:3] == -123.0).all())
    smp.window.copy_(torch.tensor([7, -1, 1 << 30], dtype=torch.int32))
    smp.v_aug.fill_(V_AUG)
    smp.a_aug.fill_(-1)
    smp.valid.fill_(1)
    L.call("timhip_window_batch", C.byref(smp._descriptor()), _stream())
    torch.cuda.synchronize()
    zero = {"window": np.zeros(3, np.int32), "valid": np.ones(3, np.uint8), "v_aug": np.zeros((3, NF), np.int64), "a_aug": np.zeros((3, NF), np.int64)}
    assert_batch((smp.visual, smp.audio, smp.times, smp.label, smp.metadata), expected_batch(tb, zero), smp)


def test_sharded_sampler_without_shuffle_and_drop():
    tb, ds = tables("audio_visual")
    smp = ds.sampler(2, seed=1, shuffle=False, rank=2, world=3, last="drop")
    assert smp.iterations_per_epoch == 1 and smp.per_rank == 3
    for t in range(3):
        out = smp.next_batch()
        torch.cuda.synchronize()
        d = R.draw(1, t, 7, 3, 2, 2, False, "drop", NF, V_AUG, V_AUG)
        assert d["window"].tolist() == [2, 5] and d["valid"].all()
        assert_batch(out, expected_batch(tb, d), smp)


# ---- 3. capture -------------------------------------------------------------------------------------------------------
def snapshot(out, pos):
    v, a, t, label, meta = out
    return [x.clone() for x in [v, a, t] + [label[k] for k in sorted(label)] + [meta[k] for k in sorted(meta)] + [pos.pos_1, pos.pos_2, pos.deltax]]


def test_captured_sampler_and_drloc_draw_redraw_on_every_replay():
    tb, ds = tables("audio_visual")
    B, seed = 3, 5
    smp, eager = ds.sampler(B, seed=seed), ds.sampler(B, seed=seed)
    pos, epos = DrlocPositions(B, 8, NF, DEV, seed=9), DrlocPositions(B, 8, NF, DEV, seed=9)
    I = smp.iterations_per_epoch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        smp.next_batch()                 # warm-up (library); then the sequence starts over
        pos.draw()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    smp.set_iteration(0)
    pos.counter.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = smp.next_batch()
        pos.draw()
    torch.cuda.synchronize()
    assert int(smp.counter.item()) == 0 and int(pos.counter.item()) == 0          # capture launches nothing
    epochs, windows, j, resumed = [], [], 2, None
    for k in range(2 * I + 1):                                                    # an epoch boundary falls inside the replays
        graph.replay()
        torch.cuda.synchronize()
        got = snapshot(out, pos)
        want = snapshot(eager.next_batch(), epos.draw())
        torch.cuda.synchronize()
        assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(got, want)), k
        d = R.draw(seed, k, 7, 1, 0, B, True, "wrap", NF, V_AUG, V_AUG)
        assert np.array_equal(smp.window.cpu().numpy(), d["window"]) and np.array_equal(pos.pos_1.cpu().numpy(), R.drloc(9, k, B, 8, NF)[0])
        assert_batch(out, expected_batch(tb, d), smp)
        epochs.append(int(smp.epoch.item()))
        windows.append(tuple(smp.window.tolist()))
        if resumed is not None:                                                   # replay j + 1 against the state taken after j replays
            fresh, fpos = ds.sampler(B, seed=seed + 1), DrlocPositions(B, 8, NF, DEV, seed=1)
            fresh.load_state_dict(resumed[0])
            fpos.load_state_dict(resumed[1])
            again = snapshot(fresh.next_batch(), fpos.draw())
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(got, again))
            resumed = None
        if k + 1 == j:
            resumed = (smp.state_dict(), pos.state_dict())
            assert resumed[0]["counter"] == j and resumed[1]["counter"] == j
    assert epochs == [k // I for k in range(2 * I + 1)] and len(set(windows)) > 1
    assert int(smp.counter.item()) == 2 * I + 1
    with pytest.raises(ValueError):
        ds.sampler(B + 1, seed=seed).load_state_dict(smp.state_dict())
    with pytest.raises(ValueError):
        ds.sampler(B, seed=seed, rank=1, world=2).load_state_dict(smp.state_dict())
    with pytest.raises(ValueError):
        smp.set_iteration(I << 23)


# ---- 4. DRLoc ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,l", [(1, 1, 1), (3, 8, 6), (64, 32, 50)])
def test_drloc_draw_is_the_restatement(n, m, l):
    L.load()
    seed = 0xFEDCBA9876543210
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    f1, p1 = guarded(n * m, torch.int64, 0x5A5A5A5A5A5A5A5A)
    f2, p2 = guarded(n * m, torch.int64, 0x5A5A5A5A5A5A5A5A)
    fd, dx = guarded(n * m, torch.float32, -123.0)
    for c in range(3):
        L.call("timhip_drloc_draw", seed, ptr(counter), n, m, l, ptr(p1), ptr(p2), ptr(dx), _stream())
        torch.cuda.synchronize()
        w1, w2, wd = R.drloc(seed, c, n, m, l)
        assert np.array_equal(p1.cpu().numpy().reshape(n, m), w1) and np.array_equal(p2.cpu().numpy().reshape(n, m), w2)
        assert np.array_equal(dx.cpu().numpy().reshape(n, m).view(np.uint32), wd.view(np.uint32))
        assert int(counter.item()) == c + 1
        assert guards_intact(f1, n * m, 0x5A5A5A5A5A5A5A5A) and guards_intact(f2, n * m, 0x5A5A5A5A5A5A5A5A) and guards_intact(fd, n * m, -123.0)
    obj = DrlocPositions(n, m, l, DEV, seed=seed)
    obj.load_state_dict({"seed": seed, "counter": 2, "n": n, "m": m, "l": l})
    obj.draw()
    torch.cuda.synchronize()
    assert torch.equal(obj.pos_1.view(-1), p1) and torch.equal(obj.pos_2.view(-1), p2) and torch.equal(obj.deltax.view(-1), dx)
    assert obj.state_dict() == {"seed": seed, "counter": 3, "n": n, "m": m, "l": l}


def _tiny_model(prec):
    from tim_amd.tim import TIM
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, _ = H.synth_torch(cfg, 2, 2, 2, seed=3, dtype=torch.float32)
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=prec)
    model.load_state_dict(sd)
    return cfg, model.to(DEV).train()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_drloc_loss_with_device_positions_is_the_tuple_path(prec):
    """The loss, d x1, d x2 and the MLP's gradients with `positions=obj` are those of `positions=(pos_1, pos_2)`, bit for bit.
    The backward scatters the operand gradient into d x1 / d x2 with float atomics (positions repeat, csrc/losses.hip): three or
    more addends into one element arrive in an order that changes from run to run, on the tuple path too.  With m = 2 an element
    receives at most two, and 0 + a + b is the same sum in either order: that is the shape held bit for bit.  At m = 8 (more
    samples than the 6 positions: repeats are certain) the loss and the MLP's gradients are still bit for bit and d x is held to
    2^-20 of its largest element: seven reorderings of at most eight addends of that size, half an ulp each, leave 2^-21."""
    cfg, model = _tiny_model(prec)
    n, l = 3, cfg.num_feats
    gen, width = torch.Generator().manual_seed(1), model.drloc_mlp[0].weight.shape[1] // 2      # the MLP reads a pair of rows
    f1, f2 = torch.randn(n, l, width, generator=gen).to(DEV), torch.randn(n, l, width, generator=gen).to(DEV)

    def run(positions, m, cross=True):
        for p in model.parameters():
            p.grad = None
        x1, x2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        loss = (losses.dense_relative_localization_loss_crossmodal(x1, x2, model, m, positions=positions) if cross
                else losses.dense_relative_localization_loss(x1, model, m, positions=positions))
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if k.startswith("drloc_mlp.")}
        return loss.detach().clone(), x1.grad.clone(), None if x2.grad is None else x2.grad.clone(), grads

    for m in (2, 8):
        obj = DrlocPositions(n, m, l, DEV, seed=4).draw()
        a = run(obj, m)
        b = run((obj.pos_1.clone(), obj.pos_2.clone()), m)
        print("m = %d: loss %r / %r, largest difference d x1 %.3g, d x2 %.3g" % (m, a[0].item(), b[0].item(), (a[1] - b[1]).abs().max().item(),
                                                                                 (a[2] - b[2]).abs().max().item()))
        assert torch.isfinite(a[0]) and torch.equal(a[0], b[0])
        assert len(a[3]) == 6 and all(torch.equal(a[3][k], b[3][k]) for k in a[3])
        for x, y in ((a[1], b[1]), (a[2], b[2])):
            assert x.abs().max() > 0
            assert torch.equal(x, y) if m == 2 else bool(((x - y).abs() <= 2.0 ** -20 * y.abs().max()).all())
    obj = DrlocPositions(n, 8, l, DEV, seed=4).draw()          # the single-modality loss takes the object as well
    a, b = run(obj, 8, cross=False), run((obj.pos_1.clone(), obj.pos_2.clone()), 8, cross=False)
    assert torch.equal(a[0], b[0]) and a[2] is None and bool(((a[1] - b[1]).abs() <= 2.0 ** -20 * b[1].abs().max()).all())
    for bad in (DrlocPositions(n + 1, 8, l, DEV), DrlocPositions(n, 9, l, DEV), DrlocPositions(n, 8, l + 1, DEV)):
        with pytest.raises(ValueError):
            losses.dense_relative_localization_loss_crossmodal(f1, f2, model, 8, positions=bad.draw())


# ---- 5. argument checks -----------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_counters_alone():
    lib = L.load()
    tb, ds = tables("audio_visual")
    counter = torch.tensor([41], dtype=torch.int64, device=DEV)
    window, valid = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV)
    aug = torch.zeros((8, NF), dtype=torch.int32, device=DEV)
    good = dict(seed=1, counter=ptr(counter), N=7, W=1, r=0, B=3, shuffle=1, last=L.SAMPLER_WRAP, nf=NF, va=V_AUG, aa=A_AUG, window=ptr(window),
                valid=ptr(valid), v_aug=ptr(aug), a_aug=ptr(aug), epoch=None, iteration=None)
    draw = lambda **kw: lib.timhip_sampler_draw(*dict(good, **kw).values(), _stream())   # noqa: E731
    for bad in (dict(counter=None), dict(window=None), dict(valid=None), dict(B=0), dict(B=-3), dict(B=(1 << 20) + 1), dict(N=0), dict(W=0),
                dict(r=1), dict(r=-1), dict(W=3, r=3), dict(last=2), dict(last=L.SAMPLER_DROP, B=8), dict(last=L.SAMPLER_DROP, W=3, B=4),
                dict(va=0), dict(aa=-1), dict(nf=0), dict(B=1 << 20, nf=17)):
        assert draw(**bad) == L.EINVAL, bad
    pos = torch.zeros((3, 8), dtype=torch.int64, device=DEV)
    dx = torch.zeros((3, 8), dtype=torch.float32, device=DEV)
    dgood = dict(seed=1, counter=ptr(counter), n=3, m=8, l=6, p1=ptr(pos), p2=ptr(pos), dx=ptr(dx))
    ddraw = lambda **kw: lib.timhip_drloc_draw(*dict(dgood, **kw).values(), _stream())   # noqa: E731
    for bad in (dict(counter=None), dict(p1=None), dict(p2=None), dict(dx=None), dict(n=0), dict(m=0), dict(l=0), dict(l=(1 << 24) + 1),
                dict(n=1 << 13, m=(1 << 12) + 1)):
        assert ddraw(**bad) == L.EINVAL, bad
    smp = ds.sampler(3)
    for field, value in (("window", None), ("valid", None), ("times", None), ("visual", None), ("a_row0", None), ("verb", None), ("a_ids", None),
                         ("feat_indices", None), ("B", 0), ("num_feats", 0), ("num_windows", 0), ("window_size", 0.0), ("v_ld", 1), ("Ca", 0)):
        d = smp._descriptor()
        setattr(d, field, value)
        assert lib.timhip_window_batch(C.byref(d), _stream()) == L.EINVAL, field
    assert lib.timhip_window_batch(None, _stream()) == L.EINVAL
    d = smp._descriptor()
    d.audio = smp.audio.data_ptr() + 2
    assert lib.timhip_window_batch(C.byref(d), _stream()) == L.EALIGN
    torch.cuda.synchronize()
    assert int(counter.item()) == 41 and int(smp.counter.item()) == 0
    for kw in (dict(batch_size=0), dict(batch_size=3, rank=1), dict(batch_size=3, rank=2, world=2), dict(batch_size=8, last="drop"),
               dict(batch_size=3, last="pad"), dict(batch_size=3, world=0)):
        with pytest.raises(ValueError):
            ds.sampler(**kw)
    for args in ((0, 8, 6), (3, 0, 6), (3, 8, 0), (3, 8, (1 << 24) + 1)):
        with pytest.raises(ValueError):
            DrlocPositions(*args, DEV)
    with pytest.raises(ValueError):
        ds.narration_ids([0, 7])
