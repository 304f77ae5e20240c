"""The detection dataset on the device (tim_amd/det_data.py: DeviceDetectionDataset, DetectionWindowSampler; tim_amd/csrc/sampler.hip:
timhip_det_window_batch) against the numpy restatement tests/det_batch_ref.py (held against the reference's own outputs by
tests/test_det_batch_ref.py) and the sampler's integer restatement tests/sampler_ref.py.  Everything bit for bit; zeros are
compared by ==."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tim_amd import _lib as L  # noqa: E402
from tim_amd import losses  # noqa: E402
from tim_amd.det_data import DetectionWindowSampler, DeviceDetectionDataset, action_column  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tests import det_batch_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import sampler_ref as S  # noqa: E402
from tests.golden.det_batch_inputs import A_NUM_AUG, MAX_A, MAX_V, NF, V_NUM_AUG, make_tables  # noqa: E402

DEV = "cuda:0"
SETTINGS = {0: ("epic", False, True), 1: ("epic", False, False), 2: ("epic", True, True)}
_TABLES = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def dataset_of(tb, col=2):
    name, vn, vo = SETTINGS[col]
    return DeviceDetectionDataset(tb["windows"], tb["num_feats"], tb["window_size"], tb["max_visual_actions"], tb["max_audio_actions"],
                                  tb["model_modality"], tb["v_feats"], tb["v_feat_times"], tb["a_feats"], tb["a_feat_times"],
                                  dataset_name=name, include_verb_noun=vn, verb_only=vo, device=DEV)


def tables(modality, Cv=8, Ca=12, col=2):
    key = (modality, Cv, Ca, col)
    if key not in _TABLES:
        tb = make_tables(81, modality, Cv=Cv, Ca=Ca)
        _TABLES[key] = (tb, dataset_of(tb, col))
    return _TABLES[key]


def assert_batch(out, want, ds):
    v, a, t, label, meta = out
    wv, wa, wt, wl, wm = want
    B = wt.shape[0]
    for got, ref in ((v, wv), (a, wa), (t, wt)):
        assert tuple(got.shape) == ref.shape and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), ref)
    assert v.shape == ((B, NF, ds.v["C"]) if ds.has_v else (B, 0)) and a.shape == ((B, NF, ds.a["C"]) if ds.has_a else (B, 0))
    assert sorted(label) == sorted(wl) == sorted(R.LABEL_KEYS)
    for k in wl:
        assert label[k].dtype == (torch.float32 if k.endswith("segments") else torch.int64) and label[k].shape == wl[k].shape, k
        assert np.array_equal(label[k].cpu().numpy(), wl[k]), k
    assert meta["window_start"].dtype == torch.float64 and np.array_equal(meta["window_start"].cpu().numpy(), wm["window_start"])
    assert meta["window_size"].dtype == torch.float64 and np.array_equal(meta["window_size"].cpu().numpy(), wm["window_size"])
    assert meta["video_index"].dtype == torch.int32 and np.array_equal(meta["video_index"].cpu().numpy(), wm["video_index"])
    assert all(x.is_cuda for x in (meta["window_start"], meta["window_size"], meta["video_index"]))


# ---- 1. batch() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", [0, 1, 2])
@pytest.mark.parametrize("modality", ["audio_visual", "visual", "audio"])
def test_batch_is_the_restatement(modality, col):
    tb, ds = tables(modality, col=col)
    assert ds.action_col == col == action_column(*SETTINGS[col]) and action_column("thumos", False, True) == 2
    assert ds.video_ids == tb["video_ids"] and len(ds) == len(tb["windows"])
    idx = [5, 0, 5, 7, 2, 1, 0, 6, 3, 4]                          # windows repeat and arrive out of order
    rs = np.random.RandomState(3)
    va = rs.randint(0, V_NUM_AUG, (len(idx), NF)) if ds.has_v else None
    aa = rs.randint(0, A_NUM_AUG, (len(idx), NF)) if ds.has_a else None
    out = ds.batch(idx, va, aa)
    torch.cuda.synchronize()
    want = R.batch(tb, idx, va, aa, col)
    assert_batch(out, want, ds)
    assert out[4]["video_id"] == want[4]["video_id"] == ds.video_ids_of(idx)
    drawn = ds.batch(torch.tensor([1, 4]))                           # augmentation indices drawn on the device: rows of the store
    torch.cuda.synchronize()
    assert np.array_equal(drawn[2].cpu().numpy(), R.batch(tb, [1, 4], None, None, col)[2]) and drawn[3]["action"].shape == (2, MAX_V)
    with pytest.raises(ValueError):
        ds.batch([0, len(ds)])
    with pytest.raises(ValueError):
        ds.video_ids_of([-1])


def test_constructor_checks_and_from_reference():
    tb, ds = tables("audio_visual")
    with pytest.raises(ValueError):                                 # more actions than the maximum
        DeviceDetectionDataset(tb["windows"], NF, tb["window_size"], MAX_V - 1, MAX_A, "audio_visual", tb["v_feats"], tb["v_feat_times"],
                               tb["a_feats"], tb["a_feat_times"], device=DEV)
    with pytest.raises(ValueError):                                 # a modality without its features
        DeviceDetectionDataset(tb["windows"], NF, tb["window_size"], MAX_V, MAX_A, "audio_visual", tb["v_feats"], tb["v_feat_times"], device=DEV)
    with pytest.raises(ValueError):
        DeviceDetectionDataset(tb["windows"], NF + 1, tb["window_size"], MAX_V, MAX_A, "visual", tb["v_feats"], tb["v_feat_times"], device=DEV)

    class Ref:                                                      # the attributes a constructed reference dataset holds
        windows, num_feats, window_size = tb["windows"], NF, tb["window_size"]
        max_visual_actions, max_audio_actions, model_modality = MAX_V, MAX_A, "audio_visual"
        v_feats, v_feat_times, a_feats, a_feat_times = tb["v_feats"], tb["v_feat_times"], tb["a_feats"], tb["a_feat_times"]
        dataset_name, include_verb_noun, verb_only = "epic", False, False

    ref = DeviceDetectionDataset.from_reference(Ref, device=DEV)
    assert ref.action_col == 1
    out = ref.batch([2, 0], np.zeros((2, NF), np.int64), np.ones((2, NF), np.int64))
    torch.cuda.synchronize()
    assert_batch(out, R.batch(tb, [2, 0], np.zeros((2, NF), np.int64), np.ones((2, NF), np.int64), 1), ref)


# ---- 2. the raw call --------------------------------------------------------------------------------------------------
PATTERN = {torch.float32: -123.0, torch.float64: -123.0, torch.int64: -7777, torch.int32: 0x5A5A5A5A}


class Guarded:
    """the outputs of one call, each between two guard runs of 8 pattern elements"""

    def __init__(self, ds, B):
        self.ds, self.full = ds, []

        def fill(shape, dtype):
            n = int(np.prod(shape))
            full = torch.full((n + 16,), PATTERN[dtype], dtype=dtype, device=DEV)
            self.full.append((full, n, PATTERN[dtype]))
            return full[8:8 + n].view(shape)

        self.out = ds._outputs(B, fill)

    def guards_intact(self):
        return all(bool((f[:8] == p).all().item() and (f[8 + n:] == p).all().item()) for f, n, p in self.full)

    def untouched(self):
        return all(bool((f == p).all().item()) for f, _, p in self.full)

    def batch(self):
        v, a, t, label, start, vidx = self.out
        B = t.shape[0]
        return v, a, t, label, {"window_start": start, "video_index": vidx, "window_size": torch.full((B,), self.ds.window_size, dtype=torch.float64, device=DEV)}


def words(ds, window, valid, va, aa):
    dev = lambda x, dt: None if x is None else torch.as_tensor(np.asarray(x)).to(device=DEV, dtype=dt).contiguous()   # noqa: E731
    return dev(window, torch.int32), dev(valid, torch.uint8), dev(va if ds.has_v else None, torch.int32), dev(aa if ds.has_a else None, torch.int32)


@pytest.mark.parametrize("modality,Cv,Ca", [("audio_visual", 8, 12), ("audio_visual", 10, 1100), ("visual", 1100, 12), ("audio", 8, 10),
                                            ("visual", 10, 12)])
def test_raw_call_into_guarded_buffers(modality, Cv, Ca):
    """Cv / Ca = 10: rows off 16-byte alignment take the element path; 1100 floats: 275 chunks, more than the 256 one wave item
    group covers.  Guards stay intact, every output element is written, the outputs of an absent modality are not touched."""
    tb, ds = tables(modality, Cv, Ca)
    N = len(tb["windows"])
    window = [N - 1, 0, 3, 3, 1]
    valid = [1, 1, 0, 1, 1]
    B = len(window)
    rs = np.random.RandomState(5)
    va, aa = rs.randint(0, V_NUM_AUG, (B, NF)), rs.randint(0, A_NUM_AUG, (B, NF))
    g = Guarded(ds, B)
    w = words(ds, window, valid, va, aa)
    lib = L.load()
    assert lib.timhip_det_window_batch(C.byref(ds._descriptor(B, *w, g.out)), _stream()) == 0
    torch.cuda.synchronize()
    assert g.guards_intact()
    assert_batch(g.batch(), R.batch(tb, window, va if ds.has_v else None, aa if ds.has_a else None, 2, valid=np.array(valid)), ds)
    gone = g.out[3]
    assert bool((gone["verb"][2] == -1).all()) and bool((gone["class_id"][2] == -1).all()) and bool((gone["v_gt_segments"][2] == 0).all())
    # an absent modality: its output pointer is not written even when one is handed over
    if not (ds.has_v and ds.has_a):
        spare = torch.full((64,), -123.0, dtype=torch.float32, device=DEV)
        d = ds._descriptor(B, *w, g.out)
        if ds.has_v:
            d.audio = spare.data_ptr()
        else:
            d.visual = spare.data_ptr()
        assert lib.timhip_det_window_batch(C.byref(d), _stream()) == 0
        torch.cuda.synchronize()
        assert bool((spare == -123.0).all()) and g.guards_intact()
    # a window or an augmentation word outside its table is read as 0
    hostile = words(ds, [N, -1, 1 << 30, 0, -(1 << 31)], [1] * B, np.full((B, NF), V_NUM_AUG), np.full((B, NF), -1))
    g2 = Guarded(ds, B)
    assert lib.timhip_det_window_batch(C.byref(ds._descriptor(B, *hostile, g2.out)), _stream()) == 0
    torch.cuda.synchronize()
    zero = np.zeros((B, NF), np.int64)
    assert g2.guards_intact()
    assert_batch(g2.batch(), R.batch(tb, [0] * B, zero if ds.has_v else None, zero if ds.has_a else None, 2), ds)


def test_refused_calls_launch_nothing():
    tb, ds = tables("audio_visual")
    lib = L.load()
    B = 3
    g = Guarded(ds, B)
    w = words(ds, [0, 1, 2], [1, 1, 1], np.zeros((B, NF)), np.zeros((B, NF)))
    fresh = lambda: ds._descriptor(B, *w, g.out)   # noqa: E731
    assert lib.timhip_det_window_batch(None, _stream()) == L.EINVAL
    null = ["window", "valid", "feat_indices", "start_sec", "window_start_sec", "video_of", "times", "window_start", "video_index", "visual",
            "audio", "v_row0", "a_row0", "v_feat_times", "a_feat_times", "v_segments", "a_segments", "v_labels", "a_labels", "v_gt_segments",
            "a_gt_segments", "verb", "noun", "action", "class_id"]
    bad = [(f, None) for f in null] + [("B", 0), ("B", -2), ("num_windows", 0), ("num_feats", 0), ("window_size", 0.0), ("window_size", -2.4),
                                       ("window_size", float("nan")), ("action_col", -1), ("action_col", 3), ("v_ld", 1), ("Ca", 0),
                                       ("a_num_aug", 0), ("max_v", -1)]
    for field, value in bad:
        d = fresh()
        setattr(d, field, value)
        assert lib.timhip_det_window_batch(C.byref(d), _stream()) == L.EINVAL, (field, value)
    for side in ("v", "a"):                                          # a modality's times without its features; then neither modality
        d = fresh()
        setattr(d, side + "_feats", None)
        assert lib.timhip_det_window_batch(C.byref(d), _stream()) == L.EINVAL, side
    d = fresh()
    d.v_feats = d.a_feats = d.v_feat_times = d.a_feat_times = None
    assert lib.timhip_det_window_batch(C.byref(d), _stream()) == L.EINVAL
    for field, off, code in (("visual", 2, L.EALIGN), ("times", 1, L.EALIGN), ("a_gt_segments", 2, L.EALIGN), ("start_sec", 3, L.EALIGN),
                             ("v_feats", 2, L.EALIGN), ("window_start", 4, L.EALIGN), ("window_start_sec", 4, L.EALIGN)):
        d = fresh()
        setattr(d, field, getattr(d, field) + off)
        assert lib.timhip_det_window_batch(C.byref(d), _stream()) == code, field
    torch.cuda.synchronize()
    assert g.untouched()
    assert lib.timhip_det_window_batch(C.byref(fresh()), _stream()) == 0        # the descriptor the refusals were cut from is a good one
    torch.cuda.synchronize()
    assert g.guards_intact() and not g.untouched()


# ---- 3. the sampler ---------------------------------------------------------------------------------------------------
def expected(tb, ds, d, col=2):
    return R.batch(tb, d["window"], d["v_aug"], d["a_aug"], col, valid=d["valid"])


def restated_draw(ds, smp, t):
    return S.draw(smp.seed, t, ds.num_windows, smp.world, smp.rank, smp.batch_size, smp.shuffle, smp.last, NF,
                  V_NUM_AUG if ds.has_v else 0, A_NUM_AUG if ds.has_a else 0)


def flat(out):
    v, a, t, label, meta = out
    return [v, a, t] + [label[k] for k in sorted(label)] + [meta[k] for k in sorted(meta)]


@pytest.mark.parametrize("modality,col", [("audio_visual", 2), ("visual", 0), ("audio", 1)])
def test_sampler_eager_and_replayed_is_the_restated_draw_through_the_restatement(modality, col):
    tb, ds = tables(modality, col=col)
    B, seed = 3, 11
    eager, smp = ds.sampler(B, seed=seed), ds.sampler(B, seed=seed)
    assert isinstance(smp, DetectionWindowSampler) and smp.iterations_per_epoch == -(-ds.num_windows // B)
    calls = 3 * smp.iterations_per_epoch + 1                          # three epochs and one iteration
    assert calls < 30
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = flat(smp.next_batch())                                 # warm-up; then the sequence starts over
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    smp.set_iteration(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                     # ONE capture
        out = smp.next_batch()
    torch.cuda.synchronize()
    assert int(smp.counter.item()) == 0
    assert all(x is y for x, y in zip(flat(out), warm))               # the captured call returned the objects of the eager one
    ekeep, absent, epochs = None, 0, []
    for t in range(calls):
        graph.replay()
        e_out = eager.next_batch()
        torch.cuda.synchronize()
        d = restated_draw(ds, smp, t)
        want = expected(tb, ds, d, col)
        for got, s in ((out, smp), (e_out, eager)):
            assert np.array_equal(s.window.cpu().numpy(), d["window"]) and np.array_equal(s.valid.cpu().numpy(), d["valid"])
            assert got[4]["window"] is s.window and got[4]["valid"] is s.valid
            assert_batch(got, want, ds)
            assert (int(s.epoch.item()), int(s.iteration.item())) == (d["epoch"], d["iteration"])
        assert ds.video_ids_of(smp.window.cpu()) == want[4]["video_id"]
        ef = flat(e_out)
        assert ekeep is None or all(x is y for x, y in zip(ef, ekeep))         # the same objects on every call
        ekeep = ef
        gone = d["valid"] == 0
        absent += int(gone.sum())
        if gone.any():                                                # a short last batch: -1 labels, zero segments, a real window's rest
            g = torch.from_numpy(gone).to(DEV)
            assert all(bool((out[3][k][g] == (0 if k.endswith("segments") else -1)).all()) for k in out[3])
            assert bool((out[4]["window_start"][g] == ds.window_start_sec[smp.window.long()][g]).all())
        epochs.append(d["epoch"])
    assert absent > 0 and epochs[-1] == 3 and int(smp.counter.item()) == int(eager.counter.item()) == calls


def test_three_ranks_partition_an_epoch():
    tb, ds = tables("audio_visual")
    N, B = ds.num_windows, 2
    seen = []
    for rank in range(3):
        smp = ds.sampler(B, seed=4, rank=rank, world=3)
        assert smp.per_rank == -(-N // 3) and smp.iterations_per_epoch == -(-smp.per_rank // B)
        for t in range(smp.iterations_per_epoch):
            out = smp.next_batch()
            torch.cuda.synchronize()
            d = S.draw(4, t, N, 3, rank, B, True, "wrap", NF, V_NUM_AUG, A_NUM_AUG)
            assert_batch(out, expected(tb, ds, d), ds)
            seen += smp.window[smp.valid != 0].tolist()
    assert len(seen) == 3 * (-(-N // 3)) and set(seen) == set(range(N))      # the epoch's order padded with its own head
    perm = S.perm(4, 0, np.arange(N), N)[0].tolist()
    assert sorted(seen) == sorted(perm + perm[:len(seen) - N])


def test_sampler_position_and_checkpoint():
    tb, ds = tables("audio_visual")
    smp = ds.sampler(3, seed=6, last="drop")
    I = smp.iterations_per_epoch
    assert I == ds.num_windows // 3
    for _ in range(I + 1):
        out = smp.next_batch()
    torch.cuda.synchronize()
    assert bool(smp.valid.all()) and (int(smp.epoch.item()), int(smp.iteration.item())) == (1, 0)     # "drop": no absent rows, ever
    sd = smp.state_dict()
    assert sd["counter"] == I + 1 and sd["last"] == "drop"
    nxt = [x.clone() for x in flat(smp.next_batch())]
    fresh = ds.sampler(3, seed=99, last="drop")
    fresh.load_state_dict(sd)
    again = flat(fresh.next_batch())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(nxt, again)) and fresh.seed == 6
    smp.set_iteration(1)
    out = smp.next_batch()
    torch.cuda.synchronize()
    assert_batch(out, expected(tb, ds, restated_draw(ds, smp, 1)), ds)
    with pytest.raises(ValueError):
        ds.sampler(2, seed=6, last="drop").load_state_dict(sd)
    with pytest.raises(ValueError):
        smp.set_iteration(I << 23)
    for kw in (dict(batch_size=0), dict(batch_size=3, rank=1), dict(batch_size=ds.num_windows + 1, last="drop"), dict(batch_size=3, last="pad")):
        with pytest.raises(ValueError):
            ds.sampler(**kw)


# ---- 4. the model -----------------------------------------------------------------------------------------------------
_RUNS = []


def model_runs():
    """`next_batch()` + the tiny detection model's forward (fp32 mode) with `label_queries=True` + the side losses, captured ONCE
    and replayed four times; after every replay the eager path runs the same iteration, twice -> [(replayed, eager, eager
    again)], each a dict of clones (computed once, shared by the two tests below)"""
    if _RUNS:
        return _RUNS
    from tim_amd.detection import TIM
    cfg = H.tiny_cfg("detection", "audio_visual", "audio_visual", True)
    tb = copy.deepcopy(make_tables(81, "audio_visual", Cv=cfg.visual_input_dim, Ca=cfg.audio_input_dim))
    (nverb, nnoun, nact), ncls = cfg.num_class
    for w in tb["windows"]:                                          # labels inside the tiny model's classes
        w["v_labels"][:, :3] %= np.array([nverb, nnoun, nact])
        w["a_labels"][:, 3] %= ncls
    ds = dataset_of(tb)
    sd, _ = H.synth_torch(cfg, 2, 0, 0, seed=3, dtype=torch.float32)
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision="fp32")
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    B, seed = 3, 8

    def forward(smp, norm):
        visual, audio, times, label, _ = smp.next_batch()
        output, offsets, labels, _, ious = model([visual, audio], "encoder", times, label, label_queries=True)
        loss = None
        for m, (cls_ids, lab) in enumerate((((0, 1, 2), labels[0]), ((3,), [labels[1]]))):
            # ordered=True: the side's sums in a fixed order (the default form adds them with float atomics, and its loss differs
            # in the last place between any two runs of one input)
            side = losses.detection_side_loss([output[0][c] for c in cls_ids], lab, output[1][m], offsets[m], ious[m], norm,
                                              model.iou_threshold, lambda_reg=1.0, momentum=0.9, ordered=True)
            loss = side if loss is None else loss + side
        return {"loss": loss.detach(), "offsets": list(offsets), "ious": list(ious), "labels": [*labels[0], labels[1]], "norm": norm,
                "window": smp.window, "logits": [x.detach() for x in output[0]] + [x.detach() for x in output[1]]}

    def clones(r):
        torch.cuda.synchronize()
        return {k: ([x.clone() for x in v] if isinstance(v, list) else v.clone()) for k, v in r.items()}

    smp, eager = ds.sampler(B, seed=seed), ds.sampler(B, seed=seed)
    norm, enorm = torch.full((), 100.0, dtype=torch.float32, device=DEV), torch.full((), 100.0, dtype=torch.float32, device=DEV)
    gs = GraphedStep(model, lambda: forward(smp, norm))                 # three warm-up calls: iterations 0 - 2
    for k in range(4):                                                  # replays: iterations 3 - 6, an epoch boundary among them
        before = norm.clone()
        got = clones(gs())
        assert np.array_equal(got["window"].cpu().numpy(), restated_draw(ds, smp, 3 + k)["window"])
        refs = []
        for _ in range(2):
            eager.set_iteration(3 + k)
            enorm.copy_(before)
            refs.append(clones(forward(eager, enorm)))
        dl = max((x - y).abs().max().item() for x, y in zip(got["logits"], refs[0]["logits"]))
        print("iteration %d: loss replayed %r, eager %r, eager again %r; largest logit difference replayed - eager %.3g"
              % (3 + k, got["loss"].item(), refs[0]["loss"].item(), refs[1]["loss"].item(), dl))
        _RUNS.append((got, refs[0], refs[1]))
    gs.reset()
    return _RUNS


def test_captured_batch_and_forward_gives_the_eager_labels_and_ious_bit_for_bit():
    positives = 0
    for got, ref, _ in model_runs():
        assert torch.equal(got["window"], ref["window"]) and torch.equal(got["norm"], ref["norm"])
        for x, y in zip(got["offsets"] + got["ious"] + got["labels"], ref["offsets"] + ref["ious"] + ref["labels"]):
            assert x.shape == y.shape and torch.equal(x, y)
        positives += int(torch.isfinite(got["offsets"][0][:, 0]).sum()) + int(torch.isfinite(got["offsets"][1][:, 0]).sum())
    assert positives > 0


def test_captured_batch_and_forward_gives_the_eager_loss_bit_for_bit():
    """The loss of a replay against the loss of the eager path on the same iteration, and of the eager path run again, bit for
    bit in fp32 mode.  The side losses are computed with `ordered=True`: with the default form (float atomics onto one word, in
    the order the blocks arrive) the loss of ONE iteration is not reproducible in its last place between any two runs, eager or
    replayed - measured with it: iteration 3 replayed 44.943885803222656, eager 44.943885803222656, eager again
    44.943878173828125, with logits, labels, IoUs, offsets and normaliser equal bit for bit."""
    for got, ref, again in model_runs():
        assert torch.isfinite(got["loss"]) and torch.equal(got["loss"], ref["loss"]) and torch.equal(ref["loss"], again["loss"])


# ---- 5. the ordered side loss -------------------------------------------------------------------------------------------
def _side_inputs(rows, Cs, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [(3.0 * torch.randn(rows, c, generator=g)).to(DEV) for c in Cs]
    ts = [torch.rand(rows, c, generator=g).to(DEV) for c in Cs]
    iou = torch.rand(rows, generator=g)
    iou[::7] = -1.0                                                   # rows outside the classification loss
    off = torch.rand(rows, 2, generator=g)
    off[::3] = float("inf")                                           # non-positive rows
    return xs, ts, iou.to(DEV), off.to(DEV), torch.rand(rows, 2, generator=g).to(DEV)


@pytest.mark.parametrize("rows,Cs", [(1, (3,)), (300, (7, 11, 13)), (70000, (5,)), (1197, (97, 300, 13, 5))])
def test_ordered_side_loss_is_reproducible_and_the_atomic_sum_reordered(rows, Cs):
    """timhip_det_side_loss_fwd_ordered: the same bits in every run; block[1..3] equal those of the atomic form up to the
    reordering of one set of partial sums - P non-negative partials added in two orders differ by at most 2 (P - 1) 2^-24 of
    their sum, P <= 512 per head and 1024 for the rows; the count is a sum of integers and exact; the partials scratch is
    written inside its TIMHIP_DET_SIDE_PARTIALS floats only; the gradients through either block are those of the default form."""
    lib = L.load()
    xs, ts, iou, off, rp = _side_inputs(rows, Cs, 5)
    pa = lambda tl: (C.c_void_p * len(tl))(*[t.data_ptr() for t in tl])   # noqa: E731
    cs = (C.c_int * len(Cs))(*Cs)

    def run(ordered, scratch=None):
        norm = torch.full((), 100.0, dtype=torch.float32, device=DEV)
        block = torch.full((8,), -123.0, dtype=torch.float32, device=DEV)
        args = (pa(xs), pa(ts), cs, len(Cs), rows, iou.data_ptr(), off.data_ptr(), rp.data_ptr(), 0.5, 0.25, 2.0, 1e-8, 1.0, 0.9,
                norm.data_ptr(), block.data_ptr())
        rc = lib.timhip_det_side_loss_fwd_ordered(*args, scratch.data_ptr(), _stream()) if ordered else lib.timhip_det_side_loss_fwd(*args, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        return block.cpu().numpy(), norm.item()

    full = torch.full((L.DET_SIDE_PARTIALS + 16,), -123.0, dtype=torch.float32, device=DEV)
    scratch = full[8:8 + L.DET_SIDE_PARTIALS]
    first, norm1 = run(True, scratch)
    assert bool((full[:8] == -123.0).all()) and bool((full[8 + L.DET_SIDE_PARTIALS:] == -123.0).all())
    for _ in range(4):
        again, norm2 = run(True, scratch)
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32)) and norm1 == norm2
    atomic, norm3 = run(False)
    print("rows %d: ordered block %s, atomic block %s" % (rows, first[:5].tolist(), atomic[:5].tolist()))
    assert first[3] == atomic[3] == float((off[:, 0] != float("inf")).sum()) and norm1 == norm3 and first[4] == atomic[4]
    nblocks = sum(min(512, -(-rows * c // 256)) for c in Cs)
    assert abs(first[1] - atomic[1]) <= 2 * (nblocks - 1) * 2.0 ** -24 * atomic[1] + 0.0
    assert abs(first[2] - atomic[2]) <= 2 * (4 * min(256, -(-rows // 256)) - 1) * 2.0 ** -24 * atomic[2]
    assert np.isfinite(first[:5]).all() and (first[5:] == 0).all()
    assert lib.timhip_det_side_loss_fwd_ordered(pa(xs), pa(ts), cs, len(Cs), rows, iou.data_ptr(), off.data_ptr(), rp.data_ptr(), 0.5, 0.25, 2.0,
                                                1e-8, 1.0, 0.9, full.data_ptr(), full.data_ptr(), None, _stream()) == L.EINVAL
    # through autograd: the gradients do not depend on the form of the sum (they read the normaliser, which is exact)
    grads = []
    for ordered in (False, True):
        lx = [x.clone().requires_grad_(True) for x in xs]
        lr = rp.clone().requires_grad_(True)
        norm = torch.full((), 100.0, dtype=torch.float32, device=DEV)
        losses.detection_side_loss(lx, ts, lr, off, iou, norm, 0.5, lambda_reg=1.0, ordered=ordered).backward()
        torch.cuda.synchronize()
        grads.append([x.grad for x in lx] + [lr.grad])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
