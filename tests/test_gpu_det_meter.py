"""The detection meter on the device: timhip_det_side_loss_fwd_stats held to timhip_det_side_loss_fwd_ordered bit
for bit and to the float64 restatement (tests/det_meter_ref.py) within the derived bound of `_side_check`
(tests/test_gpu_loss_kernels.py: per-element focal_bound terms plus the summation term); timhip_det_meter_update and
tim_amd.DetectionMeter bit for bit against the restatement's slot rules; the class on the fixtures recorded from the reference's
meters; a captured iteration against eager updates; the example."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import det_meter_ref as DR  # noqa: E402
from tests import losses_ref as R  # noqa: E402
from tests.helpers import GOLDEN  # noqa: E402
from tests.test_gpu_loss_kernels import _side_inputs  # noqa: E402
from tests.test_gpu_rowops import ia, pa, same_bits, st, sync  # noqa: E402
from tim_amd import _lib as L  # noqa: E402

DEV = "cuda:0"
U = R.EPS32
NAN = float("nan")
HY = dict(thr=0.6, alpha=0.25, gamma=2.0, eps=1e-8, lam=0.5, mom=0.9, norm0=250.0)
EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
G = 8                                                        # guard words on each side of the stats block


def raw(name):
    return getattr(L.load(), name)


class Side:
    """one side's inputs on the device and the buffers of one raw call: block at words 4 .. 11 and the normaliser at word 15 of a
    NaN-filled 16-float buffer, the stats block between G NaN guard words, the partials pre-filled with a pattern"""

    def __init__(self, xs, ts, iou, off, reg):
        self.cpu = (xs, ts, iou, off, reg)
        self.Cs = [x.shape[1] for x in xs]
        self.rows = iou.numel()
        self.xd, self.td = [x.to(DEV) for x in xs], [t.to(DEV) for t in ts]
        self.ud, self.od, self.rd = iou.to(DEV), off.to(DEV), reg.to(DEV)
        if self.rows == 0:      # (empty tensors have no storage: any non-NULL pointer will do, nothing is read)
            pad = torch.zeros(4, device=DEV)
            self.xd, self.td, self.ud, self.od, self.rd = [pad] * len(xs), [pad] * len(xs), pad, pad, pad
        self.fresh()

    def fresh(self):
        self.sc = torch.full((16,), NAN, device=DEV)
        self.sc[15] = HY["norm0"]
        self.stats = torch.full((L.DET_SIDE_STATS_WORDS + 2 * G,), NAN, device=DEV)
        self.partials = torch.full((L.DET_SIDE_STATS_PARTIALS + 2 * G,), -7.25, device=DEV)
        self.before = [t.clone() for t in (self.sc, self.stats, self.partials)]

    def args(self, K=None, rows=None, logits=None):
        K = len(self.Cs) if K is None else K
        return (pa(self.xd) if logits is None else logits, pa(self.td), ia(self.Cs), K, self.rows if rows is None else rows, L.ptr(self.ud),
                L.ptr(self.od), L.ptr(self.rd), HY["thr"], HY["alpha"], HY["gamma"], HY["eps"], HY["lam"], HY["mom"],
                self.sc.data_ptr() + 60, self.sc.data_ptr() + 16)

    def ordered(self):
        rc = raw("timhip_det_side_loss_fwd_ordered")(*self.args(), self.partials.data_ptr() + 4 * G, st())
        sync()
        return rc

    def with_stats(self, partials=True, stats=True, **kw):
        rc = raw("timhip_det_side_loss_fwd_stats")(*self.args(**kw), self.partials.data_ptr() + 4 * G if partials else None,
                                                   self.stats.data_ptr() + 4 * G if stats else None, st())
        sync()
        return rc

    def untouched(self):
        return all(same_bits(a, b) for a, b in zip((self.sc, self.stats, self.partials), self.before))

    def guards_intact(self):
        return (same_bits(self.stats[:G], self.before[1][:G]) and same_bits(self.stats[-G:], self.before[1][-G:])
                and same_bits(self.partials[:G], self.before[2][:G]) and same_bits(self.partials[-G:], self.before[2][-G:])
                and same_bits(self.sc[:4], self.before[0][:4]) and same_bits(self.sc[12:15], self.before[0][12:15]))

    def words(self):
        return self.stats[G:G + L.DET_SIDE_STATS_WORDS].cpu()


def f32div(a, b):
    return np.float32(a) / np.float32(b)


def check_stats(side, key):
    """every assertion the raw entry owes on one input"""
    xs, ts, iou, off, reg = side.cpu
    K, rows = len(xs), side.rows
    side.fresh()
    assert side.ordered() == 0
    want_sc = side.sc.clone()
    side.fresh()
    assert side.with_stats() == 0
    assert same_bits(side.sc, want_sc), "%s: block[0..7] and the normaliser are those of the ordered form" % key
    assert side.guards_intact()
    w = side.words()
    assert bool(torch.isfinite(w).all()), "%s: every word is written" % key
    first = side.stats.clone()
    side.sc[15] = HY["norm0"]
    assert side.with_stats() == 0 and same_bits(side.stats, first) and same_bits(side.sc, want_sc), "%s: the call repeated" % key
    blk = want_sc[4:12].cpu().numpy()
    g = w.numpy()
    nm = blk[4]
    # the words that restate the block, and the divisions: correctly rounded fp32 quotients of the words beside them
    assert g[DR.POSITIVES] == blk[3] and g[DR.DIOU_SUM].tobytes() == blk[2].tobytes() and g[DR.NORMALISER] == nm and g[DR.LOSS].tobytes() == blk[0].tobytes()
    assert g[DR.RESERVED] == 0 and all(g[DR.HEAD_SUM + k] == 0 and g[DR.HEAD + k] == 0 for k in range(K, 4))
    for k in range(4):
        assert g[DR.HEAD + k] == f32div(g[DR.HEAD_SUM + k], nm)
    assert g[DR.POS] == f32div(g[DR.POS_SUM], nm) and g[DR.NEG] == f32div(g[DR.NEG_SUM], nm)
    assert g[DR.CLS] == f32div(blk[1], np.float32(K) * nm)
    assert g[DR.REG] == (f32div(np.float32(HY["lam"]) * blk[2], nm) if blk[3] > 0 else 0)
    # counts exact, sums within the derived bound of the float64 restatement
    ref, bound, mag = DR.side_stats(xs, ts, iou, off, reg, HY["thr"], HY["alpha"], HY["gamma"], HY["eps"], HY["lam"], HY["mom"], HY["norm0"])
    assert g[DR.VALID] == ref[DR.VALID] == float((iou >= 0).sum()) and g[DR.POSITIVES] == ref[DR.POSITIVES]
    worst = 0.0
    for i in [DR.HEAD_SUM + k for k in range(K)] + [DR.POS_SUM, DR.NEG_SUM]:
        err = abs(float(g[i]) - ref[i])
        print("%s word %2d: kernel %.9g  float64 %.9g  |diff| / bound %.3g" % (key, i, g[i], ref[i], err / bound[i]))
        assert err <= bound[i], (key, i)
        worst = max(worst, err / bound[i])
    assert abs(float(blk[1]) - ref[DR.HEAD_SUM:DR.HEAD_SUM + 4].sum()) <= bound[DR.HEAD_SUM:DR.HEAD_SUM + 4].sum()
    assert abs(float(g[DR.DIOU_SUM]) - ref[DR.DIOU_SUM]) <= bound[DR.DIOU_SUM]
    last = DR.HEAD_SUM + K - 1
    n_last = xs[-1].numel()
    assert abs((float(g[DR.POS_SUM]) + float(g[DR.NEG_SUM])) - float(g[last])) <= DR.summation_term(n_last, mag[last]), \
        "%s: positive + negative within the summation term of the last head's sum" % key
    return g, worst


def make_side(rows, Cs, seed, npos=None, all_outside=False):
    xs, ts, iou, off, reg = _side_inputs(rows, Cs, seed=seed, npos=(max(rows // 8, 1) if npos is None else npos), all_outside=all_outside)
    return Side(xs, ts, iou, off, reg)


HEADS = [(3,), (5, 7, 23), (11,)]


@pytest.mark.parametrize("Cs", HEADS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 257])
def test_stats_small_shapes(rows, Cs):
    check_stats(make_side(rows, list(Cs), seed=rows + len(Cs)), "stats/%d/%s" % (rows, Cs))


def test_stats_stride_loop_wraps():
    """65 rows of (97, 300, 3806): 247 390 elements in the last head, more than 512 blocks of 256 - every thread takes two"""
    check_stats(make_side(65, [97, 300, 3806], seed=5), "stats/wide")


def test_stats_rows_launch_wraps():
    """70 000 rows: more than the rows launch's 256 blocks of 256"""
    g, _ = check_stats(make_side(70000, [3], seed=6, npos=5000), "stats/long")
    assert g[DR.POSITIVES] == 5000


def test_stats_no_positive_row():
    g, _ = check_stats(make_side(257, [5, 7, 23], seed=7, npos=0), "stats/nopos")
    assert g[DR.POSITIVES] == 0 and g[DR.POS_SUM] == 0 and g[DR.REG] == 0 and g[DR.NEG_SUM] == g[DR.HEAD_SUM + 2]


def test_stats_every_row_outside():
    g, _ = check_stats(make_side(130, [5, 7, 23], seed=8, npos=9, all_outside=True), "stats/outside")
    assert g[DR.VALID] == 0 and g[DR.POSITIVES] == 9 and not g[:DR.VALID].any() and g[DR.CLS] == 0 and g[DR.REG] > 0


def test_stats_positive_row_outside():
    """a positive row with iou < 0 counts as a positive (and in the DIoU sum), not as a valid row, and in neither part"""
    xs, ts, iou, off, reg = _side_inputs(100, [11], seed=9, npos=12)
    pos = torch.nonzero(off[:, 0] != float("inf")).flatten()
    iou[pos[:3]] = -1.0
    g, _ = check_stats(Side(xs, ts, iou, off, reg), "stats/pos-outside")
    assert g[DR.POSITIVES] == 12 and g[DR.VALID] == float((iou >= 0).sum())
    assert float(((iou >= 0) & (off[:, 0] != float("inf"))).sum()) == 9          # the rows behind POS_SUM: three fewer than the positives


def test_stats_zero_rows():
    """rows == 0: zeros, the normaliser advanced as the ordered form advances it"""
    s = Side([torch.zeros(0, 11)], [torch.zeros(0, 11)], torch.zeros(0), torch.zeros(0, 2), torch.zeros(0, 2))
    assert s.ordered() == 0
    want = s.sc.clone()
    s.fresh()
    assert s.with_stats() == 0 and same_bits(s.sc, want) and s.guards_intact()
    g = s.words().numpy()
    nm = np.float32(HY["mom"]) * np.float32(HY["norm0"]) + (np.float32(1) - np.float32(HY["mom"])) * np.float32(1)
    assert abs(float(g[DR.NORMALISER]) - float(nm)) <= 4 * U * float(nm) and g[DR.NORMALISER] == want[8].item() == want[15].item()
    assert not np.delete(g, DR.NORMALISER).any()


def test_stats_refusals_write_nothing():
    s = make_side(65, [5, 7, 23], seed=11)
    EINVAL, EUNSUPPORTED = L.EINVAL, L.EUNSUPPORTED
    holes = (C.c_void_p * 3)(s.xd[0].data_ptr(), None, s.xd[2].data_ptr())
    for rc, want in ((s.with_stats(stats=False), EINVAL), (s.with_stats(partials=False), EINVAL),
                     (s.with_stats(rows=(1 << 24) + 1), EUNSUPPORTED), (s.with_stats(K=5), EINVAL), (s.with_stats(K=0), EINVAL),
                     (s.with_stats(rows=-1), EINVAL), (s.with_stats(logits=holes), EINVAL)):
        assert rc == want and s.untouched()
    bad = raw("timhip_det_side_loss_fwd_stats")
    a = list(s.args())
    for i in (0, 1, 2, 5, 6, 7, 14, 15):           # logits, targets, C, iou, offsets, reg_pred, normaliser, block
        b = list(a)
        b[i] = None
        assert bad(*b, s.partials.data_ptr() + 4 * G, s.stats.data_ptr() + 4 * G, st()) == EINVAL
    sync()
    assert s.untouched()


def test_autograd_with_stats_is_the_ordered_form():
    """detection_side_loss(stats=...) against ordered=True without it: loss, every dlogits and dreg bit for bit"""
    from tim_amd import losses
    xs, ts, iou, off, reg = _side_inputs(257, [5, 7, 23], seed=21, npos=30)
    res = []
    for stats in (None, torch.full((L.DET_SIDE_STATS_WORDS,), NAN, device=DEV)):
        xd = [x.to(DEV).requires_grad_(True) for x in xs]
        rd = reg.to(DEV).requires_grad_(True)
        norm = torch.full((), 250.0, device=DEV)
        loss = losses.detection_side_loss(xd, [t.to(DEV) for t in ts], rd, off.to(DEV), iou.to(DEV), norm, 0.6, ordered=True, stats=stats)
        (loss * 0.7).backward()
        res.append([loss.detach().reshape(1), norm.reshape(1), rd.grad] + [x.grad for x in xd])
    assert all(same_bits(a, b) for a, b in zip(*res))
    assert bool(torch.isfinite(stats).all()) and stats[DR.LOSS].item() == res[1][0].item()
    with pytest.raises(ValueError):
        losses.detection_side_loss(xd, [t.to(DEV) for t in ts], rd, off.to(DEV), iou.to(DEV), norm, 0.6, stats=torch.zeros(5, device=DEV))


# ================================================================================================ timhip_det_meter_update
def fake_stats(rng, valid, positives, K):
    w = np.zeros(DR.STATS_WORDS, np.float32)
    w[:] = rng.uniform(0.01, 9.0, size=DR.STATS_WORDS).astype(np.float32)
    w[DR.VALID], w[DR.POSITIVES], w[DR.RESERVED] = valid, positives, 0
    w[DR.HEAD_SUM + K:DR.HEAD_SUM + 4] = 0
    w[DR.HEAD + K:DR.HEAD + 4] = 0
    return w


# (visual (valid, positives) or None, audio or None) per update: one with v_cls == 0, one without positives
SEQ = [((30, 4), (17, 2)), ((0, 0), (9, 1)), ((25, 0), (12, 0)), ((40, 40), (1, 1)), ((7, 3), (0, 2))]


@pytest.mark.parametrize("mode", ["visual_vn", "visual_single", "audio", "av"])
def test_meter_update_bit_for_bit(mode):
    """a five-update sequence, run twice into two blocks between guard words: both equal the restatement's block, word for word;
    the DRLoc scalar is NULL in every other update"""
    K = 3 if mode in ("visual_vn", "av") else 1
    fn = raw("timhip_det_meter_update")
    blocks = []
    for run in range(2):
        rng = np.random.default_rng(77)
        ref = DR.DetMeter()
        buf = torch.full((L.DET_METER_STATE_WORDS + 8,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        state = buf[4:4 + L.DET_METER_STATE_WORDS]
        state.zero_()
        assert state.data_ptr() % 8 == 0
        for i, (vc, ac) in enumerate(SEQ):
            v = fake_stats(rng, *vc, K) if mode != "audio" else None
            a = fake_stats(rng, *ac, 1) if mode in ("audio", "av") else None
            total, drloc = np.float32(rng.uniform(0.1, 5)), (np.float32(rng.uniform(0.1, 5)) if i % 2 == 0 else None)
            vd, ad = (None if x is None else torch.from_numpy(x).to(DEV) for x in (v, a))
            td, dd = torch.tensor([total], device=DEV), (None if drloc is None else torch.tensor([drloc], device=DEV))
            assert fn(state.data_ptr(), pa([vd, ad]), K, L.ptr(td), L.ptr(dd), st()) == 0
            sync()
            ref.update(v, a, K, total, drloc)
            assert np.array_equal(state.cpu().numpy(), ref.words()), (mode, run, i)
        assert bool((buf[:4] == 0x5a5a5a5a).all() and (buf[-4:] == 0x5a5a5a5a).all()), "guard words"
        blocks.append(state.cpu())
    assert torch.equal(blocks[0], blocks[1])
    assert ref.count[DR.SLOTS.index("negative")] != 0 and (mode == "audio" or ref.count[DR.SLOTS.index("visual")] == 30 + 25 + 40 + 7)


def test_meter_update_refusals():
    fn = raw("timhip_det_meter_update")
    state = torch.zeros(L.DET_METER_STATE_WORDS // 2 + 1, dtype=torch.int64, device=DEV)
    stats = torch.ones(L.DET_SIDE_STATS_WORDS, device=DEV)
    ok = pa([stats, None])
    assert fn(None, ok, 3, None, None, st()) == L.EINVAL and fn(state.data_ptr(), None, 3, None, None, st()) == L.EINVAL
    assert fn(state.data_ptr(), pa([None, None]), 3, None, None, st()) == L.EINVAL and fn(state.data_ptr(), ok, 2, None, None, st()) == L.EINVAL
    assert fn(state.data_ptr() + 4, ok, 3, None, None, st()) == L.EALIGN
    sync()
    assert not bool(state.any())


# ================================================================================================ the class on the fixtures
NAMES = ("visual_vn", "visual_single", "audio", "av")


def load(name):
    return np.load(os.path.join(GOLDEN, "det_meter_%s.npz" % name))


def run_batch(fx, b, meter, norm, loss_fn):
    """the fixture's batch b through the side losses (stats into the meter's tensors) and one meter update -> the stats blocks"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    for side in meter.sides:
        K = len(fx["heads_" + side])
        loss_fn([T(fx["b%d_%s_logits%d" % (b, side, k)]) for k in range(K)], [T(fx["b%d_%s_targets%d" % (b, side, k)]) for k in range(K)],
                T(fx["b%d_%s_reg" % (b, side)]), T(fx["b%d_%s_offsets" % (b, side)]), T(fx["b%d_%s_iou" % (b, side)]), norm,
                float(fx["iou_threshold"]), lambda_reg=float(fx["lambda_reg"]), momentum=float(fx["momentum"]), stats=meter.side_stats(side))
    meter.update(T(fx["total"][b:b + 1]), T(fx["drloc"][b:b + 1]) if meter.mode == "train" else None)
    return [meter.side_stats(s).cpu().numpy() if s in meter.sides else None for s in DR.SIDES]


TRAIN_KEYS = {"visual": ["Train/visual_loss", "Train/visual_action_loss", "Train/visual_positive_loss", "Train/visual_negative_loss",
                         "Train/visual_reg_loss"],
              "audio": ["Train/audio_loss", "Train/audio_positive_loss", "Train/audio_negative_loss", "Train/audio_reg_loss"]}
VAL_KEYS = {"visual": ["Val/visual/loss", "Val/visual/action_loss", "Val/visual/positive_loss", "Val/visual/negative_loss", "Val/visual/reg_loss"],
            "audio": ["Val/audio/loss", "Val/audio/positive_loss", "Val/audio/negative_loss", "Val/audio/reg_loss"]}
KEY_SLOT = {"visual_loss": "visual", "visual_action_loss": "action", "visual_positive_loss": "positive", "visual_negative_loss": "negative",
            "visual_reg_loss": "visual_reg", "audio_loss": "audio", "audio_positive_loss": "positive", "audio_negative_loss": "negative",
            "audio_reg_loss": "audio_reg", "verb/visual_loss": "verb", "noun/visual_loss": "noun", "drloc_loss": "drloc", "loss": "total"}


@pytest.mark.parametrize("name", NAMES)
def test_detection_meter_on_fixture(name):
    """tim_amd.DetectionMeter over a fixture's six batches, the side losses writing its stats tensors: the block equals the
    restatement fed with the device's own stats blocks bit for bit; stats() carries the reference's get_train_stats keys and its
    averages agree with the fixture's (the reference's meters; the restatement on the flagged `av` slots) within 2e-5 relative,
    the whole-tensor tolerance of the side loss; a state_dict round trip mid-stream; reset()"""
    from tim_amd import DetectionMeter, losses
    fx = load(name)
    vn, modality = bool(fx["include_verb_noun"]), str(fx["modality"])
    meter = DetectionMeter(modality, vn, include_dr_loc=True, device=DEV)
    twin = DetectionMeter(modality, vn, include_dr_loc=True, device=DEV)
    norm = torch.full((), float(fx["norm0"]), device=DEV)
    ref = DR.DetMeter()
    for b in range(fx["stats"].shape[0]):
        if b == 3:                                # the round trip: a second meter takes over from a checkpoint of the first
            twin.load_state_dict(meter.state_dict())
            meter, twin = twin, meter
        v, a = run_batch(fx, b, meter, norm, losses.detection_side_loss)
        ref.update(v, a, 3 if vn else 1, fx["total"][b], fx["drloc"][b])
        assert np.array_equal(meter.state.cpu().numpy().view(np.int32), ref.words()), (name, b)
        for s, side in enumerate(DR.SIDES):       # the device's statistics against the reference's float32 values
            if side in meter.sides:
                got, want = (v, a)[s].astype(np.float64), fx["stats"][b, s].astype(np.float64)
                assert np.array_equal(got[[DR.VALID, DR.POSITIVES]], want[[DR.VALID, DR.POSITIVES]])
                assert np.all(np.abs(got - want) <= 2e-5 * np.abs(want) + R.TINY32), (name, b, side, got, want)
    s = meter.stats(lr=0.01, training_iterations=6)
    want_keys = {"Train/lr", "Train/normaliser", "Train/positives", "Train/negatives", "Train/positive_ratio", "train_step", "Train/drloc_loss", "Train/loss"}
    for side in meter.sides:
        want_keys |= set(TRAIN_KEYS[side])
    if vn:
        want_keys |= {"Train/verb/visual_loss", "Train/noun/visual_loss"}
    assert set(s) == want_keys
    for key in want_keys - {"Train/lr", "Train/normaliser", "Train/positives", "Train/negatives", "Train/positive_ratio", "train_step"}:
        slot = DR.SLOTS.index(KEY_SLOT[key[len("Train/"):]])
        assert s[key] == ref.avg(DR.SLOTS[slot])
        assert abs(s[key] - fx["slot_avg"][-1, slot]) <= 2e-5 * abs(fx["slot_avg"][-1, slot]), key
    last = fx["stats"][-1]
    pos = int(sum(last[DR.SIDES.index(k), DR.POSITIVES] for k in meter.sides))
    neg = int(sum(last[DR.SIDES.index(k), DR.VALID] for k in meter.sides)) - pos
    assert (s["Train/positives"], s["Train/negatives"], s["Train/lr"], s["train_step"]) == (pos, neg, 0.01, 6)
    assert s["Train/positive_ratio"] == (pos / (pos + neg) if pos + neg else 0.0)
    assert abs(s["Train/normaliser"] - float(fx["final_normaliser"])) <= 2e-5 * float(fx["final_normaliser"]) and s["Train/normaliser"] == norm.item()
    r = meter.read()
    assert r["updates"] == 6 and r["losses"]["total"]["count"] == int(fx["slot_count"][-1, 0])
    meter.best_vis_loss = 1.5
    meter.reset()
    assert not bool(meter.state.any()) and meter.best_vis_loss == 1.5 and meter.read()["losses"]["total"]["avg"] == 0.0


@pytest.mark.parametrize("name", NAMES)
def test_detection_meter_val_mode_update_epoch(name):
    """mode="val": the InferenceMeter's keys; update_epoch over three epochs of two batches gives the reference's strings and
    best losses (2e-5 relative: they are averages of the device's values)"""
    from tim_amd import DetectionMeter, losses
    fx = load(name)
    meter = DetectionMeter(str(fx["modality"]), bool(fx["include_verb_noun"]), mode="val", device=DEV)
    norm = torch.full((), float(fx["norm0"]), device=DEV)
    for b in range(fx["stats"].shape[0]):
        run_batch(fx, b, meter, norm, losses.detection_side_loss)
        if b % 2 == 1:
            if b == 1:
                s = meter.stats(training_iterations=2)
                keys = {"val_step", "Val/loss"} | {k for side in meter.sides for k in VAL_KEYS[side]}
                assert set(s) == keys | ({"Val/visual/verb_loss", "Val/visual/noun_loss"} if bool(fx["include_verb_noun"]) else set())
            before, is_best = meter.update_epoch(b // 2)
            assert is_best == str(fx["is_best"][b // 2])
            for got, want in zip((before["visual"], before["audio"]), fx["best_before"][b // 2]):
                assert got == want if math.isinf(want) or want == 0 else abs(got - want) <= 2e-5 * abs(want)
            assert meter.read()["losses"]["drloc"]["sum"] == 0.0
            meter.reset()
    assert meter.last_best_epoch is not None
    sd = meter.state_dict()
    other = DetectionMeter(str(fx["modality"]), bool(fx["include_verb_noun"]), mode="val", device=DEV)
    other.load_state_dict(sd)
    assert (other.best_vis_loss, other.best_aud_loss, other.last_best_epoch) == (meter.best_vis_loss, meter.best_aud_loss, meter.last_best_epoch)


# ================================================================================================ capture
def test_captured_iteration_equals_eager_updates():
    """both side losses and the meter update in one torch.cuda.graph: three replays over changing inputs leave the bits three
    eager updates leave - state block, stats tensors, normaliser and loss"""
    from tim_amd import DetectionMeter, losses
    heads = {"visual": [5, 7, 23], "audio": [11]}
    rows = 65
    batches = [{s: _side_inputs(rows, heads[s], seed=100 + 10 * i + j, npos=(0 if i == 1 else 9)) for j, s in enumerate(DR.SIDES)} for i in range(3)]

    def to_dev(inp):
        xs, ts, iou, off, reg = inp
        return [x.to(DEV) for x in xs], [t.to(DEV) for t in ts], iou.to(DEV), off.to(DEV), reg.to(DEV)

    def iteration(meter, norm, static, drloc):
        loss = None
        for s in DR.SIDES:
            xs, ts, iou, off, reg = static[s]
            side = losses.detection_side_loss(xs, ts, reg, off, iou, norm, 0.6, stats=meter.side_stats(s))
            loss = side if loss is None else loss + 0.7 * side
        meter.update(loss, drloc)
        return loss

    def fill(static, batch):
        for s in DR.SIDES:
            for dst, src in zip(static[s][:2], batch[s][:2]):
                for d, x in zip(dst, src):
                    d.copy_(x)
            for d, x in zip(static[s][2:], batch[s][2:]):
                d.copy_(x)

    results = []
    for graphed in (False, True):
        meter = DetectionMeter("audio_visual", True, device=DEV)
        norm = torch.full((), 250.0, device=DEV)
        drloc = torch.tensor([0.375], device=DEV)
        static = {s: to_dev(batches[0][s]) for s in DR.SIDES}
        out = torch.zeros(1, device=DEV)
        if graphed:
            side_stream = torch.cuda.Stream()
            side_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side_stream), torch.no_grad():
                iteration(meter, norm, static, drloc)
            torch.cuda.current_stream().wait_stream(side_stream)
            sync()
            meter.reset()
            norm.fill_(250.0)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), torch.no_grad():
                out.copy_(iteration(meter, norm, static, drloc).reshape(1))
        seen = []
        for batch in batches:
            fill(static, batch)
            if graphed:
                g.replay()
            else:
                with torch.no_grad():
                    out.copy_(iteration(meter, norm, static, drloc).reshape(1))
            sync()
            seen.append([meter.state.cpu().view(torch.int32), meter.side_stats("visual").cpu(), meter.side_stats("audio").cpu(), norm.cpu().reshape(1), out.cpu()])
        results.append(seen)
    for eager, replayed in zip(*results):
        assert all(same_bits(a, b) for a, b in zip(eager, replayed))
    assert results[0][0][0].any() and not torch.equal(results[0][0][0], results[0][2][0])


# ================================================================================================ the example
def test_metered_detection_example():
    """examples/train_detection_metered_synthetic.py at its tiny shape: four replays, stats() every second; its source has no
    per-replay scalar read"""
    src = open(os.path.join(EXAMPLES, "train_detection_metered_synthetic.py")).read()
    assert ".item()" not in src and ".cpu()" not in src and "float(loss" not in src
    sys.path.insert(0, EXAMPLES)
    import train_detection_metered_synthetic as ex
    hist, final = ex.main(["--steps", "4", "--batch", "4", "--print-freq", "2", "--precision", "fp32"])
    assert len(hist) == 2 and final["updates"] == 4
    for s in hist:
        assert all(math.isfinite(v) for v in s.values())
        assert s["Train/loss"] > 0 and s["Train/visual_loss"] > 0 and s["Train/audio_loss"] > 0 and 0 <= s["Train/positive_ratio"] <= 1
    assert final["losses"]["total"]["count"] == final["sides"]["visual"]["valid"] + final["sides"]["audio"]["valid"] > 0
    assert hist[0]["Train/loss"] != hist[1]["Train/loss"]
