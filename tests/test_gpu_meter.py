"""The training meter on the HIP kernels (tim_amd/meters.py -> tim_amd/csrc/meter.hip, and the combined accuracy of
tim_amd/csrc/recog.hip) against its numpy restatement tests/meter_ref.py and the fixtures recorded from the reference
(tests/golden/meter_small.npz, meter_ave.npz).  Every comparison of a state block is bit for bit: the block holds integers and
doubles that one thread updates in a fixed order, so there is nothing to allow for."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import meter_ref as MR  # noqa: E402
from tests import recog_ref as RR  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import RecognitionCollector, TrainMeter, meters  # noqa: E402

DEV = "cuda"
VISUAL = ("verb", "noun", "action")
GUARD, GUARD_WORD = 4, 0x5a5a5a5a          # words in front of and behind the block (the block stays 8-byte aligned)
SLOT_OF = {"verb": L.METER_HEAD_VERB, "noun": L.METER_HEAD_NOUN, "action": L.METER_HEAD_ACTION, "audio": L.METER_HEAD_AUDIO}


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pitched(x, extra=3):
    """[R, C] -> device [R, C + extra] with NaN in the guard columns (the kernels must not read them)"""
    buf = np.full((x.shape[0], x.shape[1] + extra), np.nan, np.float32)
    buf[:, :x.shape[1]] = x
    return dv(buf)


class Block:
    """a state block between guard words, as the raw entry sees it"""

    def __init__(self, fill=0):
        words = np.full(2 * GUARD + L.METER_STATE_WORDS, GUARD_WORD, np.int32)
        words[GUARD:-GUARD] = fill
        self.buf = dv(words.view(np.int64))                # int64 storage: 8-byte aligned
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def words(self):
        torch.cuda.synchronize()
        w = self.buf.cpu().numpy().view(np.int32)
        assert (w[:GUARD] == GUARD_WORD).all() and (w[-GUARD:] == GUARD_WORD).all(), "a guard word changed"
        return w[GUARD:-GUARD].copy()


def raw_update(block, logits, v_labels, a_labels, losses, flags=L.METER_VERB_NOUN | L.METER_BATCH_ACCURACY, heads=None):
    """timhip_meter_update through ctypes.  logits: {head: device [R, ld] tensor whose first C columns count} with `heads` =
    {head: C}; labels: device int64 [Rv, 3] / [Ra] or None; losses: {slot: device fp32 [1]} -> the return code"""
    groups = []
    for names in (VISUAL, ("audio",)):
        use = [h for h in names if h in heads]
        table = (L.TimMeterHead * max(len(use), 1))()
        for i, h in enumerate(use):
            x = logits[h]
            table[i].logits, table[i].ld, table[i].C = x.data_ptr() if x.numel() else None, x.stride(0), heads[h]
            table[i].label_col, table[i].slot = MR.LABEL_COL[h], SLOT_OF[h]
        groups.append((table, len(use)))
    (vt, nvh), (at, nah) = groups
    Rv = 0 if v_labels is None else v_labels.shape[0]
    Ra = 0 if a_labels is None else a_labels.shape[0]
    lp = (ctypes.c_void_p * L.METER_SLOTS)()
    for s, k in enumerate(MR.SLOTS):
        lp[s] = losses[k].data_ptr() if k in losses else None
    lib = L.load()
    words = lib.timhip_meter_work_words(ctypes.addressof(vt), nvh, Rv, ctypes.addressof(at), nah, Ra)
    work = torch.full((max(int(words), 1) + 2,), GUARD_WORD, dtype=torch.int32, device=DEV)
    rc = lib.timhip_meter_update(ctypes.addressof(vt), nvh, L.ptr(v_labels) if Rv else None, 3, Rv, ctypes.addressof(at), nah,
                                 L.ptr(a_labels) if Ra else None, 1, Ra, ctypes.addressof(lp), flags, block.ptr, work.data_ptr(),
                                 None)
    torch.cuda.synchronize()
    assert (work[int(words):].cpu().numpy() == GUARD_WORD).all(), "the scratch was written past its size"
    return rc


def make_batch(seed, heads, Rv, Ra, pad=0.2):
    """{head: [R, C] fp32}, v_labels [Rv, 3], a_labels [Ra], {slot: fp32}: half of the rows hold small whole numbers, so
    equal logits - with the label's among them - are common; a share of the rows is padded"""
    rng = np.random.default_rng(seed)
    v_labels = np.stack([rng.integers(0, heads.get(h, 3), size=Rv) for h in VISUAL], axis=1).astype(np.int64)
    v_labels[rng.uniform(size=Rv) < pad] = -1
    a_labels = rng.integers(0, heads.get("audio", 3), size=Ra).astype(np.int64)
    a_labels[rng.uniform(size=Ra) < pad] = -1
    logits = {}
    for h, C in heads.items():
        R = Ra if h == "audio" else Rv
        x = rng.normal(0, 2.0, size=(R, C)).astype(np.float32)
        whole = rng.uniform(size=R) < 0.5
        x[whole] = rng.integers(-2, 3, size=(int(whole.sum()), C)).astype(np.float32)
        logits[h] = x
    losses = {k: np.float32(v) for k, v in zip(MR.SLOTS, rng.uniform(0.05, 6.0, size=len(MR.SLOTS)).astype(np.float32))}
    return logits, v_labels, a_labels, losses


def device_losses(losses):
    return {k: dv(np.array([v], np.float32)) for k, v in losses.items()}


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1600])
@pytest.mark.parametrize("C", [3, 97, 257, 3806])
def test_raw_entry_between_guard_words(C, R):
    """three visual heads (the verb and the action head C wide) and a 44-wide audio head, logits at pitch C + 3 with NaN in the
    guard columns, two updates into a block between guard words: the block is the restatement's, everything else keeps its bits"""
    heads = {"verb": C, "noun": 5, "action": C, "audio": 44}
    Ra = (2 * R + 4) // 5
    ref, block = MR.Meter(), Block()
    for t in range(2):
        logits, vl, al, losses = make_batch(1000 * t + 7 * C + R, heads, R, Ra)
        del losses["drloc"]                                  # a missing loss counts as 0
        dev_logits = {h: pitched(x) for h, x in logits.items()}
        before = {h: x.clone() for h, x in dev_logits.items()}
        dvl, dal = dv(vl), dv(al)
        assert raw_update(block, dev_logits, dvl, dal, device_losses(losses), heads=heads) == 0
        ref.update(logits, vl, al, losses)
        assert np.array_equal(block.words(), ref.words()), t
        for h in heads:                                      # inputs untouched (compared as bits: the guards are NaN)
            assert torch.equal(dev_logits[h].view(torch.int32), before[h].view(torch.int32)), h
        assert np.array_equal(dvl.cpu().numpy(), vl) and np.array_equal(dal.cpu().numpy(), al)
    if C == 3:                                               # three classes: every valid row with a usable label is a top-5 hit
        s = meters.decode_state(block.words())
        assert s["acc"]["verb"]["hits5"] == s["acc"]["verb"]["rows"] > 0 or R == 1


def test_edge_rows():
    C = 6
    heads = {"verb": C, "noun": C, "action": C, "audio": C}
    x = np.array([[5, 1, 2, 3, 4, 0],                        # label 0 on top
                  [0, 1, 2, 3, 4, 5],                        # label C - 1 on top
                  [1, 7, 7, 0, 0, 0],                        # a tie, the label (1) at the lower index: rank 0
                  [1, 7, 7, 0, 0, 0],                        # the same tie, the label (2) at the higher index: rank 1
                  [3, 2, 1, 0, 0, 0],                        # verb label == C, noun label -5, on a row whose action label is valid
                  [np.nan, 2, 1, 0, 0, 0],                   # a NaN label logit: no rank
                  [1, np.nan, np.inf, -np.inf, 0, 2],        # NaN / inf elsewhere: only +inf and 2 rank above the label (0)
                  [9, 9, 9, 9, 9, 9]], np.float32)           # padded
    vl = np.array([[0, 0, 0], [5, 5, 5], [1, 1, 1], [2, 2, 2], [C, -5, 0], [0, 0, 0], [0, 0, 0], [-1, -1, -1]], np.int64)
    assert [MR.row_rank(x[i], vl[i, 2]) for i in range(7)] == [0, 0, 0, 1, 0, MR.NO_RANK, 2]
    al = np.array([0, -1, 1, 2, 0, 0, -1, -1], np.int64)
    logits = {h: x for h in heads}
    _, _, _, losses = make_batch(3, heads, 1, 1)
    ref, block = MR.Meter(), Block()
    assert raw_update(block, {h: pitched(x) for h in heads}, dv(vl), dv(al), device_losses(losses), heads=heads) == 0
    ref.update(logits, vl, al, losses)
    assert np.array_equal(block.words(), ref.words())
    s = meters.decode_state(block.words())
    assert s["nv"] == 7 and s["na"] == 5
    assert (s["acc"]["action"]["rows"], s["acc"]["action"]["hits1"], s["acc"]["action"]["hits5"]) == (7, 4, 6)
    assert (s["acc"]["verb"]["rows"], s["acc"]["verb"]["hits1"]) == (7, 3)          # the label == C row is counted, never a hit
    assert (s["acc"]["mt_action"]["rows"], s["acc"]["mt_action"]["hits1"]) == (7, 3)
    # ---- every visual row padded: the visual slots stay as they are, TOTAL's count grows by na only
    before = meters.decode_state(block.words())
    vl0 = np.full_like(vl, -1)
    _, _, _, losses2 = make_batch(4, heads, 1, 1)
    assert raw_update(block, {h: pitched(x) for h in heads}, dv(vl0), dv(al), device_losses(losses2), heads=heads) == 0
    ref.update(logits, vl0, al, losses2)
    assert np.array_equal(block.words(), ref.words())
    after = meters.decode_state(block.words())
    for k in ("visual", "verb", "noun", "action"):
        assert after["losses"][k] == before["losses"][k], k
    assert after["losses"]["total"]["count"] == before["losses"]["total"]["count"] + 5 and after["nv"] == 0
    assert after["acc"]["action"]["batch_rows"] == 0 and after["acc"]["action"]["rows"] == 7
    # ---- R == 0: nothing is launched, nothing changes
    kept = block.words()
    empty = {h: torch.empty((0, C + 3), dtype=torch.float32, device=DEV) for h in heads}
    assert raw_update(block, empty, None, None, device_losses(losses), heads=heads) == 0
    assert np.array_equal(block.words(), kept)


def test_sequence_of_updates_twice_the_same_bits():
    heads = {"verb": 97, "noun": 300, "action": 1100, "audio": 44}
    shapes = [(40, 16, 0.2), (40, 16, 1.0), (7, 16, 0.0), (130, 1, 0.5), (64, 64, 0.9)]      # (Rv, Ra, padded share)
    runs = []
    for _ in range(2):
        ref, block, seen = MR.Meter(), Block(), []
        for t, (Rv, Ra, pad) in enumerate(shapes):
            logits, vl, al, losses = make_batch(50 + t, heads, Rv, Ra, pad)
            assert raw_update(block, {h: pitched(x) for h, x in logits.items()}, dv(vl), dv(al), device_losses(losses), heads=heads) == 0
            ref.update(logits, vl, al, losses)
            seen.append(block.words())
            assert np.array_equal(seen[-1], ref.words()), t              # running and last-batch counters, val, sum, count
        runs.append(seen)
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    # statistics only (no batch accuracy): the counters stay zero, the slots are the same
    ref, block = MR.Meter(batch_accuracy=False), Block()
    logits, vl, al, losses = make_batch(50, heads, 40, 16)
    assert raw_update(block, {h: pitched(x) for h, x in logits.items()}, dv(vl), dv(al), device_losses(losses), flags=L.METER_VERB_NOUN,
                      heads=heads) == 0
    ref.update(logits, vl, al, losses)
    assert np.array_equal(block.words(), ref.words())


def test_refusals_leave_the_block_untouched():
    heads = {"verb": 5, "noun": 7, "action": 23, "audio": 11}
    logits, vl, al, losses = make_batch(1, heads, 9, 6)
    x = {h: pitched(v) for h, v in logits.items()}
    dvl, dal, dl = dv(vl), dv(al), device_losses(losses)
    nan_word = int(np.array([np.nan], np.float32).view(np.int32)[0])
    block = Block(fill=nan_word)
    kept = block.words()
    lib = L.load()
    vt = (L.TimMeterHead * 4)()
    for i, h in enumerate(VISUAL + ("verb",)):
        vt[i].logits, vt[i].ld, vt[i].C, vt[i].label_col, vt[i].slot = x[h].data_ptr(), x[h].stride(0), heads[h], MR.LABEL_COL[h], SLOT_OF[h]
    at = (L.TimMeterHead * 1)()
    at[0].logits, at[0].ld, at[0].C, at[0].label_col, at[0].slot = x["audio"].data_ptr(), x["audio"].stride(0), 11, 0, SLOT_OF["audio"]
    lp = (ctypes.c_void_p * L.METER_SLOTS)(*[dl[k].data_ptr() for k in MR.SLOTS])
    work = torch.zeros((64,), dtype=torch.int32, device=DEV)
    good = [ctypes.addressof(vt), 3, dvl.data_ptr(), 3, 9, ctypes.addressof(at), 1, dal.data_ptr(), 1, 6, ctypes.addressof(lp),
            L.METER_VERB_NOUN | L.METER_BATCH_ACCURACY, block.ptr, work.data_ptr(), None]

    def refused(**change):
        names = ["v_heads", "n_v", "v_labels", "ld_v", "Rv", "a_heads", "n_a", "a_labels", "ld_a", "Ra", "losses", "flags", "state",
                 "work", "stream"]
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        assert lib.timhip_meter_update(*args) == L.EINVAL, change
        assert np.array_equal(block.words(), kept), change

    refused(v_heads=None)
    refused(a_heads=None)
    refused(v_labels=None)
    refused(a_labels=None)
    refused(losses=None)
    refused(work=None)
    refused(n_v=4)                                           # more than three heads in a group
    refused(ld_v=2)
    refused(flags=8)
    for field, bad in (("C", 0), ("ld", 22), ("logits", None), ("label_col", 3), ("slot", L.METER_HEAD_MT)):
        old = getattr(vt[2], field)
        setattr(vt[2], field, bad)
        refused()
        setattr(vt[2], field, old)
    assert lib.timhip_meter_update(*[None if i == 12 else a for i, a in enumerate(good)]) == L.EINVAL       # no state block
    assert lib.timhip_meter_update(*good) == 0               # and the untouched arguments do run
    assert not np.array_equal(block.words(), kept)


def meter_batches(n, heads, Rv, Ra, seed):
    return [make_batch(seed + t, heads, Rv, Ra, pad=0.15 + 0.2 * t) for t in range(n)]


def batch_ids(seed, labels_valid, n_act):
    rng = np.random.default_rng(seed)
    return np.where(labels_valid, rng.integers(0, n_act, size=labels_valid.shape[0]), -1).astype(np.int64)


@pytest.mark.parametrize("ensemble", [False, True])
def test_update_replays_in_a_graph(ensemble):
    """update() captured once on one stream over static inputs; three replays with fresh contents equal three eager updates"""
    classes, n_act, Rv, Ra = {"verb": 5, "noun": 7, "action": 300, "audio": 11}, 30, 96, 64
    num_class = [[5, 7, 300], 11]
    batches = meter_batches(3, classes, Rv, Ra, 900)
    ids = [(batch_ids(70 + t, b[1][:, 2] != -1, n_act), batch_ids(80 + t, b[2] != -1, n_act)) for t, b in enumerate(batches)]
    eager, graphed = (TrainMeter(num_class, n_act, ensemble=ensemble) for _ in range(2))
    ref = MR.Meter()
    order = ("verb", "noun", "action", "audio")
    for (lg, vl, al, ls), (vid, aid) in zip(batches, ids):
        eager.update(tuple(dv(lg[h]) for h in order), dv(vid), dv(aid), dv(vl), dv(al), losses=device_losses(ls))
        ref.update(lg, vl, al, ls)
    lg, vl, al, ls = batches[0]
    static = [dv(lg[h]) for h in order] + [dv(ids[0][0]), dv(ids[0][1]), dv(vl), dv(al)]
    static_losses = device_losses(ls)
    run = lambda: graphed.update(tuple(static[:4]), static[4], static[5], static[6], static[7], losses=static_losses)   # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                # warm-up outside the capture (sizes the scratch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graphed.reset()
    for (lg, vl, al, ls), (vid, aid) in zip(batches, ids):
        for t, a in zip(static, [lg[h] for h in order] + [vid, aid, vl, al]):
            t.copy_(dv(a))
        for k, v in ls.items():
            static_losses[k].fill_(float(v))
        graph.replay()
    torch.cuda.synchronize()
    want = ref.words()
    assert np.array_equal(eager.state.cpu().numpy().view(np.int32), want)
    assert np.array_equal(graphed.state.cpu().numpy().view(np.int32), want)
    assert graphed.read() == eager.read()
    if ensemble:
        a, b = eager.collector, graphed.collector
        assert torch.equal(a.seen, b.seen)
        for name in a.groups:
            for s, t in zip(a.groups[name].sum, b.groups[name].sum):
                assert torch.equal(s.view(torch.int32), t.view(torch.int32))
            assert torch.equal(a.groups[name].labels, b.groups[name].labels)
        assert graphed.update_epoch() == eager.update_epoch()


def fixture_meter(g):
    heads = [str(h) for h in g["heads"]]
    cls = dict(zip(heads, (int(c) for c in g["classes"])))
    vn = bool(g["include_verb_noun"])
    num_class = [[cls["verb"], cls["noun"], cls["action"]] if vn else cls["action"], cls["audio"]]
    return TrainMeter(num_class, int(g["num_actions"]), include_verb_noun=vn, dataset=str(g["dataset"]))


def fixture_update(meter, g, b):
    heads = [str(h) for h in g["heads"]]
    feats = tuple(dv(g["logits_" + h][b]) if h in heads else None for h in ("verb", "noun", "action", "audio"))
    meter.update(feats, dv(g["v_ids"][b]), dv(g["a_ids"][b]), dv(g["v_labels"][b]), dv(g["a_labels"][b]),
                 losses=device_losses(dict(zip(MR.SLOTS, g["losses"][b]))))


@pytest.mark.parametrize("name", ["small", "ave"])
def test_train_meter_on_the_reference_fixtures(name):
    """read() averages, the batch accuracies, update_epoch() and the combined accuracy equal what the reference's TrainMeter and
    accuracy functions gave; a state_dict() round trip into a fresh meter continues the stream identically"""
    g = np.load(os.path.join(H.GOLDEN, "meter_%s.npz" % name))
    heads = [str(h) for h in g["heads"]]
    NB = g["v_ids"].shape[0]
    meter, resumed = fixture_meter(g), fixture_meter(g)
    for b in range(NB):
        if b == 3:
            resumed.load_state_dict(meter.state_dict())
        fixture_update(meter, g, b)
        if b >= 3:
            fixture_update(resumed, g, b)
        s = meter.read()
        assert s["updates"] == b + 1
        for i, k in enumerate(MR.SLOTS):
            assert s["losses"][k]["avg"] == float(g["slot_avg"][b, i]) and s["losses"][k]["count"] == int(g["slot_count"][b, i]), (b, k)
            assert s["losses"][k]["sum"] == float(g["slot_sum"][b, i]), (b, k)
        for h in heads + (["mt_action"] if "verb" in heads else []):
            assert (s["acc"][h]["batch_top1"], s["acc"][h]["batch_top5"]) == tuple(g["batch_acc_" + h][b]), (b, h)
    assert resumed.read() == meter.read()
    assert torch.equal(resumed.state, meter.state)
    stats = meter.stats(lr=0.1, training_iterations=NB)
    assert stats["Train/visual_loss"] == float(g["slot_avg"][-1, MR.SLOTS.index("visual")])
    assert stats["Train/audio_loss"] == float(g["slot_avg"][-1, MR.SLOTS.index("audio")])
    assert ("Train/verb/visual_loss" in stats) == ("verb" in heads) and "Train_batch/audio/Top1_acc" in stats
    acc = meter.update_epoch()
    assert sorted(acc) == sorted(h for h in ("verb", "noun", "action", "audio", "mt_action", "combined") if "acc_" + h in g.files)
    for h, got in acc.items():
        assert tuple(got) == tuple(float(v) for v in g["acc_" + h]), (h, got)
    assert resumed.update_epoch() == acc
    meter.reset()
    assert meter.read() == meters.decode_state(np.zeros(L.METER_STATE_WORDS, np.int32))
    assert meter.update_epoch()["action"] == (0.0, 0.0)


def test_accuracies_without_the_keyword_and_combined_refusals():
    """RecognitionCollector.accuracies() as before on the recognition fixture; combined=True needs matching counts and widths"""
    g = np.load(os.path.join(H.GOLDEN, "recog_small.npz"))
    cv, cn, ca, cu = (int(c) for c in g["classes"])
    col = RecognitionCollector([[cv, cn, ca], cu], int(g["num_actions"]))
    for b in range(g["v_ids"].shape[0]):
        col.update(tuple(dv(g["logits_" + h][b]) for h in ("verb", "noun", "action", "audio")), dv(g["v_ids"][b]), dv(g["a_ids"][b]),
                   dv(g["v_labels"][b]), dv(g["a_labels"][b]))
    acc = col.accuracies()
    assert acc == {h: tuple(float(x) for x in g["acc_" + h]) for h in ("verb", "noun", "action", "mt_action", "audio")}
    assert col.accuracies(combined=False) == acc
    with pytest.raises(ValueError, match="classes"):
        col.accuracies(combined=True)                        # 23 action classes, 11 audio classes
    same = RecognitionCollector([7, 7], 10, include_verb_noun=False)
    x = dv(np.random.default_rng(0).normal(size=(3, 7)).astype(np.float32))
    same.update((None, None, x, x), dv(np.array([0, 1, 2])), dv(np.array([5, 5, -1])), dv(np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3]])),
                dv(np.array([4, 4, -1])))
    with pytest.raises(ValueError, match="3 visual and 1 audio"):
        same.accuracies(combined=True)
    with pytest.raises(ValueError, match="both modalities"):
        RecognitionCollector([7, 7], 10, modality="audio").accuracies(combined=True)


def test_combined_ranks_on_a_strided_id_set():
    """the positional pairing on ids that leave gaps and straddle a 64-id ballot word, against the restatement"""
    C, n_act = 9, 200
    rng = np.random.default_rng(12)
    ids_v = np.sort(rng.choice(100, size=37, replace=False))
    ids_a = np.sort(100 + rng.choice(100, size=37, replace=False))
    col = RecognitionCollector([C, C], n_act, include_verb_noun=False)
    ref = RR.Collector({"action": C, "audio": C}, n_act, include_verb_noun=False)
    xv, xa = (rng.normal(0, 2, size=(37, C)).astype(np.float32) for _ in range(2))
    vl = np.repeat(rng.integers(0, C, size=(37, 1)), 3, axis=1).astype(np.int64)
    al = rng.integers(0, C, size=37).astype(np.int64)
    col.update((None, None, dv(xv), dv(xa)), dv(ids_v), dv(ids_a), dv(vl), dv(al))
    ref.update({"action": xv, "audio": xa}, ids_v, ids_a, vl, al)
    pred = ref.predictions()
    want = RR.accuracy(MR.combined_ranks(pred["action"][0], ids_v, pred["audio"][0], ids_a, vl[:, 2]))
    got = col.accuracies(combined=True)
    assert got["combined"] == want and got["action"] == ref.accuracies()["action"]


def test_the_examples_step_keeps_the_count_weighted_mean():
    """examples/train_metered_synthetic.py over 6 replays: the meter's TOTAL average is the count-weighted mean of the per-replay
    losses read back afterwards, accumulated in float64 from the same fp32 values in the same order - exactly"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_metered_synthetic as ex
    out = ex.main(["--steps", "6", "--print-freq", "3"])
    total, count = np.float64(0.0), 0
    for loss, n in out["per_replay"]:
        total = total + np.float64(np.float32(loss)) * np.float64(n)
        count += n
    s = out["read"]
    assert s["updates"] == 6 and count > 0
    assert s["losses"]["total"]["count"] == count and s["losses"]["total"]["avg"] == float(total / count)
    assert s["losses"]["total"]["val"] == out["per_replay"][-1][0]
    assert s["acc"]["action"]["rows"] == s["losses"]["visual"]["count"] and s["acc"]["audio"]["rows"] == s["losses"]["audio"]["count"]
    assert sorted(out["epoch"]) == ["action", "audio", "mt_action", "noun", "verb"]
