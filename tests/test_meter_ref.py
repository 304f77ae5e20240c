"""The training meter without a GPU: tests/meter_ref.py - the restatement the GPU tests compare the kernels with,
bit for bit - is pinned to fixtures recorded from the reference's own TrainMeter and accuracy functions
(tests/golden/make_golden_meter.py); the C ABI is declared, bound and built; without a device the class refuses."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import meter_ref as MR
from tests import recog_ref as RR
from tim_amd import _lib, recog

ROOT = os.path.dirname(os.path.dirname(H.GOLDEN))
NARGS = {"timhip_meter_update": 15, "timhip_meter_work_words": 6, "timhip_rec_combined": 13}


def load(name):
    return np.load(os.path.join(H.GOLDEN, "meter_%s.npz" % name))


def replay(g, on_batch=None):
    """the fixture's stream through meter_ref.Meter and recog_ref.Collector -> (meter, collector)"""
    heads = [str(h) for h in g["heads"]]
    vn = bool(g["include_verb_noun"])
    m = MR.Meter(include_verb_noun=vn)
    col = RR.Collector(dict(zip(heads, (int(c) for c in g["classes"]))), int(g["num_actions"]), include_verb_noun=vn)
    for b in range(g["v_ids"].shape[0]):
        logits = {h: g["logits_" + h][b] for h in heads}
        m.update(logits, g["v_labels"][b], g["a_labels"][b], dict(zip(MR.SLOTS, g["losses"][b])))
        col.update(logits, g["v_ids"][b], g["a_ids"][b], g["v_labels"][b], g["a_labels"][b])
        if on_batch:
            on_batch(b, m)
    return m, col


def bits(x):
    return np.asarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("name", ["small", "ave"])
def test_restatement_reproduces_the_reference_slots_and_accuracies(name):
    g = load(name)
    heads = [str(h) for h in g["heads"]]
    for k in ("visual", "audio"):                                                             # a batch with nv == 0, one with na == 0
        assert (np.diff(g["slot_count"][:, MR.SLOTS.index(k)]) == 0).any(), k

    def check(b, m):
        assert np.array_equal(bits(m.sum), bits(g["slot_sum"][b])), b                      # bit for bit
        assert np.array_equal(m.count, g["slot_count"][b]), b
        assert np.array_equal(bits([m.avg(k) for k in MR.SLOTS]), bits(g["slot_avg"][b])), b
        for h in heads + (["mt_action"] if "verb" in heads else []):
            rows, c1, c5 = (int(v) for v in m.last[MR.HEADS.index(h)])
            floats = recog.multitask_floats if h == "mt_action" else recog.accuracy_floats
            assert floats(c1, c5, rows) == tuple(g["batch_acc_" + h][b]), (b, h)

    m, col = replay(g, check)
    assert m.updates == g["v_ids"].shape[0]
    acc = col.accuracies()
    for h in acc:
        assert acc[h] == tuple(g["acc_" + h]), h
    if name == "ave":
        assert int(m.count[MR.SLOTS.index("verb")]) == 0 and int(m.count[MR.SLOTS.index("noun")]) == 0
        pred = col.predictions()
        (pv, ids_v), (pa, ids_a) = pred["action"], pred["audio"]
        lab = col.groups["visual"]["labels"][ids_v, 2]
        assert RR.accuracy(MR.combined_ranks(pv, ids_v, pa, ids_a, lab)) == tuple(g["acc_combined"])
        with pytest.raises(ValueError):
            MR.combined_ranks(pv[:-1], ids_v[:-1], pa, ids_a, lab[:-1])


def test_state_words_round_trip_through_the_readers_decoder():
    """meter_ref lays the block out as include/timhip.h says; tim_amd.meters.decode_state reads the same numbers back"""
    from tim_amd import meters
    m, _ = replay(load("small"))
    s = meters.decode_state(m.words())
    assert s["updates"] == m.updates and s["nv"] == m.nv and s["na"] == m.na
    for i, k in enumerate(MR.SLOTS):
        assert s["losses"][k]["avg"] == m.avg(k) and s["losses"][k]["count"] == int(m.count[i])
        assert np.float32(s["losses"][k]["val"]) == m.val[i]
    for i, h in enumerate(MR.HEADS):
        a = s["acc"][h]
        assert (a["rows"], a["hits1"], a["hits5"]) == tuple(int(v) for v in m.run[i])
        assert (a["batch_rows"], a["batch_hits1"], a["batch_hits5"]) == tuple(int(v) for v in m.last[i])
    assert meters.decode_state(np.zeros(MR.STATE_WORDS, np.int32))["losses"]["total"]["avg"] == 0.0


def test_rank_rule_is_topk_counting_on_tie_free_rows():
    rng = np.random.default_rng(5)
    for C in (3, 5, 23, 97, 300):
        x = rng.permutation(4 * C * 8).reshape(8, 4 * C)[:, :C].astype(np.float32)          # distinct values: no ties
        y = rng.integers(0, C, size=8)
        r = MR.ranks(x, y)
        top = torch.from_numpy(x).topk(min(5, C), dim=1).indices.numpy()
        for k in (1, 5):
            assert np.array_equal(r < k, (top[:, :k] == y[:, None]).any(axis=1)), (C, k)
    # ties: the lower index ranks first; a label outside the row or a NaN label logit has no rank; NaN elsewhere never counts
    assert MR.row_rank([1.0, 1.0, 0.0], 0) == 0 and MR.row_rank([1.0, 1.0, 0.0], 1) == 1
    assert MR.row_rank([1.0, 2.0], 2) == MR.NO_RANK and MR.row_rank([1.0, 2.0], -5) == MR.NO_RANK
    assert MR.row_rank([np.nan, 2.0], 0) == MR.NO_RANK and MR.row_rank([np.nan, 2.0, 1.0], 2) == 1
    assert MR.row_rank([np.inf, -np.inf, 0.0], 2) == 1


def test_abi_is_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n, k in NARGS.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, code)
        assert m, n
        assert len(m.group(1).split(",")) == k == len(_lib._SIGS[n][1]), n
    assert set(NARGS) <= set(_lib.exported_symbols())
    assert not [n for n in NARGS if n.startswith("timhip_optim_")]
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NARGS) and lib.timhip_version() == _lib.ABI_VERSION == 6
    assert re.search(r"^SRCS\s*=.*\bmeter\.hip\b", open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read(), re.M)
    assert ctypes.sizeof(_lib.TimMeterHead) == 32
    # the layout enum of the header, its mirror in the binding and the restatement's agree; 64-bit fields sit on even words
    enum = {k: int(v) for k, v in re.findall(r"\bTIMHIP_METER_([A-Z0-9_]+)\s*=\s*(\d+)", code)}
    enum.update({k: int(v) for k, v in re.findall(r"#define\s+TIMHIP_METER_([A-Z0-9_]+)\s+(\d+)", code)})
    for k in ("UPDATES", "SUM", "COUNT", "RUN", "VAL", "LAST", "NV", "NA", "STATE_WORDS"):
        assert enum[k] == getattr(_lib, "METER_" + k) == getattr(MR, k), k
    for k in ("TOTAL", "DRLOC", "VISUAL", "VERB", "NOUN", "ACTION", "AUDIO"):
        assert enum[k] == getattr(_lib, "METER_" + k) == MR.SLOTS.index(k.lower()), k
    for k, h in (("VERB", "verb"), ("NOUN", "noun"), ("ACTION", "action"), ("MT", "mt_action"), ("AUDIO", "audio")):
        assert enum["HEAD_" + k] == getattr(_lib, "METER_HEAD_" + k) == MR.HEADS.index(h), k
    assert enum["SLOTS"] == _lib.METER_SLOTS == 7 and enum["HEADS"] == _lib.METER_HEADS == 5 and enum["MAX_HEADS"] == _lib.METER_MAX_HEADS == 3
    assert all(enum[k] % 2 == 0 for k in ("UPDATES", "SUM", "COUNT", "RUN", "VAL", "STATE_WORDS"))
    assert enum["COUNT"] + 4 * 6 + 2 == enum["RUN"] and enum["RUN"] + 6 * 5 == enum["VAL"] and enum["VAL"] + 7 == enum["LAST"]
    assert enum["LAST"] + 15 == enum["NV"] and enum["NA"] + 1 == enum["STATE_WORDS"] and 4 * enum["STATE_WORDS"] <= 512


def test_work_words_and_refusals_need_no_device():
    """the host half of the entries: the scratch size, and the argument checks that return before any launch"""
    lib = _lib.load()
    heads = (_lib.TimMeterHead * 3)()
    for i, C in enumerate((97, 300, 3806)):
        heads[i].C, heads[i].ld = C, C
    aud = (_lib.TimMeterHead * 1)()
    aud[0].C, aud[0].ld = 44, 44
    assert lib.timhip_meter_work_words(ctypes.addressof(heads), 3, 1600, ctypes.addressof(aud), 1, 640) == 1600 * 6 + 640
    assert lib.timhip_meter_work_words(ctypes.addressof(heads), 4, 1600, None, 0, 0) == 0
    losses = (ctypes.c_void_p * 7)()
    state = (ctypes.c_int64 * 42)()
    # nothing here reaches a launch: every call is refused on its arguments (the pointers are never dereferenced)
    up = lambda *a: lib.timhip_meter_update(*a)   # noqa: E731
    hv, ha, st, ls = ctypes.addressof(heads), ctypes.addressof(aud), ctypes.addressof(state), ctypes.addressof(losses)
    assert up(hv, 3, None, 3, 4, ha, 1, None, 1, 0, ls, 3, st, None, None) == _lib.EINVAL        # rows without labels
    assert up(hv, 4, st, 3, 4, ha, 1, st, 1, 4, ls, 3, st, st, None) == _lib.EINVAL              # four heads in a group
    assert up(hv, 3, st, 3, 4, ha, 1, st, 1, 4, ls, 3, None, st, None) == _lib.EINVAL            # no state
    assert up(hv, 3, st, 3, 4, ha, 1, st, 1, 4, None, 3, st, st, None) == _lib.EINVAL            # no losses
    assert up(hv, 3, st, 3, 4, ha, 1, st, 1, 4, ls, 3, st, st, None) == _lib.EINVAL              # rows without logits
    assert up(hv, 3, st, 3, 0, ha, 1, st, 1, 0, ls, 3, st, None, None) == 0                      # R == 0: nothing to do
    assert up(hv, 3, st, 3, 0, ha, 1, st, 1, 0, ls, 3, st + 4, None, None) == _lib.EALIGN
    assert not any(state)


def test_train_meter_resolves_and_refuses_without_a_device(monkeypatch):
    import tim_amd
    from tim_amd import meters
    assert tim_amd.TrainMeter is meters.TrainMeter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        tim_amd.TrainMeter([[5, 7, 23], 11], 40)
