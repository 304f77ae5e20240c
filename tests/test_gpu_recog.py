"""The recognition inference tail on the HIP kernels (tim_amd/recog.py -> tim_amd/csrc/recog.hip) against its numpy
restatement tests/recog_ref.py and the fixture recorded from the reference (tests/golden/recog_small.npz).

Accumulators, seen counts, labels, touched bytes, ranks, counts and accuracy floats: exact (the accumulators bit for bit, in
every batch split).  Probabilities: within 1 ulp of the restatement - the device's double exp is within an ulp of fp64 of
glibc's, about 1e-13 relative on the quotient, so only a value on an fp32 rounding boundary can move, and then by one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import recog_ref as RR  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import RecognitionCollector  # noqa: E402

DEV = "cuda"
HEADS = ("verb", "noun", "action", "audio")


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def ulp_apart(a, b):
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def make_stream(seed, R, C, n_act, n_distinct, invalid=0.15, integer=False):
    """R audio rows over `n_distinct` of `n_act` action ids in shuffled order, a share of them padded (-1 id, -1 label)"""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(n_act)[:n_distinct]
    ids = pool[rng.integers(0, n_distinct, size=R)].astype(np.int64)
    class_of = rng.integers(0, C, size=n_act)
    labels = class_of[ids].astype(np.int64)
    pad = rng.uniform(size=R) < invalid
    ids[pad], labels[pad] = -1, -1
    if integer:                                              # small whole numbers: equal mean logits do occur
        x = rng.integers(-2, 3, size=(R, C)).astype(np.float32)
    else:
        x = (rng.normal(0, 3.0, size=(R, C)) * np.exp(rng.normal(0, 1.5, size=(R, 1)))).astype(np.float32)
    return x, ids, labels


def audio_pair(C, n_act):
    return RecognitionCollector([[3, 3, 3], C], n_act, modality="audio"), RR.Collector({"audio": C}, n_act, modality="audio")


def same_state(col, ref):
    torch.cuda.synchronize()
    assert np.array_equal(col.seen.cpu().numpy(), ref.seen)
    for name, g in col.groups.items():
        rg = ref.groups[name]
        for i, h in enumerate(g.heads):
            got, C = g.sum[i].cpu().numpy(), g.classes[i]
            assert np.array_equal(bits(got[:, :C]), bits(rg["acc"][i])), h
            assert not got[:, C:].any()                      # the padding of the pitch is never written
        assert np.array_equal(g.labels.cpu().numpy(), rg["labels"])
        assert np.array_equal(g.touched.cpu().numpy(), rg["touched"])


def same_results(col, ref, exact_prob=False):
    acc, racc = col.accuracies(), ref.accuracies()
    assert acc == racc
    ranks, rranks = col.ranks(), ref.ranks()
    preds, rpreds = col.predictions(), ref.predictions()
    for h in rranks:
        assert np.array_equal(ranks[h][1].cpu().numpy(), rranks[h][1])
        assert np.array_equal(ranks[h][0].cpu().numpy().astype(np.int64), rranks[h][0]), h
        prob, ids = preds[h]
        assert np.array_equal(ids.cpu().numpy(), rpreds[h][1]) and prob.dtype == torch.float32
        d = ulp_apart(prob.cpu().numpy(), rpreds[h][0])
        print("%s: %d probabilities, %d differ from the restatement, at most %d ulp" % (h, d.size, int((d != 0).sum()), d.max(initial=0)))
        assert d.max(initial=0) <= 1
    return acc


# C, rows of the two batches, action ids, distinct ids in the stream (7: heavy duplication; most of n_act: light)
CASES = [(1, (40, 9), 30, 7), (44, (300, 120), 500, 7), (63, (200, 64), 90, 80), (64, (257, 100), 4000, 300),
         (65, (64 * 25, 31), 700, 650), (97, (64 * 25, 960), 2000, 7), (97, (960, 960), 3000, 2500),
         (300, (960, 333), 1200, 400), (3806, (64 * 25, 200), 900, 7), (3806, (960, 64), 1500, 1400)]


@pytest.mark.parametrize("C,rows,n_act,n_distinct", CASES)
def test_accumulators_match_the_restatement(C, rows, n_act, n_distinct):
    col, ref = audio_pair(C, n_act)
    for b, R in enumerate(rows):
        x, ids, labels = make_stream(1000 + 7 * C + b, R, C, n_act, n_distinct)
        col.update((None, None, None, dv(x)), a_action_ids=dv(ids), a_labels=dv(labels))
        ref.update({"audio": x}, a_ids=ids, a_labels=labels)
        same_state(col, ref)
    assert ref.seen.max() >= 2 and not ref.err


@pytest.mark.parametrize("C", [5, 97, 3806])
def test_probabilities_ranks_and_counts(C):
    """integer logits make equal means common, so the tie rule of the rank is exercised; the second stream is continuous"""
    for integer in (True, False):
        col, ref = audio_pair(C, 300)
        for b in range(3):
            x, ids, labels = make_stream(50 + C + b, 400, C, 300, 180, integer=integer)
            col.update((None, None, None, dv(x)), a_action_ids=dv(ids), a_labels=dv(labels))
            ref.update({"audio": x}, a_ids=ids, a_labels=labels)
        same_state(col, ref)
        acc = same_results(col, ref)
        if integer and C > 5:
            mean = RR.mean_logits(ref.groups["audio"]["acc"][0], ref.seen)
            ties = sum(int((m == m[l]).sum()) > 1 for m, l in zip(mean, ref.groups["audio"]["labels"][:, 0]) if l >= 0)
            assert ties > 0                                  # the case is not vacuous
        assert 0.0 <= acc["audio"][0] <= acc["audio"][1] <= 100.0


def test_edges_all_invalid_single_row_strided_view():
    C, n_act = 97, 50
    col, ref = audio_pair(C, n_act)
    x, ids, labels = make_stream(3, 60, C, n_act, 20)
    none = np.full(60, -1, np.int64)
    col.update((None, None, None, dv(x)), a_action_ids=dv(none), a_labels=dv(none))          # nothing is valid
    ref.update({"audio": x}, a_ids=none, a_labels=none)
    same_state(col, ref)
    assert not ref.seen.any()
    col.update((None, None, None, dv(x[:1])), a_action_ids=dv(np.array([9])), a_labels=dv(np.array([4])))   # a single row
    ref.update({"audio": x[:1]}, a_ids=np.array([9]), a_labels=np.array([4]))
    same_state(col, ref)
    wide = torch.full((60, C + 40), 1e30, device=DEV)        # anything read outside the slice would wreck the sums
    wide[:, 13:13 + C] = dv(x)
    view = wide[:, 13:13 + C]
    assert view.stride(0) == C + 40 and not view.is_contiguous()
    col.update((None, None, None, view), a_action_ids=dv(ids), a_labels=dv(labels))
    ref.update({"audio": x}, a_ids=ids, a_labels=labels)
    same_state(col, ref)
    same_results(col, ref)


def visual_stream(seed, R, classes, n_act, n_distinct):
    rng = np.random.default_rng(seed)
    pool = rng.permutation(n_act)[:n_distinct]
    ids = pool[rng.integers(0, n_distinct, size=R)].astype(np.int64)
    labels = np.stack([rng.integers(0, c, size=R) for c in classes], axis=1).astype(np.int64)   # differ row by row: the last wins
    pad = rng.uniform(size=R) < 0.2
    ids[pad], labels[pad] = -1, -1
    logits = {h: rng.normal(0, 4.0, size=(R, c)).astype(np.float32) for h, c in zip(HEADS, classes)}
    return logits, ids, labels


def test_batch_splits_leave_bit_identical_state():
    """one stream of the three visual heads fed as one batch, as three batches and row by row"""
    classes, n_act, R = (44, 97, 300), 60, 240
    logits, ids, labels = visual_stream(77, R, classes, n_act, 25)
    dl = {h: dv(x) for h, x in logits.items()}
    dids, dlab = dv(ids), dv(labels)
    states = []
    for cuts in ([0, R], [0, 100, 101, R], list(range(R + 1))):
        col = RecognitionCollector([list(classes), 4], n_act, modality="visual")
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            col.update((dl["verb"][lo:hi], dl["noun"][lo:hi], dl["action"][lo:hi], None), dids[lo:hi], None, dlab[lo:hi])
        torch.cuda.synchronize()
        g = col.groups["visual"]
        states.append([s.clone() for s in g.sum] + [col.seen.clone(), g.labels.clone(), g.touched.clone()])
    for other in states[1:]:
        for x, y in zip(states[0], other):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
    ref = RR.Collector(dict(zip(HEADS, classes)), n_act, modality="visual")
    ref.update(logits, v_ids=ids, v_labels=labels)
    same_state(col, ref)
    acc = same_results(col, ref)
    assert sorted(acc) == ["action", "mt_action", "noun", "verb"]


def test_collector_on_the_reference_fixture():
    """sums bit-equal to the reference's meters, every accuracy float equal to the reference's"""
    g = np.load(os.path.join(H.GOLDEN, "recog_small.npz"))
    cv, cn, ca, cu = (int(c) for c in g["classes"])
    col = RecognitionCollector([[cv, cn, ca], cu], int(g["num_actions"]))
    for b in range(g["v_ids"].shape[0]):
        col.update(tuple(dv(g["logits_" + h][b]) for h in HEADS), dv(g["v_ids"][b]), dv(g["a_ids"][b]), dv(g["v_labels"][b]),
                   dv(g["a_labels"][b]))
    torch.cuda.synchronize()
    for name, grp in col.groups.items():
        for i, h in enumerate(grp.heads):
            assert np.array_equal(bits(grp.sum[i].cpu().numpy()[:, :grp.classes[i]]), bits(g["sum_" + h])), h
    assert np.array_equal(col.seen.cpu().numpy(), g["seen"])
    assert np.array_equal(col.groups["visual"].labels.cpu().numpy(), g["state_v_labels"])
    assert np.array_equal(col.groups["audio"].labels.cpu().numpy()[:, 0], g["state_a_labels"])
    acc = col.accuracies()
    assert sorted(acc) == ["action", "audio", "mt_action", "noun", "verb"]
    for h, got in acc.items():
        assert tuple(got) == tuple(float(x) for x in g["acc_" + h]), (h, got)
    preds = col.predictions()
    for h in HEADS:                                          # the reference's torch softmax: see tests/test_recog_ref.py
        assert ulp_apart(preds[h][0].cpu().numpy(), g["prob_" + h]).max() <= 12 + 1
    col.reset()
    torch.cuda.synchronize()
    assert not col.seen.any() and not col.groups["visual"].sum[2].any() and bool((col.groups["audio"].labels == -1).all())
    assert col.accuracies()["action"] == (0.0, 0.0)


def test_valid_masks_replace_the_label_test():
    C, n_act = 44, 40
    x, ids, labels = make_stream(5, 120, C, n_act, 30)
    col, ref = audio_pair(C, n_act)
    valid = ids >= 0
    junk = np.where(valid, ids, 3)                           # ids of masked rows are not looked at
    col.update((None, None, None, dv(x)), a_action_ids=dv(junk), a_valid=dv(valid))
    ref.update({"audio": x}, a_ids=junk, a_valid=valid)
    same_state(col, ref)
    assert bool((col.groups["audio"].labels == -1).all())
    prob, pid = col.predictions()["audio"]
    rprob, rid = ref.predictions()["audio"]
    assert np.array_equal(pid.cpu().numpy(), rid) and ulp_apart(prob.cpu().numpy(), rprob).max() <= 1


def test_update_replays_in_a_graph():
    """update captured once on static inputs, replayed over three batches written into them: equal to the eager result"""
    classes, cu, n_act, Rv, Ra = (5, 7, 23), 11, 50, 96, 64
    batches = []
    for b in range(3):
        lg, vid, vlab = visual_stream(200 + b, Rv, classes, n_act, 20)
        ax, aid, alab = make_stream(300 + b, Ra, cu, n_act, 15)
        batches.append((lg, vid, vlab, ax, aid, alab))
    mk = lambda: RecognitionCollector([list(classes), cu], n_act)
    eager, graphed, ref = mk(), mk(), RR.Collector(dict(zip(HEADS, classes + (cu,))), n_act)
    for lg, vid, vlab, ax, aid, alab in batches:
        eager.update((dv(lg["verb"]), dv(lg["noun"]), dv(lg["action"]), dv(ax)), dv(vid), dv(aid), dv(vlab), dv(alab))
        ref.update(dict(lg, audio=ax), vid, aid, vlab, alab)
    lg, vid, vlab, ax, aid, alab = batches[0]
    static = [dv(lg["verb"]), dv(lg["noun"]), dv(lg["action"]), dv(ax), dv(vid), dv(aid), dv(vlab), dv(alab)]
    run = lambda: graphed.update(tuple(static[:4]), static[4], static[5], static[6], static[7])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                # warm-up outside the capture (sizes the scratch)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphed.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graphed.reset()                                          # (a capture does not run the kernels; reset all the same)
    for lg, vid, vlab, ax, aid, alab in batches:
        for t, a in zip(static, (lg["verb"], lg["noun"], lg["action"], ax, vid, aid, vlab, alab)):
            t.copy_(dv(a))
        graph.replay()
    torch.cuda.synchronize()
    same_state(eager, ref)
    same_state(graphed, ref)
    assert graphed.accuracies() == eager.accuracies() == ref.accuracies()


def test_out_of_range_id_raises_and_spares_the_other_rows():
    C, n_act = 23, 30
    x, ids, labels = make_stream(9, 80, C, n_act, 12, invalid=0.1)
    bad = np.nonzero(ids >= 0)[0][[3, 17]]
    ids[bad[0]], ids[bad[1]] = n_act, -5                     # valid rows (label set), ids outside [0, n_act)
    col, ref = audio_pair(C, n_act)
    col.update((None, None, None, dv(x)), a_action_ids=dv(ids), a_labels=dv(labels))
    ref.update({"audio": x}, a_ids=ids, a_labels=labels)
    assert ref.err
    same_state(col, ref)
    with pytest.raises(L.TimHipError):
        col.accuracies()
    with pytest.raises(L.TimHipError):
        col.predictions()
    col.reset()
    col.update((None, None, None, dv(x[:10])), a_action_ids=dv(np.arange(10)), a_labels=dv(np.zeros(10, np.int64)))
    assert col.accuracies()["audio"][1] >= 0.0


def test_cpu_tensors_and_wrong_class_counts_raise():
    col = RecognitionCollector([[5, 7, 23], 11], 10)
    lg = (torch.zeros(4, 5, device=DEV), torch.zeros(4, 7, device=DEV), torch.zeros(4, 23, device=DEV), torch.zeros(4, 11, device=DEV))
    ids, lab3, lab1 = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, 3, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    with pytest.raises(L.TimHipError, match="no CPU fallback"):
        col.update((lg[0].cpu(),) + lg[1:], ids, ids, lab3, lab1)
    with pytest.raises(L.TimHipError, match="no CPU fallback"):
        col.update(lg, ids.cpu(), ids, lab3, lab1)
    with pytest.raises(L.TimHipError, match="no CPU fallback"):
        col.update(lg, ids, ids, lab3, lab1.cpu())
    with pytest.raises(ValueError):
        col.update(lg[:3] + (torch.zeros(4, 12, device=DEV),), ids, ids, lab3, lab1)
    with pytest.raises(ValueError):
        col.update(lg, ids[:3], ids, lab3, lab1)
    torch.cuda.synchronize()
    assert not col.seen.any()                                # a refused visual group left nothing behind
    lib = L.load()
    assert lib.timhip_rec_accumulate(None, 1, None, None, None, 0, 0, 0, 4, 10, None, None, None, None, None, None) == -1
    assert lib.timhip_rec_finalize(None, 64, 65, None, None, 0, 0, None, 10, None, None, None) == -1


def test_recognition_model_to_accuracies():
    """the tiny recognition TIM in eval() over overlapping batches -> collector: equal to the restatement fed the same logits"""
    from tim_amd.tim import TIM
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    nv, na, B, n_act = 4, 2, 3, 12
    sd, _ = H.synth_torch(cfg, B, nv, na, seed=1, dtype=torch.float32)
    m = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
            nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision="fp32")
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    classes = {h: c for h, c in zip(HEADS, list(cfg.num_class[0]) + [cfg.num_class[1]])}
    col, ref = RecognitionCollector(cfg.num_class, n_act), RR.Collector(classes, n_act)
    rng = np.random.default_rng(4)
    for step in range(4):
        _, inp = H.synth_torch(cfg, B, nv, na, seed=20 + step, dtype=torch.float32)
        with torch.no_grad():
            cls, _ = m([inp["visual"].to(DEV), inp["audio"].to(DEV)], "encoder", m(inp["times"].to(DEV), "time_mlp"), nv, na)
        assert cls[0].shape == (B * nv, classes["verb"]) and cls[3].shape == (B * na, classes["audio"])
        vid = rng.integers(0, 8, size=(B, nv)).astype(np.int64)                 # overlapping windows: ids repeat
        aid = rng.integers(8, n_act, size=(B, na)).astype(np.int64)
        vlab = np.stack([vid % classes["verb"], vid % classes["noun"], vid % classes["action"]], axis=-1)
        alab = aid % classes["audio"]
        vid[:, -1], vlab[:, -1], aid[step % B, -1], alab[step % B, -1] = -1, -1, -1, -1   # padded query slots
        col.update(cls, dv(vid), dv(aid), {"verb": dv(vlab[..., 0]), "noun": dv(vlab[..., 1]), "action": dv(vlab[..., 2])},
                   {"class_id": dv(alab)})
        ref.update({h: c.cpu().numpy() for h, c in zip(HEADS, cls)}, vid.reshape(-1), aid.reshape(-1), vlab.reshape(-1, 3), alab.reshape(-1))
    same_state(col, ref)
    acc = same_results(col, ref)
    assert sorted(acc) == ["action", "audio", "mt_action", "noun", "verb"] and ref.seen.max() >= 2
