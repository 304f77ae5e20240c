"""Attention maps from a window cache (`model.query_attention_maps`) on a real MI355X: against `attention_maps(...,
rows="queries")` on the same inputs, against the reference's recorded weights, under regrouping, layer selection, capture, and
for what they add to the memory of a `query_windows` call.

The maps of the two routes come from one kernel body (tests/test_gpu_query_weights.py holds the raw entries to each other bit for
bit), so they are compared bit for bit here too: every layer of every tiny config in fp16 and bf16, C2a at 8 windows in fp16,
layer 0 in fp32, and a group asked alone against the same group inside a larger call in all three modes.  One comparison needed
the caveat `timhip_stack_query` states for its outputs: in fp32, layers >= 1 against the FULL forward.  There a layer's input rows
come out of the previous layer's GEMMs, which pick other tiles at G Q rows than at B S rows (another accumulation order in the
fp32-arithmetic kernels); the maps then differ by 1.5e-8 .. 4.5e-8 (measured, every tiny config) - held to MODEL_BOUND of
tests/test_gpu_attn_maps.py, restated below (`EXACT`).  Every comparison prints its figure before it asserts."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_maps_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import query_maps_ref as QM  # noqa: E402
from tests.test_gpu_parity import DEV, build  # noqa: E402
from tests.test_gpu_query import TINY, _cfg, _encode, _inputs, _segments  # noqa: E402
from tim_amd.config import named_config  # noqa: E402

# the project's bounds on the tiny configs' logits against the fp32 reference, per mode (tests/test_gpu_attn_maps.py) - the weights
# are <= 1 and sit no deeper than the logits
MODEL_BOUND = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 3e-2}
PRECS = ["fp32", "bf16", "fp16"]
W = 3


def bits(t):
    return t.contiguous().view(torch.uint8)


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and torch.equal(bits(x), bits(y))


def _flat(out):
    """the outputs of query_windows / query_attention_maps of either model as one flat tuple"""
    return tuple(out) if not isinstance(out[0], tuple) else tuple(out[0]) + tuple(out[1])


def _qmaps(m, cache, times_q, nv, na, **kw):
    """times_q [G, nv + na, 2] segments (None, detection: the model's own pyramid) -> (flat outputs, maps)"""
    if m.cfg.variant == "detection":
        v = None if times_q is None else (times_q[:, :nv] if nv else None)
        a = None if times_q is None else (times_q[:, nv:] if na else None)
        out, maps = m.query_attention_maps(cache, v, a, **kw)
    else:
        with torch.no_grad():
            te = m(times_q, "time_mlp")
        out, maps = m.query_attention_maps(cache, te, nv, na, **kw)
    return _flat(out), maps


def _qplain(m, cache, times_q, nv, na, **kw):
    if m.cfg.variant == "detection":
        v = None if times_q is None else (times_q[:, :nv] if nv else None)
        a = None if times_q is None else (times_q[:, nv:] if na else None)
        return _flat(m.query_windows(cache, v, a, **kw))
    with torch.no_grad():
        te = m(times_q, "time_mlp")
    return _flat(m.query_windows(cache, te, nv, na, **kw))


def _full_maps(m, inp, nv, na, **kw):
    """attention_maps of the full forward (the parent's only way to these maps)"""
    if m.cfg.variant == "detection":
        _, maps = m.attention_maps([inp["visual"], inp["audio"]], inp["times"], None, **kw)
    else:
        with torch.no_grad():
            te = m(inp["times"], "time_mlp")
        _, maps = m.attention_maps([inp["visual"], inp["audio"]], te, nv, na, **kw)
    return maps


def EXACT(prec, layer):
    """whether the cache route's map of this layer must be the full forward's bit for bit (module docstring)"""
    return prec != "fp32" or layer == 0


def _close(got, want, prec, what, exact=True):
    """-> whether the bits are equal; asserts equal bits, or MODEL_BOUND where `exact` is False"""
    assert got.shape == want.shape and got.dtype == torch.float32, what
    err = float((got - want).abs().max())
    same = torch.equal(bits(got), bits(want))
    print("QUERYMAP %s %s: max abs difference %.3g (bound %.3g), bits %s" % (what, prec, err, MODEL_BOUND[prec], "equal" if same else "differ"))
    assert err <= MODEL_BOUND[prec], (what, err)
    assert same or not exact, (what, err)
    return same


# ---- identity assignment: the full forward's query-row maps ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("variant,im,dm,vn,nv,na", TINY)
def test_tiny_maps_are_the_full_forwards_query_rows(variant, im, dm, vn, nv, na, prec):
    cfg = _cfg(variant, im, dm, vn)
    sd, inp = _inputs(cfg, W, nv, na, seed=1)
    m = build(cfg, prec, sd)
    tq = None if variant == "detection" else inp["times"][:, cfg.F:]
    cache = _encode(m, inp)
    want = _full_maps(m, inp, nv, na, layers="all", rows="queries")
    plain = _qplain(m, cache, tq, nv, na)
    outs, maps = _qmaps(m, cache, tq, nv, na, layers="all")
    torch.cuda.synchronize()
    _same_bits(outs, plain)                                      # the same launches: query_windows' outputs bit for bit
    assert maps.layers == want.layers == list(range(cfg.num_layers))
    assert (maps.F, maps.S, maps.s0) == (want.F, want.S, want.s0) == (cfg.F, want.S, cfg.F)
    equal = [_close(maps.weights[l], want.weights[l], prec, "%s %s/%s layer %d vs attention_maps" % (variant, im, dm, l), EXACT(prec, l))
             for l in maps.layers]
    print("QUERYMAP identity %s %s/%s %s: layers with equal bits %s" % (variant, im, dm, prec, equal))
    for l in maps.layers:
        w = maps.weights[l]
        assert float((w.sum(-1) - 1.0).abs().max()) <= 1e-5 and bool((w >= 0).all())


def test_c2a_eight_windows_maps_are_the_full_forwards_query_rows():
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    sd, inp = _inputs(cfg, B, nv, na, seed=2)
    m = build(cfg, "fp16", sd)
    cache = _encode(m, inp)
    tq = inp["times"][:, cfg.F:]
    want = _full_maps(m, inp, nv, na, layers="all", rows="queries")
    outs, maps = _qmaps(m, cache, tq, nv, na, layers="all")
    torch.cuda.synchronize()
    _same_bits(outs, _qplain(m, cache, tq, nv, na))
    for l in maps.layers:
        assert tuple(maps.weights[l].shape) == (B, nv * 3 + na, cfg.F + 1)
        _close(maps.weights[l], want.weights[l], "fp16", "C2a / 8 windows layer %d vs attention_maps" % l)


# ---- against the reference's recorded weights ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_maps_match_the_references_recorded_weights(name, prec):
    z, cfg = R.load_fixture(name)
    B, nv, na, Bw, S, F = (int(z[k]) for k in ("B", "nv", "na", "windows", "S", "F"))
    sd, inp = _inputs(cfg, B, nv, na, seed=int(z["seed"]))
    m = build(cfg, prec, sd)
    cache = _encode(m, inp)
    _, maps = _qmaps(m, cache, None if cfg.variant == "detection" else inp["times"][:, F:], nv, na, layers="all")
    torch.cuda.synchronize()
    assert (maps.F, maps.S, maps.s0) == (F, S, F)
    for l in maps.layers:
        want = z["attn/layer%d" % l]
        got = maps.weights[l].cpu().numpy()[:Bw]
        err = float(np.abs(got - QM.compact(want, F)).max())
        print("QUERYMAP model %s %s layer %d: max abs error against the reference %.3g (bound %.3g)" % (name, prec, l, err, MODEL_BOUND[prec]))
        assert err <= MODEL_BOUND[prec], (l, err)
        dense = maps.to_dense(l).cpu().numpy()[:Bw]             # the reference's rows of the query tokens, zero pattern included
        assert np.array_equal(dense != 0, want[:, F:] != 0)


# ---- regrouping ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_recognition_one_cache_serves_any_query_set_and_grouping(prec):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, inp = _inputs(cfg, W, 4, 2, seed=1)
    m = build(cfg, prec, sd)
    cache = _encode(m, inp)
    idx = [2, 0, 0, 1, 2, 1]
    for (nv, na), seed in (((4, 2), 4), ((6, 1), 5), ((1, 3), 6)):            # three query sets, G = 2 W groups on repeated windows
        tq = _segments(len(idx), nv + na, seed=seed).to(DEV)
        outs, maps = _qmaps(m, cache, tq, nv, na, window_index=idx, layers="all")
        _same_bits(outs, _qplain(m, cache, tq, nv, na, window_index=idx))
        again = _qmaps(m, cache, tq, nv, na, window_index=torch.tensor(idx, dtype=torch.int32, device=DEV), layers="all")[1]
        for l in maps.layers:
            assert tuple(maps.weights[l].shape) == (len(idx), nv * 3 + na, cfg.F + 1)      # (include_verb_noun: three rows per visual query)
            assert torch.equal(bits(maps.weights[l]), bits(again.weights[l]))
        for g in (0, 3, 5):                                      # the same query asked alone, of its window
            _, alone = _qmaps(m, cache, tq[g:g + 1], nv, na, window_index=[idx[g]], layers="all")
            for l in maps.layers:
                _close(alone.weights[l][0], maps.weights[l][g], prec, "group %d of (%d, %d) alone, layer %d" % (g, nv, na, l))
        # two groups with the same queries on the same window: the same rows, whatever else the launch holds
        tq2 = tq.clone()
        tq2[2] = tq2[1]
        _, twin = _qmaps(m, cache, tq2, nv, na, window_index=idx, layers="all")
        for l in twin.layers:
            assert torch.equal(bits(twin.weights[l][2]), bits(twin.weights[l][1]))


@pytest.mark.parametrize("prec", PRECS)
def test_detection_pyramid_has_one_row_per_query_visual_first(prec):
    cfg = H.tiny_cfg("detection", "audio_visual", "audio_visual", False, num_class=(13, 5))
    sd, inp = _inputs(cfg, W, 0, 0, seed=3)
    m = build(cfg, prec, sd)
    cache = _encode(m, inp)
    nq = m.num_queries
    idx = [1, 1, 2, 0]
    outs, maps = _qmaps(m, cache, None, 0, 0, window_index=idx, layers="all")
    _same_bits(outs, _qplain(m, cache, None, 0, 0, window_index=idx))
    for l in maps.layers:
        assert tuple(maps.weights[l].shape) == (len(idx), 2 * nq, cfg.F + 1)
    assert tuple(maps.for_head("action").shape) == tuple(maps.for_head("audio").shape) == (len(idx), nq, cfg.F + 1)
    assert torch.equal(maps.for_head("action"), maps.weights[maps.layers[-1]][:, :nq])
    assert torch.equal(maps.for_head("audio"), maps.weights[maps.layers[-1]][:, nq:])
    # groups 0 and 1 ask the same pyramid of the same window
    for l in maps.layers:
        assert torch.equal(bits(maps.weights[l][0]), bits(maps.weights[l][1]))
    # hand-made segments: 7 visual and 5 audio queries per group give 12 rows, visual first
    tv, ta = _segments(len(idx), 7, seed=7).to(DEV), _segments(len(idx), 5, seed=8).to(DEV)
    _, both = _qmaps(m, cache, torch.cat([tv, ta], 1), 7, 5, window_index=idx, layers="all")
    # the model's own pyramid through a cache against the full forward's, window by window
    want = _full_maps(m, inp, 0, 0, layers="all", rows="queries")
    for l in both.layers:
        assert tuple(both.weights[l].shape) == (len(idx), 12, cfg.F + 1)
        assert tuple(both.for_head("action", l).shape) == (len(idx), 7, cfg.F + 1) and tuple(both.for_head("audio", l).shape) == (len(idx), 5, cfg.F + 1)
        for g, w in enumerate(idx):
            _close(maps.weights[l][g], want.weights[l][w], prec, "detection pyramid group %d = window %d, layer %d" % (g, w, l), EXACT(prec, l))


# ---- selection and views -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_layers_select_and_views_work(prec):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    nv, na = 4, 2
    sd, inp = _inputs(cfg, W, nv, na, seed=1)
    m = build(cfg, prec, sd)
    cache = _encode(m, inp)
    tq = inp["times"][:, cfg.F:]
    Lyr, F = cfg.num_layers, cfg.F
    _, all_ = _qmaps(m, cache, tq, nv, na, layers="all")
    _, last = _qmaps(m, cache, tq, nv, na)
    _, picked = _qmaps(m, cache, tq, nv, na, layers=[-1, 0])
    _, ph = _qmaps(m, cache, tq, nv, na, layers="all", per_head=True)
    torch.cuda.synchronize()
    assert last.layers == [Lyr - 1] and picked.layers == [0, Lyr - 1] and all_.layers == list(range(Lyr))
    assert torch.equal(bits(last.weights[Lyr - 1]), bits(all_.weights[Lyr - 1]))
    for l in picked.layers:
        assert torch.equal(bits(picked.weights[l]), bits(all_.weights[l]))
    # per head: [G, H, Q, F + 1], its mean the mean map within the kernel's bound (a different order of one division and H adds on
    # values <= 1: 8 fp32 ulps of 1.0 cover it)
    assert ph.per_head and not all_.per_head
    for l in all_.layers:
        assert tuple(ph.weights[l].shape) == (W, cfg.nhead, nv * 3 + na, F + 1)
        assert float((ph.weights[l].mean(1) - all_.weights[l]).abs().max()) <= 8 * 2.0 ** -23
    # the rows of a head, the modality halves, the dense rows
    plan = m._plan(inp["times"].shape[1], nv, na)
    for slot, _, start, n in plan.heads:
        assert torch.equal(last.for_head(slot), all_.weights[Lyr - 1][:, start - F:start - F + n])
        assert tuple(ph.for_head(slot).shape) == (W, cfg.nhead, n, F + 1)
    vis, aud = last.split_modalities()
    assert vis.shape[-1] == aud.shape[-1] == cfg.num_feats and torch.equal(torch.cat([vis, aud], -1), last.weights[Lyr - 1][..., :F])
    dense = last.to_dense()
    S = F + nv * 3 + na
    assert tuple(dense.shape) == (W, S - F, S) and int((dense != 0).sum()) == W * (S - F) * (F + 1)
    assert tuple(ph.to_dense().shape) == (W, cfg.nhead, S - F, S)
    # out=: the maps of an earlier call, and its list of buffers, are written in place
    held = {l: all_.weights[l].clone() for l in all_.layers}
    for l in all_.layers:
        all_.weights[l].fill_(-1.0)
    _, again = _qmaps(m, cache, tq, nv, na, layers="all", out=all_)
    assert all(again.weights[l].data_ptr() == all_.weights[l].data_ptr() and torch.equal(bits(again.weights[l]), bits(held[l]))
               for l in all_.layers)
    with pytest.raises(ValueError, match="out"):
        _qmaps(m, cache, tq, nv, na, layers="last", out=all_)


# ---- capture -------------------------------------------------------------------------------------------------------------------------
def test_capture_replays_onto_new_queries_and_a_new_window_index_with_the_eager_maps():
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    sd, inp = _inputs(cfg, B, nv, na, seed=2)
    m = build(cfg, "fp16", sd)
    G = 2 * B
    g = torch.Generator().manual_seed(9)
    idx1, idx2 = torch.randint(0, B, (G,), generator=g), torch.randint(0, B, (G,), generator=g)
    with torch.no_grad():
        cache = _encode(m, inp)
        te1 = m(_segments(G, nv + na, seed=10).to(DEV), "time_mlp")
        te2 = m(_segments(G, nv + na, seed=11).to(DEV), "time_mlp")
    s_te, s_idx = te1.clone(), idx1.to(device=DEV, dtype=torch.int32)
    for _ in range(2):                                            # warm-up: operand copies, the arena, the row table
        _, held = m.query_attention_maps(cache, s_te, nv, na, window_index=s_idx, layers="all", validate=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, cmaps = m.query_attention_maps(cache, s_te, nv, na, window_index=s_idx, layers="all", out=held, validate=False)
    s_te.copy_(te2)
    s_idx.copy_(idx2.to(device=DEV, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    assert all(cmaps.weights[l].data_ptr() == held.weights[l].data_ptr() for l in held.layers)
    replayed = {l: cmaps.weights[l].clone() for l in cmaps.layers}
    rep_outs = tuple(None if t is None else t.clone() for t in captured)
    eager_outs, eager = m.query_attention_maps(cache, te2, nv, na, window_index=idx2.tolist(), layers="all")
    _, first = m.query_attention_maps(cache, te1, nv, na, window_index=idx1.tolist(), layers="all")
    torch.cuda.synchronize()
    _same_bits(rep_outs, eager_outs)
    for l in eager.layers:
        assert torch.equal(bits(replayed[l]), bits(eager.weights[l]))
        assert not torch.equal(first.weights[l], eager.weights[l])


# ---- peak memory ---------------------------------------------------------------------------------------------------------------------
def test_maps_of_all_layers_add_their_buffers_and_nothing_else_to_the_peak():
    """C2a at 8 windows: the peak allocated bytes of a warmed-up query_attention_maps(layers="all") exceed query_windows' by the
    map buffers plus at most 1 MB (the caching allocator does not split a large block whose remainder would be under 1 MB; the
    bound of tests/test_gpu_attn_maps.py) - the arena is query_windows', whatever is asked for"""
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    sd, inp = _inputs(cfg, B, nv, na, seed=2)
    m = build(cfg, "fp16", sd)
    with torch.no_grad():
        cache = _encode(m, inp)
        te = m(inp["times"][:, cfg.F:], "time_mlp")

    def peak(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        gc.collect()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    plain = peak(lambda: m.query_windows(cache, te, nv, na))
    with_maps = peak(lambda: m.query_attention_maps(cache, te, nv, na, layers="all"))
    map_bytes = cfg.num_layers * B * (nv * 3 + na) * (cfg.F + 1) * 4
    print("QUERYMAP memory C2a / 8 windows: query_windows peak %d, with all maps %d, map buffers %d" % (plain, with_maps, map_bytes))
    assert plain < with_maps <= plain + map_bytes + (1 << 20), (plain, with_maps, map_bytes)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_a_stale_cache_train_mode_and_a_bad_window_index_are_refused():
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    nv, na = 4, 2
    sd, inp = _inputs(cfg, W, nv, na, seed=1)
    m = build(cfg, "fp32", sd)
    cache = _encode(m, inp)
    with torch.no_grad():
        te = m(inp["times"][:, cfg.F:], "time_mlp")
    m.query_attention_maps(cache, te, nv, na)
    for bad in ([0, 1, 3], torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV), torch.tensor([0, -1, 2], dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="outside"):
            m.query_attention_maps(cache, te, nv, na, window_index=bad)
    with pytest.raises(ValueError, match="window_index"):
        m.query_attention_maps(cache, te[:2], nv, na)                           # G != W without an index
    # validate=False: the caller owns the range - the out-of-range group's maps and outputs are NaN, the others untouched
    good_out, good = m.query_attention_maps(cache, te, nv, na, layers="all")
    out, maps = m.query_attention_maps(cache, te, nv, na, layers="all", validate=False,
                                       window_index=torch.tensor([0, 7, 2], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for l in maps.layers:
        assert bool(torch.isnan(maps.weights[l][1]).all())
        assert torch.equal(bits(maps.weights[l][0]), bits(good.weights[l][0])) and torch.equal(bits(maps.weights[l][2]), bits(good.weights[l][2]))
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.query_attention_maps(cache, te, nv, na)
    m.eval()
    with torch.no_grad():
        getattr(m, m._stack_prefix).layers[0].self_attn.in_proj_weight.mul_(1.25)
    with pytest.raises(RuntimeError, match="stale"):
        m.query_attention_maps(cache, te, nv, na)
    with pytest.raises(RuntimeError, match="stale"):
        m.query_windows(cache, te, nv, na)
