"""Encode a window once, query it many times (`encode_windows` / `query_windows`) on a real MI355X: the route against the plain
evaluation forward and against the oracle, its freedom in the query set, staleness, memory, graph capture, mode.

Tolerances.  Against the plain forward the route is the same math at other GEMM row counts; the bound is the project's table for
exactly that, `_assert_close_without_feats` in tests/test_gpu_infer.py, restated in TABLE / `_bound` below: fp32 1e-5,
bf16x3 5e-5, bf16 3e-2, fp16 1e-3, each times max(1, amax); the regression outputs (sigmoids in [0, 1]) take the absolute bound
they have there."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tim_oracle as O  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import query_ref as QR  # noqa: E402
from tests.test_gpu_parity import DEV, amax, build, maxerr  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd.config import named_config  # noqa: E402

TABLE = {"fp32": 1e-5, "bf16x3": 5e-5, "bf16": 3e-2, "fp16": 1e-3}
SLOTS = ("verb", "noun", "action", "audio", "reg_visual", "reg_audio")
W = 3


def bits(t):
    return t.contiguous().view(torch.uint8)


def _bound(prec, k, want):
    if k.startswith("reg_"):
        return 2e-2 if prec == "bf16" else TABLE[prec]
    return TABLE[prec] * max(1.0, amax(want))


def _assert_close(got, want, prec, slots=SLOTS):
    for k in slots:
        assert (got.get(k) is None) == (want.get(k) is None), k
        if want.get(k) is not None:
            g, w = got[k].detach().cpu(), want[k].detach().cpu()
            assert g.shape == w.shape, (k, g.shape, w.shape)
            err, bound = maxerr(g, w), _bound(prec, k, w)
            print("%s %s: max error %.3e (bound %.3e)" % (prec, k, err, bound))
            assert err <= bound, (k, err, bound)


def _inputs(cfg, B, nv, na, seed):
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=seed, dtype=torch.float32)
    return sd, {k: v.to(DEV) for k, v in inp.items()}


def _cfg(variant, im, dm, vn):
    if variant == "detection":
        return H.tiny_cfg("detection", im, dm, isinstance(vn[0], list), num_class=vn)
    return H.tiny_cfg("recognition", im, dm, vn)


def _forward(m, inp, nv, na):
    """the plain evaluation forward, by slot"""
    if m.cfg.variant == "detection":
        (cls, reg, feats), _, _, _, _ = m([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)
    else:
        cls, feats = m([inp["visual"], inp["audio"]], "encoder", m(inp["times"], "time_mlp"), nv, na)
        reg = (None, None)
    return dict(zip(F.OUT_SLOTS, tuple(cls) + (feats,) + tuple(reg)))


def _encode(m, inp, want_feats=False):
    x = [inp["visual"], inp["audio"]]
    Fk = m.cfg.F
    if m.cfg.variant == "detection":
        return m.encode_windows(x, inp["times"][:, :Fk], want_feats=want_feats)
    return m.encode_windows(x, m(inp["times"], "time_mlp"), want_feats=want_feats)      # the usual [B, T, d] tensor, unchanged


def _query(m, cache, times_q, nv, na, **kw):
    """times_q [G, nv + na, 2] segments (None, detection: the model's own pyramid) -> outputs by slot"""
    if m.cfg.variant == "detection":
        v = None if times_q is None else (times_q[:, :nv] if nv else None)
        a = None if times_q is None else (times_q[:, nv:] if na else None)
        cls, reg = m.query_windows(cache, v, a, **kw)
    else:
        cls, reg = m.query_windows(cache, m(times_q, "time_mlp"), nv, na, **kw), (None, None)
    return dict(zip(SLOTS, tuple(cls) + tuple(reg)))


TINY = [("recognition", im, dm, vn, nv, na) for _, im, dm, vn, nv, na in H.rec_golden_cases()] + \
       [("detection", im, dm, nc, 0, 0) for im, dm, nc, _ in H.DET_CASES]


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("variant,im,dm,vn,nv,na", TINY)
def test_tiny_encode_then_query_is_the_plain_forward(variant, im, dm, vn, nv, na, prec):
    cfg = _cfg(variant, im, dm, vn)
    sd, inp = _inputs(cfg, W, nv, na, seed=1)
    m = build(cfg, prec, sd)
    with torch.no_grad():
        want = _forward(m, inp, nv, na)
    cache = _encode(m, inp, want_feats=True)
    got = _query(m, cache, None if variant == "detection" else inp["times"][:, cfg.F:], nv, na)
    torch.cuda.synchronize()
    _assert_close(got, want, prec)
    assert cache.feats.shape == want["feats"].shape
    _assert_close({"feats": cache.feats}, {"feats": want["feats"]}, prec, slots=("feats",))
    assert all(v is None or v.grad_fn is None for v in got.values())
    assert _encode(m, inp).feats is None


# ---- query-set freedom: one encode, three query sets, each against the oracle ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_case(variant):
    """(cfg, sd fp32, inputs, float64 weights, the oracle's per-layer keys and values) of the case the freedom tests share"""
    if variant == "detection":
        cfg, (nv, na) = H.tiny_cfg("detection", "audio_visual", "audio_visual", False, num_class=(13, 5)), (0, 0)
    else:
        cfg, (nv, na) = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True), (4, 2)
    sd, inp = H.synth_torch(cfg, W, nv, na, seed=1, dtype=torch.float32)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        kv, _ = QR.encode(sd64, cfg, inp["visual"].double(), inp["audio"].double(), inp["times"][:, :cfg.F].double())
    return cfg, sd, inp, sd64, kv, nv, na


def _segments(G, n, seed):
    g = torch.Generator().manual_seed(seed)
    st = torch.rand(G, n, generator=g) * 0.8
    return torch.stack([st, st + 0.05 + 0.1 * torch.rand(G, n, generator=g)], -1)


def _ref(cfg, sd64, kv, tq, nv, na, idx=None):
    with torch.no_grad():
        cls, reg = QR.query(sd64, cfg, kv, tq.double(), nv, na, idx)
    return dict(zip(SLOTS, tuple(cls) + (tuple(reg) if reg is not None else (None, None))))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_recognition_one_encode_serves_any_query_set(prec):
    cfg, sd, inp, sd64, kv, nv, na = _oracle_case("recognition")
    m = build(cfg, prec, sd)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    cache = _encode(m, dev)
    # the fixture's own queries, against the oracle's full forward
    with torch.no_grad():
        full = O.forward(sd64, cfg, inp["visual"].double(), inp["audio"].double(), inp["times"].double(), nv, na)
    _assert_close(_query(m, cache, dev["times"][:, cfg.F:], nv, na), dict(zip(SLOTS, full[0])), prec)
    # another (nv, na)
    tq = _segments(W, 6 + 1, seed=3)
    _assert_close(_query(m, cache, tq.to(DEV), 6, 1), _ref(cfg, sd64, kv, tq, 6, 1), prec)
    # G = 2 W groups on repeated, permuted windows: as a list and as a CUDA tensor
    idx = [2, 0, 0, 1, 2, 1]
    tq = _segments(len(idx), nv + na, seed=4)
    want = _ref(cfg, sd64, kv, tq, nv, na, idx)
    got = _query(m, cache, tq.to(DEV), nv, na, window_index=idx)
    _assert_close(got, want, prec)
    again = _query(m, cache, tq.to(DEV), nv, na, window_index=torch.tensor(idx, dtype=torch.int32, device=DEV))
    for k in SLOTS:
        assert (got[k] is None) == (again[k] is None) and (got[k] is None or torch.equal(bits(got[k]), bits(again[k]))), k
    with pytest.raises(ValueError, match="outside"):
        _query(m, cache, tq.to(DEV), nv, na, window_index=torch.tensor([0, 1, 2, 3, 0, 0], dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_detection_hand_made_segments_against_the_oracle(prec):
    cfg, sd, inp, sd64, kv, _, _ = _oracle_case("detection")
    m = build(cfg, prec, sd)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    cache = _encode(m, dev)
    nv, na = 7, 7
    tq = torch.cat([_segments(W, nv, seed=5), _segments(W, na, seed=6)], 1)
    with torch.no_grad():
        full = O.forward(sd64, cfg, inp["visual"].double(), inp["audio"].double(), torch.cat([inp["times"].double(), tq.double()], 1),
                         nv, na)
    _assert_close(_query(m, cache, tq.to(DEV), nv, na), dict(zip(SLOTS, tuple(full[0]) + tuple(full[2]))), prec)
    idx = [1, 1, 2, 0, 2, 0]
    tq = torch.cat([_segments(len(idx), nv, seed=7), _segments(len(idx), na, seed=8)], 1)
    _assert_close(_query(m, cache, tq.to(DEV), nv, na, window_index=idx), _ref(cfg, sd64, kv, tq, nv, na, idx), prec)


# ---- staleness, mode -----------------------------------------------------------------------------------------------------------
def test_a_parameter_update_between_encode_and_query_is_refused():
    cfg, sd, inp, _, _, nv, na = _oracle_case("recognition")
    m = build(cfg, "fp32", sd)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    cache = _encode(m, dev)
    tq = dev["times"][:, cfg.F:]
    before = _query(m, cache, tq, nv, na)
    with torch.no_grad():
        getattr(m, m._stack_prefix).layers[0].self_attn.in_proj_weight.mul_(1.25)
    with pytest.raises(RuntimeError, match="stale"):
        _query(m, cache, tq, nv, na)
    after = _query(m, _encode(m, dev), tq, nv, na)
    with torch.no_grad():
        want = _forward(m, dev, nv, na)
    _assert_close(after, want, "fp32")
    assert not torch.equal(before["action"], after["action"])


def test_train_mode_is_refused_and_outputs_carry_no_graph():
    cfg, sd, inp, _, _, nv, na = _oracle_case("recognition")
    m = build(cfg, "fp32", sd)
    dev = {k: v.to(DEV) for k, v in inp.items()}
    cache = _encode(m, dev)
    te_q = m(dev["times"][:, cfg.F:].clone().requires_grad_(True), "time_mlp")     # gradients on, a grad_fn on the input
    assert te_q.grad_fn is not None
    out = m.query_windows(cache, te_q, nv, na)
    assert all(v is None or (v.grad_fn is None and not v.requires_grad) for v in out)
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.query_windows(cache, te_q, nv, na)
    with pytest.raises(ValueError, match="eval"):
        _encode(m, dev)
    m.eval()


# ---- C2a at 8 windows: the oracle bound, memory, graph capture ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def c2a():
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    sd, inp = _inputs(cfg, B, nv, na, seed=2)
    m = build(cfg, "fp16", sd)
    return cfg, sd, inp, m, B, nv, na


def test_c2a_eight_windows_within_1e_3_of_the_fp32_oracle(c2a):
    cfg, sd, inp, m, B, nv, na = c2a
    cache = _encode(m, inp)
    opsize = 2
    assert cache.nbytes == cfg.num_layers * B * cfg.F * 2 * cfg.E * opsize == cache.kv.numel() * cache.kv.element_size()
    got = _query(m, cache, inp["times"][:, cfg.F:], nv, na)
    with torch.no_grad():
        ref_cls, _ = O.forward(sd, cfg, inp["visual"].cpu(), inp["audio"].cpu(), inp["times"].cpu(), nv, na)
    for k, b in zip(("verb", "noun", "action", "audio"), ref_cls):
        err = maxerr(got[k].cpu(), b)
        print("C2a / 8 windows fp16 %s: max error against the fp32 oracle %.3e (bound 1e-3)" % (k, err))
        assert err <= 1e-3, (k, err)


def test_c2a_one_query_call_peaks_below_one_plain_forward(c2a):
    """the method of test_c2a_production_batch_forward_holds_one_arena (peak allocated bytes of one warmed-up call), on one model:
    a call's peak = what it allocates while it runs + the cached arena it runs in"""
    cfg, sd, inp, m, B, nv, na = c2a
    tq = inp["times"][:, cfg.F:]

    def peak(fn, slot):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        level = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - level + m._ws[(torch.device(DEV), slot)].numel()
    with torch.no_grad():
        cache = _encode(m, inp)
        q = peak(lambda: _query(m, cache, tq, nv, na), "query")
        f = peak(lambda: _forward(m, inp, nv, na), "infer")
    print("peak bytes of one call at C2a / 8 windows: query_windows %d, plain forward %d, cache %d" % (q, f, cache.nbytes))
    assert q < f, (q, f)


def test_query_is_captured_as_one_graph_and_replays_on_new_queries_and_windows(c2a):
    cfg, sd, inp, m, B, nv, na = c2a
    G = 2 * B
    g = torch.Generator().manual_seed(9)
    idx1, idx2 = torch.randint(0, B, (G,), generator=g), torch.randint(0, B, (G,), generator=g)
    with torch.no_grad():
        cache = _encode(m, inp)
        te1 = m(_segments(G, nv + na, seed=10).to(DEV), "time_mlp")
        te2 = m(_segments(G, nv + na, seed=11).to(DEV), "time_mlp")
        s_te, s_idx = te1.clone(), idx1.to(device=DEV, dtype=torch.int32)
        for _ in range(2):                                        # warm-up: operand copies, the arena, the row table
            m.query_windows(cache, s_te, nv, na, window_index=s_idx, validate=False)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m.query_windows(cache, s_te, nv, na, window_index=s_idx, validate=False)
        s_te.copy_(te2)
        s_idx.copy_(idx2.to(device=DEV, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [None if v is None else v.clone() for v in captured]
        eager = m.query_windows(cache, te2, nv, na, window_index=idx2.tolist())
        first = m.query_windows(cache, te1, nv, na, window_index=idx1.tolist())
    torch.cuda.synchronize()
    for a, b in zip(eager, replayed):
        assert (a is None) == (b is None) and (a is None or torch.equal(bits(a), bits(b)))
    assert not torch.equal(first[2], eager[2])
