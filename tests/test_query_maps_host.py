"""Attention maps from a window cache, as far as they go without a GPU: what `query_attention_maps` refuses before any library
call, the `AttentionMaps` views of group-major (and per-head) maps against the numpy restatement, and the three entry points -
declared, bound, exported, and checking their arguments before any launch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import query_maps_ref as QM
from tests.candidate_helpers import ROOT
from tests.test_query_host import _fake_cache, _no_library, build
from tim_amd import _lib as L
from tim_amd import query as Q
from tim_amd.attn_maps import AttentionMaps, QueryMapRequest

EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
NARGS = {"timhip_attention_query_weights": 11, "timhip_stack_query_maps_workspace_bytes": 2, "timhip_stack_query_maps": 16}


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", code))
    assert set(NARGS) <= declared and set(NARGS) <= set(L.exported_symbols())
    for n, k in NARGS.items():
        assert len(L._SIGS[n][1]) == k, n
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, code).group(1)
        assert len(decl.split(",")) == k, n
    assert L._SIGS["timhip_stack_query_maps_workspace_bytes"][0] is C.c_size_t
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", hdr) and L.ABI_VERSION == 6      # additive: the version stays
    lib = L.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NARGS:
        assert hasattr(lib, n), n
        assert re.search(r"\bT %s\b" % n, syms), n
    # the header, the binding and the library name the same set of entry points, the new ones included
    exported = set(re.findall(r"\bT (timhip_[a-z0-9_]+)\b", syms))
    assert declared == exported == set(L._SIGS)
    # the new kernels are instances of the two budgeted families of the unit
    from tools.check_spills import BUDGET
    assert BUDGET["attn_maps.hip"] == [(r"attn_w_mfma", 0), (r"attn_w_generic", 0)]
    src = open(os.path.join(ROOT, "tim_amd", "csrc", "attn_maps.hip")).read()
    assert "timhip_attention_query_weights" in src and src.index("#pragma clang fp contract(off)") < src.index("#include")


def _qdesc(G=8, Q=25, F=100, E=1024, Hh=8, prec="fp16", p_drop=0.0, flags=0):
    return L.TimDesc(G, Q, F, E // 2, E, Hh, 4 * E, L.PRECISIONS[prec], p_drop, 0, 0, flags, None)


def test_weights_entry_checks_its_arguments_before_any_launch():
    """No GPU is needed: every refusal comes back before the first launch (the pointers below are never followed)."""
    lib = L.load()
    fake, odd, odd16 = C.c_void_p(0x1000), C.c_void_p(0x1002), C.c_void_p(0x1001)
    d = _qdesc()

    def rc(desc=d, q=fake, kv=fake, ldkv=None, wrows=None, W=8, widx=fake, per_head=0, w=fake, ld=None):
        dd = desc if desc is not None else d
        return lib.timhip_attention_query_weights(C.byref(desc) if desc is not None else None, q, kv, 2 * dd.E if ldkv is None else ldkv,
                                                  dd.F if wrows is None else wrows, W, widx, per_head, w,
                                                  dd.F + 1 if ld is None else ld, None)
    assert rc(desc=None) == EINVAL and rc(q=None) == EINVAL and rc(kv=None) == EINVAL and rc(w=None) == EINVAL
    assert rc(desc=_qdesc(p_drop=0.1)) == EINVAL
    assert rc(W=0) == EINVAL and rc(W=-3) == EINVAL
    assert rc(widx=None, W=7) == EINVAL and rc(widx=None, W=9) == EINVAL          # NULL widx: G == W required
    assert rc(ld=d.F) == EINVAL and rc(ld=0) == EINVAL
    assert rc(ldkv=2 * d.E - 1) == EINVAL and rc(wrows=d.F - 1) == EINVAL
    bad = _qdesc()
    bad.H = 3                                                                    # heads do not divide the width
    assert rc(desc=bad) == EINVAL
    assert rc(desc=_qdesc(F=193)) == EUNSUPPORTED and rc(desc=_qdesc(F=193, prec="fp32")) == EUNSUPPORTED
    assert rc(w=odd) == EALIGN and rc(w=odd, per_head=1) == EALIGN
    assert rc(kv=odd16) == EALIGN and rc(q=odd16) == EALIGN                      # not element-aligned
    assert rc(desc=_qdesc(prec="fp32"), kv=odd) == EALIGN


def test_stack_entry_checks_its_arguments_before_any_launch():
    lib = L.load()
    layers = (L.TimLayerParams * 2)()
    fake = C.c_void_p(0x1000)
    d = _qdesc()
    assert lib.timhip_stack_query_maps_workspace_bytes(C.byref(d), 6) == lib.timhip_stack_query_workspace_bytes(C.byref(d), 6) > 0
    assert lib.timhip_stack_query_maps_workspace_bytes(None, 6) == 0
    need = lib.timhip_stack_query_maps_workspace_bytes(C.byref(d), 2)
    good = (C.c_void_p * 2)(None, 0x2000)
    odd = (C.c_void_p * 2)(0x2002, None)

    def run(desc=d, maps=good, ld=None, nbytes=need, W=8, widx=fake, cache=fake, x_in=fake, per_head=0):
        return lib.timhip_stack_query_maps(C.byref(desc), 2, layers, cache, W, widx, x_in, fake, fake, fake, maps, per_head,
                                           desc.F + 1 if ld is None else ld, fake, nbytes, None)
    assert run(maps=None) == EINVAL
    assert run(ld=d.F) == EINVAL and run(ld=d.F, per_head=1) == EINVAL
    assert run(maps=odd) == EALIGN
    assert run(desc=_qdesc(p_drop=0.1)) == EINVAL
    assert run(x_in=None) == EINVAL and run(cache=None) == EINVAL
    assert run(W=0) == EINVAL and run(widx=None, W=7) == EINVAL
    assert run(desc=_qdesc(F=193)) == EUNSUPPORTED
    assert run(cache=C.c_void_p(0x1008)) == EALIGN
    assert run(nbytes=need - 1) == EWORKSPACE


# ---- AttentionMaps of query groups ----------------------------------------------------------------------------------------------
def test_views_of_group_major_maps_match_the_restatement():
    """G != W: the first axis is the group, the feature columns those of the group's own window"""
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    nv, na, Hh, F, E = 4, 2, cfg.nhead, cfg.F, cfg.E
    plan = Q.QueryPlan(cfg, nv, na)
    G, W, Qn = 5, 3, plan.S
    widx = [2, 0, 0, 1, 2]
    rng = np.random.default_rng(0)
    q, k_own, k_cache = rng.standard_normal((G, Qn, E)), rng.standard_normal((G, Qn, E)), rng.standard_normal((W, F, E))
    mean = QM.query_weights(q, k_own, k_cache, widx, Hh)
    ph = QM.query_weights(q, k_own, k_cache, widx, Hh, per_head=True)
    S = F + Qn
    for w, lead in ((mean, (G,)), (ph, (G, Hh))):
        maps = AttentionMaps([1], [torch.from_numpy(w)], F, S, F, heads=plan.full.heads, num_feats=cfg.num_feats)
        assert maps.per_head == (len(lead) == 2) and (maps.F, maps.S, maps.s0) == (F, S, F)
        dense = maps.to_dense().numpy()
        assert dense.shape == lead + (Qn, S)
        assert np.array_equal(dense[..., :F], w[..., :F])
        for i in range(Qn):
            assert np.array_equal(dense[..., i, F + i], w[..., i, F])
        assert np.count_nonzero(dense) == w.size
        vis, aud = maps.split_modalities()
        assert np.array_equal(vis.numpy(), w[..., :cfg.num_feats]) and np.array_equal(aud.numpy(), w[..., cfg.num_feats:F])
        for slot, _, start, n in plan.heads:                                  # (the query plan's rows: relative to the first query)
            got = maps.for_head(slot).numpy()
            assert got.shape == lead + (n, F + 1) and np.array_equal(got, w[..., start:start + n, :])
    # two groups of one window and the same queries: the same rows
    q[2], k_own[2] = q[1], k_own[1]
    again = QM.query_weights(q, k_own, k_cache, widx, Hh)
    assert np.array_equal(again[2], again[1]) and not np.array_equal(again[0], again[1])
    with pytest.raises(ValueError):
        AttentionMaps([0], [torch.zeros((G, Hh, Qn, F))], F, S, F)
    with pytest.raises(ValueError):
        AttentionMaps([0], [torch.zeros((G, Qn + 1, F + 1))], F, S, F)


def test_request_checks_layers_and_out_buffers():
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, _ = H.synth_torch(cfg, 3, 4, 2, seed=1, dtype=torch.float32)
    m = build(cfg, "fp32", sd)
    for bad in ([cfg.num_layers], "some", [], [0, 0], 3, None, [True]):
        with pytest.raises(ValueError, match="layers"):
            QueryMapRequest(m, bad)
    assert QueryMapRequest(m, "all").layers == list(range(cfg.num_layers)) and QueryMapRequest(m, [-1]).layers == [cfg.num_layers - 1]
    G, Qn, F, Hh, cpu = 5, 6, cfg.F, cfg.nhead, torch.device("cpu")
    req = QueryMapRequest(m, "all")
    bufs = req._buffers(G, Qn, F, Hh, cpu)
    assert len(bufs) == cfg.num_layers and all(tuple(b.shape) == (G, Qn, F + 1) and b.dtype == torch.float32 for b in bufs)
    assert all(tuple(b.shape) == (G, Hh, Qn, F + 1) for b in QueryMapRequest(m, "last", per_head=True)._buffers(G, Qn, F, Hh, cpu))
    held = AttentionMaps(req.layers, bufs, F, F + Qn, F)
    assert [b.data_ptr() for b in QueryMapRequest(m, "all", out=held)._buffers(G, Qn, F, Hh, cpu)] == [b.data_ptr() for b in bufs]
    assert [b.data_ptr() for b in QueryMapRequest(m, "all", out=bufs)._buffers(G, Qn, F, Hh, cpu)] == [b.data_ptr() for b in bufs]
    for out in (held, bufs):
        with pytest.raises(ValueError, match="out"):
            QueryMapRequest(m, "last", out=out)._buffers(G, Qn, F, Hh, cpu)             # other layers / another count
        with pytest.raises(ValueError, match="out"):
            QueryMapRequest(m, "all", out=out)._buffers(G + 1, Qn, F, Hh, cpu)           # another group count
        with pytest.raises(ValueError, match="out"):
            QueryMapRequest(m, "all", per_head=True, out=out)._buffers(G, Qn, F, Hh, cpu)
    with pytest.raises(ValueError, match="out"):
        QueryMapRequest(m, "all", out=[b.double() for b in bufs])._buffers(G, Qn, F, Hh, cpu)
    with pytest.raises(ValueError, match="out"):
        QueryMapRequest(m, "all", out=[b.transpose(1, 2) for b in bufs])._buffers(G, F + 1, Qn, Hh, cpu)


# ---- what the methods refuse, before any library call ----------------------------------------------------------------------------
def test_recognition_refusals_come_before_any_library_call(monkeypatch):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, _ = H.synth_torch(cfg, 3, 4, 2, seed=1, dtype=torch.float32)
    m = build(cfg, "fp32", sd).eval()
    _no_library(monkeypatch)
    d = cfg.d_model
    te_q = torch.zeros(3, 6, d)
    cache = _fake_cache(m)
    for bad in ([cfg.num_layers], "first", []):
        with pytest.raises(ValueError, match="layers"):
            m.query_attention_maps(cache, te_q, 4, 2, layers=bad)
    with pytest.raises(ValueError, match="d_model"):
        m.query_attention_maps(cache, torch.zeros(3, 6, d + 1), 4, 2)
    with pytest.raises(ValueError, match="rows per group"):
        m.query_attention_maps(cache, torch.zeros(3, 5, d), 4, 2)
    with pytest.raises(ValueError, match="window_index"):
        m.query_attention_maps(cache, torch.zeros(4, 6, d), 4, 2)               # G != W without an index
    for bad in ([0, 1, 3], [-1, 0, 1], [0, 1], [0.5, 1.0, 2.0]):
        with pytest.raises(ValueError):
            m.query_attention_maps(cache, te_q, 4, 2, window_index=bad)
    with pytest.raises(ValueError, match="keys and values"):
        m.query_attention_maps(_fake_cache(m, precision="fp16"), te_q, 4, 2)
    with pytest.raises(ValueError, match="WindowCache"):
        m.query_attention_maps(object(), te_q, 4, 2)
    with pytest.raises(RuntimeError, match="stale"):
        m.query_attention_maps(_fake_cache(m, versions=Q.param_versions(m)[:-1] + ((0, 0),)), te_q, 4, 2)
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.query_attention_maps(cache, te_q, 4, 2)


def test_detection_refusals_come_before_any_library_call(monkeypatch):
    cfg = H.tiny_cfg("detection", "audio_visual", "visual", False, num_class=(13, 5))
    sd, _ = H.synth_torch(cfg, 3, 0, 0, seed=3, dtype=torch.float32)
    m = build(cfg, "fp32", sd).eval()
    _no_library(monkeypatch)
    cache = _fake_cache(m)
    with pytest.raises(ValueError, match="layers"):
        m.query_attention_maps(cache, layers=[cfg.num_layers])
    with pytest.raises(ValueError, match="segments"):
        m.query_attention_maps(cache, v_queries=torch.zeros(3, 7, 3))
    with pytest.raises(ValueError, match="data_modality"):
        m.query_attention_maps(cache, a_queries=torch.zeros(3, 7, 2))
    with pytest.raises(ValueError, match="window_index"):
        m.query_attention_maps(cache, v_queries=torch.zeros(4, 7, 2))
    with pytest.raises(ValueError, match="outside"):
        m.query_attention_maps(cache, v_queries=torch.zeros(2, 7, 2), window_index=[0, 3])
    with pytest.raises(RuntimeError, match="stale"):
        m.query_attention_maps(_fake_cache(m, versions=()), v_queries=torch.zeros(3, 7, 2))
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.query_attention_maps(cache)
