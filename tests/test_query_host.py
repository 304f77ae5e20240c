"""Host side of encode-once / query-many (tim_amd/query.py), no GPU: the query-only plan against the full EncoderPlan, the cache's
size arithmetic, the declarations of the new entry points, and the refusals that come before any library call."""
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tim_amd import _lib as L
from tim_amd import functional as Fn
from tim_amd import query as Q

HEADER = os.path.join(os.path.dirname(H.GOLDEN), "..", "include", "timhip.h")
NEW = ("timhip_attention_query_fwd", "timhip_window_cache_bytes", "timhip_stack_encode", "timhip_stack_query_workspace_bytes",
       "timhip_stack_query")


def build(cfg, precision, sd):
    """the model on the CPU: construction and the host-side checks need no device"""
    kw = dict(visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, feat_drop=cfg.feat_drop,
              seq_drop=cfg.seq_drop, d_model=cfg.d_model, nhead=cfg.nhead, num_layers=cfg.num_layers, enc_dropout=cfg.enc_dropout,
              input_modality=cfg.input_modality, data_modality=cfg.data_modality, num_feats=cfg.num_feats,
              include_verb_noun=cfg.include_verb_noun, precision=precision)
    if cfg.variant == "detection":
        from tim_amd.detection import TIM
        m = TIM(cfg.num_class, feedfoward_scale=cfg.feedforward_scale, **kw)
    else:
        from tim_amd.tim import TIM
        m = TIM(cfg.num_class, feedforward_scale=cfg.feedforward_scale, **kw)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return m.eval()


def _det_counts(dm):
    return (7 if "visual" in dm else 0), (5 if "audio" in dm else 0)


CASES = [("recognition", im, dm, vn, None, nv, na) for (_, im, dm, vn, nv, na) in H.rec_golden_cases()] + \
        [("detection", im, dm, tag == "vn", nc) + _det_counts(dm) for (im, dm, nc, tag) in H.DET_CASES]


def test_header_binding_and_build_know_the_entry_points():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L._SIGS, name
    assert len(L._SIGS["timhip_attention_query_fwd"][1]) == 9
    assert len(L._SIGS["timhip_stack_encode"][1]) == 10 and len(L._SIGS["timhip_stack_query"][1]) == 13
    csrc = os.path.join(os.path.dirname(HEADER), "..", "tim_amd", "csrc")
    assert "attention_query.hip" in re.search(r"^SRCS = (.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1)
    from tools.check_spills import BUDGET
    assert BUDGET["attention_query.hip"] == [(r"attn_query_mfma", 0)] and BUDGET["attention_mfma.hip"] == [(r"attn_fwd_mfma", 0)]


@pytest.mark.parametrize("variant,im,dm,vn,nc,nv,na", CASES)
def test_query_plan_is_the_kind_1_part_of_the_full_plan(variant, im, dm, vn, nc, nv, na):
    cfg = H.tiny_cfg(variant, im, dm, vn, num_class=nc)
    F = cfg.F
    full = Fn.EncoderPlan(cfg, F + nv + na, nv, na)
    plan = Q.QueryPlan(cfg, nv, na)
    assert all(r[0] != 1 for r in full.rows[:F]) and all(r[0] == 1 for r in full.rows[F:])
    assert plan.S == full.S - F and plan.F == F
    assert plan.rows == [(k, src, te - F, mod) for (k, src, te, mod) in full.rows[F:]]
    assert all(0 <= r[2] < nv + na for r in plan.rows)
    assert plan.heads == [(slot, p, s0 - F, n) for (slot, p, s0, n) in full.heads]
    assert plan.reg == [(slot, p, s0 - F, n) for (slot, p, s0, n) in full.reg]
    assert all(0 <= s0 and s0 + n <= plan.S for (_, _, s0, n) in plan.heads + plan.reg)
    assert (plan.cls_names, plan.mod_names) == (full.cls_names, full.mod_names)
    t = plan.table("cpu")
    assert t.dtype == torch.int32 and t.tolist() == [list(r) for r in plan.rows]


def test_cache_size_arithmetic():
    for prec, ts in (("fp16", 2), ("bf16", 2), ("fp32", 4), ("bf16x3", 4)):
        c = Q.WindowCache(None, W=64, F=100, E=1024, nlayers=6, precision=prec, feats=None, versions=())
        assert c.nbytes == 6 * 64 * 100 * 2 * 1024 * ts
    # one C2a window in fp16: the 2.4 MB the design quotes
    assert Q.WindowCache(None, 1, 100, 1024, 6, "fp16", None, ()).nbytes == 2457600


def test_window_index_rules():
    r = Q.resolve_window_index
    assert r(None, 3, 3, "cpu") is None
    with pytest.raises(ValueError, match="window_index"):
        r(None, 4, 3, "cpu")                                     # G != W without an index
    for good in ([2, 0, 1, 1], np.array([2, 0, 1, 1]), torch.tensor([2, 0, 1, 1])):
        t = r(good, 4, 3, "cpu")
        assert t.dtype == torch.int32 and t.tolist() == [2, 0, 1, 1]
    for bad in ([0, 3], [-1, 0], np.array([0, 3]), torch.tensor([0, 3]), [0.5, 1.0]):
        with pytest.raises(ValueError):
            r(bad, 2, 3, "cpu")
    with pytest.raises(ValueError):
        r([0, 1, 2], 2, 3, "cpu")                                # one entry per group
    with pytest.raises(ValueError):
        r([[0, 1]], 2, 3, "cpu")


def _no_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a library call was reached")
    monkeypatch.setattr(L, "call", boom)
    monkeypatch.setattr(Fn, "call", boom)
    monkeypatch.setattr(L, "load", boom)


def _fake_cache(m, W=3, **over):
    cfg = m.cfg
    kw = dict(kv=torch.zeros(1), W=W, F=cfg.F, E=cfg.E, nlayers=cfg.num_layers, precision=m.rt.precision_name, feats=None,
              versions=Q.param_versions(m))
    kw.update(over)
    return Q.WindowCache(**kw)


def test_recognition_refusals_come_before_any_library_call(monkeypatch):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, inp = H.synth_torch(cfg, 3, 4, 2, seed=1, dtype=torch.float32)
    m = build(cfg, "fp32", sd).eval()
    _no_library(monkeypatch)
    d, F = cfg.d_model, cfg.F
    te_q = torch.zeros(3, 6, d)
    cache = _fake_cache(m)
    with pytest.raises(ValueError, match="d_model"):
        m.query_windows(cache, torch.zeros(3, 6, d + 1), 4, 2)                  # wrong width
    with pytest.raises(ValueError, match="rows per group"):
        m.query_windows(cache, torch.zeros(3, 5, d), 4, 2)                      # wrong row count
    with pytest.raises(ValueError, match="window_index"):
        m.query_windows(cache, torch.zeros(4, 6, d), 4, 2)                      # G != W without an index
    with pytest.raises(ValueError, match="outside"):
        m.query_windows(cache, te_q, 4, 2, window_index=[0, 1, 3])
    with pytest.raises(ValueError, match="keys and values"):
        m.query_windows(_fake_cache(m, precision="fp16"), te_q, 4, 2)           # precision mismatch
    with pytest.raises(ValueError, match="F = "):
        m.query_windows(_fake_cache(m, F=F + 1), te_q, 4, 2)                    # F mismatch
    with pytest.raises(ValueError, match="WindowCache"):
        m.query_windows(object(), te_q, 4, 2)
    with pytest.raises(RuntimeError, match="stale"):
        m.query_windows(_fake_cache(m, versions=Q.param_versions(m)[:-1] + ((0, 0),)), te_q, 4, 2)
    with pytest.raises(ValueError, match="d_model"):
        m.encode_windows([inp["visual"], inp["audio"]], torch.zeros(3, F, d + 1))
    with pytest.raises(ValueError, match="feature tokens"):
        m.encode_windows([inp["visual"], inp["audio"]], torch.zeros(3, F - 1, d))
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.query_windows(cache, te_q, 4, 2)
    with pytest.raises(ValueError, match="eval"):
        m.encode_windows([inp["visual"], inp["audio"]], torch.zeros(3, F, d))


def test_a_parameter_update_makes_the_recorded_versions_differ():
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    sd, _ = H.synth_torch(cfg, 3, 4, 2, seed=1, dtype=torch.float32)
    m = build(cfg, "fp32", sd).eval()
    cache = _fake_cache(m)
    Q.check_cache(m, cache)
    with torch.no_grad():
        next(iter(m.cls_head.parameters())).mul_(1.0)            # an in-place update, whatever it writes
    with pytest.raises(RuntimeError, match="stale"):
        Q.check_cache(m, cache)
    m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="stale"):
        Q.check_cache(m, cache)
    Q.check_cache(m, _fake_cache(m))


def test_detection_refusals_come_before_any_library_call(monkeypatch):
    cfg = H.tiny_cfg("detection", "audio_visual", "visual", False, num_class=(13, 5))
    sd, inp = H.synth_torch(cfg, 3, 0, 0, seed=3, dtype=torch.float32)
    m = build(cfg, "fp32", sd).eval()
    _no_library(monkeypatch)
    cache = _fake_cache(m)
    with pytest.raises(ValueError, match="segments"):
        m.query_windows(cache, v_queries=torch.zeros(3, 7, 3))
    with pytest.raises(ValueError, match="data_modality"):
        m.query_windows(cache, a_queries=torch.zeros(3, 7, 2))
    with pytest.raises(ValueError, match="window_index"):
        m.query_windows(cache, v_queries=torch.zeros(4, 7, 2))
    with pytest.raises(ValueError, match="outside"):
        m.query_windows(cache, v_queries=torch.zeros(2, 7, 2), window_index=[0, 3])
    with pytest.raises(ValueError, match="feature_times"):
        m.encode_windows([inp["visual"], inp["audio"]], torch.zeros(3, cfg.F - 1, 2))
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.query_windows(cache)
