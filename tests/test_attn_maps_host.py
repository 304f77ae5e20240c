"""Attention maps, as far as they go without a GPU: the `AttentionMaps` views against the numpy restatement on CPU tensors, what
`model.attention_maps` refuses, and the three entry points - declared, bound, exported, and checking their arguments before any
launch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import attn_maps_ref as R
from tests import helpers as H
from tests.candidate_helpers import ROOT
from tests.test_infer_host import _desc
from tim_amd import _lib as L
from tim_amd.attn_maps import AttentionMaps, resolve_layers, resolve_rows
from tim_amd.functional import EncoderPlan

EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
NARGS = {"timhip_attention_weights": 7, "timhip_stack_infer_maps_workspace_bytes": 3, "timhip_stack_infer_maps": 14}


def _rec_cfg():
    return H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)


def _build_cpu(cfg, sd):
    if cfg.variant == "detection":
        from tim_amd.detection import TIM
    else:
        from tim_amd.tim import TIM
    m = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
            nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, input_modality=cfg.input_modality,
            data_modality=cfg.data_modality, include_verb_noun=cfg.include_verb_noun, precision="fp32")
    m.load_state_dict(sd)
    return m.eval()


# ---- AttentionMaps on CPU tensors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["all", "queries"])
def test_views_match_the_restatement(rows):
    cfg = _rec_cfg()
    B, nv, na, Hh = 2, 4, 2, cfg.nhead
    plan = EncoderPlan(cfg, 2 * cfg.num_feats + nv + na, nv, na)
    S, F = plan.S, cfg.F
    s0 = resolve_rows(rows, F)
    rng = np.random.default_rng(0)
    qkv = [rng.standard_normal((B * S, 3 * cfg.E)) for _ in range(2)]
    ws = [R.weights(x, B, S, F, Hh, s0=s0) for x in qkv]
    maps = AttentionMaps([0, 1], [torch.from_numpy(w) for w in ws], F, S, s0, heads=plan.heads, num_feats=cfg.num_feats)
    assert maps.layers == [0, 1] and (maps.F, maps.S, maps.s0) == (F, S, s0)
    for l in (0, 1):
        dense = maps.to_dense(l).numpy()
        assert dense.shape == (B, S - s0, S)
        assert np.array_equal(dense, R.to_dense(ws[l], S, F, s0))
        assert np.array_equal(dense, R.to_dense(R.weights(qkv[l], B, S, F, Hh), S, F, 0)[:, s0:])
        vis, aud = maps.split_modalities(l)
        assert np.array_equal(vis.numpy(), ws[l][..., :cfg.num_feats]) and np.array_equal(aud.numpy(), ws[l][..., cfg.num_feats:F])
    assert np.array_equal(maps.to_dense().numpy(), maps.to_dense(1).numpy())          # default: the last layer asked for
    assert {h[0] for h in plan.heads} == {"verb", "noun", "action", "audio"}
    for slot, _, start, n in plan.heads:
        got = maps.for_head(slot, 0).numpy()
        assert got.shape == (B, n, F + 1) and np.array_equal(got, ws[0][:, start - s0:start - s0 + n])
    with pytest.raises(KeyError):
        maps.for_head("reg_visual")
    with pytest.raises(KeyError):
        maps.to_dense(5)


def test_views_refuse_what_the_layout_cannot_give():
    w = torch.zeros((1, 4, 7))
    one = AttentionMaps([0], [w], 6, 10, 6, heads=[("action", "fc_visual_action", 6, 4)], num_feats=None)
    with pytest.raises(ValueError):
        one.split_modalities()
    late = AttentionMaps([0], [torch.zeros((1, 2, 7))], 6, 10, 8, heads=[("action", "fc_visual_action", 6, 4)])
    with pytest.raises(ValueError):
        late.for_head("action")
    with pytest.raises(ValueError):
        AttentionMaps([0], [torch.zeros((1, 4, 6))], 6, 10, 6)


def test_layer_and_row_selection():
    assert resolve_layers("last", 6) == [5] and resolve_layers("all", 3) == [0, 1, 2]
    assert resolve_layers([-1, 0], 6) == [0, 5] and resolve_layers((2,), 6) == [2] and resolve_layers([-6], 6) == [0]
    for bad in ([6], [-7], [], [1, 1], [0, -6], "first", [1.0], [True], 3, None, ["0"]):
        with pytest.raises(ValueError):
            resolve_layers(bad, 6)
    assert resolve_rows("queries", 100) == 100 and resolve_rows("all", 100) == 0
    with pytest.raises(ValueError):
        resolve_rows("features", 100)


# ---- what the method refuses --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["recognition", "detection"])
def test_method_refuses_train_mode_bad_layers_and_cpu_tensors(variant):
    if variant == "detection":
        cfg = H.tiny_cfg("detection", "audio_visual", "audio_visual", False, num_class=(13, 5))
    else:
        cfg = _rec_cfg()
    sd, inp = H.synth_torch(cfg, 2, 4, 2, seed=1, dtype=torch.float32)
    m = _build_cpu(cfg, sd)
    if variant == "detection":
        def run(**kw):
            return m.attention_maps([inp["visual"], inp["audio"]], inp["times"], None, **kw)
    else:
        te = torch.zeros((2, inp["times"].shape[1], cfg.d_model))

        def run(**kw):
            return m.attention_maps([inp["visual"], inp["audio"]], te, 4, 2, **kw)
    m.train()
    with pytest.raises(ValueError, match="dropout"):
        run()
    m.eval()
    for bad in ([cfg.num_layers], "some", []):
        with pytest.raises(ValueError):
            run(layers=bad)
    with pytest.raises(ValueError):
        run(rows="features")
    with pytest.raises(L.TimHipError):
        run()
    with pytest.raises(L.TimHipError):
        run(layers="all", rows="all")


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    """the check of tests/candidate_helpers.check_entry_points for this unit (that helper also asserts the candidate units' shared
    header, which this unit has no use for): declared in the header, bound with as many arguments, exported under ABI 6, and the
    unit compiled with contraction set explicitly"""
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", code))
    assert set(NARGS) <= declared and set(NARGS) <= set(L.exported_symbols())
    for n, k in NARGS.items():
        assert len(L._SIGS[n][1]) == k, n
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, code).group(1)
        assert len(decl.split(",")) == k, n
    assert L._SIGS["timhip_stack_infer_maps_workspace_bytes"][0] is C.c_size_t
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", hdr) and L.ABI_VERSION == 6      # additive: the version stays
    lib = L.load()
    for n in NARGS:
        assert hasattr(lib, n), n
    syms = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NARGS:
        assert re.search(r"\bT %s\b" % n, syms), n
    src = open(os.path.join(ROOT, "tim_amd", "csrc", "attn_maps.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")
    assert "attn_maps.hip" in open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read()


def test_weights_entry_checks_its_arguments_before_any_launch():
    """No GPU is needed: every refusal comes back before the first launch (the pointers below are never followed)."""
    lib = L.load()
    fake, odd = C.c_void_p(0x1000), C.c_void_p(0x1002)
    d = _desc("C2a", 8, "fp16")

    def rc(desc=d, qkv=fake, s0=0, per_head=0, w=fake, ld=None):
        return lib.timhip_attention_weights(C.byref(desc) if desc is not None else None, qkv, s0, per_head, w,
                                            (desc.F + 1 if desc is not None else 1) if ld is None else ld, None)
    assert rc(desc=None) == EINVAL and rc(qkv=None) == EINVAL and rc(w=None) == EINVAL
    assert rc(desc=_desc("C2a", 8, "fp16", p_drop=0.1)) == EINVAL             # dropped weights are a mask, not a map
    assert rc(s0=-1) == EINVAL and rc(s0=d.S) == EINVAL
    assert rc(ld=d.F) == EINVAL and rc(ld=0) == EINVAL
    assert rc(w=odd) == EALIGN and rc(w=odd, per_head=1) == EALIGN
    bad = _desc("C2a", 8, "fp16")
    bad.H = 3                                                                # heads do not divide the width
    assert rc(desc=bad) == EINVAL
    wide = _desc("C2a", 8, "fp16")
    wide.F, wide.S = 193, 200                                                # past the 192 keys a head's LDS image holds
    assert rc(desc=wide) == EUNSUPPORTED


def test_stack_entry_checks_its_arguments_before_any_launch():
    lib = L.load()
    layers = (L.TimLayerParams * 2)()
    fake = C.c_void_p(0x1000)
    d = _desc("C2a", 8, "fp16")
    for tail in (0, 1):                                                       # the arena is timhip_stack_infer's, whatever is asked for
        assert lib.timhip_stack_infer_maps_workspace_bytes(C.byref(d), 6, tail) == lib.timhip_stack_infer_workspace_bytes(C.byref(d), 6, tail)
    assert lib.timhip_stack_infer_maps_workspace_bytes(None, 6, 0) == 0
    need = lib.timhip_stack_infer_maps_workspace_bytes(C.byref(d), 2, 1)
    good = (C.c_void_p * 2)(None, 0x2000)
    odd = (C.c_void_p * 2)(0x2002, None)

    def run(desc=d, maps=good, s0=None, ld=None, tail=0, nbytes=need, x_in=fake):
        return lib.timhip_stack_infer_maps(C.byref(desc), 2, layers, x_in, fake, fake, fake, tail, maps,
                                           desc.F if s0 is None else s0, desc.F + 1 if ld is None else ld, fake, nbytes, None)
    assert run(maps=None) == EINVAL
    assert run(s0=-1) == EINVAL and run(s0=d.S) == EINVAL and run(ld=d.F) == EINVAL
    assert run(maps=odd) == EALIGN
    assert run(desc=_desc("C2a", 8, "fp16", p_drop=0.1)) == EINVAL
    assert run(x_in=None) == EINVAL
    assert run(tail=1, nbytes=need - 1) == EWORKSPACE
