"""Evaluation-forward entry points of the library, as far as they go without a GPU: declarations, the arena size of
timhip_stack_infer, and the argument checks it makes before it launches anything."""
import ctypes as C
import os
import re

import pytest

from tests import helpers as H
from tim_amd import _lib as L
from tim_amd.config import named_config

HEADER = os.path.join(os.path.dirname(H.GOLDEN), "..", "include", "timhip.h")
NEW = ("timhip_stack_infer_workspace_bytes", "timhip_stack_infer", "timhip_attention_fwd_rows")
EINVAL, EWORKSPACE = -1, -3


def _desc(cname, B, prec, nq=None, p_drop=0.0, flags=0):
    cfg = named_config(cname)
    S = cfg.F + (nq if nq is not None else cfg.num_queries(15, 10))
    return L.TimDesc(B, S, cfg.F, cfg.d_model, cfg.E, cfg.nhead, cfg.FF, L.PRECISIONS[prec], p_drop, 0, 0, flags, None)


def test_header_and_binding_declare_the_inference_entry_points():
    hdr = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L._SIGS, name
    assert re.search(r"TIMHIP_EPI_GELU_T\s*=\s*14\b", code)
    assert L.EPI_GELU_T == 14
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", code) and L.ABI_VERSION == 6   # additive: the version stays
    assert L._SIGS["timhip_stack_infer_workspace_bytes"][0] is C.c_size_t
    assert len(L._SIGS["timhip_stack_infer"][1]) == 11 and len(L._SIGS["timhip_attention_fwd_rows"][1]) == 5
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("prec", sorted(L.PRECISIONS))
@pytest.mark.parametrize("cname,B,nq", [("C2a", 64, None), ("C2a", 8, None), ("C4", 16, 399), ("C4", 16, 798)])
def test_arena_is_one_layer_whatever_the_depth(cname, B, nq, prec):
    lib = L.load()
    d = _desc(cname, B, prec, nq)
    M, ts = d.B * d.S, 2 if L.PRECISIONS[prec] in L.H16 else 4
    bound = lib.timhip_layer_saved_bytes(C.byref(d)) + M * d.E * 4 + M * d.E * ts
    for tail in (0, 1):
        sizes = {lib.timhip_stack_infer_workspace_bytes(C.byref(d), n, tail) for n in (1, 6, 12)}
        assert len(sizes) == 1
        need = sizes.pop()
        assert 0 < need <= bound, (need, bound)
    full, tail = (lib.timhip_stack_infer_workspace_bytes(C.byref(d), 6, t) for t in (0, 1))
    assert full <= tail                                          # (the tail adds its gathered residual rows)
    # the training route keeps a saved block per layer and L + 1 operand row buffers: six layers of it are several arenas
    assert 6 * lib.timhip_layer_saved_bytes(C.byref(d)) >= 3 * tail


def test_arena_of_nothing_is_nothing():
    lib = L.load()
    assert lib.timhip_stack_infer_workspace_bytes(None, 6, 0) == 0
    bad = _desc("C2a", 8, "fp16")
    bad.E = 1000                                                 # not a multiple of 64: no kernels, no arena
    assert lib.timhip_stack_infer_workspace_bytes(C.byref(bad), 6, 0) == 0


def test_stack_infer_checks_its_arguments_before_any_launch():
    """No GPU is needed for these: every refusal comes back before the first launch (the pointers below are never followed)."""
    lib = L.load()
    layers = (L.TimLayerParams * 2)()
    fake = C.c_void_p(0x1000)
    d = _desc("C2a", 8, "fp16")
    need = lib.timhip_stack_infer_workspace_bytes(C.byref(d), 2, 1)

    def run(desc, nlayers=2, lay=layers, x_in=fake, x_in_T=fake, x_out=fake, x_out_T=fake, tail=0, ws=fake, nbytes=need):
        return lib.timhip_stack_infer(C.byref(desc) if desc is not None else None, nlayers, lay, x_in, x_in_T, x_out, x_out_T, tail,
                                      ws, nbytes, None)
    assert run(_desc("C2a", 8, "fp16", p_drop=0.1)) == EINVAL     # evaluation arithmetic only
    only_feats = _desc("C2a", 8, "fp16", nq=0)
    assert only_feats.S == only_feats.F
    assert run(only_feats, tail=1) == EINVAL                      # no query rows: no tail
    assert run(None) == EINVAL
    assert run(d, lay=None) == EINVAL
    assert run(d, nlayers=0) == EINVAL
    for k in ("x_in", "x_in_T", "x_out_T", "ws"):
        assert run(d, **{k: None}) == EINVAL, k
    assert run(d, tail=1, nbytes=need - 1) == EWORKSPACE
    assert run(d, nbytes=0) == EWORKSPACE
    # the row-range attention hook: same rules
    assert lib.timhip_attention_fwd_rows(None, fake, 0, fake, None) == EINVAL
    assert lib.timhip_attention_fwd_rows(C.byref(_desc("C2a", 8, "fp16", p_drop=0.1)), fake, 100, fake, None) == EINVAL
    assert lib.timhip_attention_fwd_rows(C.byref(d), None, 100, fake, None) == EINVAL
    assert lib.timhip_attention_fwd_rows(C.byref(d), fake, d.S, fake, None) == EINVAL   # s0 past the last row
    assert lib.timhip_attention_fwd_rows(C.byref(d), fake, -1, fake, None) == EINVAL


def test_attention_checks_its_descriptor_before_its_pointers():
    """timhip_attention_fwd / _bwd judge the descriptor first, then the pointers, then launch: none of the pointers below is followed"""
    lib = L.load()
    fake = C.c_void_p(0x1000)

    def fwd(d, qkv=fake):
        return lib.timhip_attention_fwd(C.byref(d), qkv, fake, fake, None)

    def bwd(d, qkv=fake):
        return lib.timhip_attention_bwd(C.byref(d), qkv, fake, fake, fake, fake, fake, 1 << 20, None)
    for prec in sorted(L.PRECISIONS):
        for flags in (0, L.DESC_ATTN_BWD_ONE_KERNEL):
            wide = _desc("C2a", 8, prec, flags=flags)
            wide.S, wide.F = 200, 193                              # more feature keys than any attention kernel holds
            late = _desc("C2a", 8, prec, flags=flags)
            late.F = late.S + 1
            ragged = _desc("C2a", 8, prec, flags=flags)
            ragged.H = 7
            assert ragged.E % ragged.H != 0
            for call in (fwd, bwd):
                assert call(wide) == L.EUNSUPPORTED, (prec, flags)
                assert call(late) == EINVAL, (prec, flags)
                assert call(ragged) == EINVAL, (prec, flags)
                assert call(_desc("C2a", 8, prec, flags=flags), qkv=None) == EINVAL, (prec, flags)
            # TIMHIP_DESC_ATTN_BWD_ONE_KERNEL is accepted and ignored: a sound descriptor of the rows + keys form (64 feature keys) with
            # a workspace of a few bytes is refused for the workspace, flag or no flag - no kernel runs without one any more
            small = _desc("C2a", 8, prec, flags=flags)
            small.F = 64
            assert lib.timhip_attention_bwd(C.byref(small), fake, fake, fake, fake, fake, fake, 16, None) == EWORKSPACE, (prec, flags)


def test_route_switch_is_read_per_call(monkeypatch):
    """`functional.encoder` picks the evaluation route from the model's mode, the grad mode and TIM_AMD_INFER - nothing cached"""
    import torch

    from tim_amd import functional as F
    taken = []
    monkeypatch.setattr(F, "_infer_forward", lambda model, *a: taken.append("infer") or (None,) * 7)
    monkeypatch.setattr(F.EncoderFn, "apply", staticmethod(lambda model, *a: taken.append("fn") or (None,) * 7))

    class M:
        training = False

        def _encoder_param_list(self):
            return []
    m = M()
    with torch.no_grad():
        F.encoder(m, 1, 0, None, None, None)
    with torch.inference_mode():
        F.encoder(m, 1, 0, None, None, None)
    F.encoder(m, 1, 0, None, None, None)                          # gradients on: somebody may differentiate it
    m.training = True
    with torch.no_grad():
        F.encoder(m, 1, 0, None, None, None)
    m.training = False
    monkeypatch.setenv("TIM_AMD_INFER", "0")
    with torch.no_grad():
        F.encoder(m, 1, 0, None, None, None)
    monkeypatch.delenv("TIM_AMD_INFER")
    with torch.no_grad():
        F.encoder(m, 1, 0, None, None, None)
    assert taken == ["infer", "infer", "fn", "fn", "fn", "infer"]
