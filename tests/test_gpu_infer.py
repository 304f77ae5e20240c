"""The evaluation forward (`model.eval()` under no-grad) on a real MI355X: its two kernels against the kernels they derive from,
bit for bit; the route against the training route's evaluation forward, bit for bit with `feats` and within the precision
mode's tolerance without; its memory, its dispatch and its capture as one linear graph."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tim_oracle as O  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_parity import DEV, amax, build, maxerr  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.functional import Runtime  # noqa: E402


def st():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def bits(t):
    return t.contiguous().view(torch.uint8)


# ---- kernel (a): linear1's store-only epilogue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("M,p8", [(9920, "1"), (1240, "1"), (37 * 155, "1"), (9920, "0"), (5120, "0")])
def test_gelu_store_epilogue_is_the_training_epilogue_without_its_second_store(prec, M, p8, knobs):
    """TIMHIP_EPI_GELU_T against TIMHIP_EPI_GELU_DROP_G2 at p_drop = 0 on the layer's linear1 shape [M, 1024] x [2048, 1024]^T:
    out0 bit for bit.  Both take the same kernel for a shape: 64 windows the eight-phase kernel, 8 windows the small-problem
    kernel, the ragged 37 windows the two-blocks-per-CU kernel; with the eight-phase kernel switched off, the tile-walking
    (M = 9920) and the one-tile (M = 5120) loader-wave kernels"""
    knobs(TIMHIP_GEMM_P8=p8)
    rt = Runtime(prec)
    N, K = 2048, 1024
    A = rnd(M, K, seed=1).to(DEV).to(rt.op_dtype)
    W = rnd(N, K, seed=2, scale=K ** -0.5).to(DEV).to(rt.op_dtype)
    bias = rnd(N, seed=3).to(DEV)
    h_ref = torch.empty((M, N), dtype=rt.op_dtype, device=DEV)
    u = torch.empty((M, N), dtype=rt.op_dtype, device=DEV)
    h = torch.full((M, N), 7.0, dtype=rt.op_dtype, device=DEV)
    rt.gemm(L.EPI_GELU_DROP_G2, A, W, M, N, K, h_ref, N, out1=u, ld1=N, bias=bias)
    rt.gemm(L.EPI_GELU_T, A, W, M, N, K, h, N, bias=bias)
    torch.cuda.synchronize()
    assert torch.equal(bits(h), bits(h_ref))
    want = torch.nn.functional.gelu(A.float() @ W.float().t() + bias)
    assert maxerr(h.float().cpu(), want.cpu()) <= {"fp32": 1e-4, "bf16": 4e-2, "fp16": 5e-3}[prec] * max(1.0, amax(want))
    assert L.load().timhip_gemm_p8_choice(L.EPI_GELU_T, M, N, K) == L.load().timhip_gemm_p8_choice(L.EPI_GELU_DROP_G2, M, N, K)


# ---- kernel (b): attention over a row range ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32", "bf16x3"])
@pytest.mark.parametrize("B,S,F,H,Dh,s0", [(3, 155, 100, 8, 128, 100), (2, 898, 100, 8, 128, 100), (2, 155, 100, 2, 128, 0),
                                           (4, 80, 50, 2, 128, 50), (2, 155, 100, 2, 128, 37), (2, 40, 12, 2, 32, 12),
                                           (2, 30, 12, 3, 16, 12)])   # the last: no matrix-core instance, the plain kernel
def test_attention_rows_are_the_full_kernels_rows(prec, B, S, F, H, Dh, s0):
    rt = Runtime(prec)
    E = H * Dh
    qkv = rnd(B * S, 3 * E, seed=5).to(DEV).to(rt.op_dtype)
    desc = L.TimDesc(B, S, F, E // 2, E, H, 4 * E, rt.prec, 0.0, 0, 0, 0)
    o = torch.zeros((B * S, E), dtype=rt.op_dtype, device=DEV)
    lse = torch.empty((B, H, S), device=DEV)
    L.call("timhip_attention_fwd", C.byref(desc), L.ptr(qkv), L.ptr(o), L.ptr(lse), st())
    n = S - s0
    guard = 64                                                    # rows in front of and behind the output: nothing may land there
    buf = torch.full((B * n + 2 * guard, E), -3.0, dtype=rt.op_dtype, device=DEV)
    o_rows = buf[guard:guard + B * n]
    L.call("timhip_attention_fwd_rows", C.byref(desc), L.ptr(qkv), s0, L.ptr(o_rows), st())
    o_nolse = torch.zeros_like(o)
    L.call("timhip_attention_fwd", C.byref(desc), L.ptr(qkv), L.ptr(o_nolse), None, st())
    torch.cuda.synchronize()
    assert torch.equal(bits(o_rows.view(B, n, E)), bits(o.view(B, S, E)[:, s0:]))
    assert bool((buf[:guard] == -3.0).all()) and bool((buf[guard + B * n:] == -3.0).all())
    assert torch.equal(bits(o_nolse), bits(o))


# ---- the route ----------------------------------------------------------------------------------------------------------------
def _rec_inputs(cfg, B, nv, na, seed):
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=seed, dtype=torch.float32)
    return sd, {k: v.to(DEV) for k, v in inp.items()}


def _forward(m, inp, nv, na):
    """all OUT_SLOTS of one evaluation forward as a dict (detection: through forward_inference with its own query pyramid)"""
    if m.cfg.variant == "detection":
        (cls, reg, feats), _, _, _, _ = m([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)
    else:
        cls, feats = m([inp["visual"], inp["audio"]], "encoder", m(inp["times"], "time_mlp"), nv, na)
        reg = (None, None)
    return dict(zip(F.OUT_SLOTS, tuple(cls) + (feats,) + tuple(reg)))


def _both_routes(m, inp, nv, na, monkeypatch):
    with torch.no_grad():
        monkeypatch.setenv("TIM_AMD_INFER", "0")
        old = _forward(m, inp, nv, na)
        monkeypatch.setenv("TIM_AMD_INFER", "1")
        new = _forward(m, inp, nv, na)
    torch.cuda.synchronize()
    return old, new


def _assert_same_bits(old, new):
    assert set(old) == set(new) == set(F.OUT_SLOTS)
    for k in F.OUT_SLOTS:
        assert (old[k] is None) == (new[k] is None), k
        if old[k] is not None:
            assert old[k].shape == new[k].shape and old[k].grad_fn is None and new[k].grad_fn is None, k
            assert torch.equal(bits(old[k]), bits(new[k])), (k, maxerr(old[k].cpu(), new[k].cpu()))


TINY = [("recognition", im, dm, vn, nv, na) for _, im, dm, vn, nv, na in H.rec_golden_cases()] + \
       [("detection", im, dm, nc, 0, 0) for im, dm, nc, _ in H.DET_CASES]


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("variant,im,dm,vn,nv,na", TINY)
def test_tiny_route_equals_the_training_routes_evaluation(variant, im, dm, vn, nv, na, prec, monkeypatch):
    if variant == "detection":
        cfg = H.tiny_cfg("detection", im, dm, isinstance(vn[0], list), num_class=vn)
    else:
        cfg = H.tiny_cfg("recognition", im, dm, vn)
    sd, inp = _rec_inputs(cfg, 3, nv, na, seed=1)
    m = build(cfg, prec, sd)
    assert m.eval_feats is True
    old, new = _both_routes(m, inp, nv, na, monkeypatch)
    _assert_same_bits(old, new)
    assert new["feats"] is not None
    # without feats: the heads' outputs within the mode's tolerance, from the query rows alone
    m.eval_feats = False
    with torch.no_grad():
        tail = _forward(m, inp, nv, na)
    torch.cuda.synchronize()
    _assert_close_without_feats(new, tail, prec)


def _assert_close_without_feats(full, tail, prec):
    assert tail["feats"] is None
    rel = {"fp32": 1e-5, "bf16x3": 5e-5, "bf16": 3e-2, "fp16": 1e-3}[prec]
    for k in F.OUT_SLOTS:
        if k == "feats":
            continue
        assert (full[k] is None) == (tail[k] is None), k
        if full[k] is not None:
            assert full[k].shape == tail[k].shape, k
            bound = (2e-2 if prec == "bf16" else rel) if k.startswith("reg_") else rel * max(1.0, amax(full[k]))
            assert maxerr(tail[k].cpu(), full[k].cpu()) <= bound, (k, maxerr(tail[k].cpu(), full[k].cpu()), bound)


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_c2a_eight_windows_route(prec, monkeypatch):
    """the published validation batch: 8 windows per GPU.  Bit for bit with feats; fp16 logits within 1e-3 of the fp32 oracle"""
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    sd, inp = _rec_inputs(cfg, B, nv, na, seed=2)
    m = build(cfg, prec, sd)
    old, new = _both_routes(m, inp, nv, na, monkeypatch)
    _assert_same_bits(old, new)
    m.eval_feats = False
    with torch.no_grad():
        tail = _forward(m, inp, nv, na)
    torch.cuda.synchronize()
    _assert_close_without_feats(new, tail, prec)
    if prec == "fp16":
        with torch.no_grad():
            ref_cls, _ = O.forward(sd, cfg, inp["visual"].cpu(), inp["audio"].cpu(), inp["times"].cpu(), nv, na)
        for route in (new, tail):
            for k, b in zip(("verb", "noun", "action", "audio"), ref_cls):
                assert maxerr(route[k].cpu(), b) <= 1e-3, (k, maxerr(route[k].cpu(), b))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_c4_detection_inference_form_without_feats(prec, monkeypatch):
    """C4 as forward_inference runs it: 100 feature tokens + 399 dense queries per window"""
    cfg = named_config("C4")
    sd, inp = _rec_inputs(cfg, 4, 0, 0, seed=4)
    m = build(cfg, prec, sd)
    old, new = _both_routes(m, inp, 0, 0, monkeypatch)
    _assert_same_bits(old, new)
    assert new["action"].shape[0] == 4 * 399 and new["reg_visual"].shape == (4 * 399, 2)
    m.eval_feats = False
    with torch.no_grad():
        tail = _forward(m, inp, 0, 0)
    torch.cuda.synchronize()
    _assert_close_without_feats(new, tail, prec)


# ---- memory -------------------------------------------------------------------------------------------------------------------
def _peak_of_one_forward(cfg, sd, inp, nv, na):
    """peak allocated bytes of one warmed-up forward, counted from the level before the model existed (what other tests of the
    process still hold is not this route's): parameters, operand copies, cached workspaces and everything the forward allocates"""
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    m = build(cfg, "fp16", sd)
    with torch.no_grad():
        for _ in range(2):
            _forward(m, inp, nv, na)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        _forward(m, inp, nv, na)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del m
    gc.collect()
    torch.cuda.empty_cache()
    return peak


def test_c2a_production_batch_forward_holds_one_arena(monkeypatch):
    cfg, (B, nv, na) = named_config("C2a"), (64, 15, 10)
    sd, inp = _rec_inputs(cfg, B, nv, na, seed=2)
    torch.cuda.empty_cache()
    monkeypatch.setenv("TIM_AMD_INFER", "0")
    old = _peak_of_one_forward(cfg, sd, inp, nv, na)
    monkeypatch.setenv("TIM_AMD_INFER", "1")
    new = _peak_of_one_forward(cfg, sd, inp, nv, na)
    print("peak allocated bytes of one C2a forward at 64 windows: training route %d, evaluation route %d" % (old, new))
    assert 2 * new <= old, (new, old)


# ---- dispatch -----------------------------------------------------------------------------------------------------------------
def test_dispatch_follows_the_models_mode_and_the_grad_mode(monkeypatch):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na = 3, 4, 2
    sd, inp = _rec_inputs(cfg, B, nv, na, seed=1)
    m = build(cfg, "fp32", sd)
    taken = []
    real = F._infer_forward
    monkeypatch.setattr(F, "_infer_forward", lambda *a: (taken.append(1), real(*a))[1])
    with torch.no_grad():
        a = _forward(m, inp, nv, na)
    with torch.inference_mode():
        b = _forward(m, inp, nv, na)
    assert len(taken) == 2
    _assert_same_bits(a, b)
    # gradients on: the autograd Function, outputs carry a grad_fn and the backward is the one the parity tests pin
    g = _forward(m, inp, nv, na)
    assert len(taken) == 2 and g["action"].grad_fn is not None and g["feats"].grad_fn is not None
    for k in F.OUT_SLOTS:
        if a[k] is not None:
            assert torch.equal(bits(g[k].detach()), bits(a[k])), k
    sum(v.square().sum() for v in g.values() if v is not None).backward()
    ref = build(cfg, "fp32", sd)
    monkeypatch.setenv("TIM_AMD_INFER", "0")
    r = _forward(ref, inp, nv, na)
    sum(v.square().sum() for v in r.values() if v is not None).backward()
    monkeypatch.delenv("TIM_AMD_INFER")
    for (k, p), (_, pr) in zip(m.named_parameters(), ref.named_parameters()):
        assert (p.grad is None) == (pr.grad is None), k
        if p.grad is not None:   # (two passes of one backward: the accumulated sums differ in their last bits at most)
            assert maxerr(p.grad.cpu(), pr.grad.cpu()) <= 1e-5 * max(1.0, amax(pr.grad)), k
    m.train()
    with torch.no_grad():
        t = _forward(m, inp, nv, na)
    assert len(taken) == 2 and t["action"] is not None        # train mode (dropout on): never the evaluation route
    m.eval()


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_an_optimizer_step_between_two_evaluations_is_seen(prec):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na = 3, 4, 2
    sd, inp = _rec_inputs(cfg, B, nv, na, seed=1)
    m = build(cfg, prec, sd)
    with torch.no_grad():
        before = _forward(m, inp, nv, na)
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    out = _forward(m, inp, nv, na)
    sum(v.square().sum() for v in out.values() if v is not None).backward()
    opt.step()
    m.eval()
    with torch.no_grad():
        after = _forward(m, inp, nv, na)
        again = _forward(m, inp, nv, na)
    torch.cuda.synchronize()
    assert not torch.equal(before["action"], after["action"]) and not torch.equal(before["feats"], after["feats"])
    _assert_same_bits(after, again)
    fresh = build(cfg, prec, {k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        _assert_same_bits(after, _forward(fresh, inp, nv, na))


# ---- graph ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eval_feats", [True, False])
def test_route_is_captured_as_one_graph_and_replays_on_new_inputs(eval_feats):
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    sd, inp = _rec_inputs(cfg, B, nv, na, seed=2)
    _, inp2 = _rec_inputs(cfg, B, nv, na, seed=7)
    m = build(cfg, "fp16", sd)
    m.eval_feats = eval_feats
    static = {k: v.clone() for k, v in inp.items()}
    with torch.no_grad():
        for _ in range(2):                                        # warm-up: operand copies, the arena, the row table
            _forward(m, static, nv, na)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = _forward(m, static, nv, na)
        for k in static:
            static[k].copy_(inp2[k])
        graph.replay()
        torch.cuda.synchronize()
        replayed = {k: (None if v is None else v.clone()) for k, v in captured.items()}
        eager = _forward(m, inp2, nv, na)
        first = _forward(m, inp, nv, na)
    torch.cuda.synchronize()
    _assert_same_bits(eager, replayed)
    assert not torch.equal(first["action"], eager["action"])
    assert (replayed["feats"] is None) == (not eval_feats)
