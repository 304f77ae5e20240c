"""Query attention maps on a real MI355X: `timhip_attention_weights` elementwise against the float64 restatement
(tests/attn_maps_ref.py, pinned to the reference's own weights by tests/test_attn_maps_ref.py) evaluated on the STORED qkv - the
16-bit values widened to float64, so that the kernel's arithmetic is tested and not the storage rounding - and
`model.attention_maps` against the reference's recorded weights, the plain evaluation forward, its capture and its memory.

The kernel's bound per shape: the restatement once more in float32 numpy on the test's own inputs, its largest deviation from
float64, times 4 (another summation order, the fast exp), plus 8 fp32 ulps of 1.0.  Products of 16-bit operands are exact in
fp32; what remains is accumulation order, one exp, one divide and the head mean on values <= 1.  The measured figures:
docs/measurement_log.md."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attn_maps_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.candidate_helpers import ulp_apart  # noqa: E402
from tests.test_gpu_parity import DEV, build  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd.config import named_config  # noqa: E402
from tim_amd.functional import Runtime  # noqa: E402

ULPS8 = 8 * 2.0 ** -23          # 8 fp32 ulps of 1.0 = 9.5e-7
EINVAL, EALIGN = -1, -5

# head width, H, F, S, B - the smallest shapes that reach each branch
SHAPES = [(32, 2, 12, 26, 3),      # the tiny model; one key block
          (64, 2, 33, 70, 2),      # two key blocks; S not a multiple of 32
          (128, 8, 100, 155, 2),   # C2a's geometry
          (128, 8, 127, 160, 2),   # F + 1 = 128 ...
          (128, 8, 128, 160, 2),   # ... and 129: either side of a block edge
          (64, 2, 96, 120, 2),     # a (width, blocks) pair absent from attn_for_shape: the generic kernel
          (16, 4, 20, 40, 2),      # a head width outside the table: the generic kernel
          (32, 2, 192, 200, 1),    # the model's F limit
          # the remaining (width, key blocks) instances of attn_for_shape, one small shape each: every matrix-core instance runs
          (128, 2, 150, 170, 1),   # five key blocks: the largest LDS image and register footprint
          (128, 2, 70, 80, 1), (128, 2, 40, 64, 1), (128, 2, 20, 33, 1),
          (64, 2, 120, 130, 1), (64, 2, 20, 40, 1), (32, 2, 40, 50, 1)]
PRECS = ["fp16", "bf16", "fp32"]


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.uint8)


def desc_of(Dh, Hh, F, S, B, prec, p_drop=0.0, flags=0):
    E = Dh * Hh
    return L.TimDesc(B, S, F, E // 2, E, Hh, 4 * E, L.PRECISIONS[prec], p_drop, 0, 0, flags)


def stored(qkv_f32, prec):
    """the operand-dtype tensor the kernel reads (CPU) and its values widened to float64"""
    t = torch.from_numpy(qkv_f32).to(Runtime(prec).op_dtype)
    return t, t.to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def case(Dh, Hh, F, S, B, prec):
    """random qkv with scores of ordinary size (unit normal q and k: scale q . k ~ N(0, 1)); the float64 restatement on the stored
    values, once, shared by every test of the shape; the bound from the float32 restatement of the same inputs (CPU)"""
    rng = np.random.default_rng(1000 * Dh + 10 * F + Hh)
    t, wide = stored(rng.standard_normal((B * S, 3 * Dh * Hh)).astype(np.float32), prec)
    ph64 = R.weights(wide, B, S, F, Hh, per_head=True)
    mean64 = R.weights(wide, B, S, F, Hh)
    dev32 = max(np.abs(R.weights(wide, B, S, F, Hh, per_head=True, dtype=np.float32) - ph64).max(),
                np.abs(R.weights(wide, B, S, F, Hh, dtype=np.float32) - mean64).max())
    for a in (ph64, mean64):
        a.setflags(write=False)
    return {"qkv": t, "ph64": ph64, "mean64": mean64, "dev32": float(dev32), "bound": 4.0 * float(dev32) + ULPS8}


def run_kernel(desc, qkv_dev, s0, per_head, pad=0, guard=5):
    """-> the [B, (H,) S - s0, F + 1] weights (numpy).  The output sits between NaN-filled guard rows, with `pad` NaN-filled guard
    columns behind every row: all of them must still be NaN afterwards"""
    B, S, F, Hh = desc.B, desc.S, desc.F, desc.H
    n, ld = S - s0, F + 1 + pad
    rows = B * (Hh if per_head else 1) * n
    buf = torch.full(((rows + 2 * guard), ld), float("nan"), dtype=torch.float32, device=DEV)
    w = buf[guard:guard + rows]
    rc = L.load().timhip_attention_weights(C.byref(desc), L.ptr(qkv_dev), s0, int(per_head), L.ptr(w), ld, st())
    torch.cuda.synchronize()
    assert rc == 0, rc
    out = buf.cpu().numpy()
    assert np.isnan(out[:guard]).all() and np.isnan(out[guard + rows:]).all(), "guard rows written"
    assert np.isnan(out[guard:guard + rows, F + 1:]).all(), "guard columns written"
    body = out[guard:guard + rows, :F + 1]
    return body.reshape((B, Hh, n, F + 1) if per_head else (B, n, F + 1))


def head_mean(ph):
    """the kernel's own mean of the per-head form: fp32 sum in ascending head order, times 1 / H"""
    acc = np.zeros(ph.shape[:1] + ph.shape[2:], dtype=np.float32)
    for h in range(ph.shape[1]):
        acc += ph[:, h]
    return acc * (np.float32(1.0) / np.float32(ph.shape[1]))


# ---- the kernel against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,S,B", SHAPES)
def test_weights_match_the_restatement_on_the_stored_qkv(Dh, Hh, F, S, B, prec):
    c = case(Dh, Hh, F, S, B, prec)
    bound = c["bound"]
    desc = desc_of(Dh, Hh, F, S, B, prec)
    qkv = c["qkv"].to(DEV)
    worst = 0.0
    for s0 in (0, F, F + 3):                                   # (the last: not a multiple of 32)
        want_m, want_h = c["mean64"][:, s0:], c["ph64"][:, :, s0:]
        for pad in (0, 7):                                     # ld = F + 1, and a padded pitch
            mean = run_kernel(desc, qkv, s0, False, pad)
            ph = run_kernel(desc, qkv, s0, True, pad)
            for got, want in ((mean, want_m), (ph, want_h)):
                assert got.dtype == np.float32 and not np.isnan(got).any()
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                assert err <= bound, (s0, pad, err, bound)
                assert float(np.abs(got.sum(-1, dtype=np.float64) - 1.0).max()) <= bound * (F + 1)
                if s0 < F:
                    assert np.all(got[..., :F - s0, F] == 0.0) and not np.signbit(got[..., :F - s0, F]).any()
            assert int(ulp_apart(head_mean(ph), mean).max()) <= 2
    print("ATTNMAP kernel Dh=%d H=%d F=%d S=%d B=%d %s: float32-numpy deviation %.3g, bound %.3g, GPU max abs error %.3g"
          % (Dh, Hh, F, S, B, prec, c["dev32"], bound, worst))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,S", [(32, 2, 12, 26), (64, 2, 33, 70), (64, 2, 96, 120), (128, 8, 100, 155)])
def test_edge_inputs(Dh, Hh, F, S, prec):
    E, B = Dh * Hh, 1
    desc = desc_of(Dh, Hh, F, S, B, prec)
    dt = Runtime(prec).op_dtype
    rng = np.random.default_rng(3)
    # q = 0: every score is 0 and every weight of a row the same value.  H = 2: the head mean v + v is exact, the weights ARE
    # 1 / (F + 1) as fp32 computes it; at H = 8 the fixed-order sum v, 2v, 3v, .. rounds at 3v, 5v, 6v, 7v (a 24-bit mantissa
    # times 3 needs 26 bits), so there the weights are all equal and within 2 ulps of it
    qkv = rng.standard_normal((B * S, 3 * E)).astype(np.float32)
    qkv[:, :E] = 0.0
    w = run_kernel(desc, torch.from_numpy(qkv).to(dt).to(DEV), 0, False)
    vq, vf = np.float32(1.0) / np.float32(F + 1), np.float32(1.0) / np.float32(F)
    assert np.all(w[:, F:] == w[0, F, 0]) and np.all(w[:, :F, :F] == w[0, 0, 0]) and np.all(w[:, :F, F] == 0.0)
    if Hh == 2:
        assert w[0, F, 0] == vq and w[0, 0, 0] == vf
    else:
        assert int(ulp_apart(w[0, F, 0], vq).max()) <= 2 and int(ulp_apart(w[0, 0, 0], vf).max()) <= 2
    # one key's score far above the rest (scale * Dh * c^2 >= 90 against 0): that weight is 1.0, the others underflow to 0
    c = 4.5 if Dh >= 32 else 6.0
    j0 = F // 2
    assert c * c * Dh / np.sqrt(Dh) >= 90.0
    qkv = np.zeros((B * S, 3 * E), dtype=np.float32)
    qkv[:, :E] = c
    qkv[j0, E:2 * E] = c
    w = run_kernel(desc, torch.from_numpy(qkv).to(dt).to(DEV), 0, False)
    assert not np.isnan(w).any()
    assert np.all(w[:, :, j0] == 1.0) and np.all(np.delete(w, j0, axis=-1) == 0.0)
    # scores all <= -60 before the max subtraction: no NaNs, the (equal) scores give the uniform row
    qkv[:, E:2 * E] = -c
    w = run_kernel(desc, torch.from_numpy(qkv).to(dt).to(DEV), 0, False)
    assert np.isfinite(w).all()
    assert np.abs(w[:, F:] - vq).max() <= ULPS8 and np.abs(w[:, :F, :F] - vf).max() <= ULPS8 and np.all(w[:, :F, F] == 0.0)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Dh,Hh,F,S", [(128, 8, 100, 155), (32, 2, 12, 26), (16, 4, 20, 40)])
def test_a_window_gives_the_same_bits_alone_in_a_batch_and_on_every_run(Dh, Hh, F, S, prec):
    c = case(Dh, Hh, F, S, 3, prec) if (Dh, Hh, F, S, 3) in SHAPES else None
    E = Dh * Hh
    t = c["qkv"] if c else stored(np.random.default_rng(5).standard_normal((3 * S, 3 * E)).astype(np.float32), prec)[0]
    batch, alone = t.to(DEV), t[S:2 * S].contiguous().to(DEV)
    for s0 in (0, F):
        for per_head in (False, True):
            a = run_kernel(desc_of(Dh, Hh, F, S, 3, prec), batch, s0, per_head)
            b = run_kernel(desc_of(Dh, Hh, F, S, 3, prec), batch, s0, per_head)
            one = run_kernel(desc_of(Dh, Hh, F, S, 1, prec), alone, s0, per_head)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.array_equal(a[1].view(np.uint32), one[0].view(np.uint32))
    # rows s0 .. S - 1 of the full map, whatever s0: a row's arithmetic does not depend on where the grid starts
    full = run_kernel(desc_of(Dh, Hh, F, S, 3, prec), batch, 0, False)
    for s0 in (F, F + 3):
        assert np.array_equal(run_kernel(desc_of(Dh, Hh, F, S, 3, prec), batch, s0, False).view(np.uint32), full[:, s0:].view(np.uint32))


def test_the_fp32_switch_selects_the_generic_kernel():
    """TIMHIP_DESC_ATTN_FP32 sends a matrix-core shape through the generic kernel: within the same bound, other bits"""
    Dh, Hh, F, S, B = 128, 8, 100, 155, 2
    c = case(Dh, Hh, F, S, B, "fp16")
    qkv = c["qkv"].to(DEV)
    mfma = run_kernel(desc_of(Dh, Hh, F, S, B, "fp16"), qkv, 0, False)
    plain = run_kernel(desc_of(Dh, Hh, F, S, B, "fp16", flags=1), qkv, 0, False)
    assert float(np.abs(plain - c["mean64"]).max()) <= c["bound"]
    assert not np.array_equal(mfma.view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_per_head_weights_reproduce_the_forwards_output(prec):
    """P . V per head from the per-head weights against timhip_attention_fwd's o on the same qkv (head width 128, F = 100): within
    the operand dtype's rounding of o - half an ulp of the 16-bit format at |o|max - plus the kernel bound x (F + 1) x |v|max"""
    Dh, Hh, F, S, B = 128, 8, 100, 155, 2
    E = Dh * Hh
    c = case(Dh, Hh, F, S, B, prec)
    desc = desc_of(Dh, Hh, F, S, B, prec)
    qkv = c["qkv"].to(DEV)
    o = torch.zeros((B * S, E), dtype=qkv.dtype, device=DEV)
    L.call("timhip_attention_fwd", C.byref(desc), L.ptr(qkv), L.ptr(o), None, st())
    P = run_kernel(desc, qkv, 0, True).astype(np.float64)                       # [B, H, S, F + 1]
    v = c["qkv"].to(torch.float64).numpy().reshape(B, S, 3, Hh, Dh)[:, :, 2]      # [B, S, H, Dh]
    want = np.einsum("bhsj,bjhd->bshd", P[..., :F], v[:, :F]) + P[..., F].transpose(0, 2, 1)[..., None] * v
    got = o.to(torch.float64).cpu().numpy().reshape(B, S, Hh, Dh)
    omax, vmax = float(np.abs(want).max()), float(np.abs(v).max())
    mant = 10 if prec == "fp16" else 7
    half_ulp = 0.5 * 2.0 ** (np.floor(np.log2(omax)) - mant)
    tol = half_ulp + c["bound"] * (F + 1) * vmax
    err = float(np.abs(got - want).max())
    print("ATTNMAP forward consistency %s: |P V - o| max %.3g, tolerance %.3g (|o|max %.3g, |v|max %.3g)" % (prec, err, tol, omax, vmax))
    assert err <= tol, (err, tol)


def test_refusals_return_their_code_and_write_nothing():
    Dh, Hh, F, S, B = 32, 2, 12, 26, 2
    lib = L.load()
    qkv = torch.zeros((B * S, 3 * Dh * Hh), dtype=torch.float16, device=DEV)
    buf = torch.full((B * S * (F + 1) + 4,), float("nan"), dtype=torch.float32, device=DEV)
    d = desc_of(Dh, Hh, F, S, B, "fp16")

    def rc(desc, q, s0, w, ld, per_head=0):
        return lib.timhip_attention_weights(C.byref(desc) if desc is not None else None, q, s0, per_head, w, ld, st())
    assert rc(None, L.ptr(qkv), 0, L.ptr(buf), F + 1) == EINVAL
    assert rc(d, None, 0, L.ptr(buf), F + 1) == EINVAL
    assert rc(d, L.ptr(qkv), 0, None, F + 1) == EINVAL
    assert rc(desc_of(Dh, Hh, F, S, B, "fp16", p_drop=0.1), L.ptr(qkv), 0, L.ptr(buf), F + 1) == EINVAL
    assert rc(d, L.ptr(qkv), -1, L.ptr(buf), F + 1) == EINVAL
    assert rc(d, L.ptr(qkv), S, L.ptr(buf), F + 1) == EINVAL
    assert rc(d, L.ptr(qkv), 0, L.ptr(buf), F) == EINVAL
    assert rc(d, L.ptr(qkv), 0, L.ptr(buf) + 2, F + 1) == EALIGN
    assert rc(d, L.ptr(qkv), 0, L.ptr(buf) + 2, F + 1, per_head=1) == EALIGN
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    assert rc(d, L.ptr(qkv), S - 1, L.ptr(buf), F + 1) == 0     # (the last row alone is a valid request)
    torch.cuda.synchronize()
    assert int((~torch.isnan(buf)).sum()) == B * (F + 1)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _model_and_inputs(cfg, prec, B, nv, na, seed):
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=seed, dtype=torch.float32)
    return build(cfg, prec, sd), {k: v.to(DEV) for k, v in inp.items()}


def _maps(m, inp, nv, na, **kw):
    """(flat tuple of the outputs, maps) of one attention_maps call"""
    if m.cfg.variant == "detection":
        outs, maps = m.attention_maps([inp["visual"], inp["audio"]], inp["times"], None, **kw)
        flat = tuple(outs[0][0]) + tuple(outs[0][1]) + (outs[0][2],)
    else:
        with torch.no_grad():
            te = m(inp["times"], "time_mlp")
        (cls, feats), maps = m.attention_maps([inp["visual"], inp["audio"]], te, nv, na, **kw)
        flat = tuple(cls) + (feats,)
    return flat, maps


def _plain(m, inp, nv, na):
    with torch.no_grad():
        if m.cfg.variant == "detection":
            outs = m([inp["visual"], inp["audio"]], "encoder", inp["times"], None, label_queries=False)
            return tuple(outs[0][0]) + tuple(outs[0][1]) + (outs[0][2],)
        cls, feats = m([inp["visual"], inp["audio"]], "encoder", m(inp["times"], "time_mlp"), nv, na)
        return tuple(cls) + (feats,)


def _same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and torch.equal(bits(x), bits(y))


# the project's bounds on the tiny configs' logits against the fp32 reference, per mode (tests/test_gpu_parity.py: TOL_FP32; the
# fp16 mode's 1e-3; the bf16 kernels' 3e-2 against the fp32 reference) - the weights are <= 1 and sit no deeper than the logits
MODEL_BOUND = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 3e-2}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", R.FIXTURES)
def test_model_maps_match_the_references_recorded_weights(name, prec):
    z, cfg = R.load_fixture(name)
    B, nv, na, Bw, S, F = (int(z[k]) for k in ("B", "nv", "na", "windows", "S", "F"))
    m, inp = _model_and_inputs(cfg, prec, B, nv, na, int(z["seed"]))
    _, maps = _maps(m, inp, nv, na, layers="all", rows="all")
    torch.cuda.synchronize()
    assert maps.layers == list(range(cfg.num_layers)) and (maps.F, maps.S, maps.s0) == (F, S, 0)
    for l in maps.layers:
        w = maps.weights[l]
        assert w.dtype == torch.float32 and tuple(w.shape) == (B, S, F + 1)
        dense = maps.to_dense(l).cpu().numpy()[:Bw]
        want = z["attn/layer%d" % l]
        err = float(np.abs(dense - want).max())
        print("ATTNMAP model %s %s layer %d: max abs error against the reference %.3g (bound %.3g)" % (name, prec, l, err, MODEL_BOUND[prec]))
        assert err <= MODEL_BOUND[prec], (l, err)
        assert np.array_equal(dense != 0, want != 0)           # exactly the reference's zero pattern


@pytest.mark.parametrize("eval_feats", [True, False])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_outputs_are_the_plain_forwards_and_rows_and_layers_select(prec, eval_feats):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na = 3, 4, 2
    m, inp = _model_and_inputs(cfg, prec, B, nv, na, 1)
    m.eval_feats = eval_feats
    plain = _plain(m, inp, nv, na)
    outs_all, all_ = _maps(m, inp, nv, na, layers="all", rows="all")
    outs_q, q = _maps(m, inp, nv, na, layers="all", rows="queries")
    outs_last, last = _maps(m, inp, nv, na)                     # layers="last", rows="queries"
    _, picked = _maps(m, inp, nv, na, layers=[-1, 0], rows="queries")
    torch.cuda.synchronize()
    for o in (outs_all, outs_q, outs_last):
        _same_bits(o, plain)
    assert (plain[-1] is None) == (not eval_feats)
    F, S = cfg.F, all_.S
    assert q.s0 == F and last.layers == [cfg.num_layers - 1] and picked.layers == [0, cfg.num_layers - 1]
    for l in all_.layers:
        assert torch.equal(bits(q.weights[l]), bits(all_.weights[l][:, F:]))
        assert torch.equal(bits(picked.weights[l]), bits(q.weights[l])) if l in picked.layers else True
    assert torch.equal(bits(last.weights[cfg.num_layers - 1]), bits(q.weights[cfg.num_layers - 1]))
    # the rows of a head: the EncoderPlan's ranges; the modality halves of the feature columns
    plan = m._plan(inp["times"].shape[1], nv, na)
    for slot, _, start, n in plan.heads:
        assert torch.equal(last.for_head(slot), all_.weights[cfg.num_layers - 1][:, start:start + n])
    vis, aud = last.split_modalities()
    assert vis.shape[-1] == aud.shape[-1] == cfg.num_feats and torch.equal(torch.cat([vis, aud], -1), last.weights[last.layers[0]][..., :F])
    assert tuple(last.to_dense().shape) == (B, S - F, S)


def test_c2a_outputs_are_the_plain_forwards():
    cfg, (B, nv, na) = named_config("C2a"), (2, 15, 10)
    m, inp = _model_and_inputs(cfg, "fp16", B, nv, na, 2)
    for eval_feats in (True, False):
        m.eval_feats = eval_feats
        plain = _plain(m, inp, nv, na)
        outs, maps = _maps(m, inp, nv, na, layers="all")
        torch.cuda.synchronize()
        _same_bits(outs, plain)
        for l in maps.layers:
            w = maps.weights[l]
            assert tuple(w.shape) == (B, nv * 3 + na, cfg.F + 1) and bool(torch.isfinite(w).all())
            assert float((w.sum(-1) - 1.0).abs().max()) <= 1e-5


def test_detection_maps_cover_every_query_of_the_pyramid():
    cfg = H.tiny_cfg("detection", "audio_visual", "audio_visual", False, num_class=(13, 5))
    B = 2
    m, inp = _model_and_inputs(cfg, "fp16", B, 0, 0, 3)
    plain = _plain(m, inp, 0, 0)
    outs, maps = _maps(m, inp, 0, 0, layers="all", rows="queries")
    torch.cuda.synchronize()
    _same_bits(outs, plain)
    nq_total = 2 * m.num_queries                                # the visual and the audio pyramid
    for l in maps.layers:
        assert tuple(maps.weights[l].shape) == (B, nq_total, cfg.F + 1)
    assert tuple(maps.for_head("action").shape) == (B, m.num_queries, cfg.F + 1)
    assert tuple(maps.for_head("audio").shape) == (B, m.num_queries, cfg.F + 1)


def test_capture_replays_onto_new_inputs_with_the_eager_maps():
    cfg, (B, nv, na) = named_config("C2a"), (2, 15, 10)
    m, inp = _model_and_inputs(cfg, "fp16", B, nv, na, 2)
    _, inp2 = _model_and_inputs(cfg, "fp16", B, nv, na, 7)
    static = {k: v.clone() for k, v in inp.items()}
    for _ in range(2):                                          # warm-up: operand copies, the arena, the row table
        _, held = _maps(m, static, nv, na, layers="all")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, cmaps = _maps(m, static, nv, na, layers="all", out=held)     # the map buffers exist before the capture
    for k in static:
        static[k].copy_(inp2[k])
    graph.replay()
    torch.cuda.synchronize()
    assert all(cmaps.weights[l].data_ptr() == held.weights[l].data_ptr() for l in held.layers)
    replayed = {l: cmaps.weights[l].clone() for l in cmaps.layers}
    rep_outs = tuple(None if t is None else t.clone() for t in captured)
    eager_outs, eager = _maps(m, inp2, nv, na, layers="all")
    _, first = _maps(m, inp, nv, na, layers="all")
    torch.cuda.synchronize()
    _same_bits(rep_outs, eager_outs)
    for l in eager.layers:
        assert torch.equal(bits(replayed[l]), bits(eager.weights[l]))
        assert not torch.equal(first.weights[l], eager.weights[l])


def test_maps_of_all_layers_add_their_buffers_and_nothing_else_to_the_peak():
    """C2a at 8 windows: the peak of attention_maps(layers="all") exceeds the plain evaluation forward's by at most the map buffers
    plus 1 MB - the arena does not grow with the number of layers asked for"""
    cfg, (B, nv, na) = named_config("C2a"), (8, 15, 10)
    m, inp = _model_and_inputs(cfg, "fp16", B, nv, na, 2)

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
    plain = peak(lambda: _plain(m, inp, nv, na))
    with_maps = peak(lambda: _maps(m, inp, nv, na, layers="all"))
    map_bytes = cfg.num_layers * B * (nv * 3 + na) * (cfg.F + 1) * 4
    print("ATTNMAP memory C2a B=8: plain forward peak %d, with all maps %d, map buffers %d" % (plain, with_maps, map_bytes))
    assert with_maps <= plain + map_bytes + (1 << 20), (plain, with_maps, map_bytes)
