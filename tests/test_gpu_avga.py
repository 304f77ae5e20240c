"""AVGA pooling on the device (tim_amd/csrc/avga.hip) against the float64 restatement and its rounding model
(tests/avga_ref.py): the C ABI at the smallest shapes at which the kernels can go wrong, the edges, the error codes, and the
route through `TIM(pool_features=True)`, a captured step and `model.pool.attention_map`.

Bounds, relative to the largest |element| of the reference tensor of the case:
  fp32          forward 1e-5 * max(1, m) (m: the test's own amplification of z), gradients 1e-4 - the project's fp32 figures
  fp16 / bf16   2 * err(rounding model vs float64) + 1e-5, the model's error computed here on the same inputs
Every figure is printed before it is asserted (pytest -s shows them; docs/measurement_log.md records a run)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.avga_ref import PARAMS, avga_f64, avga_rounded

pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PRECS = ("fp32", "fp16", "bf16")


def _ru(x, m=64):
    return (x + m - 1) // m * m


def make_case(R, S, Cv, Ca, seed, bias_video=0.1, wh_mult=1.0, zero=False):
    """|randn| cells (post-ReLU maps are non-negative), randn audio, Xavier weights as the module initialises them"""
    g = torch.Generator().manual_seed(seed)

    def xavier(n, k):
        b = (6.0 / (n + k)) ** 0.5
        return (torch.rand(n, k, generator=g, dtype=torch.float64) * 2 - 1) * b
    P = {"affine_video.weight": xavier(Cv, Cv), "affine_video.bias": torch.randn(Cv, generator=g, dtype=torch.float64) * 0.1 + bias_video,
         "affine_audio.weight": xavier(Cv, Ca), "affine_audio.bias": torch.randn(Cv, generator=g, dtype=torch.float64) * 0.1,
         "affine_v.weight": xavier(S, Cv), "affine_g.weight": xavier(S, Cv), "affine_h.weight": xavier(1, S) * wh_mult}
    video = torch.randn(R, S, Cv, generator=g, dtype=torch.float64).abs()
    audio = torch.randn(R, Ca, generator=g, dtype=torch.float64)
    if zero:
        video.zero_(); audio.zero_(); P["affine_audio.bias"].zero_()
    P = {k: v.float().double() for k, v in P.items()}          # the values the device holds in fp32
    return P, audio.float().double(), video.float().double(), torch.randn(R, Cv, generator=g, dtype=torch.float64).float().double()


def _copy(w, dt, transposed=False):
    """operand copy as Runtime.weight makes it: [N, ru(K)] (or the transposed [K, ru(N)]), zero padded"""
    w = w.t() if transposed else w
    out = torch.zeros((w.shape[0], _ru(w.shape[1])), dtype=dt, device="cuda")
    out[:, :w.shape[1]] = w.to(dt)
    return out


def _split(w, dt):
    """split copy as Runtime.weight_split(mode 1) makes it: [hi | hi | lo] blocks of ru(K) columns, hi = T(w), lo = T(w - hi)"""
    w = w.float()
    hi = w.to(dt)
    lo = (w - hi.float()).to(dt)
    kp = _ru(w.shape[1])
    out = torch.zeros((w.shape[0], 3 * kp), dtype=dt, device="cuda")
    out[:, :w.shape[1]], out[:, kp:kp + w.shape[1]], out[:, 2 * kp:2 * kp + w.shape[1]] = hi, hi, lo
    return out


class Abi:
    """one call's device buffers and descriptor"""

    def __init__(self, prec, P, audio, video, map_size=None, H_=None, video_dev=None, pitch=None):
        from tim_amd import _lib as L
        self.L, self.prec, dt = L, L.PRECISIONS[prec], DT[prec]
        R, S, Cv = video.shape
        Ca = audio.shape[1]
        self.R, self.S, self.Cv, self.Ca = R, S, Cv, Ca
        self.video = video_dev if video_dev is not None else video.float().cuda().contiguous()
        if Ca % 4:     # an odd width travels as rows one float apart from contiguous, one float off the allocation's alignment
            base = torch.full((R * (Ca + 1) + 1,), float("nan"), device="cuda")
            self.audio = base[1:].view(R, Ca + 1)[:, :Ca]
            self.audio.copy_(audio.float())
        else:
            self.audio = audio.float().cuda().contiguous()
        f = lambda k: P[k].float().cuda().contiguous()   # noqa: E731
        self.keep = [_copy(P["affine_video.weight"].cuda(), dt), _copy(P["affine_audio.weight"].cuda(), dt),
                     _copy(P["affine_v.weight"].cuda(), dt), _copy(P["affine_g.weight"].cuda(), dt),
                     _copy(P["affine_v.weight"].cuda(), dt, True), _copy(P["affine_g.weight"].cuda(), dt, True),
                     f("affine_video.bias"), f("affine_audio.bias"), f("affine_h.weight").reshape(-1)]
        sp = [_split(P["affine_video.weight"].cuda(), dt), _split(P["affine_audio.weight"].cuda(), dt)] if prec != "fp32" else [None, None]
        self.keep += sp
        k = self.keep
        self.desc = L.TimAvga(self.video.data_ptr(), self.audio.data_ptr(), k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                              k[3].data_ptr(), k[4].data_ptr(), k[5].data_ptr(), sp[0].data_ptr() if sp[0] is not None else None,
                              sp[1].data_ptr() if sp[1] is not None else None, k[6].data_ptr(), k[7].data_ptr(), k[8].data_ptr(),
                              pitch if pitch is not None else S * Cv, R, S, Cv, Ca, H_ if H_ is not None else Cv,
                              map_size if map_size is not None else S, self.audio.stride(0), k[0].shape[1], k[1].shape[1], k[2].shape[1],
                              k[3].shape[1], k[4].shape[1], k[5].shape[1], sp[0].shape[1] if sp[0] is not None else 0,
                              sp[1].shape[1] if sp[1] is not None else 0, 0)

    def ws(self, backward):
        n = self.L.load().timhip_avga_workspace_bytes(self.prec, self.R, self.S, self.Cv, self.Ca, backward)
        assert n > 0
        return torch.empty(n, dtype=torch.uint8, device="cuda"), n

    def fwd(self, want_alpha=True):
        """outputs between NaN guard rows, with padded leading dimensions"""
        R, S, Cv = self.R, self.S, self.Cv
        ldo, lda = Cv + 4, S + 3
        out = torch.full((R + 2, ldo), float("nan"), device="cuda")
        al = torch.full((R + 2, lda), float("nan"), device="cuda")
        ws, n = self.ws(0)
        rc = self.L.load().timhip_avga_fwd(self.prec, C.byref(self.desc), out[1].data_ptr(), ldo,
                                           al[1].data_ptr() if want_alpha else None, lda, ws.data_ptr(), n,
                                           torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert torch.isnan(out[0]).all() and torch.isnan(out[-1]).all() and torch.isnan(out[1:-1, Cv:]).all()
        assert torch.isnan(al[0]).all() and torch.isnan(al[-1]).all() and torch.isnan(al[1:-1, S:]).all()
        if not want_alpha:
            assert torch.isnan(al).all()
        return out[1:-1, :Cv].double().cpu(), (al[1:-1, :S].double().cpu() if want_alpha else None)

    def bwd(self, cot, scaled=False):
        """the seven gradients, pre-filled with NaN; scaled: through a timhip_grad_scale block (fp16)"""
        L, R, S, Cv, Ca = self.L, self.R, self.S, self.Cv, self.Ca
        shapes = {"affine_video.weight": (Cv, Cv), "affine_video.bias": (Cv,), "affine_audio.weight": (Cv, Ca),
                  "affine_audio.bias": (Cv,), "affine_v.weight": (S, Cv), "affine_g.weight": (S, Cv), "affine_h.weight": (1, S)}
        G = {k: torch.full(sh, float("nan"), device="cuda") for k, sh in shapes.items()}
        gr = L.TimAvgaGrads(*[G[k].data_ptr() for k in PARAMS])
        ldd = Cv + 8
        d = torch.full((R, ldd), float("nan"), device="cuda")
        d[:, :Cv] = cot.float().cuda()
        st = torch.cuda.current_stream().cuda_stream
        gs = None
        if scaled:
            gs = torch.zeros(8, device="cuda")
            dc = d[:, :Cv].contiguous()
            L.call("timhip_grad_scale", (C.c_void_p * 1)(dc.data_ptr()), (C.c_longlong * 1)(dc.numel()), 1, 16.0, gs.data_ptr(), st)
        ws, n = self.ws(1)
        rc = L.load().timhip_avga_bwd(self.prec, C.byref(self.desc), d.data_ptr(), ldd, C.byref(gr),
                                      gs.data_ptr() if gs is not None else None, ws.data_ptr(), n, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        if gs is not None:
            assert gs[0].item() > 1.0 and gs.view(torch.int32)[4].item() == 0
        return {k: v.double().cpu() for k, v in G.items()}


def fwd_bound(prec, P, audio, video, ref, m=1.0):
    if prec == "fp32":
        return 1e-5 * max(1.0, m), 0.0
    model = avga_rounded(DT[prec])(P, audio, video)
    e = (model["out"] - ref["out"]).abs().max().item() / ref["out"].abs().max().item()
    return 2 * e + 1e-5, e


def check_fwd(prec, P, audio, video, m=1.0, tag="", want_alpha=True, **kw):
    ref = avga_f64(P, audio, video)
    out, al = Abi(prec, P, audio, video, **kw).fwd(want_alpha=want_alpha)
    scale = ref["out"].abs().max().item()
    err = (out - ref["out"]).abs().max().item() / scale
    bound, model = fwd_bound(prec, P, audio, video, ref, m)
    print("avga fwd %-10s %-5s R %3d S %2d Cv %4d Ca %3d: err %.3e  model %.3e  ratio %s  bound %.3e"
          % (tag, prec, video.shape[0], video.shape[1], video.shape[2], audio.shape[1], err, model,
             ("%.2f" % (err / model)) if model else "-", bound))
    assert torch.isfinite(out).all()
    assert err <= bound, (err, bound)
    if not want_alpha:
        assert al is None
        return out, al, ref
    assert torch.isfinite(al).all() and (al.sum(1) - 1).abs().max().item() <= 1e-6
    if prec == "fp32":
        assert (al - ref["alpha"]).abs().max().item() <= 1e-5 * max(1.0, m)
    return out, al, ref


FWD_SHAPES = [(1, 49, 64, 40), (6, 49, 64, 40), (37, 49, 128, 128), (5, 64, 64, 40), (5, 7, 64, 128), (4, 49, 1024, 40), (3, 49, 192, 40),
              (5, 49, 64, 37), (2, 49, 64, 1)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", FWD_SHAPES, ids=lambda s: "R%d_S%d_Cv%d_Ca%d" % s)
def test_forward_shapes(prec, shape):
    R, S, Cv, Ca = shape
    P, audio, video, _ = make_case(R, S, Cv, Ca, seed=100 + R + Cv)
    check_fwd(prec, P, audio, video, tag="shape")


@pytest.mark.parametrize("prec", PRECS)
def test_forward_fixture_and_strided_5d_view(prec):
    """the recorded fixture (R = 6), read in place from a [B, T, 7, 7, Cv] view whose rows are 64 floats apart"""
    g = np.load(os.path.join(H.GOLDEN, "avga_grads.npz"))
    P = {k: torch.from_numpy(g["param/" + k]).float().double() for k in PARAMS}
    video = torch.from_numpy(g["video"]).float().double().reshape(6, 49, 64)
    audio = torch.from_numpy(g["audio"]).float().double().reshape(6, 40)
    pitch = 49 * 64 + 64
    base = torch.full((6, pitch), float("nan"), device="cuda")
    v5 = base.as_strided((3, 2, 7, 7, 64), (2 * pitch, pitch, 7 * 64, 64, 1))
    v5.copy_(video.float().reshape(3, 2, 7, 7, 64))
    out, _, ref = check_fwd(prec, P, audio, video, tag="fixture5d", video_dev=v5, pitch=pitch)
    if prec == "fp32":
        assert (out - torch.from_numpy(g["out"]).reshape(6, 64)).abs().max().item() <= 2e-5 * ref["out"].abs().max().item()


@pytest.mark.parametrize("prec", PRECS)
def test_forward_edges(prec):
    # all-zero cells (and a silent audio term): alpha uniform over the S real cells, out = 0
    P, audio, video, _ = make_case(3, 49, 64, 40, seed=7, zero=True)
    out, al = Abi(prec, P, audio, video).fwd()
    assert (out == 0).all() and (al - 1.0 / 49).abs().max().item() <= 1e-6
    # padded rows carry relu(b_video) through hv.  Cases built so that they would WIN the softmax if they were counted: negative
    # W_video makes every real cell's hv smaller than the pad rows' relu(b_video), and w_h is aligned with the sign of
    # c_pad = W_v relu(b_video), so a pad row's score sum_j |w_h[j]| tanh|c_pad[j]| tops every real one; checked here in
    # float64 before the kernel runs (the real cells would be left with under a tenth of the mass)
    for S, seed, tag in ((49, 8, "padwins"), (7, 9, "padwins7")):
        P, audio, video, _ = make_case(5, S, 64, 40, seed=seed, bias_video=1.0)
        P["affine_video.weight"] = (-0.1 * P["affine_video.weight"].abs()).float().double()
        c_pad = P["affine_v.weight"] @ torch.relu(P["affine_video.bias"])
        P["affine_h.weight"] = (P["affine_h.weight"].abs() * torch.sign(c_pad) * 3).float().double()
        z_pad = (P["affine_h.weight"].reshape(-1) * torch.tanh(c_pad)).sum()
        hv = torch.relu(video @ P["affine_video.weight"].t() + P["affine_video.bias"])
        g = torch.relu(audio @ P["affine_audio.weight"].t() + P["affine_audio.bias"]) @ P["affine_g.weight"].t()
        z = torch.tanh(hv @ P["affine_v.weight"].t() + g.unsqueeze(2)) @ P["affine_h.weight"].reshape(-1)
        counted = torch.softmax(torch.cat([z, z_pad.expand(5, 64 - S)], 1), 1)
        assert z_pad.item() > z.max().item() + 1 and counted[:, :S].sum(1).max().item() < 0.1
        check_fwd(prec, P, audio, video, tag=tag)
    # saturated softmax: z amplified by m = 40
    P, audio, video, _ = make_case(5, 49, 64, 40, seed=10, wh_mult=40.0)
    _, al, _ = check_fwd(prec, P, audio, video, m=40.0, tag="saturated")
    assert al.max().item() > 0.9
    # alpha = NULL
    P, audio, video, _ = make_case(2, 49, 64, 40, seed=11)
    check_fwd(prec, P, audio, video, tag="noalpha", want_alpha=False)


def test_error_codes():
    from tim_amd import _lib as L
    lib = L.load()
    P, audio, video, _ = make_case(2, 49, 64, 40, seed=3)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros(2, 64, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")

    def fwd(a, prec=None, out_=out):
        return lib.timhip_avga_fwd(a.prec if prec is None else prec, C.byref(a.desc), out_.data_ptr() if out_ is not None else None,
                                   64, None, 0, ws.data_ptr(), ws.numel(), st)
    assert fwd(Abi("fp16", P, audio, video)) == 0
    a = Abi("fp16", P, audio, video); a.desc.S = 65; a.desc.map_size = 65
    assert fwd(a) == L.EUNSUPPORTED
    a = Abi("fp16", P, audio, video, map_size=48)
    assert fwd(a) == L.EUNSUPPORTED
    a = Abi("fp16", P, audio, video, H_=128)
    assert fwd(a) == L.EUNSUPPORTED
    a = Abi("fp16", P, audio, video); a.desc.Cv = 96; a.desc.H = 96
    assert fwd(a) == L.EUNSUPPORTED
    assert fwd(Abi("fp32", P, audio, video), prec=L.PREC_BF16X3) == L.EUNSUPPORTED
    a = Abi("fp16", P, audio, video); a.desc.w_video = None
    assert fwd(a) == L.EINVAL
    a = Abi("fp16", P, audio, video); a.desc.video = None
    assert fwd(a) == L.EINVAL
    assert fwd(Abi("fp16", P, audio, video), out_=None) == L.EINVAL
    a = Abi("fp16", P, audio, video); a.desc.pitch = 49 * 64 + 2
    assert fwd(a) == L.EALIGN
    a = Abi("fp16", P, audio, video); a.desc.pitch = 49 * 64 - 4
    assert fwd(a) == L.EINVAL
    a = Abi("fp16", P, audio, video)
    assert lib.timhip_avga_fwd(a.prec, C.byref(a.desc), out.data_ptr(), 64, None, 0, ws.data_ptr(), 16, st) == L.EWORKSPACE
    gr = L.TimAvgaGrads(*[out.data_ptr()] * 7)
    a = Abi("fp16", P, audio, video); a.desc.w_v_t = None
    assert lib.timhip_avga_bwd(a.prec, C.byref(a.desc), out.data_ptr(), 64, C.byref(gr), None, ws.data_ptr(), ws.numel(), st) == L.EINVAL
    torch.cuda.synchronize()


# ---- backward -------------------------------------------------------------------------------------------------------
def bwd_case(prec, P, audio, video, cot, tag, scaled=False):
    """(reference, rounding model or None, device gradients, tag, shape) of one backward call"""
    ref = avga_f64(P, audio, video, cot=cot)["grads"]
    model = avga_rounded(DT[prec])(P, audio, video, cot=cot)["grads"] if prec != "fp32" else None
    return ref, model, Abi(prec, P, audio, video).bwd(cot, scaled=scaled), tag, video.shape


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.reshape(-1), b.reshape(-1), dim=0).item()


def check_bwd(prec, case):
    """against avga_f64's autograd, per gradient: every element written, cosine >= 0.9999, elementwise error relative to the
    tensor's largest element fp32 <= 1e-4, 16-bit <= 2 x err(rounding model) + 1e-5.  (The rounding model itself is below
    cosine 0.9999 on affine_video.* / affine_audio.* at these shapes - rounding X and W moves pre-activations across zero and
    flips relu-mask bits; the kernels take the backward's masks from split products for that reason, include/timhip.h.)"""
    ref, model, got, tag, shp = case
    bad = []
    for k in PARAMS:
        r, v = ref[k], got[k].reshape(ref[k].shape)
        assert not torch.isnan(v).any(), k                      # written, every element
        scale = r.abs().max().item()
        err = (v - r).abs().max().item() / scale
        cos = _cos(v, r)
        if prec == "fp32":
            bound, me, cm = 1e-4, 0.0, 1.0
        else:
            me = (model[k] - r).abs().max().item() / scale
            bound, cm = 2 * me + 1e-5, _cos(model[k], r)
        print("avga bwd %-9s %-5s R %3d S %2d Cv %4d %-20s err %.3e  model %.3e  ratio %s  bound %.3e  cos %.7f  (model's cos %.7f)"
              % (tag, prec, shp[0], shp[1], shp[2], k, err, me, ("%.2f" % (err / me)) if me else "-", bound, cos, cm))
        if not (err <= bound and cos >= 0.9999):
            bad.append((k, err, bound, cos))
    assert not bad, bad


BWD_SHAPES = [(1, 49, 64, 40), (37, 49, 128, 128), (5, 64, 64, 40), (5, 7, 64, 128), (4, 49, 1024, 40), (3, 49, 192, 40), (5, 49, 64, 37)]
BWD_IDS = ["R%d_S%d_Cv%d_Ca%d" % s for s in BWD_SHAPES] + ["fixture"]


def _bwd_inputs(prec, shape):
    if shape == "fixture":
        g = np.load(os.path.join(H.GOLDEN, "avga_grads.npz"))
        P = {k: torch.from_numpy(g["param/" + k]).float().double() for k in PARAMS}
        video = torch.from_numpy(g["video"]).float().double().reshape(6, 49, 64)
        audio = torch.from_numpy(g["audio"]).float().double().reshape(6, 40)
        return bwd_case(prec, P, audio, video, torch.from_numpy(g["cot"]).float().double().reshape(6, 64), "fixture")
    R, S, Cv, Ca = shape
    P, audio, video, cot = make_case(R, S, Cv, Ca, seed=200 + R + Cv)
    return bwd_case(prec, P, audio, video, cot, "shape")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", BWD_SHAPES + ["fixture"], ids=BWD_IDS)
def test_backward_shapes(prec, shape):
    check_bwd(prec, _bwd_inputs(prec, shape))


def _tiny_cot_case():
    P, audio, video, cot = make_case(6, 49, 64, 40, seed=31)
    return bwd_case("fp16", P, audio, video, cot * 1e-7, "tinycot", scaled=True)


def test_backward_fp16_small_cotangent_needs_the_gradient_scale():
    """cotangents of 1e-7: d_c and d_pre (products of the cotangent with values below 1) lie under fp16's smallest subnormal
    (6e-8) unless they are stored times the scale timhip_grad_scale picks"""
    check_bwd("fp16", _tiny_cot_case())


# ---- through the model ----------------------------------------------------------------------------------------------------
def _tiny_model(prec, seed=3):
    from tim_amd.tim import TIM
    torch.manual_seed(seed)
    m = TIM([[7, 11, 13], 5], visual_input_dim=64, audio_input_dim=40, d_model=32, nhead=2, num_layers=2, num_feats=6,
            pool_features=True, precision=prec)
    with torch.no_grad():
        m.pool.affine_video.bias.normal_(0, 0.1)
    return m.cuda()


def _tiny_inputs(B=3, T=6, seed=4):
    g = torch.Generator().manual_seed(seed)
    video = torch.randn(B, T, 7, 7, 64, generator=g).abs().cuda()
    audio = torch.randn(B, T, 40, generator=g).cuda()
    times = torch.rand(B, 2 * T + 3, 2, generator=g).sort(-1)[0].cuda()
    return video, audio, times


def _step(m, video, audio, times):
    m.zero_grad(set_to_none=True)
    te = m(times, "time_mlp")
    cls, feats = m([video, audio], "encoder", te, 2, 1)
    loss = sum(c.float().square().mean() for c in cls if c is not None)
    loss.backward()
    torch.cuda.synchronize()
    return [c.detach().double().cpu() for c in cls if c is not None], {n: p.grad.detach().double().cpu() for n, p in m.named_parameters()
                                                                      if p.grad is not None}


def _cos_or_zero(a, b):
    return 1.0 if a.abs().max().item() == 0 and b.abs().max().item() == 0 else _cos(a, b)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("train", (False, True), ids=("eval", "train"))
def test_model_matches_the_torch_route(prec, train, monkeypatch):
    """one forward + backward of TIM(pool_features=True): device route against the same model under TIM_AMD_AVGA=0 (the
    module's fp32 torch ops, in the place of float64), same dropout seed, with the ABI tests' bounds:
      logits            fp32 1e-5;  16-bit 2 x err(rounding model) + 1e-5
      every gradient    cosine >= 0.9999
      pool.* gradients  fp32 1e-4;  16-bit 2 x err(rounding model) + 1e-5 - both routes' pool backward on ONE cotangent (the one
                        the encoder handed the torch route), the model = avga_rounded against avga_f64 on the same inputs
      other gradients   fp32 1e-4;  16-bit 2 x err(rounding model) + 1e-5
    For the logits and the non-pool gradients the rounding model's error is what avga_rounded's pooled tokens do to them
    against the torch route's: one more step of the same model with those tokens fed in place of the pool (the encoder behind
    the pool is not part of the route under test, and nothing else states how a rounding of its input reaches its outputs)."""
    m = _tiny_model(prec)
    m.train(train)
    video, audio, times = _tiny_inputs()
    seen = {}

    def grab(mod, inp, out):          # the cotangent the encoder hands back to the pool's output
        out.register_hook(lambda g: seen.__setitem__("cot", g.detach().clone()))
    hook = m.pool.register_forward_hook(grab)
    st = m.dropout_rng_state()
    monkeypatch.setenv("TIM_AMD_AVGA", "0")
    cls0, g0 = _step(m, video, audio, times)
    hook.remove()
    P = {k: v.detach().double().cpu() for k, v in m.pool.state_dict().items()}
    a_, v_, c_ = audio.reshape(18, 40).cpu(), video.cpu(), seen["cot"].reshape(18, 64).cpu()
    if prec == "fp32":
        lbound, bound = [1e-5] * len(cls0), {k: 1e-4 for k in g0}
    else:
        rounded = avga_rounded(DT[prec])
        fed = rounded(P, a_, v_)["out"].float().reshape(3, 6, 64).cuda()
        m.pool.forward = lambda a, v: fed                   # the rounding model's pooled tokens through the same encoder
        m.set_dropout_rng_state(st)
        clsm, gm = _step(m, video, audio, times)
        del m.pool.forward
        lbound = [2 * (a - b).abs().max().item() / a.abs().max().item() + 1e-5 for a, b in zip(cls0, clsm)]
        bound = {k: 2 * (g0[k] - gm[k]).abs().max().item() / max(1e-30, g0[k].abs().max().item()) + 1e-5 for k in gm}
        ref, mod = avga_f64(P, a_, v_, cot=c_)["grads"], rounded(P, a_, v_, cot=c_)["grads"]
        bound.update({"pool." + k: 2 * (mod[k] - ref[k]).abs().max().item() / ref[k].abs().max().item() + 1e-5 for k in PARAMS})
    m.set_dropout_rng_state(st)
    monkeypatch.setenv("TIM_AMD_AVGA", "1")
    cls1, g1 = _step(m, video, audio, times)
    assert set(g0) == set(g1) and sum(k.startswith("pool.") for k in g1) == 7
    tag = "%s %s" % (prec, "train" if train else "eval")
    for a, b, lb in zip(cls0, cls1, lbound):
        err = (a - b).abs().max().item() / max(1e-30, a.abs().max().item())
        print("avga model %s logits err %.3e (bound %.3e)" % (tag, err, lb))
        assert err <= lb
    # the pool's backward of both routes on the one cotangent
    shared = {}
    for env in ("0", "1"):
        monkeypatch.setenv("TIM_AMD_AVGA", env)
        m.zero_grad(set_to_none=True)
        m.pool(audio, video).backward(seen["cot"])
        torch.cuda.synchronize()
        shared[env] = {"pool." + n: p.grad.detach().double().cpu() for n, p in m.pool.named_parameters()}
    bad, worst, wcos = [], (0.0, None), (2.0, None)
    for k in g0:
        cos = _cos_or_zero(g0[k], g1[k])
        wcos = min(wcos, (cos, k))
        if k.startswith("pool."):
            a, b = shared["0"][k], shared["1"][k]
            err, c2 = (a - b).abs().max().item() / a.abs().max().item(), _cos(a, b)
            print("avga model %s %-28s shared cotangent: err %.3e bound %.3e cos %.7f;  in the step: cos %.7f" % (tag, k, err, bound[k], c2, cos))
            cos = min(cos, c2)
        else:
            err = (g0[k] - g1[k]).abs().max().item() / max(1e-30, g0[k].abs().max().item())
            worst = max(worst, (err / bound[k], k))
        if not (err <= bound[k] and cos >= 0.9999):
            bad.append((k, err, bound[k], cos))
    print("avga model %s other gradients: largest err / bound %.2f (%s); smallest cosine of any gradient %.7f (%s)"
          % (tag, worst[0], worst[1], wcos[0], wcos[1]))
    assert not bad, bad


def test_attention_map_equals_the_abi_alpha_and_no_grad_forward():
    m = _tiny_model("fp16").eval()
    video, audio, _ = _tiny_inputs()
    al = m.pool.attention_map(audio, video)
    assert al.shape == (3, 6, 49) and (al.sum(-1) - 1).abs().max().item() <= 1e-6
    P = {k: v.detach().double().cpu() for k, v in m.pool.state_dict().items()}
    _, want = Abi("fp16", P, audio.reshape(18, 40).double().cpu(), video.reshape(18, 49, 64).double().cpu()).fwd()
    assert torch.equal(al.reshape(18, 49).double().cpu(), want)
    with torch.no_grad():
        a = m.pool(audio, video)
    with torch.inference_mode():
        b = m.pool(audio, video)
    assert a.shape == (3, 6, 64) and torch.equal(a, b) and not a.requires_grad
    ref = avga_f64(P, audio.reshape(18, 40).cpu(), video.cpu())
    assert (a.reshape(18, 64).double().cpu() - ref["out"]).abs().max().item() <= 2e-3 * ref["out"].abs().max().item()


def test_graphed_step_replays_the_device_route():
    """a captured training step over a pool_features=True model, two replays against eager steps (the second on new inputs
    through the static buffers): logits bit for bit; pool.* gradients within 1e-6 of their largest element (dW_v and dw_h end
    in float atomics, include/timhip.h)"""
    from tim_amd import functional as F
    from tim_amd.graph import GraphedStep
    m = _tiny_model("fp16").eval()          # eval: no dropout, replays and eager steps compute the same function
    static = [t.clone() for t in _tiny_inputs()]

    def fn():
        for p in m.parameters():
            p.grad = None
        te = m(static[2], "time_mlp")
        cls, feats = m([static[0], static[1]], "encoder", te, 2, 1)
        loss = sum(c.float().square().mean() for c in cls if c is not None)
        loss.backward()
        return cls[2]

    def snap(logits):
        torch.cuda.synchronize()
        return logits.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if n.startswith("pool.")}

    def same(a, b):
        assert torch.equal(a[0], b[0])
        assert len(a[1]) == 7 and a[1].keys() == b[1].keys()
        for n in a[1]:
            err = (a[1][n] - b[1][n]).abs().max().item() / b[1][n].abs().max().item()
            assert err <= 1e-6, (n, err)

    try:
        eager1 = snap(fn())
        gs = GraphedStep(m, fn)
        same(snap(gs()), eager1)
        for t, new in zip(static, _tiny_inputs(seed=12)):
            t.copy_(new)
        rep2 = snap(gs())
        same(rep2, snap(fn()))
        assert not torch.equal(rep2[0], eager1[0])
    finally:
        F.graph_safe_dropout("cuda:0", enable=False)
