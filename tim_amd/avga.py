"""Device route of the AVGA pooling (`tim.py:_AVGAParams`, reference helpers/pool.py:6-43): `timhip_avga_fwd` /
`timhip_avga_bwd` (tim_amd/csrc/avga.hip) behind an autograd Function.

`_AVGAParams.forward` asks `route()` per call; the device route needs the module to belong to a `TIM` (its `Runtime` owns the
operand copies of the weights - `FusedAdamW`'s refresh and `invalidate_weights` keep them current - and its `_workspace` the
scratch), GPU tensors, a supported shape, inputs that need no gradient (the features are pre-extracted: the library computes
parameter gradients only) and `TIM_AMD_AVGA` other than 0.  Everything else runs the module's stock torch ops.
"""
import ctypes as C
import os

import torch

from . import _lib as L
from ._lib import ptr
from .functional import _f32c, _stream

def shape_supported(S, Cv, Ca, H, map_size):
    """the shapes `timhip_avga_*` take (include/timhip.h); everything else is TIMHIP_EUNSUPPORTED there"""
    return 1 <= S <= 64 and S == map_size and H == Cv and Cv % 64 == 0 and 64 <= Cv <= 1024 and Ca >= 1


def classify(env, bound, prec, on_gpu, fp32, inputs_need_grad, R, S, Cv, Ca, H, map_size):
    """the decision of `route()` from the call's metadata alone: env = the value of TIM_AMD_AVGA, bound = the module belongs to
    a TIM, prec = its Runtime's precision number, on_gpu / fp32 = where and what the tensors and parameters are"""
    if env == "0" or not bound or prec not in (L.PREC_BF16, L.PREC_F16, L.PREC_FP32):
        return "torch"
    if not on_gpu or not fp32 or inputs_need_grad:
        return "torch"
    if R < 1 or R * 64 * Cv >= 2 ** 31:
        return "torch"
    return "device" if shape_supported(S, Cv, Ca, H, map_size) else "torch"


def route(pool, audio, video, env=None):
    """"device" or "torch" for one call of `pool(audio, video)` - decided from the tensors' metadata, nothing is launched"""
    env = os.environ.get("TIM_AMD_AVGA", "1") if env is None else env
    owner = pool.owner()
    if env == "0" or owner is None or video.dim() < 3 or video.numel() == 0:
        return "torch"
    R, Cv = video.shape[0] * video.shape[1], video.shape[-1]
    if audio.numel() == 0 or audio.numel() % R:
        return "torch"
    ts = [audio, video] + list(pool.parameters())
    return classify(env, True, owner.rt.prec, all(t.is_cuda for t in ts), all(t.dtype == torch.float32 for t in ts),
                    video.requires_grad or audio.requires_grad, R, video.numel() // (R * Cv), Cv, audio.numel() // R,
                    pool.affine_video.out_features, pool.affine_v.out_features)


def _rows(video, R, S, Cv):
    """(tensor to keep alive, pitch in floats): the [B, T, ..., Cv] tensor read in place when its pooled rows are evenly spaced
    and their cells contiguous; a contiguous copy otherwise"""
    v = video
    ok = v.data_ptr() % 16 == 0
    if ok:
        want, inner = 1, True
        for d in range(v.dim() - 1, 1, -1):           # the cell dimensions: contiguous [S, Cv]
            if v.shape[d] != 1 and v.stride(d) != want:
                inner = False
            want *= v.shape[d]
        pitch = v.stride(1) if v.shape[1] > 1 else (v.stride(0) if v.shape[0] > 1 else S * Cv)
        ok = inner and pitch >= S * Cv and pitch % 4 == 0 and (v.shape[0] == 1 or v.shape[1] == 1 or v.stride(0) == v.shape[1] * pitch)
        if ok:
            return v, pitch
    return v.contiguous(), S * Cv


class _Call:
    """descriptor and buffers of one call; `keep` holds what the descriptor points into"""

    def __init__(self, owner, audio, video, params, backward):
        rt = owner.rt
        wvid, bvid, waud, baud, wv, wg, wh = params
        B, T, Cv = video.shape[0], video.shape[1], video.shape[-1]
        R = B * T
        S = video.numel() // (R * Cv)
        a2 = _f32c(audio).reshape(R, -1)
        Ca = a2.shape[1]
        vid, pitch = _rows(video.detach(), R, S, Cv)
        cp = [rt.weight(wvid), rt.weight(waud), rt.weight(wv), rt.weight(wg)]
        tr = [rt.weight(wv, True), rt.weight(wg, True)] if backward else [None, None]
        # 16-bit backward: split copies [hi | hi | lo] of the two weights in front of a relu (the masks come from split products)
        sp = [rt.weight_split(wvid, 1), rt.weight_split(waud, 1)] if backward and rt.h16 else [None, None]
        vec = [_f32c(bvid), _f32c(baud), _f32c(wh).reshape(-1)]
        self.keep = [a2, vid] + cp + tr + sp + vec
        self.R, self.S, self.Cv, self.Ca, self.B, self.T = R, S, Cv, Ca, B, T
        self.prec, self.dev = rt.prec, video.device
        self.desc = L.TimAvga(ptr(vid), ptr(a2), ptr(cp[0]), ptr(cp[1]), ptr(cp[2]), ptr(cp[3]), ptr(tr[0]), ptr(tr[1]),
                              ptr(sp[0]), ptr(sp[1]), ptr(vec[0]), ptr(vec[1]), ptr(vec[2]), pitch, R, S, Cv, Ca, wvid.shape[0], wv.shape[0], a2.stride(0),
                              cp[0].stride(0), cp[1].stride(0), cp[2].stride(0), cp[3].stride(0),
                              tr[0].stride(0) if backward else 0, tr[1].stride(0) if backward else 0,
                              sp[0].stride(0) if sp[0] is not None else 0, sp[1].stride(0) if sp[1] is not None else 0, 0)
        nbytes = L.load().timhip_avga_workspace_bytes(self.prec, R, S, Cv, Ca, 1 if backward else 0)
        if nbytes == 0:
            raise L.TimHipError("timhip_avga_workspace_bytes: unsupported shape R %d S %d Cv %d Ca %d" % (R, S, Cv, Ca))
        self.nbytes = nbytes
        self.ws = owner._workspace(nbytes, self.dev, slot="avga_bwd" if backward else "avga")

    def forward(self, want_alpha):
        out = torch.empty((self.R, self.Cv), dtype=torch.float32, device=self.dev)
        alpha = torch.empty((self.R, self.S), dtype=torch.float32, device=self.dev) if want_alpha else None
        L.check(L.load().timhip_avga_fwd(self.prec, C.byref(self.desc), ptr(out), self.Cv, ptr(alpha), self.S, ptr(self.ws),
                                         self.nbytes, _stream()), "timhip_avga_fwd")
        return out, alpha


def _params(pool):
    return (pool.affine_video.weight, pool.affine_video.bias, pool.affine_audio.weight, pool.affine_audio.bias,
            pool.affine_v.weight, pool.affine_g.weight, pool.affine_h.weight)


class AvgaFn(torch.autograd.Function):
    """out [B, T, Cv] = AVGA(audio, video) with the seven parameter gradients from `timhip_avga_bwd`.  Nothing of the forward
    is saved but its inputs: the backward recomputes hv, c and alpha per pooled row."""

    @staticmethod
    def forward(ctx, owner, audio, video, *params):
        call = _Call(owner, audio, video, params, backward=False)
        out, _ = call.forward(False)
        ctx.owner = owner
        ctx.save_for_backward(audio, video, *params)
        return out.view(call.B, call.T, call.Cv)

    @staticmethod
    def backward(ctx, d_out):
        owner = ctx.owner
        audio, video, *params = ctx.saved_tensors
        rt = owner.rt
        call = _Call(owner, audio, video, params, backward=True)
        g = _f32c(d_out).reshape(call.R, call.Cv)
        sizes = [(p.numel() + 3) // 4 * 4 for p in params]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=call.dev)     # every element is written by the library
        grads, off = [], 0
        for p, n in zip(params, sizes):
            grads.append(flat[off:off + p.numel()].view(p.shape))
            off += n
        gs = rt.grad_scale([g], call.dev)
        gr = L.TimAvgaGrads(*[ptr(t) for t in grads])
        L.check(L.load().timhip_avga_bwd(call.prec, C.byref(call.desc), ptr(g), g.stride(0), C.byref(gr), ptr(gs), ptr(call.ws),
                                         call.nbytes, _stream()), "timhip_avga_bwd")
        return (None, None, None) + tuple(grads)


def pool_forward(pool, audio, video):
    """the device route of `_AVGAParams.forward` (`route()` said "device")"""
    owner = pool.owner()
    params = _params(pool)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return AvgaFn.apply(owner, audio, video, *params)
    call = _Call(owner, audio, video, params, backward=False)     # evaluation: the forward alone, no alpha kept
    out, _ = call.forward(False)
    return out.view(call.B, call.T, call.Cv)


def attention_map(pool, audio, video):
    """alpha [B, T, S] of the device route (no gradient)"""
    if route(pool, audio, video, env="1") != "device":
        raise L.TimHipError("attention_map: the device route of the AVGA pooling does not cover this call (GPU fp32 tensors "
                            "of a supported shape on a module that belongs to a TIM model; there is no CPU fallback)")
    with torch.no_grad():
        call = _Call(pool.owner(), audio, video, _params(pool), backward=False)
        _, alpha = call.forward(True)
    return alpha.view(call.B, call.T, call.S)
