"""Float64 restatement of the AVGA pooling (reference helpers/pool.py:27-43) and its rounding model: the yardsticks of the
device route's tests (tests/test_gpu_avga.py), pinned themselves to reference-recorded fixtures by tests/test_avga_ref.py.

    hv = relu(X W_video^T + b_video)   ha = relu(a W_audio^T + b_audio)   g = ha W_g^T            (g is indexed by the CELL)
    c[s, j] = (hv[s] W_v^T)[j] + g[s]  z[s] = sum_j w_h[j] tanh(c[s, j])  alpha = softmax_s(z)    out = alpha X
"""
import torch

PARAMS = ("affine_video.weight", "affine_video.bias", "affine_audio.weight", "affine_audio.bias", "affine_v.weight",
          "affine_g.weight", "affine_h.weight")


def _rounder(dtype):
    if dtype is None:
        return lambda t: t

    def rnd(t):   # the value the matrix cores read; straight-through for the gradient
        return t + (t.detach().to(dtype).to(t.dtype) - t.detach())
    return rnd


def _avga(params, audio, video, cot, dtype):
    P = {k: torch.as_tensor(params[k]).detach().double().clone().requires_grad_(cot is not None) for k in PARAMS}
    X = torch.as_tensor(video).detach().double()
    C = X.shape[-1]
    X = X.reshape(-1, X.shape[-3] * X.shape[-2] if X.dim() == 5 else X.shape[-2], C)       # [R, S, Cv]
    a = torch.as_tensor(audio).detach().double().reshape(X.shape[0], -1)
    rnd = _rounder(dtype)
    hv = torch.relu(rnd(X) @ rnd(P["affine_video.weight"]).t() + P["affine_video.bias"])
    ha = torch.relu(rnd(a) @ rnd(P["affine_audio.weight"]).t() + P["affine_audio.bias"])
    g = rnd(ha) @ rnd(P["affine_g.weight"]).t()                                             # [R, S]
    c = rnd(hv) @ rnd(P["affine_v.weight"]).t() + g.unsqueeze(2)                            # [R, S, S]
    z = torch.tanh(c) @ P["affine_h.weight"].reshape(-1)
    alpha = torch.softmax(z, dim=-1)
    out = torch.einsum("rs,rsc->rc", alpha, X)
    res = {"out": out.detach(), "alpha": alpha.detach()}
    if cot is not None:
        grads = torch.autograd.grad(out, [P[k] for k in PARAMS], torch.as_tensor(cot).double().reshape(out.shape))
        res["grads"] = {k: g_.detach() for k, g_ in zip(PARAMS, grads)}
    return res


def avga_f64(params, audio, video, cot=None):
    """params: {name: tensor} of an `_AVGAParams` / reference AVGA state_dict; audio [..., Ca]; video [R, S, Cv] or
    [B, T, h, w, Cv].  -> {"out" [R, Cv], "alpha" [R, S], "grads" {name: tensor} when a cotangent [R, Cv] is given}"""
    return _avga(params, audio, video, cot, None)


def avga_rounded(dtype):
    """the same with X, W_video, hv, W_v, a, W_audio, ha, W_g rounded to `dtype` where a matrix product reads them and
    everything else (biases, tanh, softmax, the weighted sum over the fp32 cells) in float64"""
    def fn(params, audio, video, cot=None):
        return _avga(params, audio, video, cot, dtype)
    return fn
