"""Fixture of the AVGA pooling's parameter gradients from the reference's own module in float64 (build container only).

    python tests/golden/make_golden_avga.py

Imports recognition/time_interval_machine/models/helpers/pool.py of the reference checkout, runs its AVGA module in float64 at
B = 3, T = 2, S = 49, Cv = H = 64, Ca = 40 and records parameters, inputs, the pooled output, the attention map (softmax of the
affine_h output, taken with a forward hook: the module does not return it) and the seven parameter gradients under a fixed
cotangent into tests/golden/avga_grads.npz.
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/recognition/time_interval_machine/models/helpers/pool.py"


def main():
    spec = importlib.util.spec_from_file_location("ref_pool", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(11)
    B, T, Cv, Ca = 3, 2, 64, 40
    m = mod.AVGA(a_dim=Ca, v_dim=Cv, hidden_size=Cv, map_size=49).double()
    with torch.no_grad():   # biases off their zero initialisation: the relu mask and the bias gradients must be exercised
        m.affine_video.bias.normal_(0, 0.1)
        m.affine_audio.bias.normal_(0, 0.1)
    audio = torch.randn(B, T, Ca, dtype=torch.float64)
    video = torch.randn(B, T, 7, 7, Cv, dtype=torch.float64).abs()          # post-ReLU VGG maps are non-negative
    cot = torch.randn(B, T, Cv, dtype=torch.float64)
    z = {}
    h = m.affine_h.register_forward_hook(lambda _m, _i, o: z.__setitem__("z", o.detach()))
    out = m(audio, video)
    h.remove()
    alpha = torch.softmax(z["z"].squeeze(2), dim=-1)
    out.backward(cot)
    res = {"audio": audio.numpy(), "video": video.numpy(), "cot": cot.numpy(), "out": out.detach().numpy(), "alpha": alpha.numpy()}
    for k, p in m.named_parameters():
        res["param/" + k] = p.detach().numpy()
        res["grad/" + k] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "avga_grads.npz"), **res)
    print("avga_grads.npz:", os.path.getsize(os.path.join(HERE, "avga_grads.npz")), "bytes; out", tuple(out.shape))


if __name__ == "__main__":
    main()
