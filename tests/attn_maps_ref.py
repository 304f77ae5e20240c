"""TEST INFRASTRUCTURE ONLY: numpy restatement of the attention weights the reference's encoder layers return
(transformers.py:102 over nn.MultiheadAttention with TIM's mask, tim.py:161-166) in the compact layout of
`timhip_attention_weights` - float64 by default; `dtype=np.float32` restates the kernel's own arithmetic (what a different
summation order moves is what the GPU tests' bound is made of)."""
import numpy as np


def weights(qkv, B, S, F, H, s0=0, per_head=False, dtype=np.float64):
    """qkv [B * S, 3 E] -> [B, S - s0, F + 1] (per_head: [B, H, S - s0, F + 1]): softmax over the F feature keys and, for query
    rows (s >= F), the row's own key in column F (0 for feature rows); mean over the heads as a sum in ascending head order
    times 1 / H"""
    qkv = np.asarray(qkv, dtype=dtype).reshape(B, S, 3, H, -1)
    Dh = qkv.shape[-1]
    scale = dtype(1.0) / np.sqrt(dtype(Dh))
    q, k = qkv[:, s0:, 0], qkv[:, :, 1]
    n = S - s0
    sc = np.full((B, H, n, F + 1), -np.inf, dtype=dtype)
    sc[..., :F] = np.einsum("bnhd,bjhd->bhnj", q, k[:, :F]) * scale
    own = np.einsum("bnhd,bnhd->bhn", q, k[:, s0:]) * scale
    isq = np.arange(s0, S) >= F
    sc[:, :, isq, F] = own[:, :, isq]
    p = np.exp(sc - sc.max(axis=-1, keepdims=True))
    tot = p.sum(axis=-1, keepdims=True, dtype=dtype)
    w = p / tot if dtype == np.float64 else p * (dtype(1.0) / tot)     # (the kernel multiplies by the rounded reciprocal)
    if per_head:
        return w
    acc = np.zeros((B, n, F + 1), dtype=dtype)
    for h in range(H):
        acc += w[:, h]
    return acc * (dtype(1.0) / dtype(H))


def to_dense(w, S, F, s0):
    """[B, S - s0, F + 1] -> [B, S - s0, S] as the reference lays a row out: feature columns, the own key on the diagonal"""
    w = np.asarray(w)
    dense = np.zeros(w.shape[:2] + (S,), dtype=w.dtype)
    dense[:, :, :F] = w[:, :, :F]
    for s in range(max(F, s0), S):
        dense[:, s - s0, s] = w[:, s - s0, F]
    return dense


# ---- the fixtures of tests/golden/make_golden_attn.py ----------------------------------------------------------------------------
FIXTURES = ("attn_maps_rec_av", "attn_maps_rec_visual", "attn_maps_det_av")


def load_fixture(name):
    """-> (npz, cfg): the recorded layer inputs / dense weights and the tiny config they were made with"""
    import os

    from tests import helpers as H
    z = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    variant = str(z["variant"])
    num_class = None
    if "num_class" in z.files:
        num_class = tuple(int(v) for v in z["num_class"])
    cfg = H.tiny_cfg(variant, str(z["input_modality"]), str(z["data_modality"]), bool(int(z["include_verb_noun"])),
                     num_class=num_class)
    assert (cfg.num_layers, cfg.nhead, cfg.d_model, cfg.num_feats, cfg.F) == tuple(
        int(z[k]) for k in ("num_layers", "nhead", "d_model", "num_feats", "F"))
    return z, cfg


def fixture_qkv(z, cfg, layer):
    """the layer's packed in-projection of the recorded input rows, float64: [windows * S, 3 E] (weights from tim_amd.synth)"""
    from tim_amd import synth
    sd = synth.make_state_dict(cfg, seed=int(z["seed"]), dtype=np.float64)
    pre = "%s.layers.%d.self_attn." % ("backbone" if cfg.variant == "detection" else "transformer_encoder", layer)
    x = z["x/layer%d" % layer]
    return x.reshape(-1, x.shape[-1]) @ sd[pre + "in_proj_weight"].T + sd[pre + "in_proj_bias"]
