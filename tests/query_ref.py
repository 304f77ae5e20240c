"""Encode-once / query-many as a two-phase restatement of the oracle's forward, from the oracle's own functions
(`feature_encoding`, `encoder_layer`, `attention_structured`, `cls_heads`, `reg_heads`).  tests/test_query_ref.py pins it to
`O.forward` in float64; the GPU tests take from it the expectation for query sets a single full forward cannot express (groups that
share a window, another query count per group)."""
import torch

from oracle import tim_oracle as O


def _stack(cfg):
    return "backbone" if cfg.variant == "detection" else "transformer_encoder"


def encode(sd, cfg, visual, audio, times_feat):
    """times_feat [W, F, 2] -> (kv: per layer (K, V) of the feature rows, [W, H, F, Dh] each; feats [W, F, E])"""
    te = O.time_mlp(sd, times_feat)
    x = O.feature_encoding(sd, cfg, visual, audio, te, 0, 0)          # the feature rows alone: nothing in them reads a query
    W, F, E = x.shape
    assert F == cfg.F
    H = cfg.nhead
    kv = []
    for l in range(cfg.num_layers):
        p = "%s.layers.%d." % (_stack(cfg), l)
        qkv = O._lin(x, sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"])
        _, k, v = [t.reshape(W, F, H, E // H).transpose(1, 2) for t in qkv.split(E, -1)]
        kv.append((k, v))
        x = O.encoder_layer(sd, p, x, H, F)
    return kv, x


def query_rows(sd, cfg, times_q, nv, na):
    """the assembled query rows [G, Q, E]: the oracle's own sequence assembly with placeholder features, feature rows dropped"""
    G = times_q.shape[0]
    nf, dt = cfg.num_feats, times_q.dtype
    te = torch.cat([torch.zeros(G, cfg.F, cfg.d_model, dtype=dt), O.time_mlp(sd, times_q)], 1)
    has_v = cfg.input_modality in ("audio_visual", "visual")
    has_a = cfg.input_modality in ("audio_visual", "audio")
    vis = torch.zeros(G, nf, cfg.visual_input_dim, dtype=dt) if has_v else torch.zeros(G, 0, dtype=dt)
    aud = torch.zeros(G, nf, cfg.audio_input_dim, dtype=dt) if has_a else torch.zeros(G, 0, dtype=dt)
    return O.feature_encoding(sd, cfg, vis, aud, te, nv, na)[:, cfg.F:]


def query(sd, cfg, kv, times_q, nv, na, widx=None):
    """times_q [G, nv + na, 2] (visual queries first) against the cached keys and values of window widx[g] (None: window g)
    -> (cls tuple, reg tuple or None)"""
    x = query_rows(sd, cfg, times_q, nv, na)
    G, Q, E = x.shape
    H, F = cfg.nhead, cfg.F
    idx = torch.arange(G) if widx is None else torch.as_tensor(widx, dtype=torch.long)
    for l in range(cfg.num_layers):
        p = "%s.layers.%d." % (_stack(cfg), l)
        qkv = O._lin(x, sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"])
        q, k, v = [t.reshape(G, Q, H, E // H).transpose(1, 2) for t in qkv.split(E, -1)]
        kf, vf = kv[l][0][idx], kv[l][1][idx]
        # (the F leading rows of q are placeholders: a feature row's output is dropped, a query row reads none of them)
        o = O.attention_structured(torch.cat([torch.zeros_like(kf), q], 2), torch.cat([kf, k], 2), torch.cat([vf, v], 2), F)
        o = o[:, :, F:].transpose(1, 2).reshape(G, Q, E)
        # the rest of O.encoder_layer, on the query rows
        a = O._lin(o, sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"])
        x = O._ln(x + a, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        f = O._lin(O._gelu(O._lin(x, sd[p + "linear1.weight"], sd[p + "linear1.bias"])), sd[p + "linear2.weight"],
                   sd[p + "linear2.bias"])
        x = O._ln(x + f, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
    # (the heads slice from the end of the sequence: the query rows alone are enough)
    cls = O.cls_heads(sd, cfg, x, nv, na)
    reg = O.reg_heads(sd, cfg, x, nv, na) if cfg.variant == "detection" else None
    return cls, reg
