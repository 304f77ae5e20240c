"""Generate the attention-map fixtures by importing the reference (build container only), one variant per process:

    python tests/golden/make_golden_attn.py rec_av        -> attn_maps_rec_av.npz
    python tests/golden/make_golden_attn.py rec_visual    -> attn_maps_rec_visual.npz
    python tests/golden/make_golden_attn.py det_av        -> attn_maps_det_av.npz

(one process each: both reference variants use the package name `time_interval_machine`).  Every encoder layer of the
reference model is hooked in float64 `eval()`; per layer the fixture holds

    x/layer{l}      the layer's input [B, S, E], batch-first
    attn/layer{l}   the reference's dense head-averaged attention weights [B, S, S], unmodified

plus the config fields and the seed.  Nothing of the reference is written to the repo: weights and inputs are regenerated on
the test side from `tim_amd.synth`.  float64, compressed (the zeros of the dense rows compress); a fixture that would pass
512 KB stores fewer windows (`windows`), never a lossy form."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CASES = {   # name -> (reference variant, input modality, data modality, num_class, verb/noun, B, nv, na, seed)
    "rec_av": ("recognition", "audio_visual", "audio_visual", None, True, 3, 4, 2, 1),
    "rec_visual": ("recognition", "visual", "visual", None, True, 3, 5, 0, 1),
    # (audio-visual input, visual queries: with both query pyramids one window alone - S = 810 rows of float64 - passes 512 KB)
    "det_av": ("detection", "audio_visual", "visual", (13, 5), False, 2, 0, 0, 3),
}
NAME = sys.argv[1] if len(sys.argv) > 1 else "rec_av"
VARIANT, IM, DM, NUM_CLASS, VN, B, NV, NA, SEED = CASES[NAME]
LIMIT = 512 * 1024

# ---- logging-only stand-ins so that models/tim.py imports (as tests/golden/make_golden.py) ----
sj = types.ModuleType("simplejson")
sj.dumps = lambda *a, **k: ""
sys.modules["simplejson"] = sj
for name in ("fvcore", "fvcore.common", "fvcore.common.file_io"):
    sys.modules[name] = types.ModuleType(name)


class _PM:
    open = staticmethod(open)


sys.modules["fvcore.common.file_io"].PathManager = _PM
sys.path.insert(0, "/root/reference/" + VARIANT)
from time_interval_machine.models.tim import TIM  # noqa: E402

from tim_amd import synth  # noqa: E402
from tim_amd.config import named_config  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)


def main():
    cfg = named_config("tiny")
    cfg.input_modality, cfg.data_modality, cfg.include_verb_noun, cfg.variant = IM, DM, VN, VARIANT
    if NUM_CLASS is not None:
        cfg.num_class = NUM_CLASS
    kw = dict(visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, feat_drop=cfg.feat_drop,
              seq_drop=cfg.seq_drop, d_model=cfg.d_model, nhead=cfg.nhead, num_layers=cfg.num_layers,
              enc_dropout=cfg.enc_dropout, input_modality=cfg.input_modality, data_modality=cfg.data_modality,
              num_feats=cfg.num_feats, include_verb_noun=cfg.include_verb_noun)
    kw["feedfoward_scale" if VARIANT == "detection" else "feedforward_scale"] = cfg.feedforward_scale
    dt = torch.float64
    m = TIM(cfg.num_class, **kw).to(dt).eval()
    sd = synth.make_state_dict(cfg, seed=SEED, dtype=np.float64)
    m.load_state_dict({k: torch.from_numpy(v).to(dt) for k, v in sd.items()})
    inp = synth.make_inputs(cfg, B, NV, NA, seed=SEED, dtype=np.float64)
    vis, aud, times = (torch.from_numpy(inp[k]).to(dt) for k in ("visual", "audio", "times"))
    stack = m.backbone if VARIANT == "detection" else m.transformer_encoder
    rec = {}
    hooks = [lyr.register_forward_hook(lambda mod, a, o, i=i: rec.update({
        "x/layer%d" % i: a[0].detach().transpose(0, 1).numpy().copy(),        # [S, B, E] -> batch-first
        "attn/layer%d" % i: o[1].detach().numpy().copy()})) for i, lyr in enumerate(stack.layers)]
    with torch.no_grad():
        if VARIANT == "detection":
            m.train_pool = m.train_pool.to(dt)
            m.inference_queries = m.inference_queries.to(dt)
            m([vis, aud], "encoder", times, None, label_queries=False)
        else:
            m([vis, aud], "encoder", m(times, "time_mlp"), NV, NA)
    for h in hooks:
        h.remove()
    assert len(rec) == 2 * cfg.num_layers
    S = rec["x/layer0"].shape[1]
    meta = dict(variant=VARIANT, input_modality=IM, data_modality=DM, include_verb_noun=int(VN), B=B, nv=NV, na=NA, seed=SEED,
                num_layers=cfg.num_layers, nhead=cfg.nhead, d_model=cfg.d_model, num_feats=cfg.num_feats, F=cfg.F, S=S)
    if NUM_CLASS is not None:
        meta["num_class"] = np.asarray(NUM_CLASS)
    path = os.path.join(HERE, "attn_maps_%s.npz" % NAME)
    for windows in range(B, 0, -1):   # fewer windows rather than a lossy form
        np.savez_compressed(path, windows=windows, **{k: np.asarray(v) for k, v in meta.items()},
                            **{k: np.ascontiguousarray(v[:windows], dtype=np.float64) for k, v in rec.items()})
        if os.path.getsize(path) <= LIMIT:
            break
    print(os.path.basename(path), "S", S, "F", cfg.F, "windows", windows, "of", B, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
