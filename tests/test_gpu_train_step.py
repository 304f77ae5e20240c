"""End-to-end training steps on the HIP path the way recognition/scripts/train.py:190-366 composes them:
time_mlp -> mixup of the inputs -> encoder -> label-smoothed mixup CE per head + cross-modal DRLoc -> backward -> AdamW.
Checks the first loss against the oracle, that the operand copies follow the optimizer's in-place updates (the loss of a
fixed batch goes down), and that a second model driven by the oracle's gradients stays on the same trajectory."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tim_oracle as O  # noqa: E402
from tests import helpers as H  # noqa: E402
from tim_amd import losses  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402

DEV = "cuda:0"


def _targets(B, nv, na, seed):
    g = torch.Generator().manual_seed(seed)
    t = {"verb": torch.randint(0, 7, (B * nv,), generator=g), "noun": torch.randint(0, 11, (B * nv,), generator=g),
         "action": torch.randint(0, 13, (B * nv,), generator=g), "class_id": torch.randint(0, 5, (B * na,), generator=g)}
    t["action"][::5] = -1            # padded queries (train.py:223-224 masks them by target != -1)
    t["verb"][::5] = -1
    t["noun"][::5] = -1
    t["class_id"][1::4] = -1
    return t


def _loss_hip(model, inp, ta, tb, lam, pos, nv, na, nf):
    te = model(inp["times"], "time_mlp")
    (verb, noun, action, audio), feats = model([inp["visual"], inp["audio"]], "encoder", te, nv, na)
    ce = lambda x, k: losses.mixup_cross_entropy(x, ta[k].to(DEV), tb[k].to(DEV), lam, 0.2)
    vis = (ce(verb, "verb") + ce(noun, "noun") + ce(action, "action")) / 3.0
    dr = losses.dense_relative_localization_loss_crossmodal(feats[:, :nf], feats[:, nf:], model, pos[0].shape[1], positions=pos)
    return vis + 1.0 * ce(audio, "class_id") + 0.3 * dr


def _loss_oracle(sd, cfg, inp, ta, tb, lam, pos, nv, na, nf):
    te = O.time_mlp(sd, inp["times"])
    (verb, noun, action, audio), feats = O.encoder(sd, cfg, inp["visual"], inp["audio"], te, nv, na)
    ce = lambda x, k: O.mixup_ce(x, ta[k], tb[k], lam, 0.2)
    vis = (ce(verb, "verb") + ce(noun, "noun") + ce(action, "action")) / 3.0
    dr = O.drloc_loss(sd, feats[:, :nf], feats[:, nf:], pos[0], pos[1])
    return vis + 1.0 * ce(audio, "class_id") + 0.3 * dr


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 3e-2)])
def test_training_steps_follow_the_oracle(prec, tol):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    cfg.feat_drop = cfg.seq_drop = cfg.enc_dropout = 0.0          # deterministic arithmetic: comparable with the oracle
    B, nv, na, nf = 4, 4, 2, cfg.num_feats
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    ta, tb = _targets(B, nv, na, 1), _targets(B, nv, na, 2)
    lam = 0.7
    g = torch.Generator().manual_seed(5)
    pos = (torch.randint(nf, (B, 5), generator=g), torch.randint(nf, (B, 5), generator=g))
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, feat_drop=0.0,
                seq_drop=0.0, d_model=cfg.d_model, nhead=cfg.nhead, num_layers=cfg.num_layers, enc_dropout=0.0,
                num_feats=nf, precision=prec)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    ref = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=1e-4)
    opt_ref = torch.optim.AdamW(list(ref.values()), lr=2e-3, weight_decay=1e-4)
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    rinp = {k: v.double() for k, v in inp.items()}
    hist = []
    for step in range(6):
        loss = _loss_hip(model, dinp, ta, tb, lam, pos, nv, na, nf)
        opt.zero_grad()
        loss.backward()
        opt.step()
        lref = _loss_oracle(ref, cfg, rinp, ta, tb, lam, pos, nv, na, nf)
        opt_ref.zero_grad()
        lref.backward()
        opt_ref.step()
        hist.append((loss.item(), lref.item()))
        assert abs(loss.item() - lref.item()) <= tol * max(1.0, abs(lref.item())), (step, hist)
    assert hist[-1][0] < hist[0][0] - 0.05, hist        # the updates reached the kernels' operand copies
    # parameters after 6 AdamW steps.  Adam normalises each update to ~lr whatever the gradient's size, so an entry whose
    # gradient is at rounding level (fp32 atomics order, 1e-8) can move by up to 2*lr per step differently: the bound is a
    # fraction of 6 * 2 * lr = 2.4e-2, not of the gradient accuracy
    worst = max((p.detach().cpu().double() - ref[n].detach()).abs().max().item() for n, p in model.named_parameters())
    assert worst <= (4e-3 if prec == "fp32" else 2.4e-2), worst


def test_fp16_nonfinite_gradient_flag():
    """`model.rt.grads_finite()` - the device-side word the weight-gradient kernels OR when they write inf / nan (include/timhip.h:
    timhip_grad_scale), the fp16 mode's counterpart of GradScaler's inf check (reference scripts/train.py:351,357-363).
    A healthy step reads True; a step whose gradient operands were pushed over the fp16 range (scale target 2^60: S is clamped
    to 2^40, every cotangent of order 1e-2 becomes inf in 16 bits) reads False - and the parameter gradients really are
    non-finite; reading resets the watch, the next healthy step is True again.  fp32 / bf16: always True."""
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na, nf = 4, 4, 2, cfg.num_feats
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    ta, tb = _targets(B, nv, na, 1), _targets(B, nv, na, 2)
    g = torch.Generator().manual_seed(5)
    pos = (torch.randint(nf, (B, 5), generator=g), torch.randint(nf, (B, 5), generator=g))
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    for prec in ("fp16", "bf16"):
        model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim,
                    d_model=cfg.d_model, nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=nf, precision=prec)
        model.load_state_dict(sd)
        model = model.to(DEV).train()

        def step():
            for p in model.parameters():
                p.grad = None
            _loss_hip(model, dinp, ta, tb, 0.7, pos, nv, na, nf).backward()
            return all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)

        assert step() and model.rt.grads_finite()
        assert model.rt.grads_finite()                      # nothing since the last read
        if prec != "fp16":
            continue
        target = model.rt.grad_scale_target
        model.rt.grad_scale_target = 2.0 ** 60
        finite = step()
        model.rt.grad_scale_target = target
        assert not finite                                   # the overflow is real ...
        assert not model.rt.grads_finite(reset=False)       # ... and the kernels saw it, without a pass over the gradients
        assert not model.rt.grads_finite()
        assert step() and model.rt.grads_finite()           # reading reset the watch
        # many passes without a reader: folded on the device, an early overflow is not forgotten
        model.rt.grad_scale_target = 2.0 ** 60
        step()
        model.rt.grad_scale_target = target
        for _ in range(12):
            assert step()
        assert not model.rt.grads_finite()
        # ... and neither is the pass whose block TRIGGERS the fold (round-4 advisor finding: the fold used to read the new
        # block's flag before that pass's kernels had been issued, and dropped it): each step appends two blocks (time MLP +
        # encoder), so after 8 healthy steps the list holds 16 and the overflowing step's first append folds
        assert step() and model.rt.grads_finite()
        assert step()
        per_step = model.rt.nonfinite.n_pending       # blocks one step appends (one per backward pass: time MLP, encoder, ...)
        assert 1 <= per_step <= 4
        while model.rt.nonfinite.n_pending < 16 - (per_step - 1):
            assert step()
        assert model.rt.nonfinite.n_pending <= 16     # no fold yet: the next step's appends reach the limit
        model.rt.grad_scale_target = 2.0 ** 60
        assert not step()
        model.rt.grad_scale_target = target
        assert model.rt.nonfinite.n_pending <= per_step   # the fold ran inside that step ...
        assert not model.rt.grads_finite()        # ... and the step's own flag survived it
        assert step() and model.rt.grads_finite()


def test_fp16_gradient_stream_16bit_opt_in():
    """TIM_AMD_GRAD_STREAM=16 / `rt.grad_stream16` (the round-4 default, an opt-in since round 5): the residual part of the
    backward's gradient stream between LayerNorm-backward launches as fp16 under the gradient scale.  Same model, same batch,
    deterministic arithmetic: every parameter gradient finite and within 4e-3 of its tensor's largest element of the fp32-stream
    pass's (the C2a figures: 1.4e-3 against 8.7e-4 of the oracle's), and NOT bit-identical (the path really ran)."""
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    cfg.num_layers = 3                                           # a middle layer: 16-bit stream in AND out
    B, nv, na, nf = 4, 4, 2, cfg.num_feats
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    ta, tb = _targets(B, nv, na, 1), _targets(B, nv, na, 2)
    g = torch.Generator().manual_seed(5)
    pos = (torch.randint(nf, (B, 5), generator=g), torch.randint(nf, (B, 5), generator=g))
    dinp = {k: v.to(DEV) for k, v in inp.items()}
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, feat_drop=0.0,
                seq_drop=0.0, d_model=cfg.d_model, nhead=cfg.nhead, num_layers=cfg.num_layers, enc_dropout=0.0,
                num_feats=nf, precision="fp16")
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    assert model.rt.grad_stream16 is False                       # the default follows the reference's AMP recipe (fp32 residual gradient)
    grads = {}
    for flag in (False, True):
        model.rt.grad_stream16 = flag
        for p in model.parameters():
            p.grad = None
        _loss_hip(model, dinp, ta, tb, 0.7, pos, nv, na, nf).backward()
        torch.cuda.synchronize()
        grads[flag] = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    differs = 0
    for n, a in grads[False].items():
        b = grads[True][n]
        assert torch.isfinite(b).all(), n
        s = a.abs().max().item() + 1e-20
        assert (a - b).abs().max().item() <= 4e-3 * s, (n, (a - b).abs().max().item(), s)
        differs += int(not torch.equal(a, b))
    assert differs > 0
