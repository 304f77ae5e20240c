"""The fused optimizer step on the GPU (tim_amd/optim.py over timhip_optim_*): the kernels against `reference_step`, the operand
copies they write against `timhip_cast_weights`' bits, the hand-over to the next forward (no cast launch), the training loop
of tests/test_gpu_train_step.py with `FusedAdamW`, and the step captured in a HIP graph (replay == eager, device-side learning
rate and skip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests.test_gpu_graph import _model, _step  # noqa: E402
from tests.test_gpu_train_step import _loss_hip, _loss_oracle, _targets  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import functional as F  # noqa: E402
from tim_amd.graph import GraphedStep  # noqa: E402
from tim_amd.optim import FusedAdamW, reference_step  # noqa: E402
from tim_amd.tim import TIM  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1,), (3,), (63,), (4097,), (64, 64), (100, 52), (52, 100), (1024, 3072), (3806, 1024)]


def _tensors(shapes, seed, misaligned=True):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in shapes]
    if misaligned:   # a parameter (and its gradient) that starts 4 bytes past a 16-byte boundary
        base = torch.randn(1001, generator=g).to(DEV)
        ps.append(base[1:].detach().requires_grad_(True))
        assert ps[-1].data_ptr() % 16 == 4
    return ps


def _grads(ps, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        if p.data_ptr() % 16 == 4:
            buf = torch.empty(p.numel() + 1, device=DEV)
            p.grad = buf[1:]
            p.grad.copy_(torch.randn(p.shape, generator=g).to(DEV) * scale)
        else:
            p.grad = (torch.randn(p.shape, generator=g) * scale).to(DEV)


def _ref_groups(ps, opt, steps):
    return [{"params": [p.detach().clone() for p in ps], "grads": None, "exp_avg": [torch.zeros_like(p) for p in ps],
             "exp_avg_sq": [torch.zeros_like(p) for p in ps], "lr": opt.param_groups[0]["lr"], "betas": opt.param_groups[0]["betas"],
             "eps": opt.param_groups[0]["eps"], "weight_decay": opt.param_groups[0]["weight_decay"], "state": steps}]


def _close(a, b, tol):
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_kernels_follow_reference_step(max_norm):
    """fp32 arithmetic in a different association than torch's (fused multiply-adds, one division more or less): parameters and
    moments within 1e-6 of the tensor's largest entry - about 8 ulp - after 5 steps, the total norm within 1e-6 relative."""
    ps = _tensors(SHAPES, 0)
    opt = FusedAdamW(ps, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.05, max_grad_norm=max_norm)
    ref = _ref_groups(ps, opt, {"step": 0, "skipped": 0})
    if max_norm is None:    # moments at the same 4-byte offset as the parameter and its gradient: the 16-byte path with a
        # shifted start; with the optimizer's own (aligned) moments the item takes the scalar path
        opt.state[ps[-1]].update(exp_avg=torch.zeros(1001, device=DEV)[1:], exp_avg_sq=torch.zeros(1001, device=DEV)[1:])
    for it in range(5):
        _grads(ps, 100 + it, scale=0.01 if it == 2 else 1.0)      # (step 2: below the clip threshold)
        kept = [p.grad.clone() for p in ps]
        ref[0]["grads"] = kept
        norm, coef, bad = reference_step(ref, max_norm)
        opt.step()
        assert not bad and abs(opt.last_grad_norm.item() - norm.item()) <= 1e-6 * norm.item()
        assert abs(opt.last_clip_coef.item() - coef.item()) <= 2e-6 * coef.item()
        for p, g0 in zip(ps, kept):
            assert torch.equal(p.grad, g0)                        # the gradient itself is not rescaled
    for i, p in enumerate(ps):
        assert _close(p.detach(), ref[0]["params"][i], 1e-6), i
        assert _close(opt.state[p]["exp_avg"], ref[0]["exp_avg"][i], 1e-6), i
        assert _close(opt.state[p]["exp_avg_sq"], ref[0]["exp_avg_sq"][i], 1e-6), i
    assert float(opt.state_dict()["state"][0]["step"]) == 5.0 and int(opt.skipped_steps) == 0


def test_table_longer_than_one_launch_and_two_groups():
    """130 small tensors (three chunks of the 48-item kernel-argument table) in two groups with their own learning rates,
    sharing one norm; a parameter without a gradient is left out; a non-finite entry anywhere skips both groups."""
    shapes = [(1 + (7 * i) % 50,) if i % 3 else (3 + i % 5, 2 + i % 7) for i in range(130)]
    ps = _tensors(shapes, 1, misaligned=False)
    idle = torch.randn(5, device=DEV, requires_grad=True)
    opt = FusedAdamW([{"params": ps[:100] + [idle], "lr": 1e-2}, {"params": ps[100:], "lr": 3e-3, "weight_decay": 0.0}],
                     weight_decay=0.02, max_grad_norm=0.5)
    refs = []
    for gi, sl in enumerate((ps[:100], ps[100:])):
        grp = _ref_groups(sl, opt, {"step": 0, "skipped": 0})[0]
        grp["lr"], grp["weight_decay"] = opt.param_groups[gi]["lr"], opt.param_groups[gi]["weight_decay"]
        refs.append(grp)
    for it in range(3):
        _grads(ps, 7 + it)
        refs[0]["grads"], refs[1]["grads"] = [p.grad.clone() for p in ps[:100]], [p.grad.clone() for p in ps[100:]]
        norm, _, _ = reference_step(refs, 0.5)
        opt.step()
        assert abs(opt.last_grad_norm.item() - norm.item()) <= 1e-6 * norm.item()
    want = refs[0]["params"] + refs[1]["params"]
    for i, p in enumerate(ps):
        assert _close(p.detach(), want[i], 1e-6), i
    assert idle not in opt.state
    snap = [p.detach().clone() for p in ps]
    _grads(ps, 99)
    ps[117].grad.view(-1)[0] = float("nan")
    opt.step()
    assert int(opt.skipped_steps) == 1 and int(opt.found_inf) == 1
    assert all(torch.equal(p.detach(), s) for p, s in zip(ps, snap))
    assert [int(float(opt.state_dict()["state"][i]["step"])) for i in (0, 129)] == [3, 3]


def test_external_flag_word_skips_the_step():
    ps = _tensors([(64, 64), (5,)], 2, misaligned=False)
    opt = FusedAdamW(ps, lr=1e-2)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    opt.extra_flags.append(flag)
    _grads(ps, 1)
    opt.step()
    snap = [p.detach().clone() for p in ps] + [opt.state[p]["exp_avg"].clone() for p in ps]
    flag.fill_(1)
    _grads(ps, 2)
    opt.step()
    assert int(opt.skipped_steps) == 1
    assert all(torch.equal(a, b) for a, b in zip([p.detach() for p in ps] + [opt.state[p]["exp_avg"] for p in ps], snap))
    flag.zero_()
    opt.step()
    assert int(opt.skipped_steps) == 1 and int(opt.found_inf) == 0 and float(opt.state_dict()["state"][0]["step"]) == 2.0
    assert not torch.equal(ps[0].detach(), snap[0])


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_operand_copies_are_written_with_cast_weights_bits(prec):
    rt = F.Runtime(prec)
    shapes = [(64, 64), (100, 52), (52, 100), (1024, 3072), (3806, 1024), (7, 3)]
    ps = _tensors(shapes, 3, misaligned=False)
    for p in ps:
        rt.weight(p)                                            # the runtime's own cast: copies exist, padding zeroed
    opt = FusedAdamW(ps, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0, runtime=rt)
    for it in range(2):
        _grads(ps, 40 + it)
        opt.step()
    for p in ps:
        assert rt.copies.is_current(p)                          # recorded as current: the next forward casts nothing
        plain, tr = _pair(rt, p)
        N, K = p.shape
        want = p.detach().to(rt.op_dtype)
        assert torch.equal(plain[:, :K], want) and torch.equal(tr[:, :N], want.t())
        assert not plain[:, K:].any() and not tr[:, N:].any()   # padding columns still zero
        fresh = F.Runtime(prec)                                 # ... and both are what timhip_cast_weights makes of the master
        assert torch.equal(fresh.weight(p), plain) and torch.equal(fresh.weight(p, True), tr)


def _pair(rt, p):
    """(plain, transposed) operand copies the runtime holds for `p`, as they are (no refresh)"""
    return next((plain, tr) for q, plain, tr in rt.copies.pairs(p.device) if q is p)


def _record_calls(monkeypatch):
    names = []
    real = L.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    import tim_amd.losses
    import tim_amd.tim
    for mod in (L, F, tim_amd.tim, tim_amd.losses):                # (the modules that bound `call` by name at import)
        if hasattr(mod, "call"):
            monkeypatch.setattr(mod, "call", spy)
    return names


@pytest.mark.parametrize("which,prec", [("tiny", "fp16"), ("tiny", "bf16"), ("c2a", "fp16")])
def test_next_forward_casts_nothing_and_sees_the_update(which, prec, monkeypatch):
    from tests.test_gpu_parity import build
    from tim_amd.config import named_config
    if which == "tiny":
        cfg, (B, nv, na) = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True), (4, 4, 2)
    else:
        cfg, (B, nv, na) = named_config("C2a"), (2, 15, 10)
    cfg.feat_drop = cfg.seq_drop = cfg.enc_dropout = 0.0
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    inp = {k: v.to(DEV) for k, v in inp.items()}
    models = [build(cfg, prec, sd).train() for _ in range(2)]
    R = []
    fns = [_step(m, inp, nv, na, R) for m in models]
    fused = FusedAdamW.for_model(models[0], lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    params = [p for p in models[1].parameters()]
    ref = None
    for it in range(2):
        fns[0]()
        fused.step()
        fns[1]()
        live = [p for p in params if p.grad is not None]
        if ref is None:
            ref = [{"params": live, "grads": None, "exp_avg": [torch.zeros_like(p) for p in live],
                    "exp_avg_sq": [torch.zeros_like(p) for p in live], "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8,
                    "weight_decay": 0.01, "state": {"step": 0, "skipped": 0}}]
        ref[0]["grads"] = [p.grad for p in live]
        reference_step(ref, 1.0)
        models[1].invalidate_weights()
    assert int(fused.skipped_steps) == 0
    names = _record_calls(monkeypatch)

    def logits(m):
        with torch.no_grad():
            return m([inp["visual"], inp["audio"]], "encoder", m(inp["times"], "time_mlp"), nv, na)[0]
    ours = logits(models[0])
    assert names and "timhip_cast_weights" not in names        # the fused update left its copies current ...
    want = logits(models[1])
    assert "timhip_cast_weights" in names                      # ... the reference-updated model had to cast
    for a, b in zip(ours, want):
        if a is not None:
            # masters agree to ~1e-6, the 16-bit copies to one of their ulps (bf16: 4e-3 of a weight)
            assert (a - b).abs().max().item() <= (3e-2 if prec == "bf16" else 5e-3) * max(1.0, b.abs().max().item())


def test_fused_forward_after_step_issues_no_cast(monkeypatch):
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na = 4, 4, 2
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    inp = {k: v.to(DEV) for k, v in inp.items()}
    model = _model(cfg, sd, "bf16", 0.0)
    fn = _step(model, inp, nv, na, [])
    opt = FusedAdamW.for_model(model, lr=1e-3)
    fn()
    opt.step()                                                  # (copies exist since the forward: this step writes them)
    names = _record_calls(monkeypatch)
    fn()
    assert "timhip_cast_weights" not in names and any(n.startswith("timhip_layer_fwd") for n in names)
    opt.step()
    assert [n for n in names if n.startswith("timhip_optim_")] == ["timhip_optim_norm", "timhip_optim_finish", "timhip_optim_update"]


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-5), ("bf16", 3e-2), ("fp16", 3e-2)])
def test_training_steps_follow_the_oracle_with_the_fused_optimizer(prec, tol):
    """tests/test_gpu_train_step.py's loop with `FusedAdamW` in place of torch's optimizer: same oracle, same tolerances"""
    from oracle import tim_oracle as O  # noqa: F401
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    cfg.feat_drop = cfg.seq_drop = cfg.enc_dropout = 0.0
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
    opt = FusedAdamW.for_model(model, lr=2e-3, weight_decay=1e-4)
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
    assert hist[-1][0] < hist[0][0] - 0.05, hist
    assert int(opt.skipped_steps) == 0
    worst = max((p.detach().cpu().double() - ref[n].detach()).abs().max().item() for n, p in model.named_parameters())
    assert worst <= (4e-3 if prec == "fp32" else 2.4e-2), worst


def _opt_snapshot(model, opt):
    out = {n: p.detach().clone() for n, p in model.named_parameters()}
    for n, p in model.named_parameters():
        if p in opt.state:
            out[n + ".m"], out[n + ".v"] = opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()
    for q, plain, tr in model.rt.copies.pairs(torch.device(DEV)):
        out["plain%d" % id(q)], out["tr%d" % id(q)] = plain.clone(), tr.clone()
    return out


def _near(a, b, moved, what):
    d = (a.float() - b.float()).abs()
    # (the key third of an in-projection bias has no gradient in exact arithmetic - softmax ignores a shift of every key - so
    # what it receives is rounding noise and Adam walks it by lr per step in either run: only the maximum is bounded there)
    mean_ok = what.endswith("in_proj_bias") or d.mean().item() <= 0.1 * moved
    assert d.max().item() <= 2 * moved and mean_ok, (what, d.max().item(), d.mean().item())


def test_captured_optimizer_step_replays_bit_for_bit():
    """The optimizer alone in a HIP graph over static gradients (no backward, hence no atomics anywhere): N replays == N eager
    steps bit for bit in masters, moments and operand copies; a learning rate written on the host between replays takes
    effect; a flag word raised on the device makes one replay a no-op that counts one skipped step, and the next replay
    continues with the bias corrections of the un-advanced step count."""
    shapes = [(64, 64), (100, 52), (300, 1024), (4097,), (3,)]

    def make():
        rt = F.Runtime("fp16")
        ps = _tensors(shapes, 5)
        for p in ps[:3]:
            rt.weight(p)
        opt = FusedAdamW(ps, lr=1e-2, weight_decay=0.01, max_grad_norm=1.0, runtime=rt)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        opt.extra_flags.append(flag)
        _grads(ps, 11)
        return rt, ps, opt, flag, [p.grad for p in ps]

    def state(rt, ps, opt):
        out = [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps for k in ("exp_avg", "exp_avg_sq")]
        return out + [t.clone() for p in ps[:3] for t in _pair(rt, p)]

    plan = [(1e-2, 21, False), (1e-2, 22, False), (3e-2, 23, False), (3e-2, 24, True), (3e-2, 25, False)]

    def drive(step, rt, ps, opt, flag, grads):
        snaps = []
        for lr, seed, poison in plan:
            g = torch.Generator().manual_seed(seed)
            for t in grads:
                t.copy_(torch.randn(t.shape, generator=g).to(DEV))
            opt.param_groups[0]["lr"] = lr
            flag.fill_(1 if poison else 0)
            step()
            snaps.append(state(rt, ps, opt))
        return snaps

    rt, ps, opt, flag, grads = make()
    opt.step()                                                    # (the step the capture below also takes once, eagerly)
    eager = drive(opt.step, rt, ps, opt, flag, grads)
    rt2, ps2, opt2, flag2, grads2 = make()
    opt2.step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    snap0 = state(rt2, ps2, opt2)
    flag2.fill_(1)                                                # captured as a skipped step: recording moves nothing anyway
    with torch.cuda.graph(graph, stream=side):
        opt2.step()
    flag2.zero_()
    assert all(torch.equal(a, b) for a, b in zip(state(rt2, ps2, opt2), snap0))   # capture launches nothing

    def replay():
        opt2._push_lr()
        graph.replay()
    rep = drive(replay, rt2, ps2, opt2, flag2, grads2)
    for i, (a, b) in enumerate(zip(eager, rep)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), i
    assert all(torch.equal(x, y) for x, y in zip(rep[2], rep[3]))             # the poisoned replay left everything untouched
    assert not torch.equal(rep[4][0], rep[3][0])
    assert int(opt2.skipped_steps) == 1 and int(opt.skipped_steps) == 1
    assert float(opt2.state_dict()["state"][0]["step"]) == 1 + 4
    for p in ps2[:3]:
        plain, tr = _pair(rt2, p)
        assert torch.equal(plain[:, :p.shape[1]], p.detach().half()) and torch.equal(tr[:, :p.shape[0]], p.detach().half().t())


def test_graphed_step_with_the_fused_optimizer():
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    B, nv, na = 4, 4, 2
    sd, inp = H.synth_torch(cfg, B, nv, na, seed=3, dtype=torch.float32)
    static = {k: v.to(DEV).clone() for k, v in inp.items()}
    N = 3

    def run(graphed, lrs, poison_at=None):
        model = _model(cfg, sd, "fp16", 0.0)
        opt = FusedAdamW.for_model(model, lr=lrs[0], weight_decay=0.01, max_grad_norm=1.0)
        R = []
        inner = _step(model, static, nv, na, R)

        def fn():
            outs = inner()
            opt.step()
            return outs
        step = fn
        gs = None
        if graphed:
            gs = GraphedStep(model, fn, warmup=3, count_nodes=True, optimizer=opt)
            step = gs
        else:
            for _ in range(3):     # the wrapper's warm-up steps are real steps
                fn()
        snaps = []
        for i, lr in enumerate(lrs):
            opt.param_groups[0]["lr"] = lr
            if i == poison_at:
                good = R[0].clone()
                R[0].fill_(float("inf"))       # the captured backward reads its cotangents from these static tensors
            step()
            if i == poison_at:
                R[0].copy_(good)
            snaps.append(_opt_snapshot(model, opt))
        torch.cuda.synchronize()
        F.graph_safe_dropout(DEV, enable=False)
        return snaps, opt, gs, model

    lrs = [1e-3] * N + [5e-3, 5e-3]
    eager, opt_e, _, _ = run(False, lrs)
    rep, opt_g, gs, model = run(True, lrs)
    assert int(opt_g.skipped_steps) == 0 and float(opt_g.state_dict()["state"][0]["step"]) == 3 + len(lrs)
    # N replays follow N eager steps.  Not bit for bit at model level: the backward's column sums use fp32 atomics, so two
    # eager runs differ in the last bits of a few gradients too, and Adam turns a rounding-level gradient into a full lr-sized
    # move (tests/test_gpu_train_step.py argues the same bound); the optimizer alone IS bit-exact under replay (test below)
    for a, b in zip(eager, rep):
        for n, _ in model.named_parameters():
            _near(a[n], b[n], sum(lrs) + 3e-3, n)
    # the learning rate written on the host between replays took effect: the step-3 update is larger than a 1e-3 one
    name = next(n for n, p in model.named_parameters() if p.dim() == 2 and n + ".m" in rep[0])
    d_small = (rep[2][name] - rep[1][name]).abs().max().item()
    d_large = (rep[3][name] - rep[2][name]).abs().max().item()
    assert d_large > 2.5 * d_small, (d_small, d_large)
    # the copies the captured update wrote are the casts of the masters it wrote
    for p, plain, tr in model.rt.copies.pairs(torch.device(DEV)):
        Nn, K = p.shape
        assert torch.equal(plain[:, :K], p.detach().to(model.rt.op_dtype)) and torch.equal(tr[:, :Nn], p.detach().to(model.rt.op_dtype).t())
    # a poisoned replay: nothing moves, one skipped step counted on the device; the next replay continues from the old count
    pois, opt_p, gs_p, model_p = run(True, [1e-3, 1e-3, 1e-3], poison_at=1)
    for n in pois[0]:
        assert torch.equal(pois[0][n], pois[1][n]), n
    assert int(opt_p.skipped_steps) == 1 and int(opt_p.found_inf) == 0
    assert float(opt_p.state_dict()["state"][0]["step"]) == 3 + 2
    clean, _, _, _ = run(True, [1e-3, 1e-3])
    for n, _ in model_p.named_parameters():
        _near(pois[2][n], clean[1][n], 5e-3, n)                   # as if the bad step had never happened
    # launches of one captured iteration: fused tail against torch's capturable AdamW + clip + the cast at the head
    model_t = _model(cfg, sd, "fp16", 0.0)
    opt_t = torch.optim.AdamW(model_t.parameters(), lr=1e-3, weight_decay=0.01, capturable=True)
    inner_t = _step(model_t, static, nv, na, [])

    def fn_t():
        outs = inner_t()
        torch.nn.utils.clip_grad_norm_(model_t.parameters(), 1.0)
        opt_t.step()
        return outs
    gs_t = GraphedStep(model_t, fn_t, count_nodes=True)
    F.graph_safe_dropout(DEV, enable=False)
    print("captured nodes per iteration: FusedAdamW %s (kernels %s), torch clip + AdamW %s (kernels %s)"
          % (gs.nodes, gs.kernel_nodes, gs_t.nodes, gs_t.kernel_nodes))
    if gs.nodes is not None and gs_t.nodes is not None:
        assert gs.nodes < gs_t.nodes
