"""Fused optimizer step: gradient clipping, AdamW, non-finite skip and the refresh of the operand copies as device-side passes
(include/timhip.h: timhip_optim_*, tim_amd/csrc/optim.hip).

The tail of the reference's training iteration (recognition/scripts/train.py:351-363) is `unscale_` -> `clip_grad_norm_(1.0)` ->
`scaler.step(optimizer)` -> `scaler.update()`: two passes over the gradients, one over parameters and moments, a host decision
about inf / nan, and on this project one more pass (`timhip_cast_weights`) for the 16-bit operand copies of the updated weights.
`FusedAdamW` does the same work in one norm pass and one update pass that writes the copies, keeps the learning rate, the step
count and the skip decision in device memory (a captured step replays correctly, with no host round trip), and is a
`torch.optim.Optimizer` whose `state_dict` is interchangeable with `torch.optim.AdamW`'s.

    opt = FusedAdamW.for_model(model, lr=1e-4, weight_decay=5e-4, max_grad_norm=1.0)
    loss.backward(); opt.step()          # no `if rt.grads_finite():`, no clip_grad_norm_, no cast at the next forward

`reference_step` is the same semantics in plain torch: what CPU tensors run, and what the GPU tests check the kernels against.
"""
import ctypes as C
import math

import torch

from . import _lib as L
from .functional import GS_FLAG_WORD, any_flag_set

_TORCH_ONLY = ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay")


def reference_step(groups, max_grad_norm=None, found_inf=False):
    """One fused step in plain torch, in place, in the tensors' own dtype.

    groups  [{"params", "grads", "exp_avg", "exp_avg_sq": equally long lists of tensors, "lr", "betas", "eps", "weight_decay",
             "state": {"step": int, "skipped": int}}]; every group shares ONE gradient norm
    found_inf  an external non-finite verdict (the fp16 backward's flag words), ORed with "the norm is inf / nan"
    -> (norm, coef, found_inf).  A skipped step changes nothing but state["skipped"]."""
    grads = [g for grp in groups for g in grp["grads"]]
    if grads:
        total = torch.stack([g.detach().double().square().sum() for g in grads]).sum()
        norm = total.sqrt().to(grads[0].dtype)
    else:
        norm = torch.zeros(())
    found_inf = bool(found_inf) or not bool(torch.isfinite(norm))
    coef = torch.clamp(max_grad_norm / (norm + 1e-6), max=1.0) if max_grad_norm is not None and max_grad_norm > 0 else torch.ones_like(norm)
    for grp in groups:
        st = grp["state"]
        if found_inf:
            st["skipped"] += 1
            continue
        st["step"] += 1
        t, lr, (b1, b2) = st["step"], grp["lr"], grp["betas"]
        bc1, bc2s = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
        with torch.no_grad():
            for p, g, m, v in zip(grp["params"], grp["grads"], grp["exp_avg"], grp["exp_avg_sq"]):
                g = g * coef.to(g.dtype)
                p.mul_(1.0 - lr * grp["weight_decay"])
                m.mul_(b1).add_(g, alpha=1.0 - b1)
                v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                p.addcdiv_(m, (v.sqrt() / bc2s).add_(grp["eps"]), value=-lr / bc1)
    return norm, coef, found_inf


def _parr(ptrs):
    return (C.c_void_p * max(1, len(ptrs)))(*ptrs)


class FusedAdamW(torch.optim.Optimizer):
    """AdamW with the global-norm clip, the non-finite skip and (with a runtime) the operand-copy refresh fused in.

    max_grad_norm  None / <= 0: no clipping (the norm is still computed: `last_grad_norm`); the clip is global over all groups
    runtime        a model's `rt`: the operand copies it holds are written by the update (the next forward casts nothing), and
                   the fp16 mode's non-finite words of the backward passes since the last step decide whether the step is
                   skipped (they are consumed: no `rt.grads_finite()` call is needed, or wanted, around `step()`)

    One step count per parameter group (torch keeps one per parameter; they differ only when a parameter sat out some steps
    without a gradient, which `state_dict()` cannot express here: every parameter reports its group's count).
    `last_grad_norm`, `skipped_steps`, `found_inf` are device tensors: reading them is the caller's synchronisation.

    The learning rate is the host number `group["lr"]`, copied into the state block when it changed (before an eager step, and by
    `GraphedStep` before every replay) - unless a `tim_amd.schedule.CosineWarmupSchedule` is attached: then the same two places
    write the schedule's rate of that iteration, every step counts one iteration, and `group["lr"]` is not read."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, runtime=None,
                 amsgrad=False, maximize=False):
        if amsgrad:
            raise ValueError("FusedAdamW: amsgrad=True is not implemented")
        if maximize:
            raise ValueError("FusedAdamW: maximize=True is not implemented")
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdamW: lr is a host number; the device copy is kept by the optimizer")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdamW: invalid hyper-parameter (lr %r, betas %r, eps %r, weight_decay %r)" % (lr, betas, eps, weight_decay))
        # torch.optim.AdamW's own group keys ride along with their defaults, so a state_dict of this class loads into torch's
        proto = torch.optim.AdamW([torch.zeros(1)]).defaults
        defaults = {k: proto[k] for k in _TORCH_ONLY if k in proto}
        defaults.update(lr=float(lr), betas=tuple(betas), eps=float(eps), weight_decay=float(weight_decay),
                        max_grad_norm=None if max_grad_norm is None else float(max_grad_norm))
        super().__init__(params, defaults)
        if len(self.param_groups) > L.OPT_MAX_STATES:
            raise ValueError("FusedAdamW: at most %d parameter groups" % L.OPT_MAX_STATES)
        self.rt = runtime
        self._steps = [{"step": 0, "skipped": 0} for _ in self.param_groups]   # host copy: CPU tensors / before the block exists
        self._blocks = None      # [groups, 8] fp32 device tensor: one state block per group (include/timhip.h: TIMHIP_OPT_*)
        self._lr_pushed = None
        self._tables = None
        self._sig = None
        self._cpu_stats = None
        self.extra_flags = []    # 1-element 32-bit tensors: a non-zero word skips the step (a caller's own non-finite watch)
        self._capture_since = 0  # GraphedStep: first of the runtime's captured flag blocks that belongs to the capture in progress
        self._schedule = None    # a tim_amd.schedule.CosineWarmupSchedule: its rates go to the LR words, `group["lr"]` is not pushed
        self._replay_pushes = False   # a GraphedStep pushes the schedule's rate before every replay (before_capture was called)

    @classmethod
    def for_model(cls, model, **kw):
        inner = model.module if hasattr(model, "module") else model
        return cls(inner.parameters(), runtime=inner.rt, **kw)

    # ---- what the caller may read ------------------------------------------------------------------------------------
    def _stat(self, word, as_int):
        if self._blocks is None:
            if self._cpu_stats is None:
                return torch.zeros((), dtype=torch.int32 if as_int else torch.float32)
            return self._cpu_stats[word]
        row = self._blocks[0]
        return row.view(torch.int32)[word] if as_int else row[word]

    @property
    def device_lr(self):
        """the LR words of the state blocks, one per group: the rates the latest GPU step read (None before the first)"""
        return None if self._blocks is None else self._blocks[:, L.OPT_LR]

    @property
    def last_grad_norm(self):
        return self._stat(L.OPT_NORM, False)

    @property
    def last_clip_coef(self):
        return self._stat(L.OPT_COEF, False)

    @property
    def found_inf(self):
        return self._stat(L.OPT_FOUND_INF, True)

    @property
    def skipped_steps(self):
        return self._stat(L.OPT_SKIPPED, True)

    # ---- state_dict: torch.optim.AdamW's format ----------------------------------------------------------------------
    def _pull_steps(self):
        if self._blocks is not None:
            words = self._blocks.view(torch.int32).cpu()
            for gi, st in enumerate(self._steps):
                st["step"], st["skipped"] = int(words[gi, L.OPT_STEP]), int(words[gi, L.OPT_SKIPPED])

    def state_dict(self):
        self._pull_steps()
        for gi, grp in enumerate(self.param_groups):
            for p in grp["params"]:
                if p in self.state:
                    self.state[p]["step"] = torch.tensor(float(self._steps[gi]["step"]))
        return super().state_dict()

    def load_state_dict(self, state_dict):
        for grp in state_dict["param_groups"]:
            if grp.get("amsgrad") or grp.get("maximize"):
                raise ValueError("FusedAdamW: the state_dict was written with amsgrad / maximize, which are not implemented")
        super().load_state_dict(state_dict)
        for gi, grp in enumerate(self.param_groups):
            grp.setdefault("max_grad_norm", self.defaults["max_grad_norm"])
            steps = {int(float(self.state[p]["step"])) for p in grp["params"] if p in self.state and "step" in self.state[p]}
            if len(steps) > 1:
                raise ValueError("FusedAdamW keeps one step count per parameter group; the state_dict has %s" % sorted(steps))
            self._steps[gi] = {"step": steps.pop() if steps else 0, "skipped": 0}
        if self._blocks is not None:
            words = torch.zeros((len(self.param_groups), L.OPT_STATE_WORDS), dtype=torch.int32)
            for gi, st in enumerate(self._steps):
                words[gi, L.OPT_STEP] = st["step"]
            self._blocks.view(torch.int32).copy_(words)
        self._lr_pushed = None
        self._tables = self._sig = None

    # ---- the step ----------------------------------------------------------------------------------------------------
    def _moments(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st["exp_avg"], st["exp_avg_sq"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = [[p for p in grp["params"] if p.grad is not None] for grp in self.param_groups]
        flat = [p for ps in live for p in ps]
        if not flat:
            return loss
        if any(p.device != flat[0].device for p in flat):
            raise ValueError("FusedAdamW: every parameter on one device")
        if flat[0].device.type == "cuda":
            self._step_gpu(live, flat[0].device)
        else:
            self._step_cpu(live)
        return loss

    def _step_cpu(self, live):
        groups = []
        sch = self._schedule
        lrs = None if sch is None else sch._next_rates()    # (the attached schedule's rates; a skipped step counts too, as in the reference)
        for gi, (grp, ps) in enumerate(zip(self.param_groups, live)):
            mv = [self._moments(p) for p in ps]
            groups.append({"params": ps, "grads": [p.grad for p in ps], "exp_avg": [a for a, _ in mv], "exp_avg_sq": [b for _, b in mv],
                           "lr": grp["lr"] if lrs is None else lrs[gi], "betas": grp["betas"], "eps": grp["eps"],
                           "weight_decay": grp["weight_decay"], "state": self._steps[gi]})
        flagged = any(bool(f.view(torch.int32).ne(0).any()) for f in self.extra_flags)
        norm, coef, bad = reference_step(groups, self.param_groups[0]["max_grad_norm"], found_inf=flagged)
        self._cpu_stats = {L.OPT_NORM: norm.float(), L.OPT_COEF: coef.float(), L.OPT_FOUND_INF: torch.tensor(int(bad), dtype=torch.int32),
                           L.OPT_SKIPPED: torch.tensor(self._steps[0]["skipped"], dtype=torch.int32)}

    def _copies_of(self, dev):
        """data_ptr -> (the runtime's parameter, plain, tr) of every operand copy the runtime holds on `dev`"""
        return {} if self.rt is None else {q.data_ptr(): (q, plain, tr) for q, plain, tr in self.rt.copies.pairs(dev)}

    def _build(self, live, dev, copies):
        """the item tables (host arrays: they travel in the launches' arguments), one per group, and the partials buffer"""
        tables, n_part = [], 0
        for ps in live:
            items, keys = [], []
            for p in ps:
                if p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise ValueError("FusedAdamW: GPU parameters and gradients are contiguous fp32 tensors (got %s / %s)"
                                     % (p.dtype, p.grad.dtype))
                m, v = self._moments(p)
                rows, cols = (p.shape if p.dim() == 2 else (1, p.numel()))
                if p.numel() == 0:
                    continue
                ent = copies.get(p.data_ptr()) if p.dim() == 2 else None
                if ent is None:
                    items.append(L.TimOptItem(p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), None, None, rows, cols, 0, 0))
                else:
                    q, plain, tr = ent
                    items.append(L.TimOptItem(p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), plain.data_ptr(),
                                              tr.data_ptr(), rows, cols, plain.shape[1], tr.shape[1]))
                    keys.append(ent)
            arr = (L.TimOptItem * max(1, len(items)))(*items)
            cnt = L.load().timhip_optim_norm_partials(C.cast(arr, C.c_void_p), len(items))
            L.check(min(cnt, 0), "timhip_optim_norm_partials")
            tables.append({"arr": arr, "n": len(items), "part0": n_part, "copies": keys, "params": ps})
            n_part += cnt
        partials = torch.empty(max(1, n_part), dtype=torch.float64, device=dev)
        return {"groups": tables, "n_part": n_part, "partials": partials}

    def _push_lr(self, lrs=None):
        """host `group["lr"]` -> the state blocks' LR words when it changed (a scheduler's write); no synchronisation.
        With a schedule attached the LR words are the schedule's: `group["lr"]` is not pushed on any path, only the rates the
        schedule hands over (`lrs`)."""
        if self._blocks is None:
            return
        if lrs is None:
            if self._schedule is not None:
                return
            lrs = [float(g["lr"]) for g in self.param_groups]
        if lrs != self._lr_pushed:
            for gi, lr in enumerate(lrs):
                if self._lr_pushed is None or self._lr_pushed[gi] != lr:
                    self._blocks[gi, L.OPT_LR].fill_(lr)
            self._lr_pushed = lrs

    def _flag_words(self, dev, capturing):
        """device addresses of the non-finite words this step must honour (+ the tensors that keep them alive)"""
        rt = self.rt
        mine = [f for f in self.extra_flags if f.device == dev]
        if any(f.numel() != 1 or f.element_size() != 4 for f in mine):
            raise ValueError("FusedAdamW.extra_flags: 1-element 32-bit tensors")
        if rt is None or rt.prec != L.PREC_F16:
            if len(mine) > L.OPT_MAX_FLAGS:
                raise ValueError("FusedAdamW.extra_flags: at most %d words" % L.OPT_MAX_FLAGS)
            return [f.data_ptr() for f in mine], mine
        if capturing:
            blocks, extra = rt.nonfinite.captured_from(self._capture_since), []
        else:
            blocks, extra = rt.nonfinite.take()   # (extra: the passes folded earlier for want of a reader)
        blocks = [b for b in blocks if b.device == dev]
        extra += mine
        if len(blocks) + len(extra) > L.OPT_MAX_FLAGS:   # fold the surplus on the device
            keep = max(0, L.OPT_MAX_FLAGS - 1 - len(extra))
            extra.append(any_flag_set(blocks[keep:]).to(torch.int32).reshape(1))
            blocks = blocks[:keep]
        return [b.data_ptr() + 4 * GS_FLAG_WORD for b in blocks] + [e.data_ptr() for e in extra], blocks + extra

    def _step_gpu(self, live, dev):
        capturing = torch.cuda.is_current_stream_capturing()
        if self._blocks is None or self._blocks.device != dev:
            words = torch.zeros((len(self.param_groups), L.OPT_STATE_WORDS), dtype=torch.int32)
            for gi, st in enumerate(self._steps):
                words[gi, L.OPT_STEP], words[gi, L.OPT_SKIPPED] = st["step"], st["skipped"]
            self._blocks = words.to(dev).view(torch.float32)
            self._lr_pushed = None
        if self._schedule is not None:
            if not capturing:
                self._push_lr(self._schedule._next_rates())
            elif not self._replay_pushes:
                raise RuntimeError("FusedAdamW: a step with a CosineWarmupSchedule attached is captured through "
                                   "tim_amd.graph.GraphedStep(..., optimizer=opt), which writes the rate before every replay; a "
                                   "bare capture would replay the rate it was captured with")
        elif not capturing:    # (a captured fill would freeze the rate: GraphedStep pushes it before every replay)
            self._push_lr()
        copies = self._copies_of(dev)
        sig = tuple((p.data_ptr(), p.grad.data_ptr()) + tuple(t.data_ptr() for t in copies.get(p.data_ptr(), (0,))[1:])
                    for ps in live for p in ps)
        if self._tables is None or sig != self._sig:
            self._tables, self._sig = self._build(live, dev, copies), sig
        tb = self._tables
        stream = torch.cuda.current_stream(dev).cuda_stream
        prec = self.rt.prec if self.rt is not None else L.PREC_FP32
        for t in tb["groups"]:
            if t["n"]:
                L.call("timhip_optim_norm", C.cast(t["arr"], C.c_void_p), t["n"], tb["partials"].data_ptr() + 8 * t["part0"], stream)
        flags, keep = self._flag_words(dev, capturing)
        gi_all = range(len(self.param_groups))
        max_norm = self.param_groups[0]["max_grad_norm"]
        L.call("timhip_optim_finish", tb["partials"].data_ptr(), tb["n_part"], _parr(flags), len(flags),
               float(max_norm) if max_norm is not None else 0.0, _parr([self._blocks[gi].data_ptr() for gi in gi_all]),
               (C.c_double * len(gi_all))(*[g["betas"][0] for g in self.param_groups]),
               (C.c_double * len(gi_all))(*[g["betas"][1] for g in self.param_groups]), len(gi_all), stream)
        for gi, (grp, t) in enumerate(zip(self.param_groups, tb["groups"])):
            if t["n"]:
                L.call("timhip_optim_update", prec, C.cast(t["arr"], C.c_void_p), t["n"], self._blocks[gi].data_ptr(),
                       float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]), stream)
        del keep
        self._mark_updated()

    def _mark_updated(self):
        """Host bookkeeping of one update: the kernels wrote the masters through raw pointers, so the version counters autograd
        and the runtime's caches key on are advanced here; the operand copies the update wrote are recorded as current for the
        new version (the next forward casts nothing for them), the split copies of the same weights as stale (they stay on
        their own grouped refresh).  On a skipped step the masters did not change and the copies still equal them."""
        for t in self._tables["groups"]:
            if t["params"]:
                torch.autograd.graph.increment_version(t["params"])
        rt = self.rt
        if rt is None:
            return
        for t in self._tables["groups"]:
            for q, plain, tr in t["copies"]:
                rt.copies.record(q, plain, tr)
        rt.copies.invalidate(split_only=True)

    # ---- HIP-graph replay (tim_amd/graph.py: GraphedStep(..., optimizer=self)) ---------------------------------------------
    def before_capture(self, since):
        """Called by GraphedStep after its eager warm-up steps: the captured update writes the operand copies, so the cast at
        the head of the captured step is recorded only for what the update does not cover (split copies, weights outside the
        optimizer); the flag words of the capture's own backward passes (the runtime's captured blocks from position `since`)
        feed the captured update."""
        self._capture_since = since
        self._push_lr()
        self._replay_pushes = True
        rt = self.rt
        if rt is None:
            return
        covered = [q for t in (self._tables["groups"] if self._tables else []) for q, _, _ in t["copies"]]
        if not all(rt.copies.is_current(q) for q in covered):
            rt.copies.refresh(self._blocks.device)   # (a covered copy somebody invalidated by hand: rebuilt eagerly, once)
        rt.copies.invalidate(keep=covered)

    def before_replay(self):
        """the learning rate a host scheduler wrote since the last replay - with a CosineWarmupSchedule attached, the rate of the
        coming replay, which is counted here - and a refresh of copies somebody invalidated between
        replays (`load_state_dict`, `invalidate_weights()`): the captured step itself no longer casts them"""
        self._push_lr(None if self._schedule is None else self._schedule._next_rates())
        rt = self.rt
        if rt is None or self._tables is None:
            return
        for t in self._tables["groups"]:
            for q, _, _ in t["copies"]:
                if not rt.copies.is_current(q):
                    rt.copies.refresh(q.device)
                    return

    def after_replay(self):
        """a replay moved the masters without touching any version counter: the split copies (refreshed at the head of the
        captured step, i.e. BEFORE its update) no longer match them for an eager forward that might follow"""
        if self.rt is not None:
            self.rt.copies.invalidate(split_only=True)
