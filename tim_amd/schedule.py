"""Cosine annealing under a linear warm-up for `FusedAdamW`: the reference's learning-rate schedule, counted and evaluated on the
host and handed to the optimizer's state block through the push it already has.

The reference's training iteration (recognition/scripts/train.py, and the detection train.py alike) ends with

    with warmup_scheduler.dampening():
        lr_scheduler.step()

i.e. `torch.optim.lr_scheduler.CosineAnnealingLR(T_max=len(loader) * epochs, eta_min=1e-6)` under
`pytorch_warmup.LinearWarmup(warmup_period=len(loader) * warmup_epochs)`, once per iteration whether or not the GradScaler
skipped the update.  torch has the first half; the second is a package of its own.  `CosineWarmupSchedule` is both, as one closed
form, attached to the optimizer so that the loop has no scheduler line to forget or to run twice:

    opt = FusedAdamW.for_model(model, lr=1e-4, weight_decay=5e-4, max_grad_norm=1.0)
    sched = CosineWarmupSchedule(opt, T_max=len(loader) * epochs, eta_min=1e-6, warmup_period=len(loader) * warmup_epochs)
    loss.backward(); opt.step()          # trains at lr(t) and counts t: there is no sched.step() to call

The definition (float64, rounded once to fp32; t = 0, 1, 2, ... counts the optimizer's steps, skipped ones included; an
`opt.step()` that finds no gradient at all returns before it is a step and is not counted):

    cos_lr(t) = eta_min + (base_lr - eta_min) * (1 + cos(pi * t / T_max)) / 2
    omega(t)  = min(1, (t + 1) / warmup_period)   if warmup_period >= 1, else 1
    lr(t)     = cos_lr(t) * omega(t)

Iteration 0 trains at base_lr / warmup_period; past T_max the closed form continues, as torch's scheduler does.  One deviation
from torch: the closed form is evaluated afresh every step, torch carries a Python double through a recursion - the two agree
to ~1e-13 relative, in every fp32 bit on the cases tests/test_lr_schedule_host.py pins.

The counter is a host integer.  An eager step writes the rate into the optimizer's LR words before its passes; under
`tim_amd.graph.GraphedStep(..., optimizer=opt)` the rate of the coming replay is written before every replay (`before_replay`, the
hook that pushes `group["lr"]` without a schedule).  A step captured in a bare `torch.cuda.graph` cannot be reached that way and
is refused.  (A counter in device memory advanced by a node of the captured step is not part of this module.)
"""
import math
import struct

from .optim import FusedAdamW


def _f32(x):
    """a Python float rounded once to fp32"""
    return struct.unpack("f", struct.pack("f", x))[0]


class CosineWarmupSchedule:
    """Attaches itself to a `FusedAdamW`: from then on every `opt.step()` trains at `lr_at(t)` and counts one iteration, on CPU
    and GPU tensors, eagerly and replayed by a `GraphedStep`.  While it is attached `group["lr"]` is neither read nor written;
    `base_lrs` are the groups' `lr` at construction.

    t          the iteration the next step trains at (one host integer: the groups share it)
    last_lr()  the rates of the latest step, one per group (0.0 before the first)
    set_step(t)  moves the schedule; allowed between replays"""

    def __init__(self, optimizer, T_max, eta_min=1e-6, warmup_period=0):
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError("CosineWarmupSchedule drives a tim_amd.optim.FusedAdamW (the LR words of its state blocks); got %s"
                            % type(optimizer).__name__)
        self._check(T_max, eta_min, warmup_period)
        if optimizer._schedule is not None:
            raise RuntimeError("CosineWarmupSchedule: this optimizer already has a schedule attached (detach() it first)")
        self.optimizer = optimizer
        self.T_max, self.eta_min, self.warmup_period = T_max, float(eta_min), warmup_period
        self.base_lrs = [float(g["lr"]) for g in optimizer.param_groups]
        self._t = 0
        self._last = [0.0] * len(self.base_lrs)
        optimizer._schedule = self

    @staticmethod
    def _check(T_max, eta_min, warmup_period):
        if isinstance(T_max, bool) or not isinstance(T_max, int) or T_max < 1:
            raise ValueError("CosineWarmupSchedule: T_max is an int >= 1 (got %r)" % (T_max,))
        if isinstance(warmup_period, bool) or not isinstance(warmup_period, int) or warmup_period < 0:
            raise ValueError("CosineWarmupSchedule: warmup_period is an int >= 0 (got %r)" % (warmup_period,))
        if isinstance(eta_min, bool) or not isinstance(eta_min, (int, float)) or not math.isfinite(eta_min) or eta_min < 0:
            raise ValueError("CosineWarmupSchedule: eta_min is a finite number >= 0 (got %r)" % (eta_min,))

    # ---- the definition ----------------------------------------------------------------------------------------------------
    def lr_at(self, t, group=0):
        """the rate iteration `t` trains group `group` at: the float64 formula rounded once to fp32, as a Python float"""
        base = self.base_lrs[group]
        cos_lr = self.eta_min + (base - self.eta_min) * (1 + math.cos(math.pi * t / self.T_max)) / 2
        omega = min(1.0, (t + 1) / self.warmup_period) if self.warmup_period >= 1 else 1.0
        return _f32(cos_lr * omega)

    def step(self, *args, **kwargs):
        raise RuntimeError("CosineWarmupSchedule.step(): the optimizer advances the schedule - every FusedAdamW.step() trains at "
                           "its rate and counts one iteration, eagerly and replayed by a GraphedStep; a loop ported from a torch "
                           "scheduler drops its lr_scheduler.step() / warmup_scheduler.dampening() lines")

    def detach(self):
        """the optimizer is host-driven again: its next step pushes `group["lr"]`, whatever the schedule wrote last"""
        opt = self.optimizer
        if opt is not None and opt._schedule is self:
            opt._schedule = None
            opt._lr_pushed = None
        self.optimizer = None

    # ---- reading and setting -----------------------------------------------------------------------------------------------
    @property
    def t(self):
        return self._t

    def last_lr(self):
        return list(self._last)

    def set_step(self, t):
        if isinstance(t, bool) or not isinstance(t, int) or t < 0:
            raise ValueError("CosineWarmupSchedule.set_step: an int >= 0 (got %r)" % (t,))
        self._t = t

    def state_dict(self):
        return {"t": self._t, "base_lrs": list(self.base_lrs), "T_max": self.T_max, "eta_min": self.eta_min,
                "warmup_period": self.warmup_period}

    def load_state_dict(self, sd):
        self._check(sd["T_max"], sd["eta_min"], sd["warmup_period"])
        base = [float(x) for x in sd["base_lrs"]]
        if len(base) != len(self.base_lrs):
            raise ValueError("CosineWarmupSchedule: the state_dict has %d groups, the optimizer %d" % (len(base), len(self.base_lrs)))
        if any(not math.isfinite(x) or x < 0 for x in base):
            raise ValueError("CosineWarmupSchedule: base_lrs are finite numbers >= 0 (got %r)" % (base,))
        self.T_max, self.eta_min, self.warmup_period, self.base_lrs = sd["T_max"], float(sd["eta_min"]), sd["warmup_period"], base
        self.set_step(sd["t"])

    # ---- what FusedAdamW calls ---------------------------------------------------------------------------------------------
    def _next_rates(self):
        """the rates of iteration t, one per group; the iteration is counted"""
        if len(self.optimizer.param_groups) != len(self.base_lrs):
            raise RuntimeError("CosineWarmupSchedule: the optimizer has %d parameter groups, the schedule was built for %d"
                               % (len(self.optimizer.param_groups), len(self.base_lrs)))
        self._last = [self.lr_at(self._t, gi) for gi in range(len(self.base_lrs))]
        self._t += 1
        return self._last
