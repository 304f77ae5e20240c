"""Mixup of the inputs on the device (utils/mixup.py:4-22 of the reference), in a form a captured step can redraw.

The reference draws `lam = np.random.beta(alpha, alpha)` and `index = torch.randperm(B)` on the host every iteration.  Inside
a HIP graph (`tim_amd.graph.GraphedStep`) host draws are frozen at capture: every replay would train on one lam and one
permutation.  Here the state lives in device memory and a kernel redraws it:

    mix = Mixup(batch_size, alpha=0.2, device=dev, seed=rank)
    def step():                                   # eager, or the `fn` of a GraphedStep: the same sequence of draws
        mix.draw()                                # one launch: lam ~ Beta(alpha, alpha), a permutation and its inverse
        visual, audio, te = mix.mix([visual_in, audio_in, model(times, "time_mlp")])     # one launch for all three
        y_a, y_b = mix.targets(labels)            # (labels, labels[index]): device gathers
        ... losses.mixup_cross_entropy(logits, y_a[k], y_b[k], mix.lam) ...              # lam stays a device word

The k-th draw of a seed is a function of (seed, k) alone (Philox keyed by the seed, numbered by a 64-bit counter the draw
kernel advances in device memory): eager and replayed steps give the same sequence, the dropout salt takes no part, and
`state_dict()` / `load_state_dict()` continue it across a restart.  Data parallel: every rank mixes within its local batch,
as each DDP process of the reference does - construct with `seed=rank` so the ranks draw different sets.

`set(lam, index)` puts host values (numpy's / torch's own draw) on the device instead: a loop that must keep the
reference's RNG stream uses it, at the price of not being capturable.

Everything runs on libtimhip (tim_amd/csrc/mixup.hip); there is no CPU path.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import call, ptr
from .functional import _require_gpu, _stream

_DTYPES = {torch.float32: L.PREC_FP32, torch.float16: L.PREC_F16, torch.bfloat16: L.PREC_BF16}


def _apply(srcs, lam, index, B):
    """one timhip_mixup_apply launch over contiguous tensors [B, ...] -> new tensors"""
    n = len(srcs)
    outs = [torch.empty_like(s) for s in srcs]
    vps, i64s, i32s = (C.c_void_p * n), (C.c_int64 * n), (C.c_int32 * n)
    call("timhip_mixup_apply", n, vps(*[ptr(s) for s in srcs]), vps(*[ptr(o) for o in outs]),
         i64s(*[s.numel() // B for s in srcs]), i32s(*[_DTYPES[s.dtype] for s in srcs]), B, ptr(lam), ptr(index), _stream())
    return outs


def _check_alpha(alpha):
    alpha = float(alpha)
    if alpha != alpha or (alpha > 0 and not L.MIXUP_ALPHA_MIN <= alpha <= L.MIXUP_ALPHA_MAX):
        raise ValueError("alpha %r: the sampler supports [%g, %g] (alpha <= 0 turns the mix off: lam = 1)"
                         % (alpha, L.MIXUP_ALPHA_MIN, L.MIXUP_ALPHA_MAX))
    return alpha


class _MixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, *tensors):
        srcs = [t.detach().contiguous() for t in tensors]
        outs = _apply(srcs, state.lam, state.index, state.batch_size)
        ctx.state, ctx.draws = state, state.draws
        ctx.mark_non_differentiable(*[o for o, t in zip(outs, tensors) if not t.requires_grad])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        st = ctx.state
        if st.draws != ctx.draws:
            raise RuntimeError("Mixup.mix backward: the state was redrawn (draw() or set()) after this forward - %d draws then, %d "
                               "now; the gradient would be mixed with another permutation.  Run the backward before the next "
                               "draw (inside a captured step the order is recorded and this cannot happen)" % (ctx.draws, st.draws))
        need = [i for i, g in enumerate(grads) if ctx.needs_input_grad[1 + i] and g is not None]
        res = [None] * len(grads)
        if need:
            # dX[j] = lam dY[j] + (1 - lam) dY[inverse[j]]: the same kernel with the inverse permutation
            for i, d in zip(need, _apply([grads[i].contiguous() for i in need], st.lam, st.inverse, st.batch_size)):
                res[i] = d
        return (None,) + tuple(res)


class Mixup:
    """Device-side mixup state of one batch size: `lam` fp32 [1], `index` / `inverse` int32 [B], the int64 draw counter."""

    def __init__(self, batch_size, alpha=0.2, device=None, seed=0):
        device = torch.device("cuda" if device is None else device)
        if device.type != "cuda":
            raise L.TimHipError("Mixup: the TIM hot path runs on the MI355X HIP kernels only; got device %s (there is no CPU "
                                "fallback)" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        L.load()
        self.batch_size, self.alpha, self.seed, self.device = int(batch_size), _check_alpha(alpha), int(seed) & (2 ** 64 - 1), device
        self.lam = torch.ones(1, dtype=torch.float32, device=device)
        self.index = torch.arange(self.batch_size, dtype=torch.int32, device=device)
        self.inverse = self.index.clone()
        self.counter = torch.zeros(1, dtype=torch.int64, device=device)
        self.draws = 0       # host count of the states issued (draw + set); a captured draw counts once, at capture

    # ---- state ------------------------------------------------------------------------------------------------------
    def draw(self):
        """One launch on the current stream: a new (lam, index, inverse).  Capturable; never synchronises."""
        with torch.cuda.device(self.device):
            call("timhip_mixup_draw", self.seed, ptr(self.counter), self.alpha, self.batch_size, 1, ptr(self.lam), ptr(self.index),
                 ptr(self.inverse), _stream())
        self.draws += 1
        return self

    def set(self, lam, index):
        """Host values (or the reference's own draw) onto the device."""
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:
            raise ValueError("lam must lie in [0, 1], got %r" % lam)
        idx = torch.as_tensor(index).detach().to("cpu", torch.int64).reshape(-1)
        B = self.batch_size
        if idx.numel() != B or not torch.equal(torch.sort(idx).values, torch.arange(B)):
            raise ValueError("index must be a permutation of range(%d)" % B)
        inv = torch.empty_like(idx)
        inv[idx] = torch.arange(B)
        self.lam.copy_(torch.tensor([lam], dtype=torch.float32))
        self.index.copy_(idx.to(torch.int32))
        self.inverse.copy_(inv.to(torch.int32))
        self.draws += 1
        return self

    # ---- use --------------------------------------------------------------------------------------------------------
    def mix(self, tensors):
        """[lam * t + (1 - lam) * t[index] for t in tensors] in one launch (at most 4 tensors per launch, more are split)."""
        tensors = list(tensors)
        for t in tensors:
            _require_gpu(t, "mixup")
            if t.dtype not in _DTYPES:
                raise TypeError("mixup: fp32, fp16 or bf16 tensors, got %s" % t.dtype)
            if t.dim() < 1 or t.shape[0] != self.batch_size:
                raise ValueError("mixup: leading dimension %s, the state was built for batch size %d"
                                 % (tuple(t.shape[:1]), self.batch_size))
        out = []
        for i in range(0, len(tensors), L.MIXUP_MAX_TENSORS):
            part = tensors[i:i + L.MIXUP_MAX_TENSORS]
            live = [t for t in part if t.numel() > 0]
            mixed = iter(_MixFn.apply(self, *live)) if live else iter(())
            out += [next(mixed) if t.numel() > 0 else t.clone() for t in part]
        return out

    def targets(self, y):
        """(y, y[index]) for a tensor or a dict of tensors: device gathers, capturable."""
        idx = self.index   # (index_select takes an int32 index: no widening launch)
        if isinstance(y, dict):
            return y, {k: v.index_select(0, idx) for k, v in y.items()}
        return y, y.index_select(0, idx)

    # ---- checkpoint -------------------------------------------------------------------------------------------------
    def state_dict(self):
        """seed, alpha and the counter (a host read: synchronises).  The NEXT draw of a loaded state is the one this state
        would have made next."""
        return {"seed": self.seed, "alpha": self.alpha, "counter": int(self.counter.item()), "batch_size": self.batch_size}

    def load_state_dict(self, sd):
        if int(sd.get("batch_size", self.batch_size)) != self.batch_size:
            raise ValueError("state of batch size %s loaded into one of %d" % (sd.get("batch_size"), self.batch_size))
        self.seed, self.alpha = int(sd["seed"]) & (2 ** 64 - 1), _check_alpha(sd["alpha"])
        self.counter.copy_(torch.tensor([int(sd["counter"])], dtype=torch.int64))
        self.draws += 1   # (whatever forward is pending no longer matches what the next draw belongs to)


_STATES = {}


def mixup_data(x, y, alpha=1.0, state=None):
    """utils/mixup.py:4-22, same arguments and return tuple (mixed_x, y_a, y_b, lam) - with lam the state's DEVICE tensor
    (pass it on to `losses.mixup_cross_entropy` / `losses.mixup_criterion`).  Without `state`, one `Mixup` per (device, batch
    size) is kept by the module; its alpha follows the call."""
    x = list(x)
    B, dev = x[0].size(0), x[0].device
    _require_gpu(x[0], "mixup_data")
    if state is None:
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), B)
        state = _STATES.get(key)
        if state is None:
            state = _STATES[key] = Mixup(B, alpha=alpha, device=dev)
        elif state.alpha != float(alpha):
            state.alpha = _check_alpha(alpha)
    state.draw()
    mixed = state.mix(x)
    y_a, y_b = state.targets(y)
    return mixed, y_a, y_b, state.lam
