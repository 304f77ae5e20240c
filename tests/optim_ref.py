"""float64 restatement of the fused optimizer step (tim_amd/csrc/optim.hip), its per-element error bounds and the input families
of the tests that use them.

Written from the contract in include/timhip.h (the state-block comment and timhip_optim_*), in plain torch on the CPU; nothing
here imports tim_amd.optim.  tests/test_optim_ref.py pins it against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in
float64 and shows, with an fp32 emulation of the kernel's formula, that the bounds hold on every input family;
tests/test_gpu_optim_edges.py holds the three kernels to it element by element.

What is compared is the kernels' ARITHMETIC: the reference starts from the fp32 values the kernel reads - tensors, the state
block's scalars, and the launch arguments as the kernel receives them ((float)beta1, (float)(1 - beta1), ...) - and continues in
float64.  u = 2^-24 is fp32's unit roundoff.

One step from given state, per element (c = COEF, t = the new step count):
    gc = g c;  m' = b1 m + (1 - b1) gc;  v' = b2 v + (1 - b2) gc^2
    den = sqrt(v') / BC2_SQRT + eps;  upd = (lr / BC1) m' / den;  p' = p (1 - lr wd) - upd

Bounds (the constants below; each counts the fp32 roundings of the kernel's formula and keeps about one ulp of slack for a
sqrtf / division that rounds to 1 ulp where the CPU's round to half):
    lim_m   = 4u (|b1 m| + |(1 - b1) gc|)        two products of two roundings each (gc itself is rounded) and one sum
    lim_v   = 6u v'                              all terms positive: b2 v (1), gc (1), (1 - b2) gc gc (2), the sum (1), slack
    rel_den = (lim_v / (2 v') + 3u) (sqrt(v') / BC2_SQRT) / den + u      the root halves v''s error; root, division, sum round
    lim_upd = |upd| (rel_den + 4u) + (lr / BC1) lim_m / den              lr / BC1, m' / den and the product round
    lim_p   = 3u |p| + lim_upd + u |p'|          1 - lr wd, p decay, and the final subtraction
The inputs must keep fp32 denormals out of the question (v >= 1e-30 or exactly 0, no product of the formula below 1e-37 unless
it is exactly 0): a relative bound cannot speak about them.
"""
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
# the constants of the bounds above, in u: (lim_m, lim_v, root / division / sum of den, upd, p decay, p' store)
C_M, C_V, C_DEN, C_UPD, C_P, C_P1 = 4.0, 6.0, 3.0, 4.0, 3.0, 1.0
NORM_LIMIT = 10 * U    # 16 squares and 15 adds per lane in fp32: 16u on the sum of squares; fp64 across lanes and tiles; the
#                        root halves it (8u), one rounding to fp32 (1u)
COEF_LIMIT = 12 * U    # the norm's 10u, the rounding of norm + 1e-6 and of the division
CLIP_EPS = float(np.float32(1e-6))


def f32(x):
    """a number rounded to fp32 once, as a Python float"""
    with np.errstate(over="ignore"):
        return float(np.float32(x))


def bits32(x):
    return int(np.float32(x).view(np.uint32))


def d64(t):
    return t.detach().to("cpu").to(F64)


def norm(grads):
    """sqrt(sum g^2) over every tensor, in float64 from the gradients' fp32 values -> Python float"""
    total = 0.0
    for g in grads:
        total += float(d64(g).square().sum())
    return math.sqrt(total)


def finish(norm64, max_norm, flags, step, beta1, beta2, exact=False):
    """The scalars of one step for one state block -> (norm32, coef32, found_inf, step', bc1_32, bc2sqrt_32), fp32 values as
    Python floats.  found_inf: a non-zero flag word, or a norm that is not finite as fp32; then the step count stays and the bias
    corrections returned are those of the unchanged count (the kernel leaves the BC words alone).
    exact=True rounds nothing to fp32: the same step in float64 throughout (what tests/test_optim_ref.py compares with torch)."""
    f32 = float if exact else globals()["f32"]
    norm32 = f32(norm64)
    found_inf = any(int(f) != 0 for f in flags) or not math.isfinite(norm32)
    max32 = f32(max_norm)
    if max32 > 0 and math.isfinite(norm64):
        coef = f32(min(1.0, max32 / (norm64 + (1e-6 if exact else CLIP_EPS))))
    elif max32 > 0:
        coef = 0.0 if math.isinf(norm64) else 1.0     # fminf(1, max_norm / inf) = 0, fminf(1, nan) = 1
    else:
        coef = 1.0
    t = step if found_inf else step + 1
    bc1 = f32(1.0 - beta1 ** t)
    bc2s = f32(math.sqrt(1.0 - beta2 ** t))
    return norm32, coef, found_inf, t, bc1, bc2s


def _coefs(beta1, beta2, eps, wd, exact=False):
    f32 = float if exact else globals()["f32"]
    return f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps), f32(wd)


def _parts(p, g, m, v, coef32, lr32, bc1_32, bc2sqrt_32, beta1, beta2, eps, wd, exact=False):
    b1, omb1, b2, omb2, eps32, wd32 = _coefs(beta1, beta2, eps, wd, exact)
    p, g, m, v = d64(p), d64(g), d64(m), d64(v)
    gc = g * coef32
    tm, tg = b1 * m, omb1 * gc
    m1 = tm + tg
    v1 = b2 * v + omb2 * gc * gc
    root = v1.sqrt() / bc2sqrt_32
    den = root + eps32
    step_size = lr32 / bc1_32
    upd = step_size * m1 / den
    p1 = p * (1.0 - lr32 * wd32) - upd
    return dict(p=p, tm=tm, tg=tg, m1=m1, v1=v1, root=root, den=den, step_size=step_size, upd=upd, p1=p1)


def update(p, g, m, v, coef32, lr32, bc1_32, bc2sqrt_32, beta1, beta2, eps, wd, exact=False):
    """AdamW on g * coef32 -> (p', m', v') in float64, from fp32 inputs and the fp32 scalars the kernel reads (exact=True: the
    coefficients are not rounded to fp32 either)"""
    q = _parts(p, g, m, v, coef32, lr32, bc1_32, bc2sqrt_32, beta1, beta2, eps, wd, exact)
    return q["p1"], q["m1"], q["v1"]


def bounds(p, g, m, v, coef32, lr32, bc1_32, bc2sqrt_32, beta1, beta2, eps, wd):
    """-> (lim_p, lim_m, lim_v): what |kernel - update(...)| may reach per element (the module's docstring)"""
    q = _parts(p, g, m, v, coef32, lr32, bc1_32, bc2sqrt_32, beta1, beta2, eps, wd)
    lim_m = C_M * U * (q["tm"].abs() + q["tg"].abs())
    lim_v = C_V * U * q["v1"]
    half = torch.where(q["v1"] > 0, lim_v / (2 * q["v1"]), torch.zeros_like(lim_v))
    rel_den = (half + C_DEN * U) * q["root"] / q["den"] + U
    lim_upd = q["upd"].abs() * (rel_den + C_UPD * U) + q["step_size"] * lim_m / q["den"]
    lim_p = C_P * U * q["p"].abs() + lim_upd + C_P1 * U * q["p1"].abs()
    return lim_p, lim_m, lim_v


def emulate_fp32(p, g, m, v, coef32, lr32, bc1_32, bc2sqrt_32, beta1, beta2, eps, wd):
    """The kernel's formula (optim.hip: adamw1) in torch's fp32 on the CPU, every operation rounded on its own (no fused
    multiply-add) -> (p', m', v') as fp32 tensors.  The CPU check of the bounds, not a reference."""
    b1, omb1, b2, omb2, eps32, wd32 = (torch.tensor(x, dtype=torch.float32) for x in _coefs(beta1, beta2, eps, wd))
    one = np.float32(1.0)
    decay = torch.tensor(one - np.float32(lr32) * np.float32(wd), dtype=torch.float32)
    step_size = torch.tensor(np.float32(lr32) / np.float32(bc1_32), dtype=torch.float32)
    coef, bc2s = torch.tensor(coef32, dtype=torch.float32), torch.tensor(bc2sqrt_32, dtype=torch.float32)
    p, g, m, v = (t.detach().to("cpu").to(torch.float32) for t in (p, g, m, v))
    g = g * coef
    p = p * decay
    m = b1 * m + omb1 * g
    v = b2 * v + omb2 * g * g
    p = p - step_size * (m / (v.sqrt() / bc2s + eps32))
    return p, m, v


def ratio(out, ref, lim):
    """largest |out - ref| / lim over the elements; an element whose limit is 0 must be exact (inf otherwise)"""
    d = (d64(out).reshape(-1) - ref.reshape(-1)).abs()
    lim = lim.reshape(-1)
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    r = torch.where(lim > 0, d / lim.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------- input families
# Each returns fp32 CPU tensors (p, g, m, v) of `n` elements.  v is the square of a random tensor, floored at 1e-30 or exactly 0.
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _v_of(r, zeros):
    v = r.square().clamp_min(1e-30)
    if zeros:
        v[::zeros] = 0.0
    return v


def family_normal(n, seed, g_scale=1.0, zeros=7):
    """p, m, g ~ N(0, 1) (g times g_scale), v = N(0, 1)^2 with every `zeros`-th entry exactly 0 (0: none)"""
    gn = _gen(seed)
    p, m, r = torch.randn(n, generator=gn), torch.randn(n, generator=gn), torch.randn(n, generator=gn)
    g = torch.randn(n, generator=gn) * g_scale
    return p, g, m, _v_of(r, zeros)


def family_wide(n, seed):
    """gradients whose magnitudes span 1e-6 .. 100 (log-uniform), moments and v spread likewise: the shape of a trained state,
    where most of exp_avg_sq is far below its largest entry"""
    gn = _gen(seed)
    p = torch.randn(n, generator=gn)
    mag = lambda: 10.0 ** (torch.rand(n, generator=gn) * 8 - 6)      # noqa: E731
    sign = lambda: torch.where(torch.rand(n, generator=gn) < 0.5, -1.0, 1.0)   # noqa: E731
    g, m = mag() * sign(), mag() * sign()
    return p, g, m, _v_of(mag(), 0)


def family_zero_grad(n, seed):
    """an all-zero gradient over random state (every 7th v exactly 0: den = eps there)"""
    p, g, m, v = family_normal(n, seed)
    return p, torch.zeros_like(g), m, v


def family_huge(n, seed):
    """gradient entries of size 1e15 (1e15 .. 4e15, both signs): with max_norm = 1 the clip coefficient is ~1e-17 and g * coef is
    ordinary again; v has no exact zeros (v' stays far above the denormals whatever the coefficient)"""
    p, g, m, v = family_normal(n, seed, zeros=0)
    gn = _gen(seed + 1)
    g = 1e15 * (1.0 + 3.0 * torch.rand(n, generator=gn)) * torch.where(g < 0, -1.0, 1.0)
    return p, g, m, v


FAMILIES = {"normal": family_normal, "small_grad": lambda n, s: family_normal(n, s, g_scale=1e-3), "wide": family_wide,
            "zero_grad": family_zero_grad, "huge": family_huge}
# (step preset, betas) of tests/test_gpu_optim_edges.py's scalar cases
STEPS = (0, 9, 999, 99999)
BETAS = ((0.9, 0.999), (0.9, 0.99), (0.0, 0.5))
