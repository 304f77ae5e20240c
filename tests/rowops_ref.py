"""float64 restatements of the row kernels around the encoder layers (tim_amd/csrc/rowops.hip).

Written from the contracts in include/timhip.h and from what the model computes (oracle/tim_oracle.py): plain loops
over (b, s) that read a TimSeqRow table, plain matrix products, autograd for the gradients.  tests/test_rowops_ref.py
pins them against the oracle on the CPU; tests/test_gpu_rowops.py holds every C entry point to them on the GPU.
All tensors are CPU float64 unless said otherwise.
"""
import math

import torch

F64 = torch.float64
EPS32 = 2.0 ** -24      # unit roundoff of fp32 (half an ulp, relative)
# half an ulp of a STORED value, relative: a type with p significand bits rounds to nearest within 2^-p of the value (bf16 p = 8, fp16 p = 11)
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY16 = {torch.float32: 0.0, torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}   # half the fp16 subnormal step (absolute)


def d64(t):
    return t.detach().to("cpu").to(F64)


def store_bound(ref, dtype):
    """what rounding a value to `dtype` (round to nearest) may add to an error, elementwise: half an ulp of the stored type"""
    return ref.abs() * HALF_ULP[dtype] + TINY16[dtype]


# ---------------------------------------------------------------------------------------------- time MLP, layer 1
def time_l1(times, w, b):
    """h[r, j] = relu(times[r, 0] w[j, 0] + times[r, 1] w[j, 1] + b[j])      times [rows, 2], w [d, 2], b [d]"""
    return torch.relu(times @ w.t() + b)


def time_l1_abs_terms(times, w, b):
    """sum of |terms| of every pre-activation: the scale of its fp32 rounding error"""
    return times.abs() @ w.abs().t() + b.abs()


def time_l1_bwd(times, w, dh):
    """dh: gradient w.r.t. h with the relu mask ALREADY applied (include/timhip.h) -> (dw [d, 2], db [d], dt [rows, 2]):
    autograd through the affine part"""
    t = times.clone().requires_grad_(True)
    ww = w.clone().requires_grad_(True)
    bb = torch.zeros(w.shape[0], dtype=F64, requires_grad=True)
    ((t @ ww.t() + bb) * dh).sum().backward()
    return ww.grad, bb.grad, t.grad


# ---------------------------------------------------------------------------------------------- sequence assembly
def assemble(table, B, d, e0, e1, cls, te, mod):
    """table: S rows (kind, src, te_row, mod) as TimSeqRow.  x[b, s, :d] = e0[b, src] (kind 0) | e1[b, src] (kind 2) |
    cls[src] (kind 1); x[b, s, d:] = te[b, te_row]; + mod[mod] over all 2 d columns when mod >= 0.
    e0 / e1: [B, n_e, d] or None; cls: list of [d]; te: [B, T, d]; mod: list of [2 d].  Returns [B, S, 2 d]."""
    out = []
    for b in range(B):
        for (kind, src, te_row, m) in table:
            left = cls[src] if kind == 1 else (e0 if kind == 0 else e1)[b, src]
            row = torch.cat([left, te[b, te_row]])
            if m >= 0:
                row = row + mod[m]
            out.append(row)
    return torch.stack(out).reshape(B, len(table), 2 * d)


def assemble_bwd(table, B, d, dx, n_e, T, ncls, nmod):
    """dx [B, S, 2 d] -> dict: d_e0 / d_e1 [B, n_e, d] (rows the table does not name stay zero; `wrote0` / `wrote1` say which
    were written), d_cls (ncls x [d]), d_mod (nmod x [2 d]), d_te [B, T, d] - the sums over every (b, s) that read them."""
    g = {"d_e0": torch.zeros(B, n_e, d, dtype=F64), "d_e1": torch.zeros(B, n_e, d, dtype=F64),
         "wrote0": torch.zeros(n_e, dtype=torch.bool), "wrote1": torch.zeros(n_e, dtype=torch.bool),
         "d_cls": [torch.zeros(d, dtype=F64) for _ in range(ncls)], "d_mod": [torch.zeros(2 * d, dtype=F64) for _ in range(nmod)],
         "d_te": torch.zeros(B, T, d, dtype=F64)}
    for b in range(B):
        for s, (kind, src, te_row, m) in enumerate(table):
            row = dx[b, s]
            if kind == 1:
                g["d_cls"][src] += row[:d]
            else:
                g["d_e0" if kind == 0 else "d_e1"][b, src] += row[:d]
                g["wrote0" if kind == 0 else "wrote1"][src] = True
            g["d_te"][b, te_row] += row[d:]
            if m >= 0:
                g["d_mod"][m] += row
    return g


def assemble_abs(table, B, d, dx, T, ncls, nmod):
    """sum of |terms| of d_cls / d_mod / d_te (the scale of their fp32 summation error) and the number of terms of each"""
    a = assemble_bwd(table, B, d, dx.abs(), 1 + max([r[1] for r in table if r[0] != 1] or [0]), T, ncls, nmod)
    n_cls = [B * sum(1 for r in table if r[0] == 1 and r[1] == i) for i in range(ncls)]
    n_mod = [B * sum(1 for r in table if r[3] == i) for i in range(nmod)]
    n_te = [sum(1 for r in table if r[2] == t) for t in range(T)]
    return a, n_cls, n_mod, n_te


# ---------------------------------------------------------------------------------------------- LayerNorm
def act(a, x):
    if a == 1:
        return torch.relu(x)
    if a == 2:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x


def layernorm(y, w, b, a=0, eps=1e-5):
    """LN(act(y)) * w + b over the last dim, biased variance, two passes; also returns (mean, rstd)"""
    x = act(a, y)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * w + b, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(y, w, dx, a=0):
    """(dy, dgamma, dbeta) by autograd through layernorm()"""
    yy = y.clone().requires_grad_(True)
    ww = w.clone().requires_grad_(True)
    bb = torch.zeros_like(w).requires_grad_(True)
    (layernorm(yy, ww, bb, a)[0] * dx).sum().backward()
    return yy.grad, ww.grad, bb.grad


# ---------------------------------------------------------------------------------------------- split operands
def split3(v32, dtype):
    """fp32 tensor -> (hi, lo) of the 16-bit type: hi = T(v), lo = T(v - hi) with the difference taken in fp32"""
    hi = v32.to(dtype)
    lo = (v32 - hi.float()).to(dtype)
    return hi, lo


# ---------------------------------------------------------------------------------------------- row moves
def gather_ranges(x, ranges):
    """x [B, S, E] -> per range (s0, n): [B * n, E] = x[b, s0 + j]"""
    B, _, E = x.shape
    return [x[:, s0:s0 + n].reshape(B * n, E).clone() for s0, n in ranges]


def scatter_ranges_add(dx, ranges, rows):
    """dx [B, S, E] += rows of each range (the inverse move, added)"""
    out = dx.clone()
    B, _, E = dx.shape
    for (s0, n), r in zip(ranges, rows):
        out[:, s0:s0 + n] += r.reshape(B, n, E)
    return out


def sigmoid_bwd(g, y, scale=1.0):
    return scale * g * y * (1.0 - y)
