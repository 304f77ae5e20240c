"""Golden vectors for the mixup of the inputs from the reference's own `mixup_data` (build container only).

    TIM_REFERENCE=<checkout of the reference> python tests/golden/make_golden_mixup.py

Loads recognition/time_interval_machine/utils/mixup.py of the reference (torch + numpy only) with `Tensor.cuda` patched to the
identity, fixes numpy's and torch's seeds, and calls `mixup_data(x, y, alpha=0.2)` on three fp32 tensors of batch size 5 and a
dict of int64 targets with ignored (-1) entries.  tests/golden/mixup_small.npz keeps the inputs, lam, the permutation, the
three mixed tensors and the permuted targets as plain numbers.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# seed 3: the smallest seed whose permutation moves every item and whose lam is further than 1e-3 from 0 and 1, so that both
# terms of the mix carry weight in every row (Beta(0.2, 0.2) puts most seeds at a lam of 1e-6 or 1 - 1e-6)
SEED, ALPHA, B = 3, 0.2, 5
SHAPES = [(B, 3, 7), (B, 3, 10), (B, 4, 6)]
KEYS = ("verb", "noun", "action", "class_id")


def main():
    ref = os.environ.get("TIM_REFERENCE")
    if not ref:
        sys.exit("set TIM_REFERENCE to a checkout of the reference project")
    spec = importlib.util.spec_from_file_location(
        "ref_mixup", os.path.join(ref, "recognition", "time_interval_machine", "utils", "mixup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.Tensor.cuda = lambda self, *a, **k: self
    g = torch.Generator().manual_seed(SEED)
    x = [torch.randn(s, generator=g, dtype=torch.float32) for s in SHAPES]
    y = {k: torch.randint(0, 9, (B, 2), generator=g, dtype=torch.int64) for k in KEYS}
    y["verb"][1, 0] = y["noun"][1, 0] = y["action"][1, 0] = -1
    y["class_id"][:, 1] = -1
    y["class_id"][3, 0] = -1
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    mixed, y_a, y_b, lam = mod.mixup_data(x, y, alpha=ALPHA)
    torch.manual_seed(SEED)   # the permutation the call drew: torch's generator replays it from the same seed
    index = torch.randperm(B)
    assert all(torch.equal(y_b[k], y[k][index]) for k in KEYS)
    out = {"lam": np.float64(lam), "index": index.numpy().astype(np.int64), "alpha": np.float64(ALPHA)}
    for i, (a, m) in enumerate(zip(x, mixed)):
        out["x%d" % i], out["mixed%d" % i] = a.numpy(), m.numpy()
        assert m.dtype == torch.float32
    for k in KEYS:
        out["y_" + k], out["yb_" + k] = y[k].numpy(), y_b[k].numpy()
    np.savez(os.path.join(HERE, "mixup_small.npz"), **out)
    print("lam %.17g index %s" % (lam, index.tolist()))


if __name__ == "__main__":
    main()
