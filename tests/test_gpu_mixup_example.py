"""examples/train_graphed_synthetic.py: the captured training iteration redraws its mixup state on every replay."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

from tests import mixup_ref as R  # noqa: E402


def test_graphed_example_redraws_per_replay():
    import train_graphed_synthetic
    hist = train_graphed_synthetic.main(["--steps", "5", "--batch", "8", "--seed", "3"])
    assert len(hist) == 5 and all(math.isfinite(loss) for loss, _, _ in hist)
    assert len({lam for _, lam, _ in hist}) == 5
    # GraphedStep's three warm-up steps drew sets 0 - 2 of the seed; replay k is draw 3 + k, the same bits as anywhere else
    for k, (_, lam, index) in enumerate(hist):
        rl, margin = R.beta(3, 3 + k, 0.2)
        assert index == R.permutation(3, 3 + k, 8)[0].tolist()
        assert margin < R.NEAR or abs(lam - rl) <= 1e-5 * rl + 1e-45
    assert all(0.0 <= lam <= 1.0 for _, lam, _ in hist) and np.isfinite([h[0] for h in hist]).all()
