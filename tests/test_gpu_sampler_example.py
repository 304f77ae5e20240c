"""examples/train_graphed_device_data_synthetic.py: the captured training iteration draws its batch, its mixup state and its
DRLoc positions on the device on every replay."""
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

from tests import sampler_ref as R  # noqa: E402


def test_device_data_example_redraws_per_replay():
    import train_graphed_device_data_synthetic as ex
    hist = ex.main(["--steps", "5", "--batch", "8", "--seed", "3"])
    assert len(hist) == 5 and all(math.isfinite(loss) for loss, *_ in hist)
    assert len({tuple(w) for _, _, w, _, _ in hist}) == 5                 # window sets differ between replays
    assert len({lam for _, lam, *_ in hist}) == 5 and all(0.0 <= lam <= 1.0 for _, lam, *_ in hist)
    assert len({tuple(p) for *_, p in hist}) == 5                         # so do the DRLoc positions
    # GraphedStep's three warm-up steps drew iterations 0 - 2 of the seed; replay k is iteration 3 + k, the same bits as anywhere else
    for k, (_, _, windows, epoch, pos) in enumerate(hist):
        d = R.draw(3, 3 + k, 64, 1, 0, 8, True, "wrap")
        assert windows == d["window"].tolist() and epoch == d["epoch"] == 0
        assert pos == R.drloc(3, 3 + k, 8, 8, 6)[0][0].tolist()         # (tiny: 6 features per modality, 8 samples per window)
    assert len({w for _, _, ws, _, _ in hist for w in ws}) == 40          # five batches of one epoch: no window twice
    again = ex.main(["--steps", "5", "--batch", "8", "--seed", "3"])
    assert [h[1:] for h in again] == [h[1:] for h in hist]                # the same windows, lam and positions
    assert np.isfinite([h[0] for h in again]).all()
