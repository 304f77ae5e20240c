"""examples/train_detection_graphed_synthetic.py: the captured detection iteration draws and assembles its batch on the device
on every replay."""
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

from tests import sampler_ref as R  # noqa: E402

_HIST = []


def two_runs():
    """the example twice with one seed, 6 steps at batch 4, in fp32 mode: the mode whose training step repeats its bits from run
    to run but for a rare last place (run once, shared by the tests below)"""
    if not _HIST:
        import train_detection_graphed_synthetic as ex
        for _ in range(2):
            _HIST.append(ex.main(["--steps", "6", "--batch", "4", "--seed", "5", "--precision", "fp32"]))
    return _HIST


def test_detection_example_redraws_per_replay():
    hist, again = two_runs()
    assert len(hist) == 6 and all(math.isfinite(loss) for loss, *_ in hist + again)      # every loss is finite
    assert len({tuple(w) for _, w, _, _ in hist}) == 6                    # window lists differ between replays
    # GraphedStep's three warm-up steps drew iterations 0 - 2 of the seed; replay k is iteration 3 + k (48 windows, 12 per epoch)
    for k, (_, windows, epoch, norm) in enumerate(hist):
        d = R.draw(5, 3 + k, 48, 1, 0, 4, True, "drop")
        assert windows == d["window"].tolist() and epoch == d["epoch"] == 0 and d["valid"].all()
        assert all(math.isfinite(n) and n > 0 for n in norm)
    assert len({w for _, ws, _, _ in hist for w in ws}) == 24             # six batches of one epoch: no window twice
    assert hist[0][3] != hist[-1][3]                                      # the normalisers advanced on the device
    assert [h[1:3] for h in again] == [h[1:3] for h in hist]              # one seed, two runs: the same windows and epochs


def test_two_runs_with_one_seed_print_identical_histories():
    """The lines the example prints (window numbers and the loss to four decimals), two runs with one seed.

    The example sums its side losses in a fixed order (`ordered=True`), so the loss of one state is one number.  In fp32 mode the
    step itself repeated its bits in 11 of 12 measured runs (the twelfth differed in the last place of one loss, 8.91257381 /
    8.91257477, both printed 8.9126).  In the example's default fp16 mode the backward is not reproducible from run to run
    (tests/test_gpu_graph.py holds a replay to an eager step within 1e-5 for that reason): three runs printed 14.8246 / 14.8245 /
    14.8246 at replay 0 and 8.9095 / 8.9095 / 8.9095 at replay 2, the windows identical - which is why this test runs fp32."""
    hist, again = two_runs()
    line = lambda h: "epoch %d  windows %s  loss %.4f" % (h[2], h[1], h[0])   # noqa: E731
    print("\n".join("%s   |   %s" % (line(a), line(b)) for a, b in zip(hist, again)))
    assert [line(h) for h in again] == [line(h) for h in hist]
