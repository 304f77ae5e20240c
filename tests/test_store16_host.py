"""The host side of the 16-bit feature stores (tim_amd/data.py: store_dtypes, round_to_store): the rounding a store is built
with against numpy's and torch's own casts, the bit-for-bit pass of an input already in the storage type, the refusal of an
overflow.  Needs no GPU."""
import os

import numpy as np
import pytest
import torch

from tim_amd.data import DeviceWindowDataset, round_to_store, store_dtypes
from tim_amd.det_data import DeviceDetectionDataset
from tests.golden.batch_inputs import make_tables
from tests.helpers import GOLDEN
from tests.test_batch_oracle import CASES


def feature_tables():
    """(modality, video, array) of every feature table the golden batch cases are built from"""
    out = []
    for case in CASES:
        g = np.load(os.path.join(GOLDEN, case))
        tb = make_tables(int(g["seed"]), str(g["modality"]))
        out += [("visual", v, x) for v, x in sorted((tb["v_feats"] or {}).items())]
        out += [("audio", v, x) for v, x in sorted((tb["a_feats"] or {}).items())]
    assert out
    return out


def test_rounding_is_numpys_and_torchs_own_cast_and_changes_the_tables():
    """every value of the golden feature tables stays finite in fp16 (largest magnitude below 4) and essentially all of them
    change when rounded: a store that silently stayed fp32 cannot pass the GPU tests"""
    total, changed = 0, {torch.float16: 0, torch.bfloat16: 0}
    for modality, video, x in feature_tables():
        assert x.dtype == np.float32 and np.abs(x).max() < 4.0
        h = round_to_store(x, torch.float16, modality, video)
        assert h.dtype == torch.float16 and h.shape == x.shape
        assert np.array_equal(h.numpy().view(np.uint16), x.astype(np.float16).view(np.uint16))
        b = round_to_store(x, torch.bfloat16, modality, video)
        assert b.dtype == torch.bfloat16 and torch.equal(b.view(torch.int16), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16))
        assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(b).all())
        total += x.size
        changed[torch.float16] += int((h.float().numpy() != x).sum())
        changed[torch.bfloat16] += int((b.float().numpy() != x).sum())
        # float64 input: rounded by the same one call
        assert torch.equal(round_to_store(x.astype(np.float64), torch.float16), torch.from_numpy(x.astype(np.float64)).to(torch.float16))
        # fp32 store: the .float() the store always did
        f = round_to_store(x, torch.float32)
        assert f.dtype == torch.float32 and np.array_equal(f.numpy().view(np.uint32), x.view(np.uint32))
    assert changed[torch.float16] / total >= 0.9997 and changed[torch.bfloat16] / total == 1.0


def test_a_16_bit_input_comes_back_with_the_same_bits():
    words = np.arange(65536, dtype=np.uint16).reshape(32, 1, 2048)            # every pattern, NaNs and subnormals included
    h = round_to_store(words.view(np.float16), torch.float16)
    assert h.dtype == torch.float16 and np.array_equal(h.numpy().view(np.uint16), words)
    b_in = torch.from_numpy(words.view(np.int16)).view(torch.bfloat16)
    b = round_to_store(b_in, torch.bfloat16)
    assert b.dtype == torch.bfloat16 and torch.equal(b.view(torch.int16), b_in.view(torch.int16))
    assert b.data_ptr() == b_in.data_ptr()                                   # not even a copy


def test_overflow_is_refused_with_the_count_and_non_finite_inputs_pass():
    x = np.ones((5, 2, 8), np.float32)
    x[1, 0, 3], x[4, 1, 7], x[2, 1, 0] = 1e5, -70000.0, 65504.0                   # two beyond fp16, its largest finite value
    with pytest.raises(ValueError) as e:
        round_to_store(x, torch.float16, "visual", "P01_07")
    assert "2 finite values" in str(e.value) and "visual" in str(e.value) and "P01_07" in str(e.value) and "float16" in str(e.value)
    assert bool(torch.isfinite(round_to_store(x, torch.bfloat16)).all())       # bf16 has fp32's range
    top = np.array([[[3.4028234e38, 1.0]]], np.float32)                           # the top of fp32 rounds up to inf in bf16
    with pytest.raises(ValueError) as e:
        round_to_store(top, torch.bfloat16, "audio", "P02")
    assert "1 finite value " in str(e.value) and "audio" in str(e.value) and "bfloat16" in str(e.value)
    y = np.array([[[np.inf, -np.inf, np.nan, 2.5]]], np.float32)
    for dt in (torch.float16, torch.bfloat16):
        r = round_to_store(y, dt).float().numpy()
        assert r[0, 0, 0] == np.inf and r[0, 0, 1] == -np.inf and np.isnan(r[0, 0, 2]) and r[0, 0, 3] == 2.5


def test_store_dtype_argument():
    assert store_dtypes(torch.float32) == {"visual": torch.float32, "audio": torch.float32}
    assert store_dtypes(torch.bfloat16) == {"visual": torch.bfloat16, "audio": torch.bfloat16}
    assert store_dtypes({"visual": torch.float16, "audio": torch.bfloat16}) == {"visual": torch.float16, "audio": torch.bfloat16}
    assert store_dtypes({"audio": torch.float16}) == {"visual": torch.float32, "audio": torch.float16}
    for bad in (torch.float64, torch.int16, "fp16", None, np.float16, {"visual": torch.int8}, {"video": torch.float16}, [torch.float16]):
        with pytest.raises(ValueError):
            store_dtypes(bad)
    # the constructors refuse it before anything else (no GPU is touched)
    tb = make_tables(4, "audio_visual")
    args = (tb["windows"], tb["num_feats"], tb["window_size"], tb["max_visual_actions"], tb["max_audio_actions"], tb["model_modality"],
            tb["v_feats"], tb["v_feat_times"], tb["a_feats"], tb["a_feat_times"])
    with pytest.raises(ValueError):
        DeviceWindowDataset(*args, store_dtype=torch.float64)
    with pytest.raises(ValueError):
        DeviceDetectionDataset(*args, store_dtype="bf16")
