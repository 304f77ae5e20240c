"""16-bit feature stores (tim_amd/data.py, tim_amd/det_data.py: store_dtype; tim_amd/csrc/batch.hip: timhip_window_gather_st;
tim_amd/csrc/sampler.hip: timhip_window_batch_st, timhip_det_window_batch_st).  The fp32 element a batch returns is the exact
widening of the stored 16-bit one, everything else in a batch is what the fp32 path computes: all comparisons are bit for bit."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import data_oracle as D  # noqa: E402
from tim_amd import _lib as L  # noqa: E402
from tim_amd import synth  # noqa: E402
from tim_amd._lib import ptr  # noqa: E402
from tim_amd.data import DeviceWindowDataset, store_code  # noqa: E402
from tim_amd.det_data import DeviceDetectionDataset  # noqa: E402
from tests import det_batch_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.golden import batch_inputs, det_batch_inputs  # noqa: E402
from tests.test_batch_oracle import CASES  # noqa: E402

DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
MIXED = {"visual": F16, "audio": BF16}
STORES = [F16, BF16, MIXED]
IDS = ["fp16", "bf16", "mixed"]
I16 = torch.int16


def _stream():
    return torch.cuda.current_stream().cuda_stream


def per_modality(sd):
    return sd if isinstance(sd, dict) else {"visual": sd, "audio": sd}


def widened(x, dtype):
    """numpy fp32 -> rounded once to the storage type (torch CPU) and widened again, numpy fp32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def bits(t):
    """a tensor's words as integers (NaNs compare by their bits)"""
    t = t.detach()
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype)) if t.numel() else t


def same_bits(got, want):
    """device fp32 tensor against a numpy fp32 array, as uint32"""
    return tuple(got.shape) == want.shape and got.dtype == F32 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def rec_dataset(tb, store_dtype=F32):
    return DeviceWindowDataset(tb["windows"], tb["num_feats"], tb["window_size"], tb["max_visual_actions"], tb["max_audio_actions"],
                               tb["model_modality"], tb["v_feats"], tb["v_feat_times"], tb["a_feats"], tb["a_feat_times"], device=DEV,
                               store_dtype=store_dtype)


def det_dataset(tb, store_dtype=F32):
    return DeviceDetectionDataset(tb["windows"], tb["num_feats"], tb["window_size"], tb["max_visual_actions"], tb["max_audio_actions"],
                                  tb["model_modality"], tb["v_feats"], tb["v_feat_times"], tb["a_feats"], tb["a_feat_times"], device=DEV,
                                  store_dtype=store_dtype)


# ---- 1. every bit pattern ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,non_nan", [(F16, 63490), (BF16, 65282)], ids=["fp16", "bf16"])
def test_every_bit_pattern_is_widened_exactly(dtype, non_nan):
    """A one-video store whose 32 rows of 2048 hold all 65536 words, read back through the gather entry (`batch()`) and the
    batch entry (`next_batch()`): every non-NaN pattern - subnormals, +-0, +-inf - equals torch's CPU widening as uint32 (a
    flushed fp16 subnormal fails here), every NaN pattern comes out NaN.  The NaN patterns are those with all exponent bits
    set and a mantissa that is not 0: 2 * 1023 of fp16 and 2 * 127 of bf16, which leaves 63490 and 65282 patterns compared bit
    for bit, the two infinities of each type among them."""
    NFX, W = 4, 8
    words = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).reshape(32, 1, 2048)
    stored = words.view(dtype)
    ft = np.stack([np.arange(32) * 0.2, np.arange(32) * 0.2 + 1.0], 1).astype(np.float32)
    none = {"v_queries": np.zeros((0, 2), np.float32), "v_labels": np.zeros((0, 4), np.int64), "v_action_ids": np.zeros(0, np.int64),
            "v_narration_ids": [], "a_queries": np.zeros((0, 2), np.float32), "a_labels": np.zeros((0, 4), np.int64),
            "a_action_ids": np.zeros(0, np.int64), "a_narration_ids": []}
    windows = [dict(none, video_id="v", start_sec=0.0, feat_indices=np.arange(NFX * w, NFX * w + NFX)) for w in range(W)]
    ds = DeviceWindowDataset(windows, NFX, 1.6, 0, 0, "visual", {"v": stored}, {"v": ft}, device=DEV, store_dtype=dtype)
    assert ds.v["dtype"] == dtype and ds.v["feats"].dtype == dtype and ds.v["feats"].shape == (32, 2048) and ds.store_bytes() == 65536 * 2
    assert torch.equal(ds.v["feats"].cpu().view(I16), words.reshape(32, 2048))               # stored as they came, bit for bit
    want = stored.float().reshape(-1)
    nan = torch.isnan(want)
    assert int((~nan).sum()) == non_nan
    gathered = ds.batch(list(range(W)), np.zeros((W, NFX), np.int64))[0]
    smp = ds.sampler(W, shuffle=False)
    smp.visual.fill_(float("nan"))
    batched = smp.next_batch()[0]
    torch.cuda.synchronize()
    assert smp.window.tolist() == list(range(W))
    for got in (gathered, batched):
        got = got.cpu().reshape(-1)
        assert got.dtype == F32 and got.numel() == 65536
        assert torch.equal(bits(got)[~nan], bits(want)[~nan])
        assert bool(torch.isnan(got[nan]).all())
    sub = slice(1, 1024) if dtype == F16 else slice(1, 128)                                  # the positive subnormals: none flushed
    assert bool((batched.cpu().reshape(-1)[sub] > 0).all()) and bool((gathered.cpu().reshape(-1)[sub] > 0).all())


# ---- 2. against the reference's own samples -----------------------------------------------------------------------------
@pytest.mark.parametrize("store_dtype", STORES, ids=IDS)
@pytest.mark.parametrize("case", CASES)
def test_batch_is_the_references_samples_rounded_to_the_store(case, store_dtype):
    """tests/test_gpu_batch.py's call on a 16-bit store: features = the golden per-sample features rounded to the storage type
    and widened (C = 8: the aligned fast path; C = 12: the element path, every odd source row 8 bytes off 16); times, labels and
    ids the golden ones."""
    g = np.load(os.path.join(H.GOLDEN, case))
    tb = batch_inputs.make_tables(int(g["seed"]), str(g["modality"]))
    ds = rec_dataset(tb, store_dtype)
    sd = per_modality(store_dtype)
    idx = [5, 0, 3, 3, 6, 1, 2, 4]
    has_v, has_a = "visual" in tb["model_modality"], "audio" in tb["model_modality"]
    assert (not has_v or ds.v["feats"].dtype == sd["visual"] == ds.v["dtype"]) and (not has_a or ds.a["feats"].dtype == sd["audio"] == ds.a["dtype"])
    va = np.stack([g["va%d" % i] for i in idx]) if has_v else None
    aa = np.stack([g["aa%d" % i] for i in idx]) if has_a else None
    v, a, t, label, meta = ds.batch(idx, va, aa)
    torch.cuda.synchronize()
    changed = 0
    for b, i in enumerate(idx):
        if has_v:
            assert same_bits(v[b], widened(g["v%d" % i], sd["visual"]))
            changed += int((v[b].cpu().numpy() != g["v%d" % i]).sum())
        if has_a:
            assert same_bits(a[b], widened(g["a%d" % i], sd["audio"]))
            changed += int((a[b].cpu().numpy() != g["a%d" % i]).sum())
        assert np.array_equal(t[b].cpu().numpy(), g["t%d" % i]) and t.dtype == F32
        for k in ("verb", "noun", "action", "class_id"):
            assert np.array_equal(label[k][b].cpu().numpy(), g["%s%d" % (k, i)])
        assert np.array_equal(meta["v_action_ids"][b].cpu().numpy(), g["vid%d" % i])
        assert np.array_equal(meta["a_action_ids"][b].cpu().numpy(), g["aid%d" % i])
    assert changed > 0                                                # the store is 16-bit: the fp32 values are not what comes back
    ref = D.collate([D.getitem(tb, i, g["va%d" % i], g["aa%d" % i]) for i in idx])
    assert tuple(v.shape) == ref[0].shape and tuple(a.shape) == ref[1].shape and tuple(t.shape) == ref[2].shape


def det_want(tb, sd, window, va, aa, col=2, valid=None):
    """tests/det_batch_ref.batch with the features rounded to the store and widened"""
    has_v, has_a = "visual" in tb["model_modality"], "audio" in tb["model_modality"]
    v, a, t, label, meta = R.batch(tb, window, va if has_v else None, aa if has_a else None, col, valid=valid)
    return (widened(v, sd["visual"]) if has_v else v), (widened(a, sd["audio"]) if has_a else a), t, label, meta


def assert_det(out, want, nf):
    v, a, t, label, meta = out
    wv, wa, wt, wl, wm = want
    B = wt.shape[0]
    for got, ref in ((v, wv), (a, wa), (t, wt)):
        assert same_bits(got, ref) if ref.size else tuple(got.shape) == (B, 0)
    assert sorted(label) == sorted(wl) == sorted(R.LABEL_KEYS)
    for k in wl:
        assert label[k].dtype == (F32 if k.endswith("segments") else torch.int64) and label[k].shape == wl[k].shape, k
        assert np.array_equal(label[k].cpu().numpy(), wl[k]), k
    assert meta["window_start"].dtype == torch.float64 and np.array_equal(meta["window_start"].cpu().numpy(), wm["window_start"])
    assert meta["video_index"].dtype == torch.int32 and np.array_equal(meta["video_index"].cpu().numpy(), wm["video_index"])


@pytest.mark.parametrize("store_dtype", STORES, ids=IDS)
@pytest.mark.parametrize("modality", ["audio_visual", "visual", "audio"])
def test_detection_batch_is_the_restatement_rounded_to_the_store(modality, store_dtype):
    tb = det_batch_inputs.make_tables(81, modality)
    ds = det_dataset(tb, store_dtype)
    sd = per_modality(store_dtype)
    idx = [5, 0, 5, 7, 2, 1, 0, 6, 3, 4]
    rs = np.random.RandomState(3)
    va = rs.randint(0, det_batch_inputs.V_NUM_AUG, (len(idx), det_batch_inputs.NF))
    aa = rs.randint(0, det_batch_inputs.A_NUM_AUG, (len(idx), det_batch_inputs.NF))
    out = ds.batch(idx, va if ds.has_v else None, aa if ds.has_a else None)
    torch.cuda.synchronize()
    want = det_want(tb, sd, idx, va, aa)
    assert_det(out, want, det_batch_inputs.NF)
    assert out[4]["video_id"] == want[4]["video_id"]
    plain = R.batch(tb, idx, va if ds.has_v else None, aa if ds.has_a else None, 2)
    assert (ds.has_v and not np.array_equal(want[0], plain[0])) or (ds.has_a and not np.array_equal(want[1], plain[1]))


# ---- 3. raw calls into guarded buffers -----------------------------------------------------------------------------------
PATTERN = {torch.int64: -7777, torch.int32: 0x5A5A5A5A}
NF2, B3, AUG3 = 2, 3, 3
WIDTHS = [1, 7, 8, 9, 24, 2056]        # 2056: wider than the 2048 elements one wave covers in a 16-bit row


class Guard:
    """Outputs of raw calls, NaN-prefilled (integers: a pattern), each between two guard runs of 8 elements.  shift: floats of
    extra offset in front of a feature output, so that it lies 4 * shift bytes off 16-byte alignment."""

    def __init__(self):
        self.full = []

    def alloc(self, shape, dtype, shift=0):
        n = int(np.prod(shape))
        fill = float("nan") if dtype.is_floating_point else PATTERN[dtype]
        full = torch.full((n + 16 + shift,), fill, dtype=dtype, device=DEV)
        assert full.data_ptr() % 16 == 0
        self.full.append((full, 8 + shift, n, full.clone()))
        return full[8 + shift:8 + shift + n].view(shape)

    def guards_intact(self):
        return all(torch.equal(bits(f[:lo]), bits(p[:lo])) and torch.equal(bits(f[lo + n:]), bits(p[lo + n:])) for f, lo, n, p in self.full)

    def untouched(self):
        return all(torch.equal(bits(f), bits(p)) for f, _, _, p in self.full)

    def all_written(self):
        """no element of a floating-point output kept its NaN (the tables hold none)"""
        return all(not bool(torch.isnan(f[lo:lo + n]).any()) for f, lo, n, _ in self.full if f.dtype.is_floating_point)

    def snapshot(self):
        return [bits(f).clone() for f, _, _, _ in self.full]


def rec_tables(width):
    return batch_inputs.make_tables(4, "audio_visual", nf=NF2, num_aug=AUG3, Cv=width, Ca=width)


def det_tables(width):
    """the detection tables at num_feats = 2 with three augmentations on the audio side as well"""
    tb = det_batch_inputs.make_tables(81, "audio_visual", nf=NF2, Cv=width, Ca=width)
    tb = dict(tb, a_feats={v: synth.normal(81, "daf3" + v, (x.shape[0], AUG3, width)).astype(np.float32) for v, x in tb["a_feats"].items()},
              a_num_aug=AUG3)
    assert all(x.shape[1] == AUG3 for x in tb["v_feats"].values())
    return tb


class RecCall:
    """A WindowSampler whose outputs are guarded buffers: `desc()` is the descriptor of a raw timhip_window_batch(_st) call"""

    def __init__(self, ds, shift=0):
        self.ds, self.g = ds, Guard()
        smp = self.smp = ds.sampler(B3, shuffle=False)
        g = self.g
        smp.visual, smp.audio = g.alloc(smp.visual.shape, F32, shift), g.alloc(smp.audio.shape, F32, shift)
        smp.times = g.alloc(smp.times.shape, F32)
        for k in smp.label:
            smp.label[k] = g.alloc(smp.label[k].shape, torch.int64)
        for k in ("v_action_ids", "a_action_ids"):
            smp.metadata[k] = g.alloc(smp.metadata[k].shape, torch.int64)

    def words(self, window, valid, va, aa):
        s = self.smp
        s.window.copy_(torch.tensor(window, dtype=torch.int32))
        s.valid.copy_(torch.tensor(valid, dtype=torch.uint8))
        s.v_aug.copy_(torch.as_tensor(np.asarray(va)).to(torch.int32))
        s.a_aug.copy_(torch.as_tensor(np.asarray(aa)).to(torch.int32))

    def desc(self):
        return self.smp._descriptor()

    def call(self, lib, stores=None, d=None):
        d = self.desc() if d is None else d
        if stores is None:
            return lib.timhip_window_batch(C.byref(d), _stream())
        return lib.timhip_window_batch_st(C.byref(d), stores[0], stores[1], _stream())

    def check(self, tb, sd, window, valid, va, aa):
        s = self.smp
        v, a, t, label, meta = D.collate([D.getitem(tb, int(w), np.asarray(va)[b], np.asarray(aa)[b]) for b, w in enumerate(window)])
        gone = np.asarray(valid) == 0
        for x in list(label.values()) + list(meta.values()):
            x[gone] = -1
        assert same_bits(s.visual, widened(v, sd["visual"])) and same_bits(s.audio, widened(a, sd["audio"])) and same_bits(s.times, t.astype(np.float32))
        for k in label:
            assert np.array_equal(s.label[k].cpu().numpy(), label[k]), k
        for k in ("v_action_ids", "a_action_ids"):
            assert np.array_equal(s.metadata[k].cpu().numpy(), meta[k]), k


class DetCall:
    def __init__(self, ds, shift=0):
        self.ds, self.g = ds, Guard()
        nf = ds.num_feats
        # (the feature outputs are the three-dimensional fp32 ones whose rows are not (start, end) pairs: no width here is 2)
        self.out = ds._outputs(B3, lambda shape, dtype: self.g.alloc(shape, dtype, shift if len(shape) == 3 and shape[1] == nf and shape[2] != 2 else 0))
        self.w = None

    def words(self, window, valid, va, aa):
        dev = lambda x, dt: torch.as_tensor(np.asarray(x)).to(device=DEV, dtype=dt).contiguous()   # noqa: E731
        self.w = (dev(window, torch.int32), dev(valid, torch.uint8), dev(va, torch.int32), dev(aa, torch.int32))

    def desc(self):
        return self.ds._descriptor(B3, *self.w, self.out)

    def call(self, lib, stores=None, d=None):
        d = self.desc() if d is None else d
        if stores is None:
            return lib.timhip_det_window_batch(C.byref(d), _stream())
        return lib.timhip_det_window_batch_st(C.byref(d), stores[0], stores[1], _stream())

    def check(self, tb, sd, window, valid, va, aa):
        v, a, t, label, start, vidx = self.out
        assert_det((v, a, t, label, {"window_start": start, "video_index": vidx}),
                   det_want(tb, sd, window, va, aa, 2, valid=np.asarray(valid)), self.ds.num_feats)


_RAW = {}


def raw_case(kind, width, name):
    """(tables, dataset) of one raw-call case, built once"""
    key = (kind, width, name)
    if key not in _RAW:
        tb = rec_tables(width) if kind == "rec" else det_tables(width)
        sd = dict(zip(IDS + ["fp32"], STORES + [F32]))[name]
        _RAW[key] = (tb, (rec_dataset if kind == "rec" else det_dataset)(tb, sd), per_modality(sd))
    return _RAW[key]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "dst+4B"])
@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", ["rec", "det"])
def test_raw_call_into_guarded_buffers(kind, width, name, shift):
    """num_feats = 2, B = 3, num_aug = 3.  Widths 8, 24 and 2056 take 16-byte chunks where source row and destination row are
    aligned (a 16-bit row of 24 elements is 48 bytes: every row; the fp32 output rows too), 1, 7 and 9 go element by element, and
    so does every row once the destination lies 4 bytes off.  Guards intact, every output element written, a row with valid = 0
    as the fp32 path leaves it, a repeated call gives equal bits; window words of -1 and num_windows and augmentation words of
    -1 and num_aug are read as 0."""
    lib = L.load()
    tb, ds, sd = raw_case(kind, width, name)
    N = len(tb["windows"])
    stores = (store_code(ds.v), store_code(ds.a))
    assert stores != (L.STORE_F32, L.STORE_F32)
    window, valid = [N - 1, 0, 3], [1, 0, 1]
    rs = np.random.RandomState(width)
    va, aa = rs.randint(0, AUG3, (B3, NF2)), rs.randint(0, AUG3, (B3, NF2))
    c = (RecCall if kind == "rec" else DetCall)(ds, shift)
    c.words(window, valid, va, aa)
    assert c.call(lib, stores) == 0
    torch.cuda.synchronize()
    assert c.g.guards_intact() and c.g.all_written()
    c.check(tb, sd, window, valid, va, aa)
    first = c.g.snapshot()
    assert c.call(lib, stores) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, c.g.snapshot()))
    h = (RecCall if kind == "rec" else DetCall)(ds, shift)
    h.words([-1, N, 2], [1, 1, 1], [[-1, AUG3]] * B3, [[AUG3, -1]] * B3)
    assert h.call(lib, stores) == 0
    torch.cuda.synchronize()
    assert h.g.guards_intact() and h.g.all_written()
    zero = np.zeros((B3, NF2), np.int64)
    h.check(tb, sd, [0, 0, 2], [1, 1, 1], zero, zero)


@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("width", WIDTHS)
def test_raw_gather_into_guarded_buffers(width, name):
    """timhip_window_gather_st on the same stores: aligned and 4 bytes off, guards intact, repeated with equal bits"""
    lib = L.load()
    tb, ds, sd = raw_case("rec", width, name)
    N = len(tb["windows"])
    window = [N - 1, 0, 3]
    rs = np.random.RandomState(width + 1)
    aug = rs.randint(0, AUG3, (B3, NF2))
    win, aug_d = torch.tensor(window, dtype=torch.int32, device=DEV), torch.as_tensor(aug).to(device=DEV, dtype=torch.int32)
    v, a = D.collate([D.getitem(tb, w, aug[b], aug[b]) for b, w in enumerate(window)])[:2]
    for shift in (0, 1):
        for store, row0, ref, m in ((ds.v, ds.v_row0, v, "visual"), (ds.a, ds.a_row0, a, "audio")):
            if store_code(store) == L.STORE_F32:
                continue
            g = Guard()
            out = g.alloc((B3, NF2, width), F32, shift)
            args = (ptr(store["feats"]), store_code(store), width, AUG3, ptr(row0), ptr(ds.feat_indices), NF2, ptr(win), B3, ptr(aug_d), ptr(out), _stream())
            assert lib.timhip_window_gather_st(*args) == 0
            torch.cuda.synchronize()
            assert g.guards_intact() and same_bits(out, widened(ref, sd[m]))
            first = g.snapshot()
            assert lib.timhip_window_gather_st(*args) == 0
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(first, g.snapshot()))


@pytest.mark.parametrize("kind", ["rec", "det"])
def test_refused_calls_launch_nothing(kind):
    """A store type outside the enum: TIMHIP_EINVAL.  A 16-bit store pointer off 2 bytes: TIMHIP_EALIGN (off 2 bytes of 4 it is
    taken).  The refusals of the fp32 entries, unchanged, under 16-bit store types too.  Nothing is written."""
    lib = L.load()
    tb, ds, sd = raw_case(kind, 8, "mixed")
    c = (RecCall if kind == "rec" else DetCall)(ds)
    zero = np.zeros((B3, NF2), np.int64)
    c.words([0, 1, 2], [1, 1, 1], zero, zero)
    good = (L.STORE_F16, L.STORE_BF16)
    for stores in ((-1, L.STORE_F16), (3, L.STORE_F16), (L.STORE_F16, 3), (L.STORE_BF16, -1), (1 << 20, 0)):
        assert c.call(lib, stores) == L.EINVAL, stores
    entry = lib.timhip_window_batch_st if kind == "rec" else lib.timhip_det_window_batch_st
    assert entry(None, *good, _stream()) == L.EINVAL
    for field in ("v_feats", "a_feats"):
        d = c.desc()
        setattr(d, field, getattr(d, field) + 1)
        assert c.call(lib, good, d) == L.EALIGN, field
    d = c.desc()
    d.v_feats += 2                                                    # an fp32 store wants 4 bytes
    assert c.call(lib, (L.STORE_F32, L.STORE_BF16), d) == L.EALIGN
    bad = [("window", None), ("valid", None), ("times", None), ("visual", None), ("a_row0", None), ("verb", None), ("feat_indices", None),
           ("B", 0), ("num_feats", 0), ("num_windows", 0), ("window_size", 0.0), ("v_ld", 1), ("Ca", 0), ("a_num_aug", 0), ("max_v", -1)]
    bad += [("a_ids", None)] if kind == "rec" else [("action_col", 3), ("window_start", None), ("video_of", None), ("v_gt_segments", None)]
    for field, value in bad:
        d = c.desc()
        setattr(d, field, value)
        assert c.call(lib, good, d) == L.EINVAL, (field, value)
    for field, off in (("visual", 2), ("times", 1), ("audio", 3)):
        d = c.desc()
        setattr(d, field, getattr(d, field) + off)
        assert c.call(lib, good, d) == L.EALIGN, field
    # the gather entry
    out = c.g.alloc((B3, NF2, 8), F32)
    win, aug = torch.zeros(B3, dtype=torch.int32, device=DEV), torch.zeros((B3, NF2), dtype=torch.int32, device=DEV)
    gargs = dict(feats=ptr(ds.v["feats"]), store=L.STORE_F16, C=8, num_aug=AUG3, row0=ptr(ds.v_row0), fi=ptr(ds.feat_indices), nf=NF2, win=ptr(win), B=B3,
                 aug=ptr(aug), out=ptr(out))
    gather = lambda **kw: lib.timhip_window_gather_st(*dict(gargs, **kw).values(), _stream())   # noqa: E731
    for kw in (dict(store=-1), dict(store=3), dict(feats=None), dict(row0=None), dict(fi=None), dict(win=None), dict(out=None), dict(C=0), dict(num_aug=0),
               dict(nf=0), dict(B=-1)):
        assert gather(**kw) == L.EINVAL, kw
    assert gather(feats=ds.v["feats"].data_ptr() + 1) == L.EALIGN and gather(feats=ds.v["feats"].data_ptr() + 1, store=L.STORE_BF16) == L.EALIGN
    torch.cuda.synchronize()
    assert c.g.untouched()
    assert c.call(lib, good) == 0 and gather() == 0                  # what the refusals were cut from is good
    torch.cuda.synchronize()
    assert c.g.guards_intact() and c.g.all_written()


@pytest.mark.parametrize("width", [8, 9, 1100])
@pytest.mark.parametrize("kind", ["rec", "det"])
def test_fp32_stores_through_the_new_entries_are_the_old_entries(kind, width):
    """fp32 / fp32 under the `_st` entries: the bits of the entries without a store type (the same kernel instance), the gather
    included.  1100 floats: 275 chunks, more than one wave's 256."""
    lib = L.load()
    tb, ds, sd = raw_case(kind, width, "fp32")
    assert ds.v["feats"].dtype == F32 and ds.v["dtype"] == F32 and store_code(ds.a) == L.STORE_F32
    N = len(tb["windows"])
    window, valid = [N - 1, 0, 3], [1, 0, 1]
    rs = np.random.RandomState(7)
    va, aa = rs.randint(0, AUG3, (B3, NF2)), rs.randint(0, AUG3, (B3, NF2))
    snaps = []
    for stores in (None, (L.STORE_F32, L.STORE_F32)):
        c = (RecCall if kind == "rec" else DetCall)(ds)
        c.words(window, valid, va, aa)
        assert c.call(lib, stores) == 0
        torch.cuda.synchronize()
        assert c.g.guards_intact() and c.g.all_written()
        c.check(tb, sd, window, valid, va, aa)
        snaps.append(c.g.snapshot())
    assert all(torch.equal(x, y) for x, y in zip(*snaps))
    win, aug = torch.tensor(window, dtype=torch.int32, device=DEV), torch.as_tensor(va).to(device=DEV, dtype=torch.int32)
    old, new = torch.full((B3, NF2, width), float("nan"), device=DEV), torch.full((B3, NF2, width), float("nan"), device=DEV)
    tail = (width, AUG3, ptr(ds.v_row0), ptr(ds.feat_indices), NF2, ptr(win), B3, ptr(aug))
    assert lib.timhip_window_gather(ptr(ds.v["feats"]), *tail, ptr(old), _stream()) == 0
    assert lib.timhip_window_gather_st(ptr(ds.v["feats"]), L.STORE_F32, *tail, ptr(new), _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(old), bits(new)) and not bool(torch.isnan(new).any())


# ---- 4. the samplers -----------------------------------------------------------------------------------------------------
def flat(out):
    v, a, t, label, meta = out
    return [v, a, t] + [label[k] for k in sorted(label)] + [meta[k] for k in sorted(meta)]


@pytest.mark.parametrize("store_dtype", STORES, ids=IDS)
@pytest.mark.parametrize("kind", ["rec", "det"])
def test_sampler_over_a_16_bit_store_eager_and_replayed(kind, store_dtype):
    """Four eager `next_batch()` calls and four replays of a captured one: the same bits, equal to `batch()` on the windows and
    augmentation indices the sampler drew, in tensors that keep their addresses."""
    tb = batch_inputs.make_tables(4, "audio_visual") if kind == "rec" else det_batch_inputs.make_tables(81, "audio_visual")
    ds = (rec_dataset if kind == "rec" else det_dataset)(tb, store_dtype)
    B, seed = 3, 13
    eager, smp = ds.sampler(B, seed=seed), ds.sampler(B, seed=seed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = flat(smp.next_batch())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    smp.set_iteration(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = smp.next_batch()
    torch.cuda.synchronize()
    assert int(smp.counter.item()) == 0 and all(x is y for x, y in zip(flat(out), warm))
    addresses, absent = [x.data_ptr() for x in warm], 0
    for t in range(4):
        graph.replay()
        e_out = eager.next_batch()
        torch.cuda.synchronize()
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(flat(out), flat(e_out))), t
        assert [x.data_ptr() for x in flat(out)] == addresses
        assert out[0].dtype == out[1].dtype == F32
        bv, ba, bt, bl, bm = ds.batch(smp.window.cpu(), smp.v_aug.cpu(), smp.a_aug.cpu())
        torch.cuda.synchronize()
        ok = smp.valid != 0
        absent += int((~ok).sum())
        assert torch.equal(bits(out[0]), bits(bv)) and torch.equal(bits(out[1]), bits(ba)) and torch.equal(bits(out[2]), bits(bt))
        assert all(torch.equal(out[3][k][ok], bl[k][ok]) for k in bl)
        for k in ("v_action_ids", "a_action_ids", "window_start", "video_index"):
            if k in bm and k in out[4]:
                rows = ok if k.endswith("ids") else slice(None)
                assert torch.equal(out[4][k][rows], bm[k][rows]), k
    assert absent > 0                                                 # a short last batch was among them


# ---- 5. the model loses nothing at evaluation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,dtype", [("fp16", F16), ("bf16", BF16)])
def test_model_outputs_from_a_16_bit_store_are_those_from_the_fp32_store(prec, dtype):
    """The tiny model in a 16-bit mode under eval() / no_grad on the same batch of two datasets over the same tables, one held
    in fp32 and one in the model's operand type: the logits of all heads and `feats` are equal bit for bit, because the
    embedders' input cast (`_embedders_fwd`: timhip_cast_rows / timhip_cast_rows_pair) is a plain round-to-nearest of the fp32
    input, and rounding a value that is already a 16-bit one changes nothing."""
    from tim_amd.tim import TIM
    cfg = H.tiny_cfg("recognition", "audio_visual", "audio_visual", True)
    tb = copy.deepcopy(batch_inputs.make_tables(4, "audio_visual", nf=cfg.num_feats, Cv=cfg.visual_input_dim, Ca=cfg.audio_input_dim))
    sd, _ = H.synth_torch(cfg, 2, 2, 2, seed=3, dtype=F32)
    model = TIM(cfg.num_class, visual_input_dim=cfg.visual_input_dim, audio_input_dim=cfg.audio_input_dim, d_model=cfg.d_model,
                nhead=cfg.nhead, num_layers=cfg.num_layers, num_feats=cfg.num_feats, precision=prec)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    wide, narrow = rec_dataset(tb, F32), rec_dataset(tb, dtype)
    idx = [5, 0, 3, 3, 6, 1, 2, 4]
    rs = np.random.RandomState(2)
    va, aa = rs.randint(0, tb["num_aug"], (len(idx), cfg.num_feats)), rs.randint(0, tb["num_aug"], (len(idx), cfg.num_feats))
    outs = []
    with torch.no_grad():
        for ds in (wide, narrow):
            visual, audio, times, _, _ = ds.batch(idx, va, aa)
            cls, feats = model([visual, audio], "encoder", model(times, "time_mlp"), tb["max_visual_actions"], tb["max_audio_actions"])
            torch.cuda.synchronize()
            outs.append(([c.clone() for c in cls if c is not None] + [feats.clone()], visual.clone(), audio.clone()))
    (a, av, aa_), (b, bv, ba_) = outs
    assert not torch.equal(av, bv) and not torch.equal(aa_, ba_)      # the two batches differ: one is rounded
    assert torch.equal(av.to(dtype), bv.to(dtype)) and torch.equal(bv.to(dtype).float(), bv)
    assert len(a) == len(b) >= 2
    for x, y in zip(a, b):
        assert x.shape == y.shape and bool(torch.isfinite(x).all()) and torch.equal(bits(x), bits(y))


# ---- 6. bytes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rec", "det"])
def test_store_bytes_halve(kind):
    tb = batch_inputs.make_tables(4, "audio_visual") if kind == "rec" else det_batch_inputs.make_tables(81, "audio_visual")
    make = rec_dataset if kind == "rec" else det_dataset
    wide = make(tb, F32).store_bytes()
    elements = sum(x.size for x in tb["v_feats"].values()) + sum(x.size for x in tb["a_feats"].values())
    assert wide == 4 * elements                                       # the features alone: their times are not counted
    assert make(tb, F16).store_bytes() * 2 == wide and make(tb, BF16).store_bytes() * 2 == wide
    assert make(tb, {"visual": F16}).store_bytes() == 2 * sum(x.size for x in tb["v_feats"].values()) + 4 * sum(x.size for x in tb["a_feats"].values())
