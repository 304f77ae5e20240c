"""The detection sliding-window dataset on the device, and its capturable sampler.

The reference's detection `SlidingWindowDataset` (detection/time_interval_machine/datasets/sliding_window.py:324-399) differs
from the recognition one (`tim_amd.data.DeviceWindowDataset`) in every output but the features: `times` holds the feature times
only (the model builds its own query pyramid), times and ground-truth segments are rounded to 1e-3 s before they are divided by
the window size (`torch.round(t - start, decimals=3)`, in fp32), the targets carry `v_gt_segments` / `a_gt_segments`, the
`action` column depends on (`dataset_name`, `include_verb_noun`, `verb_only`), and the metadata is the window's start, size
and video.  `DeviceDetectionDataset` holds the same tables in HBM; `batch(indices)` returns what
`default_collate([dataset[i] for i in indices])` returns in the reference, `sampler(batch_size, ...)` a
`DetectionWindowSampler` whose `next_batch()` is two launches (`timhip_sampler_draw`, `timhip_det_window_batch`) into tensors of
fixed address, eager or replayed with the same bits.  No CPU path: the kernels run or the call raises.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import call, ptr
from .data import DeviceWindowDataset, _DeviceOrder, _batch_stores, store_dtypes
from .functional import _stream


def action_column(dataset_name="epic", include_verb_noun=True, verb_only=True):
    """the column of a window's [n, 4] label table that `label["action"]` reads (sliding_window.py:375-381)"""
    if dataset_name == "epic" and not include_verb_noun:
        return 0 if verb_only else 1
    return 2


class DeviceDetectionDataset:
    def __init__(self, windows, num_feats, window_size, max_visual_actions, max_audio_actions, model_modality="audio_visual",
                 v_feats=None, v_feat_times=None, a_feats=None, a_feat_times=None, dataset_name="epic", include_verb_noun=True,
                 verb_only=True, device="cuda", store_dtype=torch.float32):
        """Arguments are the attributes the reference dataset holds after its constructor: `windows` (list of dicts with
        video_id, start_sec, feat_indices, v_gt_segments / a_gt_segments [n, 2] in seconds, v_labels / a_labels [n, 4];
        sliding_window.py:225-282), `v_feats`/`a_feats` {video_id: [N_feat, num_aug, C]}, `v_feat_times`/`a_feat_times`
        {video_id: [N_feat, >=2]}, `num_feats`, `window_size`, `max_visual_actions`, `max_audio_actions`, `dataset_name`,
        `include_verb_noun`, `verb_only`.  A window with more actions than its maximum is a ValueError.  `store_dtype`: the
        element type of the feature stores, as in `tim_amd.data.DeviceWindowDataset` (fp32, fp16 or bf16, or one per modality)."""
        self.store_dtype = store_dtypes(store_dtype)
        if not torch.cuda.is_available():
            raise L.TimHipError("DeviceDetectionDataset needs the MI355X (no CPU fallback)")
        L.load()
        self.device = torch.device(device)
        self.num_feats, self.window_size = int(num_feats), float(window_size)
        self.max_visual_actions, self.max_audio_actions = int(max_visual_actions), int(max_audio_actions)
        self.model_modality = model_modality
        self.has_v, self.has_a = "visual" in model_modality, "audio" in model_modality
        if not (self.has_v or self.has_a):
            raise ValueError("model_modality %r names neither visual nor audio" % (model_modality,))
        self.dataset_name, self.include_verb_noun, self.verb_only = dataset_name, bool(include_verb_noun), bool(verb_only)
        self.action_col = action_column(dataset_name, include_verb_noun, verb_only)
        W = len(windows)
        self.video_ids = sorted({w["video_id"] for w in windows})
        index = {v: i for i, v in enumerate(self.video_ids)}
        store = lambda f, t, m: DeviceWindowDataset._store(self, f, t, self.video_ids, self.store_dtype[m], m)   # noqa: E731  (it reads self.device only)
        self.v = store(v_feats, v_feat_times, "visual") if self.has_v else None
        self.a = store(a_feats, a_feat_times, "audio") if self.has_a else None
        dev, mv, ma = self.device, self.max_visual_actions, self.max_audio_actions
        fi = torch.stack([torch.as_tensor(w["feat_indices"]).to(torch.int32).reshape(-1) for w in windows]) if W else torch.zeros((0, self.num_feats))
        if fi.shape[1] != self.num_feats:
            raise ValueError("every window must index num_feats features")
        self.feat_indices = fi.to(dev).contiguous()
        starts = [float(w["start_sec"]) for w in windows]
        self.start_sec = torch.tensor(starts, dtype=torch.float32, device=dev)       # what the fp32 subtraction reads
        self.window_start_sec = torch.tensor(starts, dtype=torch.float64, device=dev)   # what the collate returns
        self.window_video = [index[w["video_id"]] for w in windows]
        self.video_of = torch.tensor(self.window_video, dtype=torch.int32, device=dev)
        vs, as_ = torch.zeros((W, mv, 2)), torch.zeros((W, ma, 2))
        vl, al = torch.full((W, mv, 4), -1, dtype=torch.int64), torch.full((W, ma, 4), -1, dtype=torch.int64)
        for i, w in enumerate(windows):                       # the padding of sliding_window.py:365-372, done once
            T = torch.as_tensor
            nv, na = T(w["v_labels"]).shape[0], T(w["a_labels"]).shape[0]
            if nv > mv or na > ma:
                raise ValueError("window %d has more actions than max_visual_actions / max_audio_actions" % i)
            if nv:
                vs[i, :nv], vl[i, :nv] = T(w["v_gt_segments"]).float().reshape(nv, 2), T(w["v_labels"]).long().reshape(nv, 4)
            if na:
                as_[i, :na], al[i, :na] = T(w["a_gt_segments"]).float().reshape(na, 2), T(w["a_labels"]).long().reshape(na, 4)
        self.v_segments, self.a_segments = vs.to(dev), as_.to(dev)
        self.v_labels, self.a_labels = vl.to(dev), al.to(dev)
        row0 = lambda st: torch.tensor([st["row0"][w["video_id"]] for w in windows], dtype=torch.int64, device=dev)   # noqa: E731
        self.v_row0 = row0(self.v) if self.has_v else None
        self.a_row0 = row0(self.a) if self.has_a else None
        self.num_windows = W

    @classmethod
    def from_reference(cls, ds, device="cuda", store_dtype=torch.float32):
        """from a constructed reference detection `SlidingWindowDataset` (or anything exposing the same attributes)"""
        return cls(ds.windows, ds.num_feats, ds.window_size, ds.max_visual_actions, ds.max_audio_actions, ds.model_modality,
                   ds.v_feats, ds.v_feat_times, ds.a_feats, ds.a_feat_times, ds.dataset_name, ds.include_verb_noun, ds.verb_only, device,
                   store_dtype=store_dtype)

    def __len__(self):
        return self.num_windows

    store_bytes = DeviceWindowDataset.store_bytes

    def _assemble(self, desc, st):
        """one assembly launch: the fp32 entry, or the `_st` entry when a feature store is 16-bit"""
        stores = _batch_stores(self)
        if stores is None:
            call("timhip_det_window_batch", C.byref(desc), st)
        else:
            call("timhip_det_window_batch_st", C.byref(desc), stores[0], stores[1], st)

    def video_ids_of(self, windows):
        """The video-id strings (host data) of a list or CPU tensor of window numbers: the `video_id` entry of a collated batch."""
        idx = [int(i) for i in torch.as_tensor(windows).reshape(-1).tolist()]
        for i in idx:
            if not 0 <= i < self.num_windows:
                raise ValueError("window %d outside [0, %d)" % (i, self.num_windows))
        return [self.video_ids[self.window_video[i]] for i in idx]

    def _outputs(self, B, fill):
        """-> (visual, audio, times, label, window_start, video_index) of a batch of B rows; fill(shape, dtype) allocates"""
        dev, nf, mv, ma = self.device, self.num_feats, self.max_visual_actions, self.max_audio_actions
        f32, i64 = torch.float32, torch.int64
        visual = fill((B, nf, self.v["C"]), f32) if self.has_v else torch.empty((B, 0), device=dev)
        audio = fill((B, nf, self.a["C"]), f32) if self.has_a else torch.empty((B, 0), device=dev)
        times = fill((B, (nf if self.has_v else 0) + (nf if self.has_a else 0), 2), f32)
        label = {"v_gt_segments": fill((B, mv, 2), f32), "a_gt_segments": fill((B, ma, 2), f32), "verb": fill((B, mv), i64),
                 "noun": fill((B, mv), i64), "action": fill((B, mv), i64), "class_id": fill((B, ma), i64)}
        return visual, audio, times, label, fill((B,), torch.float64), fill((B,), torch.int32)

    def _descriptor(self, B, window, valid, v_aug, a_aug, out):
        visual, audio, times, lb, window_start, video_index = out
        d = L.TimDetWindowBatch()
        if self.has_v:
            d.v_feats, d.v_feat_times, d.v_row0, d.v_aug, d.visual = ptr(self.v["feats"]), ptr(self.v["times"]), ptr(self.v_row0), ptr(v_aug), ptr(visual)
            d.Cv, d.v_num_aug, d.v_ld = self.v["C"], self.v["num_aug"], 2
        if self.has_a:
            d.a_feats, d.a_feat_times, d.a_row0, d.a_aug, d.audio = ptr(self.a["feats"]), ptr(self.a["times"]), ptr(self.a_row0), ptr(a_aug), ptr(audio)
            d.Ca, d.a_num_aug, d.a_ld = self.a["C"], self.a["num_aug"], 2
        d.feat_indices, d.start_sec, d.window_start_sec, d.video_of = ptr(self.feat_indices), ptr(self.start_sec), ptr(self.window_start_sec), ptr(self.video_of)
        d.window, d.valid, d.times, d.window_start, d.video_index = ptr(window), ptr(valid), ptr(times), ptr(window_start), ptr(video_index)
        if self.max_visual_actions:
            d.v_segments, d.v_labels, d.v_gt_segments = ptr(self.v_segments), ptr(self.v_labels), ptr(lb["v_gt_segments"])
            d.verb, d.noun, d.action = ptr(lb["verb"]), ptr(lb["noun"]), ptr(lb["action"])
        if self.max_audio_actions:
            d.a_segments, d.a_labels, d.a_gt_segments, d.class_id = ptr(self.a_segments), ptr(self.a_labels), ptr(lb["a_gt_segments"]), ptr(lb["class_id"])
        d.num_feats, d.max_v, d.max_a, d.B, d.num_windows = self.num_feats, self.max_visual_actions, self.max_audio_actions, B, self.num_windows
        d.action_col, d.window_size = self.action_col, self.window_size
        return d

    def batch(self, indices, v_aug_indices=None, a_aug_indices=None):
        """= default_collate([dataset[i] for i in indices]) of the reference (sliding_window.py:324-399), on the device:
        (v_data, a_data, times, label, metadata) with label = {v_gt_segments, a_gt_segments, verb, noun, action, class_id} and
        metadata = {window_start float64 [B], window_size float64 [B], video_id: list of B strings, video_index int32 [B]}.
        aug indices [B, num_feats] pin the augmentation draw (tests); by default they are drawn on the device."""
        dev, nf = self.device, self.num_feats
        idx = [int(i) for i in torch.as_tensor(indices).reshape(-1).tolist()]
        for i in idx:
            if not 0 <= i < self.num_windows:
                raise ValueError("window %d outside [0, %d)" % (i, self.num_windows))
        B = len(idx)
        if B < 1:
            raise ValueError("batch() needs at least one window")
        win = torch.tensor(idx, dtype=torch.int32, device=dev)
        valid = torch.ones(B, dtype=torch.uint8, device=dev)

        def aug(store, given):
            if given is None:
                return torch.randint(0, store["num_aug"], (B, nf), device=dev, dtype=torch.int32)
            return torch.as_tensor(given).to(device=dev, dtype=torch.int32).contiguous().reshape(B, nf)

        v_aug = aug(self.v, v_aug_indices) if self.has_v else None
        a_aug = aug(self.a, a_aug_indices) if self.has_a else None
        out = self._outputs(B, lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
        with torch.cuda.device(dev):
            self._assemble(self._descriptor(B, win, valid, v_aug, a_aug, out), _stream())
        visual, audio, times, label, window_start, video_index = out
        metadata = {"window_start": window_start, "window_size": torch.full((B,), self.window_size, dtype=torch.float64, device=dev),
                    "video_id": [self.video_ids[self.window_video[i]] for i in idx], "video_index": video_index}
        return visual, audio, times, label, metadata

    def sampler(self, batch_size, seed=0, shuffle=True, rank=0, world=1, last="wrap"):
        """A `DetectionWindowSampler` over this dataset: batches drawn and assembled on the device, capturable."""
        return DetectionWindowSampler(self, batch_size, seed=seed, shuffle=shuffle, rank=rank, world=world, last=last)


class DetectionWindowSampler(_DeviceOrder):
    """The batches of a seeded, epoch-shuffled, rank-sharded order over a `DeviceDetectionDataset`, with all state on the device.

        smp = ds.sampler(batch_size, seed=0, shuffle=True, rank=rank, world=world)
        def step():                                   # eager, or the `fn` of a GraphedStep: the same sequence of batches
            visual, audio, times, label, metadata = smp.next_batch()       # two launches, no host input
            out, offsets, labels, _, ious = model([visual, audio], "encoder", times, label, label_queries=True)
            ...

    `next_batch()` returns what `ds.batch(indices)` returns, in tensors the sampler owns: the SAME objects on every call,
    refilled by `timhip_sampler_draw` + `timhip_det_window_batch`.  The order, its counter, `set_iteration`, `state_dict` /
    `load_state_dict`, `.window`, `.epoch` and `.iteration` are `tim_amd.data.WindowSampler`'s.  `metadata` carries `valid`,
    `window`, `window_start`, `window_size` and `video_index` as device tensors; the `video_id` strings are host data,
    `ds.video_ids_of(smp.window.cpu())` looks them up (evaluation: `dict(metadata, video_id=...)` is what
    `DetectionCollector.update` takes).

    With `last="wrap"` a short last batch keeps its full shape: the rows beyond the rank's share have `metadata["valid"] == 0`,
    the features, times, window start and video index of a real (wrapped) window, -1 in every label and 0.0 in every
    ground-truth segment - a window WITHOUT ground truth, which the reference's labelling makes all-negative: its queries still
    enter the focal sum as negatives.  `last="drop"` is the way to keep such rows out of the focal sum.

    No CPU path: the kernels run or the call raises."""

    def __init__(self, dataset, batch_size, seed=0, shuffle=True, rank=0, world=1, last="wrap"):
        super().__init__(dataset, batch_size, seed=seed, shuffle=shuffle, rank=rank, world=world, last=last)
        ds, B, dev = dataset, self.batch_size, dataset.device

        def fill(shape, dtype):
            return torch.full(shape, -1, dtype=dtype, device=dev) if dtype == torch.int64 else torch.zeros(shape, dtype=dtype, device=dev)

        self._out = ds._outputs(B, fill)
        self.visual, self.audio, self.times, self.label, window_start, video_index = self._out
        self.metadata = {"window_start": window_start, "window_size": torch.full((B,), ds.window_size, dtype=torch.float64, device=dev),
                         "video_index": video_index, "window": self.window, "valid": self.valid}
        self._desc = None

    def _descriptor(self):
        return self.dataset._descriptor(self.batch_size, self.window, self.valid, self.v_aug, self.a_aug, self._out)

    def next_batch(self):
        """Two launches on the current stream: the draw of the next iteration and the assembly of its batch into the sampler's
        own tensors -> (visual, audio, times, label, metadata), the same objects every time.  Capturable; never synchronises."""
        if self._desc is None:
            self._desc = self._descriptor()
        with torch.cuda.device(self.device):
            st = _stream()
            self._draw(st)
            self.dataset._assemble(self._desc, st)
        return self.visual, self.audio, self.times, self.label, self.metadata
