"""Sliding-window batch assembly on the device.

The reference's `SlidingWindowDataset` (recognition/time_interval_machine/datasets/sliding_window.py) keeps every video's
features in host memory and builds each sample in a DataLoader worker: a fancy-index gather
`feats[video][feat_indices, aug_indices]` (:358, :370), padding of the queries (:374-399) and the time normalisation
(:402-404); the batch then crosses PCIe.  At 200 k interval queries/s (2 600 windows/s x 0.67 MB) that is 1.7 GB/s of
gather + host-to-device copy per GPU.  `DeviceWindowDataset` holds the same tables in HBM (a feature set of tens of GB fits
the MI355X's 288 GB many times over) and produces whole batches with two HIP kernels (`timhip_window_gather`,
`timhip_window_times`): `batch(indices)` returns what `default_collate([dataset[i] for i in indices])` returns in the
reference, already on the device.  No CPU path: the kernels run or the call raises.

`batch()` takes host indices and allocates its outputs, so it cannot sit inside a captured step.  `ds.sampler(batch_size, ...)`
returns a `WindowSampler` whose order lives on the device: `next_batch()` is two launches (`timhip_sampler_draw`,
`timhip_window_batch`) into tensors of fixed address, eager or replayed with the same bits.

`store_dtype` (fp32 by default; `torch.float16`, `torch.bfloat16`, or one per modality) is the element type the feature stores
are held in.  The model's 16-bit modes round every input row to their operand type in front of the embedders, so a store kept
in that type loses nothing the forward would not lose one launch later, at half the bytes.  Batches stay fp32: a stored
element comes out as its exact widening (`timhip_window_gather_st`, `timhip_window_batch_st`).  A finite value that the storage
type cannot hold is refused at construction, never stored as inf.
"""
import ctypes as C

import torch

from . import _lib as L
from ._lib import call, ptr
from .functional import _stream


STORE_CODES = {torch.float32: L.STORE_F32, torch.float16: L.STORE_F16, torch.bfloat16: L.STORE_BF16}   # TIMHIP_STORE_*


def store_dtypes(store_dtype):
    """-> {"visual": dtype, "audio": dtype} of a `store_dtype` argument: one of torch.float32 / float16 / bfloat16 for both
    modalities, or a dict {"visual": ..., "audio": ...} (a modality it leaves out is fp32).  Anything else: ValueError."""
    if isinstance(store_dtype, dict):
        if not set(store_dtype) <= {"visual", "audio"}:
            raise ValueError('store_dtype: a dict names "visual" and / or "audio", got %r' % (sorted(map(str, store_dtype)),))
        out = {m: store_dtype.get(m, torch.float32) for m in ("visual", "audio")}
    else:
        out = {"visual": store_dtype, "audio": store_dtype}
    for m, dt in out.items():
        if not isinstance(dt, torch.dtype) or dt not in STORE_CODES:
            raise ValueError("store_dtype: %s store of %r, not one of torch.float32, torch.float16, torch.bfloat16" % (m, dt))
    return out


def round_to_store(feats, dtype, modality="", video=""):
    """One video's feature array as a CPU tensor of the storage type.  An array already of that type comes back as it is, bit
    for bit; anything else is rounded once, to nearest even, by `.to(dtype)` (fp32: the `.float()` the fp32 store always did).
    A finite value that rounding to a 16-bit type turns into inf is a ValueError that names the modality, the video and the
    count: an overflow is refused, not stored.  Non-finite inputs pass through as they are.  Needs no GPU."""
    f = torch.as_tensor(feats)
    if f.dtype == dtype:
        return f
    if dtype == torch.float32:
        return f.float()
    r = f.to(dtype)
    finite_in = torch.isfinite(f) if f.is_floating_point() else torch.ones_like(r, dtype=torch.bool)
    lost = int((finite_in & ~torch.isfinite(r)).sum())
    if lost:
        raise ValueError("%s features of video %s: %d finite value%s beyond the range of %s"
                         % (modality or "the", video, lost, "" if lost == 1 else "s", str(dtype).replace("torch.", "")))
    return r


def store_code(store):
    """TIMHIP_STORE_* of a store dict (one without "dtype" - a hand-built fp32 store - is fp32)"""
    return STORE_CODES[store.get("dtype", torch.float32)]


class DeviceWindowDataset:
    def __init__(self, windows, num_feats, window_size, max_visual_actions, max_audio_actions, model_modality="audio_visual",
                 v_feats=None, v_feat_times=None, a_feats=None, a_feat_times=None, device="cuda", store_dtype=torch.float32):
        """Arguments are the attributes the reference dataset holds after its constructor: `windows` (list of dicts,
        sliding_window.py:262-277), `v_feats`/`a_feats` {video_id: [N_feat, num_aug, C]}, `v_feat_times`/`a_feat_times`
        {video_id: [N_feat, >=2]}, `num_feats`, `window_size`, `max_visual_actions`, `max_audio_actions`.  `store_dtype`: the
        element type of the feature stores (`store_dtypes`); feature times stay fp32."""
        self.store_dtype = store_dtypes(store_dtype)
        if not torch.cuda.is_available():
            raise L.TimHipError("DeviceWindowDataset needs the MI355X (no CPU fallback)")
        L.load()
        self.device = torch.device(device)
        self.num_feats, self.window_size = int(num_feats), float(window_size)
        self.max_visual_actions, self.max_audio_actions = int(max_visual_actions), int(max_audio_actions)
        self.model_modality = model_modality
        self.has_v, self.has_a = "visual" in model_modality, "audio" in model_modality
        W = len(windows)
        vids = sorted({w["video_id"] for w in windows})
        self.v = self._store(v_feats, v_feat_times, vids, self.store_dtype["visual"], "visual") if self.has_v else None
        self.a = self._store(a_feats, a_feat_times, vids, self.store_dtype["audio"], "audio") if self.has_a else None
        dev, mv, ma = self.device, self.max_visual_actions, self.max_audio_actions
        fi = torch.stack([torch.as_tensor(w["feat_indices"]).to(torch.int32).reshape(-1) for w in windows])
        if fi.shape[1] != self.num_feats:
            raise ValueError("every window must index num_feats features")
        self.feat_indices = fi.to(dev).contiguous()
        self.start_sec = torch.tensor([float(w["start_sec"]) for w in windows], dtype=torch.float32, device=dev)
        vq, aq = torch.zeros((W, mv, 2)), torch.zeros((W, ma, 2))
        vl, al = torch.full((W, mv, 4), -1, dtype=torch.int64), torch.full((W, ma, 4), -1, dtype=torch.int64)
        vid_, aid_ = torch.full((W, mv), -1, dtype=torch.int64), torch.full((W, ma), -1, dtype=torch.int64)
        self.v_narration_ids, self.a_narration_ids = [], []
        for i, w in enumerate(windows):                       # the padding of sliding_window.py:374-399, done once
            T = torch.as_tensor
            nv, na = T(w["v_labels"]).shape[0], T(w["a_labels"]).shape[0]
            if nv > mv or na > ma:
                raise ValueError("window %d has more queries than max_visual_actions / max_audio_actions" % i)
            if nv:
                vq[i, :nv], vl[i, :nv], vid_[i, :nv] = T(w["v_queries"]).float(), T(w["v_labels"]).long(), T(w["v_action_ids"]).long()
            if na:
                aq[i, :na], al[i, :na], aid_[i, :na] = T(w["a_queries"]).float(), T(w["a_labels"]).long(), T(w["a_action_ids"]).long()
            self.v_narration_ids.append(list(w["v_narration_ids"]) + [""] * (mv - nv))
            self.a_narration_ids.append(list(w["a_narration_ids"]) + [""] * (ma - na))
        self.v_queries, self.a_queries = vq.to(dev), aq.to(dev)
        self.v_labels, self.a_labels = vl.to(dev), al.to(dev)
        self.v_action_ids, self.a_action_ids = vid_.to(dev), aid_.to(dev)
        row0 = lambda st: torch.tensor([st["row0"][w["video_id"]] for w in windows], dtype=torch.int64, device=dev)
        self.v_row0 = row0(self.v) if self.has_v else None
        self.a_row0 = row0(self.a) if self.has_a else None
        self.num_windows = W

    @classmethod
    def from_reference(cls, ds, device="cuda", store_dtype=torch.float32):
        """from a constructed reference `SlidingWindowDataset` (or anything exposing the same attributes)"""
        return cls(ds.windows, ds.num_feats, ds.window_size, ds.max_visual_actions, ds.max_audio_actions, ds.model_modality,
                   ds.v_feats, ds.v_feat_times, ds.a_feats, ds.a_feat_times, device, store_dtype=store_dtype)

    def _store(self, feats, feat_times, vids, dtype=torch.float32, modality=""):
        """-> {"row0", "num_aug", "C", "feats" (in the storage type), "times" (fp32), "dtype"}"""
        if feats is None or feat_times is None:
            raise ValueError("features and feature times are required for every modality of model_modality")
        if dtype != torch.float32:
            return DeviceWindowDataset._store16(self, feats, feat_times, vids, dtype, modality)
        row0, off, fl, tl = {}, 0, [], []
        num_aug, C = None, None
        for v in vids:
            f, t = torch.as_tensor(feats[v]), torch.as_tensor(feat_times[v]).float()
            if num_aug is None:
                num_aug, C = f.shape[1], f.shape[2]
            if f.shape[1] != num_aug or f.shape[2] != C or t.shape[0] != f.shape[0]:
                raise ValueError("inconsistent feature arrays for video %s" % v)
            row0[v] = off
            off += f.shape[0]
            fl.append(f.float().reshape(-1, C))
            tl.append(t[:, :2])
        return {"row0": row0, "num_aug": num_aug, "C": C, "feats": torch.cat(fl).to(self.device).contiguous(),
                "times": torch.cat(tl).to(self.device).contiguous(), "dtype": torch.float32}

    def _store16(self, feats, feat_times, vids, dtype, modality):
        """A 16-bit store, video by video into ONE preallocated device tensor: neither the host nor the device ever holds a
        second copy of the set (the host holds one video in the storage type at a time, and nothing for a video that is already
        in it)."""
        row0, off, tl = {}, 0, []
        num_aug, C = None, None
        for v in vids:                                        # shapes first: the size of the allocation
            shape, t = tuple(feats[v].shape), torch.as_tensor(feat_times[v]).float()
            if num_aug is None:
                num_aug, C = shape[1], shape[2]
            if len(shape) != 3 or shape[1] != num_aug or shape[2] != C or t.shape[0] != shape[0]:
                raise ValueError("inconsistent feature arrays for video %s" % v)
            row0[v] = off
            off += shape[0]
            tl.append(t[:, :2])
        store = torch.empty((off * (num_aug or 0), C or 0), dtype=dtype, device=self.device)
        for v in vids:
            r = round_to_store(feats[v], dtype, modality, v).reshape(-1, C)
            store[row0[v] * num_aug:row0[v] * num_aug + r.shape[0]].copy_(r)
        return {"row0": row0, "num_aug": num_aug, "C": C, "feats": store, "times": torch.cat(tl).to(self.device).contiguous(),
                "dtype": dtype}

    def __len__(self):
        return self.num_windows

    def store_bytes(self):
        """bytes the feature stores occupy in device memory (the features of the present modalities; not their times)"""
        return sum(st["feats"].numel() * st["feats"].element_size() for st in (self.v, self.a) if st is not None)

    def batch(self, indices, v_aug_indices=None, a_aug_indices=None):
        """= default_collate([dataset[i] for i in indices]) of the reference (sliding_window.py:341-421), on the device.
        aug indices [B, num_feats] pin the augmentation draw (tests); by default they are drawn on the device."""
        dev, nf = self.device, self.num_feats
        win = torch.as_tensor(indices).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        B = win.numel()
        st = _stream()

        def gather(store, row0, aug):
            if aug is None:
                aug = torch.randint(0, store["num_aug"], (B, nf), device=dev, dtype=torch.int32)
            aug = torch.as_tensor(aug).to(device=dev, dtype=torch.int32).contiguous()
            out = torch.empty((B, nf, store["C"]), dtype=torch.float32, device=dev)
            if store_code(store) == L.STORE_F32:
                call("timhip_window_gather", ptr(store["feats"]), store["C"], store["num_aug"], ptr(row0), ptr(self.feat_indices),
                     nf, ptr(win), B, ptr(aug), ptr(out), st)
            else:                                             # a 16-bit store: every element widened exactly
                call("timhip_window_gather_st", ptr(store["feats"]), store_code(store), store["C"], store["num_aug"], ptr(row0),
                     ptr(self.feat_indices), nf, ptr(win), B, ptr(aug), ptr(out), st)
            return out

        v_data = gather(self.v, self.v_row0, v_aug_indices) if self.has_v else torch.empty((B, 0), device=dev)
        a_data = gather(self.a, self.a_row0, a_aug_indices) if self.has_a else torch.empty((B, 0), device=dev)
        mv, ma = self.max_visual_actions, self.max_audio_actions
        T = (nf if self.has_v else 0) + (nf if self.has_a else 0) + mv + ma
        times = torch.empty((B, T, 2), dtype=torch.float32, device=dev)
        call("timhip_window_times", ptr(self.v["times"]) if self.has_v else None, 2, ptr(self.v_row0) if self.has_v else None,
             ptr(self.a["times"]) if self.has_a else None, 2, ptr(self.a_row0) if self.has_a else None,
             ptr(self.feat_indices), nf, ptr(win), B, ptr(self.v_queries), mv, ptr(self.a_queries), ma,
             ptr(self.start_sec), self.window_size, ptr(times), st)
        wl = win.long()
        vl, al = self.v_labels[wl], self.a_labels[wl]
        label = {"verb": vl[:, :, 0], "noun": vl[:, :, 1], "action": vl[:, :, 2], "class_id": al[:, :, 3]}
        idx = [int(i) for i in torch.as_tensor(indices).reshape(-1).tolist()]
        metadata = {
            "v_action_ids": self.v_action_ids[wl], "a_action_ids": self.a_action_ids[wl],
            # default_collate transposes lists of strings: one list (of B strings) per query slot
            "v_narration_ids": [[self.v_narration_ids[i][q] for i in idx] for q in range(mv)],
            "a_narration_ids": [[self.a_narration_ids[i][q] for i in idx] for q in range(ma)],
            "num_v_queries": torch.full((B,), mv, dtype=torch.int64), "num_a_queries": torch.full((B,), ma, dtype=torch.int64),
        }
        return v_data, a_data, times, label, metadata

    def narration_ids(self, windows):
        """The narration-id strings (host data) of a list or CPU tensor of window numbers, in `batch()`'s transposed layout:
        {"v_narration_ids": one list (of len(windows) strings) per query slot, "a_narration_ids": likewise}."""
        idx = [int(i) for i in torch.as_tensor(windows).reshape(-1).tolist()]
        for i in idx:
            if not 0 <= i < self.num_windows:
                raise ValueError("window %d outside [0, %d)" % (i, self.num_windows))
        return {"v_narration_ids": [[self.v_narration_ids[i][q] for i in idx] for q in range(self.max_visual_actions)],
                "a_narration_ids": [[self.a_narration_ids[i][q] for i in idx] for q in range(self.max_audio_actions)]}

    def sampler(self, batch_size, seed=0, shuffle=True, rank=0, world=1, last="wrap"):
        """A `WindowSampler` over this dataset: batches drawn and assembled on the device, capturable."""
        return WindowSampler(self, batch_size, seed=seed, shuffle=shuffle, rank=rank, world=world, last=last)


def _batch_stores(ds):
    """None when every feature store of the dataset is fp32 (the fp32 entries serve it), else the (visual, audio) TIMHIP_STORE_*
    arguments of the `_st` entries"""
    codes = tuple(store_code(st) if st is not None else L.STORE_F32 for st in (ds.v, ds.a))
    return None if codes == (L.STORE_F32, L.STORE_F32) else codes


class _DeviceOrder:
    """What `WindowSampler` and `det_data.DetectionWindowSampler` share: the arguments of a seeded, epoch-shuffled, rank-sharded
    order over a dataset's windows, the device words `timhip_sampler_draw` writes, position and checkpoint."""

    def __init__(self, dataset, batch_size, seed=0, shuffle=True, rank=0, world=1, last="wrap"):
        ds = self.dataset = dataset
        B, world, rank = int(batch_size), int(world), int(rank)
        if B < 1 or B > (1 << 20):
            raise ValueError("batch_size must lie in [1, 2^20], got %d" % B)
        if world < 1 or not 0 <= rank < world:
            raise ValueError("rank %d outside [0, world = %d)" % (rank, world))
        if last not in ("wrap", "drop"):
            raise ValueError('last must be "wrap" or "drop", got %r' % (last,))
        if ds.num_windows < 1:
            raise ValueError("the dataset has no windows")
        if B * ds.num_feats > L.SAMPLER_MAX_AUG:
            raise ValueError("batch_size * num_feats = %d: the augmentation draw addresses at most %d indices per modality"
                             % (B * ds.num_feats, L.SAMPLER_MAX_AUG))
        self.batch_size, self.seed, self.shuffle = B, int(seed) & (2 ** 64 - 1), bool(shuffle)
        self.rank, self.world, self.last = rank, world, last
        self.per_rank = -(-ds.num_windows // world)
        self.iterations_per_epoch = -(-self.per_rank // B) if last == "wrap" else self.per_rank // B
        if self.iterations_per_epoch < 1:
            raise ValueError('last="drop": %d windows per rank do not fill one batch of %d' % (self.per_rank, B))
        dev, nf = ds.device, ds.num_feats
        self.device = dev
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)       # the number of the NEXT iteration
        self.epoch = torch.zeros(1, dtype=torch.int64, device=dev)         # of the batch drawn last
        self.iteration = torch.zeros(1, dtype=torch.int64, device=dev)     # its number inside that epoch
        self.window = torch.zeros(B, dtype=torch.int32, device=dev)
        self.valid = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.v_aug = torch.zeros((B, nf), dtype=torch.int32, device=dev) if ds.has_v else None
        self.a_aug = torch.zeros((B, nf), dtype=torch.int32, device=dev) if ds.has_a else None

    def _draw(self, st):
        ds = self.dataset
        call("timhip_sampler_draw", self.seed, ptr(self.counter), ds.num_windows, self.world, self.rank, self.batch_size,
             int(self.shuffle), L.SAMPLER_WRAP if self.last == "wrap" else L.SAMPLER_DROP, ds.num_feats,
             ds.v["num_aug"] if ds.has_v else 0, ds.a["num_aug"] if ds.has_a else 0, ptr(self.window), ptr(self.valid),
             ptr(self.v_aug), ptr(self.a_aug), ptr(self.epoch), ptr(self.iteration), st)

    # ---- position ---------------------------------------------------------------------------------------------------
    def _check_iteration(self, k):
        k = int(k)
        if k < 0 or k // self.iterations_per_epoch >= (1 << L.SAMPLER_EPOCH_BITS):
            raise ValueError("iteration %d: the order is defined for epochs [0, 2^%d) of %d iterations"
                             % (k, L.SAMPLER_EPOCH_BITS, self.iterations_per_epoch))
        return k

    def set_iteration(self, k):
        """The next `next_batch()` returns iteration k's batch (k counts from 0 across epochs)."""
        self.counter.copy_(torch.tensor([self._check_iteration(k)], dtype=torch.int64))

    # ---- checkpoint -------------------------------------------------------------------------------------------------
    def _arguments(self):
        return {"seed": self.seed, "num_windows": self.dataset.num_windows, "batch_size": self.batch_size, "shuffle": self.shuffle,
                "rank": self.rank, "world": self.world, "last": self.last}

    def state_dict(self):
        """The arguments and the counter (a host read: synchronises).  The NEXT batch of a loaded state is the one this state
        would have returned next."""
        return dict(self._arguments(), counter=int(self.counter.item()))

    def load_state_dict(self, sd):
        mine = self._arguments()
        for k, v in mine.items():
            if k != "seed" and sd.get(k, v) != v:
                raise ValueError("sampler state with %s = %r loaded into a sampler with %s = %r" % (k, sd.get(k), k, v))
        k = self._check_iteration(sd["counter"])
        self.seed = int(sd["seed"]) & (2 ** 64 - 1)
        self.counter.copy_(torch.tensor([k], dtype=torch.int64))


class WindowSampler(_DeviceOrder):
    """The batches of a seeded, epoch-shuffled, rank-sharded order over a `DeviceWindowDataset`, with all state on the device.

        smp = ds.sampler(batch_size, seed=0, shuffle=True, rank=rank, world=world)
        def step():                                   # eager, or the `fn` of a GraphedStep: the same sequence of batches
            visual, audio, times, label, metadata = smp.next_batch()       # two launches, no host input
            ...

    `next_batch()` returns what `ds.batch(indices)` returns (shapes, dtypes, dict keys; narration-id strings aside - they are
    host data, `ds.narration_ids(metadata["window"].cpu())` looks them up), in tensors the sampler owns: the SAME objects on
    every call, refilled by `timhip_sampler_draw` + `timhip_window_batch`.  The k-th call of a seed (counted by a 64-bit word
    in device memory that the draw kernel advances) returns iteration k: epoch k // iterations_per_epoch of an order that is
    `DistributedSampler`'s in structure - the epoch's permutation, padded with its own head to a multiple of `world`, dealt
    round-robin to the ranks - with its own keyed permutation (include/timhip.h), not torch's randperm stream.  With
    `last="wrap"` a short last batch keeps its full shape: the rows beyond the rank's share have `metadata["valid"] == 0`, the
    features and times of a real window and -1 ("no query") in every label and id; `last="drop"` drops that batch.

    No CPU path: the kernels run or the call raises."""

    def __init__(self, dataset, batch_size, seed=0, shuffle=True, rank=0, world=1, last="wrap"):
        super().__init__(dataset, batch_size, seed=seed, shuffle=shuffle, rank=rank, world=world, last=last)
        ds, B = dataset, self.batch_size
        dev, nf, mv, ma = ds.device, ds.num_feats, ds.max_visual_actions, ds.max_audio_actions
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)   # noqa: E731
        i64 = lambda *s: torch.full(s, -1, dtype=torch.int64, device=dev)   # noqa: E731
        self.visual = f32(B, nf, ds.v["C"]) if ds.has_v else torch.empty((B, 0), device=dev)
        self.audio = f32(B, nf, ds.a["C"]) if ds.has_a else torch.empty((B, 0), device=dev)
        T = (nf if ds.has_v else 0) + (nf if ds.has_a else 0) + mv + ma
        self.times = f32(B, T, 2)
        self.label = {"verb": i64(B, mv), "noun": i64(B, mv), "action": i64(B, mv), "class_id": i64(B, ma)}
        self.metadata = {"v_action_ids": i64(B, mv), "a_action_ids": i64(B, ma),
                         "num_v_queries": torch.full((B,), mv, dtype=torch.int64), "num_a_queries": torch.full((B,), ma, dtype=torch.int64),
                         "window": self.window, "valid": self.valid}
        self._desc = None
        self._stores = _batch_stores(ds)

    def _descriptor(self):
        ds, lb, md = self.dataset, self.label, self.metadata
        d = L.TimWindowBatch()
        if ds.has_v:
            d.v_feats, d.v_feat_times, d.v_row0, d.v_aug, d.visual = ptr(ds.v["feats"]), ptr(ds.v["times"]), ptr(ds.v_row0), ptr(self.v_aug), ptr(self.visual)
            d.Cv, d.v_num_aug, d.v_ld = ds.v["C"], ds.v["num_aug"], 2
        if ds.has_a:
            d.a_feats, d.a_feat_times, d.a_row0, d.a_aug, d.audio = ptr(ds.a["feats"]), ptr(ds.a["times"]), ptr(ds.a_row0), ptr(self.a_aug), ptr(self.audio)
            d.Ca, d.a_num_aug, d.a_ld = ds.a["C"], ds.a["num_aug"], 2
        d.feat_indices, d.start_sec, d.window, d.valid, d.times = ptr(ds.feat_indices), ptr(ds.start_sec), ptr(self.window), ptr(self.valid), ptr(self.times)
        if ds.max_visual_actions:
            d.v_queries, d.v_labels, d.v_ids = ptr(ds.v_queries), ptr(ds.v_labels), ptr(ds.v_action_ids)
            d.verb, d.noun, d.action, d.v_action_ids = ptr(lb["verb"]), ptr(lb["noun"]), ptr(lb["action"]), ptr(md["v_action_ids"])
        if ds.max_audio_actions:
            d.a_queries, d.a_labels, d.a_ids = ptr(ds.a_queries), ptr(ds.a_labels), ptr(ds.a_action_ids)
            d.class_id, d.a_action_ids = ptr(lb["class_id"]), ptr(md["a_action_ids"])
        d.num_feats, d.max_v, d.max_a, d.B, d.num_windows = ds.num_feats, ds.max_visual_actions, ds.max_audio_actions, self.batch_size, ds.num_windows
        d.window_size = ds.window_size
        return d

    def next_batch(self):
        """Two launches on the current stream: the draw of the next iteration and the assembly of its batch into the sampler's
        own tensors -> (visual, audio, times, label, metadata), the same objects every time.  Capturable; never synchronises."""
        if self._desc is None:
            self._desc = self._descriptor()
        with torch.cuda.device(self.device):
            st = _stream()
            self._draw(st)
            if self._stores is None:
                call("timhip_window_batch", C.byref(self._desc), st)
            else:
                call("timhip_window_batch_st", C.byref(self._desc), self._stores[0], self._stores[1], st)
        return self.visual, self.audio, self.times, self.label, self.metadata
