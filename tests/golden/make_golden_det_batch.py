"""Golden vectors for the DETECTION sliding-window batch from the reference's own `__getitem__` and torch's `default_collate`
(build container only):    python tests/golden/make_golden_det_batch.py <the reference's detection/ directory>

A reference detection `SlidingWindowDataset` object is created WITHOUT its file-reading constructor (object.__new__) and given
the in-memory tables its constructor would have built, from seeded synthetic data (tests/golden/det_batch_inputs.py); then the
reference's own `__getitem__` (datasets/sliding_window.py:324-399) runs for every window, once per setting of
(dataset_name, include_verb_noun, verb_only) that selects another `action` column.  Its augmentation draw (torch.randint,
:339-344, :350-355) is replayed with the same seed and stored with the outputs.  One collated batch (windows repeated and out of
order) pins what `default_collate` makes of the metadata: float64 tensors and a list of strings.
"""
import os
import sys
import types

import numpy as np
import torch
from torch.utils.data import default_collate

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sj = types.ModuleType("simplejson")
sj.dumps = lambda *a, **k: ""
sys.modules["simplejson"] = sj
for name in ("fvcore", "fvcore.common", "fvcore.common.file_io"):
    sys.modules[name] = types.ModuleType(name)


class _PM:
    open = staticmethod(open)


sys.modules["fvcore.common.file_io"].PathManager = _PM
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ["TIM_REFERENCE_DETECTION"])
from time_interval_machine.datasets.sliding_window import SlidingWindowDataset  # noqa: E402

from tests.golden.det_batch_inputs import make_tables  # noqa: E402

# (dataset_name, include_verb_noun, verb_only) -> the label column `action` reads (sliding_window.py:375-381)
SETTINGS = {0: ("epic", False, True), 1: ("epic", False, False), 2: ("epic", True, True)}
COLLATED = [3, 0, 3, 5, 1]


def run(name, seed, modality):
    tb = make_tables(seed, modality)
    ds = object.__new__(SlidingWindowDataset)
    t = lambda d: None if d is None else {k: torch.from_numpy(v) for k, v in d.items()}
    ds.windows = [{k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in w.items()} for w in tb["windows"]]
    ds.v_feats, ds.v_feat_times, ds.a_feats, ds.a_feat_times = t(tb["v_feats"]), t(tb["v_feat_times"]), t(tb["a_feats"]), t(tb["a_feat_times"])
    ds.model_modality, ds.num_feats, ds.window_size = modality, tb["num_feats"], tb["window_size"]
    ds.max_visual_actions, ds.max_audio_actions = tb["max_visual_actions"], tb["max_audio_actions"]
    ds.v_num_aug, ds.a_num_aug = tb["v_num_aug"], tb["a_num_aug"]
    out = {}

    def sample(i, col):
        ds.dataset_name, ds.include_verb_noun, ds.verb_only = SETTINGS[col]
        torch.manual_seed(1000 + i)
        return ds[i]

    for i in range(len(ds.windows)):
        v, a, times, label, meta = sample(i, 2)
        torch.manual_seed(1000 + i)                                    # replay the draws of :339-344 / :350-355
        va = torch.randint(low=0, high=ds.v_num_aug, size=(ds.num_feats,), dtype=torch.long) if "visual" in modality else torch.zeros(0)
        aa = torch.randint(low=0, high=ds.a_num_aug, size=(ds.num_feats,), dtype=torch.long) if "audio" in modality else torch.zeros(0)
        out.update({"v%d" % i: v.numpy(), "a%d" % i: a.numpy(), "t%d" % i: times.numpy(), "va%d" % i: va.numpy(), "aa%d" % i: aa.numpy(),
                    "vseg%d" % i: label["v_gt_segments"].numpy(), "aseg%d" % i: label["a_gt_segments"].numpy(),
                    "verb%d" % i: label["verb"].numpy(), "noun%d" % i: label["noun"].numpy(), "class_id%d" % i: label["class_id"].numpy(),
                    "start%d" % i: np.float64(meta["window_start"]), "size%d" % i: np.float64(meta["window_size"]),
                    "vid%d" % i: np.array(meta["video_id"])})
        for col in SETTINGS:
            other = sample(i, col)
            assert torch.equal(other[2], times) and torch.equal(other[3]["verb"], label["verb"])
            out["action%d_c%d" % (i, col)] = other[3]["action"].numpy()
        ds.dataset_name = "thumos"                                     # not epic: the action column whatever the other two say
        ds.include_verb_noun, ds.verb_only = False, True
        torch.manual_seed(1000 + i)
        assert torch.equal(ds[i][3]["action"], torch.from_numpy(out["action%d_c2" % i]))
    v, a, times, label, meta = default_collate([sample(i, 2) for i in COLLATED])
    assert meta["window_start"].dtype == torch.float64 and meta["window_size"].dtype == torch.float64 and isinstance(meta["video_id"], list)
    out.update({"c_index": np.array(COLLATED), "c_v": v.numpy(), "c_a": a.numpy(), "c_t": times.numpy(), "c_start": meta["window_start"].numpy(),
                "c_size": meta["window_size"].numpy(), "c_vid": np.array(meta["video_id"])})
    out.update({"c_" + k: x.numpy() for k, x in label.items()})
    np.savez(os.path.join(HERE, "det_batch_%s.npz" % name), seed=seed, modality=modality, n=len(ds.windows), **out)
    print(name, "windows", len(ds.windows))


if __name__ == "__main__":
    run("av", 81, "audio_visual")
    run("visual", 82, "visual")
    run("audio", 83, "audio")
