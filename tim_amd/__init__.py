"""tim_amd — MI355X (gfx950) implementation of the TIM encoder hot path.

`tim_amd.TIM` / `tim_amd.build_model` mirror `time_interval_machine.models.{tim,build}` of the
reference; the arithmetic lives in `libtimhip.so` (tim_amd/csrc, C ABI in include/timhip.h).
"""
from .config import TimConfig, named_config  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not require torch on a build box
    if name == "TIM":
        from .tim import TIM
        return TIM
    if name == "build_model":
        from .build import build_model
        return build_model
    if name == "DetectionTIM":
        from .detection import TIM
        return TIM
    if name == "FusedAdamW":
        from .optim import FusedAdamW
        return FusedAdamW
    if name == "DetectionCollector":
        from .detect import DetectionCollector
        return DetectionCollector
    if name == "TwoStreamCollector":
        from .twostream import TwoStreamCollector
        return TwoStreamCollector
    if name == "DetectionScorer":
        from .detmap import DetectionScorer
        return DetectionScorer
    if name == "RecognitionCollector":
        from .recog import RecognitionCollector
        return RecognitionCollector
    if name == "TrainMeter":
        from .meters import TrainMeter
        return TrainMeter
    if name == "DetectionMeter":
        from .meters import DetectionMeter
        return DetectionMeter
    if name == "AttentionMaps":
        from .attn_maps import AttentionMaps
        return AttentionMaps
    if name == "WindowCache":
        from .query import WindowCache
        return WindowCache
    if name in ("Mixup", "mixup_data"):
        from . import mixup as _mixup
        return getattr(_mixup, name)
    if name == "WindowSampler":
        from .data import WindowSampler
        return WindowSampler
    if name in ("DeviceDetectionDataset", "DetectionWindowSampler"):
        from . import det_data as _det_data
        return getattr(_det_data, name)
    if name == "DrlocPositions":
        from .losses import DrlocPositions
        return DrlocPositions
    if name == "CosineWarmupSchedule":
        from .schedule import CosineWarmupSchedule
        return CosineWarmupSchedule
    if name in ("optim", "mixup", "schedule"):
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError(name)
