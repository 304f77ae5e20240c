"""CPU-only checks of the AVGA device route's host side: which calls take which route (decided from metadata, nothing is
launched), the entry points declared / bound / exported under the unchanged ABI number, the workspace query and the argument
checks that return before any launch, the kernels in the spill gate's table."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

from tim_amd import _lib, avga
from tim_amd.tim import TIM, _AVGAParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"timhip_avga_workspace_bytes", "timhip_avga_fwd", "timhip_avga_bwd"}


def _model(cv=64, **kw):
    return TIM([[7, 11, 13], 5], visual_input_dim=cv, audio_input_dim=40, d_model=32, nhead=2, num_layers=2, num_feats=6,
               pool_features=True, **kw)


def test_cpu_tensors_small_widths_and_inputs_with_gradients_take_the_torch_route(monkeypatch):
    monkeypatch.delenv("TIM_AMD_AVGA", raising=False)
    m = _model()
    a, v = torch.randn(2, 3, 40), torch.randn(2, 3, 7, 7, 64)
    assert m.pool.owner() is m and avga.route(m.pool, a, v) == "torch"                 # CPU tensors
    want = torch.einsum("rs,rsc->rc", torch.softmax(torch.zeros(6, 49), -1), v.reshape(6, 49, 64))
    with torch.no_grad():
        for p in (m.pool.affine_h.weight,):
            p.zero_()                                                                   # uniform alpha: out = mean over the cells
    assert torch.allclose(m.pool(a, v).reshape(6, 64), want, atol=1e-6)
    g = dict(env="1", bound=True, prec=_lib.PREC_F16, on_gpu=True, fp32=True, inputs_need_grad=False, R=6, S=49, Cv=64, Ca=40, H=64,
             map_size=49)
    assert avga.classify(**g) == "device"                                               # a supported GPU-shaped request
    for prec in (_lib.PREC_BF16, _lib.PREC_FP32):
        assert avga.classify(**dict(g, prec=prec)) == "device"
    for change in (dict(env="0"), dict(on_gpu=False), dict(inputs_need_grad=True), dict(Cv=24, H=24), dict(bound=False),
                   dict(fp32=False), dict(prec=_lib.PREC_BF16X3), dict(S=65, map_size=65), dict(H=128), dict(Cv=96, H=96),
                   dict(Cv=1088, H=1088), dict(map_size=48), dict(R=0)):
        assert avga.classify(**dict(g, **change)) == "torch", change
    for S, Cv in ((1, 64), (64, 1024), (7, 128)):
        assert avga.classify(**dict(g, S=S, map_size=S, Cv=Cv, H=Cv)) == "device"
    assert avga.route(_model(cv=24).pool, torch.randn(2, 3, 40), torch.randn(2, 3, 7, 7, 24)) == "torch"
    assert avga.route(_AVGAParams(40, 64, 64), a, v) == "torch"                         # a module outside a TIM
    monkeypatch.setenv("TIM_AMD_AVGA", "0")                                             # read per call
    assert avga.route(m.pool, a, v) == "torch"


def test_the_owner_link_stays_out_of_state_and_copies():
    import copy
    m = _model()
    assert not any("owner" in k for k in m.state_dict()) and [n for n, _ in m.pool.named_modules()][1:] == [
        "affine_audio", "affine_video", "affine_v", "affine_g", "affine_h"]
    c = copy.deepcopy(m)
    assert c.pool.owner() is None
    c.pool.bind(c)
    assert c.pool.owner() is c and m.pool.owner() is m
    with pytest.raises(_lib.TimHipError, match="no CPU fallback"):
        m.pool.attention_map(torch.randn(2, 3, 40), torch.randn(2, 3, 7, 7, 64))


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "timhip.h")).read()
    declared = {n for n in re.findall(r"\b(timhip_[a-z0-9_]+)\s*\(", hdr) if n.startswith("timhip_avga_")}
    assert declared == NAMES and NAMES <= set(_lib.exported_symbols())
    assert len(_lib._SIGS["timhip_avga_fwd"][1]) == 9 and len(_lib._SIGS["timhip_avga_bwd"][1]) == 9
    assert re.search(r"#define\s+TIMHIP_VERSION\s+6\b", hdr) and _lib.ABI_VERSION == 6      # additive: the version stays
    assert C.sizeof(_lib.TimAvga) == 13 * 8 + 8 + 16 * 4 and C.sizeof(_lib.TimAvgaGrads) == 7 * 8
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert re.search(r"\bT %s\b" % n, syms), n


def test_workspace_query():
    lib = _lib.load()
    q = lib.timhip_avga_workspace_bytes
    f16, f32 = _lib.PREC_F16, _lib.PREC_FP32
    fwd, bwd = q(f16, 640, 49, 512, 128, 0), q(f16, 640, 49, 512, 128, 1)
    assert 0 < fwd < 2 * 1024 * 1024                         # [R]-row intermediates only: a, ha, g
    assert bwd >= fwd + 2 * 640 * 49 * 512 * 2               # + d_pre and the cast cells, operand dtype
    assert bwd < fwd + 2 * 640 * 49 * 512 * 2 + 32 * 1024 * 1024
    assert q(f32, 640, 49, 512, 128, 1) >= 2 * 640 * 49 * 512 * 4
    assert q(f16, 1, 1, 64, 1, 0) > 0 and q(f16, 4, 64, 1024, 40, 1) > 0
    assert q(f16, 1 << 20, 49, 512, 128, 0) == 0 and q(f16, 1 << 20, 49, 512, 128, 1) == 0      # R * S * Cv >= 2^31: refused by the entry points
    assert q(f16, 640, 49, 512, 37, 1) > 0 and q(f16, 640, 49, 512, 130, 0) > 0
    for bad in ((f16, 0, 49, 512, 128), (f16, 6, 65, 512, 128), (f16, 6, 0, 512, 128), (f16, 6, 49, 96, 128), (f16, 6, 49, 1088, 128),
                (f16, 6, 49, 512, 0), (_lib.PREC_BF16X3, 6, 49, 512, 128), (7, 6, 49, 512, 128)):
        assert q(*bad, 0) == 0 and q(*bad, 1) == 0, bad


def test_argument_checks_return_before_any_launch():
    """every refusal below is decided on the host from the descriptor: the pointers are never dereferenced"""
    lib = _lib.load()
    A = 0x10000

    def desc(**kw):
        d = _lib.TimAvga(A, A, A, A, A, A, A, A, A, A, A, A, A, 49 * 64, 6, 49, 64, 40, 64, 49, 40, 64, 64, 64, 64, 64, 64, 192, 192, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def fwd(d, prec=_lib.PREC_F16, out=A, ldo=64, ws=A, nws=16):
        return lib.timhip_avga_fwd(prec, C.byref(d) if d is not None else None, out, ldo, None, 0, ws, nws, None)
    assert fwd(desc()) == _lib.EWORKSPACE                    # everything else is in order: only the 16-byte workspace is refused
    assert fwd(None) == _lib.EINVAL and fwd(desc(), out=None) == _lib.EINVAL and fwd(desc(), ws=None) == _lib.EINVAL
    for name in ("video", "audio", "w_video", "w_audio", "w_v", "w_g", "b_video", "b_audio", "w_h"):
        assert fwd(desc(**{name: None})) == _lib.EINVAL, name
    assert fwd(desc(w_v_t=None, w_g_t=None)) == _lib.EWORKSPACE          # the forward does not need the transposed copies
    assert fwd(desc(R=0)) == _lib.EINVAL and fwd(desc(pitch=49 * 64 - 4)) == _lib.EINVAL and fwd(desc(ld_audio=36)) == _lib.EINVAL
    assert fwd(desc(), ldo=60) == _lib.EINVAL
    for kw in (dict(S=65, map_size=65), dict(map_size=48), dict(H=128), dict(Cv=96, H=96), dict(Cv=1088, H=1088)):
        assert fwd(desc(**kw)) == _lib.EUNSUPPORTED, kw
    assert fwd(desc(), prec=_lib.PREC_BF16X3) == _lib.EUNSUPPORTED and fwd(desc(), prec=9) == _lib.EUNSUPPORTED
    for kw in (dict(pitch=49 * 64 + 2), dict(ld_w_video=72), dict(ld_w_v=32), dict(ld_w_audio=40), dict(video=A + 4), dict(w_g=A + 8)):
        assert fwd(desc(**kw)) == _lib.EALIGN, kw
    assert fwd(desc(), ldo=66) == _lib.EALIGN and fwd(desc(), out=A + 4) == _lib.EALIGN
    gr = _lib.TimAvgaGrads(A, A, A, A, A, A, A)

    def bwd(d, prec=_lib.PREC_F16, g=gr, gs=None, dout=A):
        return lib.timhip_avga_bwd(prec, C.byref(d), dout, 64, C.byref(g) if g is not None else None, gs, A, 16, None)
    assert bwd(desc()) == _lib.EWORKSPACE
    assert bwd(desc(w_v_t=None)) == _lib.EINVAL and bwd(desc(w_g_t=None)) == _lib.EINVAL and bwd(desc(), g=None) == _lib.EINVAL
    assert bwd(desc(), g=_lib.TimAvgaGrads(A, A, A, A, A, A, None)) == _lib.EINVAL and bwd(desc(), dout=None) == _lib.EINVAL
    assert bwd(desc(), prec=_lib.PREC_BF16, gs=A) == _lib.EINVAL         # a gradient scale belongs to the fp16 mode
    assert bwd(desc(S=65, map_size=65)) == _lib.EUNSUPPORTED and bwd(desc(ld_w_v_t=48)) == _lib.EALIGN
    # the split copies belong to the 16-bit backward only
    assert bwd(desc(w_video_s=None)) == _lib.EINVAL and bwd(desc(w_audio_s=None)) == _lib.EINVAL
    assert bwd(desc(ld_w_video_s=128)) == _lib.EALIGN and bwd(desc(ld_w_audio_s=64)) == _lib.EALIGN
    assert bwd(desc(w_video_s=None, w_audio_s=None), prec=_lib.PREC_FP32) == _lib.EWORKSPACE
    assert fwd(desc(w_video_s=None, w_audio_s=None)) == _lib.EWORKSPACE
    assert bwd(desc(ld_w_video_s=256)) == _lib.EALIGN                    # exactly three blocks of ru(K) columns
    # the audio rows: any stride >= Ca, a float's alignment
    assert fwd(desc(ld_audio=41)) == _lib.EWORKSPACE and fwd(desc(audio=A + 4)) == _lib.EWORKSPACE
    assert fwd(desc(audio=A + 2)) == _lib.EALIGN


def test_kernels_are_in_the_spill_table_and_the_unit_in_the_makefile():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_spills
    finally:
        sys.path.pop(0)
    assert dict(check_spills.BUDGET["avga.hip"])["avga_kernel"] == 0
    mk = open(os.path.join(ROOT, "tim_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bavga\.hip\b", mk, re.M)
