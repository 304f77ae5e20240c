"""tests/query_ref.py against the oracle's full forward, float64, every tiny golden case: encoding the feature rows once and
running query rows against the per-layer keys and values is the forward, exactly - also for groups that share
a window and for a query count other than the fixture's."""
import pytest
import torch

from oracle import tim_oracle as O
from tests import helpers as H
from tests import query_ref as QR

TOL = 1e-12
W = 3


def _maxerr(a, b):
    assert (a is None) == (b is None)
    if a is None:
        return 0.0
    assert a.shape == b.shape
    return (a - b).abs().max().item() if a.numel() else 0.0


def _counts(cfg, nv, na):
    """(nv, na) as the model's modalities allow them"""
    return (nv if "visual" in cfg.data_modality else 0), (na if "audio" in cfg.data_modality else 0)


def _check(cfg, sd, inp, nv, na):
    F = cfg.F
    times = inp["times"]
    assert times.shape[1] == F + nv + na
    kv, feats = QR.encode(sd, cfg, inp["visual"], inp["audio"], times[:, :F])
    full = O.forward(sd, cfg, inp["visual"], inp["audio"], times, nv, na)
    assert _maxerr(feats, full[1]) <= TOL
    # the fixture's own queries, group g on window g
    cls, reg = QR.query(sd, cfg, kv, times[:, F:], nv, na)
    for a, b in zip(cls, full[0]):
        assert _maxerr(a, b) <= TOL
    if cfg.variant == "detection":
        for a, b in zip(reg, full[2]):
            assert _maxerr(a, b) <= TOL
    # G = 2 W groups on repeated, permuted windows, with another query count per group: the expectation is the full forward on
    # the windows gathered by the index
    idx = [2, 0, 0, 1, 2, 1]
    nv2, na2 = _counts(cfg, nv + 2, max(na - 1, 1))
    if cfg.input_modality != "audio_visual":            # one modality: every query row is that modality's
        nv2, na2 = (nv2, 0) if cfg.input_modality == "visual" else (0, na2)
    g = torch.Generator().manual_seed(11)
    st = torch.rand(len(idx), nv2 + na2, generator=g, dtype=times.dtype) * 0.8
    tq = torch.stack([st, st + 0.05 + 0.1 * torch.rand(st.shape, generator=g, dtype=times.dtype)], -1)
    gather = lambda t: t[idx] if t.dim() == 3 else t.new_zeros(len(idx), 0)
    full2 = O.forward(sd, cfg, gather(inp["visual"]), gather(inp["audio"]), torch.cat([times[idx, :F], tq], 1), nv2, na2)
    cls2, reg2 = QR.query(sd, cfg, kv, tq, nv2, na2, idx)
    for a, b in zip(cls2, full2[0]):
        assert _maxerr(a, b) <= TOL
    if cfg.variant == "detection":
        for a, b in zip(reg2, full2[2]):
            assert _maxerr(a, b) <= TOL


@pytest.mark.parametrize("fname,im,dm,vn,nv,na", H.rec_golden_cases())
def test_recognition_two_phase_is_the_forward(fname, im, dm, vn, nv, na):
    cfg = H.tiny_cfg("recognition", im, dm, vn)
    sd, inp = H.synth_torch(cfg, W, nv, na, seed=1, dtype=torch.float64)
    with torch.no_grad():
        _check(cfg, sd, inp, nv, na)


@pytest.mark.parametrize("im,dm,nc,tag", H.DET_CASES)
def test_detection_two_phase_is_the_forward(im, dm, nc, tag):
    cfg = H.tiny_cfg("detection", im, dm, tag == "vn", num_class=nc)
    nv, na = _counts(cfg, 7, 5)
    sd, inp = H.synth_torch(cfg, W, nv, na, seed=3, dtype=torch.float64)
    with torch.no_grad():
        _check(cfg, sd, inp, nv, na)
