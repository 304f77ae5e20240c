"""timhip_softnms_1d as far as it goes without a GPU: the argument checks it makes before it launches anything.  Every refusal
comes back before the first HIP call, so the device pointers below are host buffers that are never followed; `count` is one of
them and must come back untouched."""
import ctypes as C

import numpy as np

from tim_amd import _lib as L

OK = 0
SENTINEL = -77


def _call(off, n_groups=None, method=2, ws_short=0, ws_null=False):
    lib = L.load()
    off = np.asarray(off, dtype=np.int32)
    G = len(off) - 1 if n_groups is None else n_groups
    n = max(int(off[-1]), 1)
    segs, scores = np.zeros((n, 2), np.float32), np.zeros(n, np.float32)
    dets, inds = np.zeros((n, 3), np.float32), np.zeros(n, np.int32)
    count = np.full(max(len(off) - 1, 1), SENTINEL, np.int32)
    need = lib.timhip_softnms_1d_workspace_bytes(int(off[-1]), max(G, 0))
    ws = np.zeros(need, np.uint8)
    rc = lib.timhip_softnms_1d(segs.ctypes.data, scores.ctypes.data, off.ctypes.data, off.ctypes.data, G, 0.1, 0.4, 0.001, method,
                               dets.ctypes.data, inds.ctypes.data, count.ctypes.data, None if ws_null else ws.ctypes.data,
                               need - ws_short, None)
    assert (count == SENTINEL).all() and not dets.any() and not inds.any()
    return rc


def test_workspace_grows_with_elements_and_groups():
    lib = L.load()
    assert lib.timhip_softnms_1d_workspace_bytes(8, 2) >= 8 * 4 * 4 + 8 * 2 * 4 + 2 * 5 * 4
    assert lib.timhip_softnms_1d_workspace_bytes(5000, 2) > lib.timhip_softnms_1d_workspace_bytes(8, 2)
    assert lib.timhip_softnms_1d_workspace_bytes(8, 3000) > lib.timhip_softnms_1d_workspace_bytes(8, 2)


def test_method_and_group_count_are_checked():
    assert _call([0, 5, 8], method=3) == L.EINVAL
    assert _call([0, 5, 8], method=-1) == L.EINVAL
    assert _call([0, 5, 8], n_groups=-1) == L.EINVAL


def test_no_groups_is_nothing_to_do():
    assert _call([0], n_groups=0) == OK
    assert _call([0, 5, 8], n_groups=0) == OK


def test_workspace_one_byte_short():
    assert _call([0, 5, 8], ws_short=1) == L.EWORKSPACE
    assert _call([0, 5, 8], ws_null=True) == L.EWORKSPACE


def test_negative_group_size_in_the_host_offsets():
    assert _call([0, 5, 3, 8]) == L.EINVAL                 # group 1 has -2 elements; the workspace is large enough
    assert _call([0, 300, 5000, 4000, 9000]) == L.EINVAL   # the same with groups in three size classes listed before it


def test_null_arguments():
    lib = L.load()
    off = np.array([0, 4], np.int32)
    buf = np.zeros(64, np.float32)
    count = np.full(1, SENTINEL, np.int32)
    args = [buf.ctypes.data, buf.ctypes.data, off.ctypes.data, off.ctypes.data, 1, 0.1, 0.4, 0.001, 2, buf.ctypes.data,
            buf.ctypes.data, count.ctypes.data, buf.ctypes.data, 256, None]
    for i in (0, 1, 2, 3, 9, 10):
        a = list(args)
        a[i] = None
        assert lib.timhip_softnms_1d(*a) == L.EINVAL, i
    assert count[0] == SENTINEL
