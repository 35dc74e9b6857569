"""The batch spectrogram's part of the C ABI without a GPU: the entry points are exported and bound, the view is 24 bytes in ctypes
and in a strict-C99 client that links, calls the entry points and fails loudly (SS_ERR_DEVICE) where there is no device, the
host arithmetic of the time columns is the floor rule, and the new kernels use no scratch."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from soundscope_amd import _lib as L
from test_abi import build_c_client, declared_symbols
from test_kernel_resources import HIPCC, _resources

ENTRY_POINTS = ("ss_batch_spectrogram", "ss_batch_spectrogram_plan", "ss_batch_download_spectrogram", "ss_spectrogram_column_windows")


def test_entry_points_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.ss_abi_version() == 2                      # entry points only: the version stays


def test_view_is_24_bytes():
    assert C.sizeof(L.SpectrogramView) == 24
    assert [f[0] for f in L.SpectrogramView._fields_] == ["t_cols", "f_cols", "w_min", "w_max", "gain_mode", "gain_db"]
    assert L.SpectrogramView.gain_mode.offset == 16 and L.SpectrogramView.gain_db.offset == 20


def test_c99_spectrogram_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_spectrogram")
    assert kv["abi"] == "2" and kv["sizeof_view"] == "24"
    # 42 windows in 5 columns: the last owns the windows with floor(w * 5 / 42) == 4, i.e. 34 ... 41
    assert (int(kv["last_first"]), int(kv["last_end"])) == (34, 42)
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["early"]) == L.SS_ERR_INVALID_MODE                    # a download before the first call
        assert int(kv["short"]) == L.SS_ERR_CAPACITY
        # 1 s at 48 kHz, N = 4096, hop 1024: 42 windows; two streams x (mid, side) x 5 x 16 cells, each with windows and bins
        assert int(kv["windows"]) == 42 and int(kv["cells"]) == 2 * 2 * 5 * 16 == int(kv["in_chart"])
        assert int(kv["runs"]) >= 1 and int(kv["runs"]) * int(kv["run_windows"]) >= 9


def column_windows(view, t):
    a, e = C.c_uint32(), C.c_uint32()
    L.lib().ss_spectrogram_column_windows(C.byref(view), t, C.byref(a), C.byref(e))
    return a.value, e.value


@pytest.mark.parametrize("w_min,w_max,t_cols", [(0, 7, 3), (5, 6, 4), (0, 1399, 1), (3, 1000, 4096), (0, 37, 64), (30, 50, 5),
                                                (0, 2 ** 32 - 1, 4096), (2 ** 32 - 2, 2 ** 32 - 1, 2)])
def test_column_windows_are_the_floor_rule(w_min, w_max, t_cols):
    view = L.SpectrogramView(t_cols, 1, w_min, w_max, L.SS_GAIN_FIXED, 0.0)
    ranges = np.array([column_windows(view, t) for t in range(t_cols)], dtype=np.uint64)
    # the ranges tile [w_min, w_max) without gap or overlap
    assert ranges[0, 0] == w_min and ranges[-1, 1] == w_max
    assert np.array_equal(ranges[1:, 0], ranges[:-1, 1]) and (ranges[:, 0] <= ranges[:, 1]).all()
    span = w_max - w_min
    if span <= 1 << 20:         # every window of the view: the column the floor rule gives it (Python integers: exact)
        owner = np.array([(w - w_min) * t_cols // span for w in range(w_min, w_max)], dtype=np.int64)
        for t in range(t_cols):
            a, e = int(ranges[t, 0]), int(ranges[t, 1])
            assert (owner[a - w_min:e - w_min] == t).all() and (owner == t).sum() == e - a, (t, a, e)
    else:                       # too many to list: the windows at every column's edges
        for t in range(t_cols):
            a, e = int(ranges[t, 0]), int(ranges[t, 1])
            for w, inside in ((a, a < e), (e - 1, a < e), (a - 1, False), (e, False)):
                if w_min <= w < w_max:
                    assert ((w - w_min) * t_cols // span == t) == inside, (t, a, e, w)
    # outside the view's columns, and degenerate views: (0, 0)
    assert column_windows(view, t_cols) == (0, 0)
    assert column_windows(L.SpectrogramView(0, 1, w_min, w_max, 0, 0.0), 0) == (0, 0)
    assert column_windows(L.SpectrogramView(4097, 1, w_min, w_max, 0, 0.0), 0) == (0, 0)
    assert column_windows(L.SpectrogramView(t_cols, 1, w_max, w_min, 0, 0.0), 0) == (0, 0)


def test_kernels_use_no_scratch():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    ks = dict(_resources("ss_spectrogram.hip"))
    assert sorted(ks) == ["k_spectrogram_columns", "k_spectrogram_join", "k_spectrogram_rows"]
    for name, x in ks.items():
        assert int(x["ScratchSize [bytes/lane]"]) == 0, (name, x)
    # the sweep folds through the chart's column slots: 512 and a spare one, whatever the rows' length
    assert int(ks["k_spectrogram_rows"]["LDS Size [bytes/block]"]) == 4 * 513
    assert int(ks["k_spectrogram_columns"]["LDS Size [bytes/block]"]) == 0 == int(ks["k_spectrogram_join"]["LDS Size [bytes/block]"])
    # ... and hides latency with resident waves: eight per SIMD, i.e. at most 64 VGPRs
    assert int(ks["k_spectrogram_rows"]["VGPRs"]) <= 64 and int(ks["k_spectrogram_rows"]["Occupancy [waves/SIMD]"]) == 8
