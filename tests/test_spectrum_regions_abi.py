"""The spectrum regions' part of the C ABI without a GPU: the entry points are exported and bound, a strict-C99 client links, calls
them and fails loudly (SS_ERR_DEVICE) where there is no device, and ss_region_windows — the host arithmetic the device path runs
on — is the rule "the windows that lie wholly inside the region", checked against an enumeration of the windows in Python integers:
window w covers the frames [first + w hop, first + w hop + fft_n), first = (fft_n // hop + 1) hop - fft_n, and region (a, n) the
frames [a S, (a + n) S), S = (rate + 5) // 10."""
import ctypes as C

import numpy as np
import pytest

from soundscope_amd import _lib as L
from test_abi import build_c_client, declared_symbols

CALLS = ("ss_batch_spectrum_regions", "ss_batch_download_region_spectra", "ss_batch_download_group_spectra",
         "ss_batch_spectrum_regions_plan")
TOP = 0xFFFFFFFF


def test_entry_points_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for name in CALLS + ("ss_region_windows",):
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    for name in CALLS:
        assert getattr(lib, name).restype is C.c_int, name
    assert lib.ss_region_windows.restype is None
    assert lib.ss_abi_version() == 2 == L.SS_ABI_VERSION          # entry points only: the version stays


def test_c99_spectrum_regions_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_spectrum_regions")
    assert kv["abi"] == "2" and kv["sizeof_region"] == "16"
    assert (kv["one"], kv["none"], kv["all"]) == ("74..75", "0..0", "0..89")
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["early"]) == L.SS_ERR_INVALID_MODE == int(kv["early_plan"])       # before the first call
        assert int(kv["short"]) == L.SS_ERR_CAPACITY and int(kv["beyond"]) == L.SS_ERR_INVALID_ARG
        assert int(kv["windows"]) == 89 and kv["counted"] == "89,1,0" and int(kv["pooled"]) == 90
        assert int(kv["finite"]) == int(kv["of"]) == 2 * 2 * 1705 and int(kv["chunks"]) >= 1


def region_windows(rate, fft_n, hop, a, n):
    first, end = C.c_uint32(12345), C.c_uint32(12345)
    L.lib().ss_region_windows(rate, fft_n, hop, a, n, C.byref(first), C.byref(end))
    return first.value, end.value


def enumerated(starts, fft_n, f0, f1):
    """(first, end) of the windows wholly inside the frames [f0, f1), by looking at every window (starts: their first frames,
    ascending, reaching beyond f1); (lo, lo) where there is none, lo the first window that starts at or behind f0"""
    inside = np.flatnonzero((starts >= f0) & (starts + fft_n <= f1))
    if inside.size:
        assert np.array_equal(inside, np.arange(inside[0], inside[-1] + 1))
        return int(inside[0]), int(inside[-1]) + 1
    lo = int(np.flatnonzero(starts >= f0)[0])
    return lo, lo


def window_starts(rate, fft_n, hop, top_subblock):
    first = (fft_n // hop + 1) * hop - fft_n
    return first + hop * np.arange(top_subblock * ((rate + 5) // 10) // hop + 2, dtype=np.int64)


def test_the_worked_example():
    assert region_windows(48000, 4096, 1024, 16, 1) == (74, 75)             # exactly window 74
    assert region_windows(48000, 4096, 1024, 0, 1) == (0, 0)                # too short for a window although n > 0
    assert region_windows(48000, 4096, 1024, 0, 20) == (0, 89)              # all of a 96 000-frame stream
    starts = window_starts(48000, 4096, 1024, 20)
    assert enumerated(starts, 4096, 16 * 4800, 17 * 4800) == (74, 75) and enumerated(starts, 4096, 0, 20 * 4800) == (0, 89)
    assert enumerated(starts, 4096, 0, 4800) == (0, 0)


@pytest.mark.parametrize("hop", [1, 512, 1000, 1024, 4096])
@pytest.mark.parametrize("rate", [22050, 44100, 48000, 96000, 192000])
def test_region_windows_against_enumeration(rate, hop):
    S = (rate + 5) // 10
    for fft_n in (1024, 4096, 16384, 32768):
        starts = window_starts(rate, fft_n, hop, 61)
        ends = starts + fft_n
        for a in range(0, 31):
            for n in range(0, 31):
                f0, f1 = a * S, (a + n) * S
                # the listed windows searched instead of tested one by one (hop 1 lists a window per frame, a million of them) ...
                lo, hi = int(np.searchsorted(starts, f0, "left")), int(np.searchsorted(ends, f1, "right"))
                want = (lo, max(lo, hi))
                if hop > 1:                 # ... which is the same thing wherever testing one by one is affordable
                    assert want == enumerated(starts, fft_n, f0, f1)
                got = region_windows(rate, fft_n, hop, a, n)
                assert got == want, (rate, fft_n, hop, a, n, got, want)


def test_degenerate_and_saturating_cases():
    assert region_windows(48000, 0, 1024, 3, 5) == (0, 0) == region_windows(48000, 4096, 0, 3, 5)
    assert region_windows(0, 4096, 1024, 3, 5) == (0, 0)                     # S = 0: every region is empty
    # a = n = 0xFFFFFFFF at hop 1: the window indices pass 2^32 and read 0xFFFFFFFF
    assert region_windows(192000, 1024, 1, TOP, TOP) == (TOP, TOP)
    assert region_windows(48000, 4096, 1024, TOP, TOP) == tuple(min(v, TOP) for v in (
        -((1024 - TOP * 4800) // 1024), (2 * TOP * 4800 - 4096 - 1024) // 1024 + 1))
    L.lib().ss_region_windows(48000, 4096, 1024, 16, 1, None, None)           # either pointer may be NULL
