"""The peak series' part of the C ABI without a GPU: the three records' layouts, the bound symbols, the unchanged ABI version and
region record, and a strict-C99 client of the seven entry points that compiles, links and fails loudly (SS_ERR_DEVICE) where there is
no device."""
import ctypes
import re

from soundscope_amd import _lib as L
from test_abi import HEADER, build_c_client, declared_symbols, offsets

NEW = ("ss_batch_peak_series", "ss_batch_peak_series_plan", "ss_batch_download_peak_series", "ss_batch_peak_regions",
       "ss_batch_download_region_peaks", "ss_batch_download_group_peaks", "ss_batch_download_region_channel_peaks")


def test_record_layouts():
    assert ctypes.sizeof(L.PeakEntry) == 16
    assert offsets(L.PeakEntry) == [("true_peak", 0), ("sample_peak", 4), ("true_peak_frame", 8), ("sample_peak_frame", 12)]
    assert ctypes.sizeof(L.RegionPeaks) == 48
    assert offsets(L.RegionPeaks) == [("true_peak", 0), ("sample_peak", 8), ("true_peak_frame", 16), ("sample_peak_frame", 24),
                                      ("true_peak_channel", 32), ("sample_peak_channel", 36), ("n_over", 40), ("first_over", 44)]
    assert ctypes.sizeof(L.GroupPeaks) == 32
    assert offsets(L.GroupPeaks) == [("true_peak", 0), ("sample_peak", 8), ("true_peak_region", 16), ("sample_peak_region", 20),
                                     ("n_over", 24)]
    assert ctypes.sizeof(L.RegionResult) == 48           # the loudness regions' record is what it was


def test_numpy_record_matches_the_c_record():
    from soundscope_amd.batch import PEAK_ENTRY_DTYPE
    assert PEAK_ENTRY_DTYPE.itemsize == 16
    assert [(n, PEAK_ENTRY_DTYPE.fields[n][1]) for n in PEAK_ENTRY_DTYPE.names] == offsets(L.PeakEntry)


def test_abi_version_stays():
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2        # additive: the version stays


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int


def test_c99_peak_series_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_peak_series")
    assert kv["abi"] == "2" and (kv["sizeof_entry"], kv["sizeof_region_peaks"], kv["sizeof_group_peaks"]) == ("16", "48", "32")
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert (int(kv["cap"]), int(kv["entries"])) == (50, 50) and 0 < int(kv["tile"]) <= 4800
        assert int(kv["tail_frame"]) < 4700                                  # the last entry is 100 frames short
        assert float(kv["album_tp"]) >= float(kv["item_tp"]) > 0.0 and int(kv["album_region"]) < 4
        assert 48000 <= int(kv["item_frame"]) < 96000 and float(kv["item_ch0"]) <= float(kv["item_tp"])
