"""The loudness regions' part of the C ABI without a GPU: the three records' layouts, the no-group mark, the bound symbols, and a
strict-C99 client of the four entry points that compiles, links and fails loudly (SS_ERR_DEVICE) where there is no device."""
import ctypes
import os
import re

from soundscope_amd import _lib as L
from test_abi import HEADER, build_c_client, offsets

NEW = ("ss_batch_loudness_regions", "ss_batch_download_region_results", "ss_batch_download_group_results", "ss_batch_group_histograms")


def test_record_layouts():
    assert ctypes.sizeof(L.LoudnessRegion) == 16
    assert offsets(L.LoudnessRegion) == [("stream", 0), ("first_subblock", 4), ("n_subblocks", 8), ("group", 12)]
    assert ctypes.sizeof(L.RegionResult) == 48
    assert offsets(L.RegionResult) == [("integrated_lufs", 0), ("loudness_range", 8), ("max_momentary", 16), ("max_shortterm", 24),
                                       ("max_momentary_at", 32), ("max_shortterm_at", 36), ("n_gating_blocks", 40), ("n_st_blocks", 44)]
    assert ctypes.sizeof(L.GroupResult) == 32
    assert offsets(L.GroupResult) == [("integrated_lufs", 0), ("loudness_range", 8), ("n_gating_blocks", 16), ("n_st_blocks", 24)]


def test_no_group_mark_and_abi_version():
    assert L.SS_REGION_NO_GROUP == 0xFFFFFFFF
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_REGION_NO_GROUP\s+0xFFFFFFFFu\b", src)
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2        # additive: the version stays


def test_entry_points_bound():
    lib = L.lib()
    for name in NEW:
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int


def test_c99_loudness_regions_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_loudness_regions")
    assert kv["abi"] == "2" and (kv["sizeof_region"], kv["sizeof_result"], kv["sizeof_group"]) == ("16", "48", "32")
    assert int(kv["no_group"]) == 0xFFFFFFFF
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["album_blocks"]) == 4 * 47 and (int(kv["item_blocks"]), int(kv["item_st"]), int(kv["item_at"])) == (27, 1, 39)
