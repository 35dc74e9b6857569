"""The pair series' part of the C ABI without a GPU: the five records' layouts against the header, the numpy dtypes, the bound
symbols, the unchanged ABI version, and a strict-C99 client of the six entry points that compiles, links and fails loudly
(SS_ERR_DEVICE) where there is no device."""
import ctypes
import re

import numpy as np

from soundscope_amd import _lib as L
from test_abi import HEADER, build_c_client, declared_symbols, dtype_offsets, offsets

NEW = ("ss_batch_pair_series", "ss_batch_pair_series_plan", "ss_batch_download_pair_series", "ss_batch_pair_regions",
       "ss_batch_download_region_pairs", "ss_batch_download_group_pairs")
SUMS = [("s_aa", 0), ("s_bb", 8), ("s_ab", 16)]
REGION_TAIL = [("frames", 24), ("skipped", 32), ("n_active", 40), ("n_below", 44), ("first_below", 48), ("longest_below", 52),
               ("longest_below_at", 56), ("below_runs", 60)]
GROUP_TAIL = [("frames", 24), ("skipped", 32), ("n_active", 40), ("n_below", 48), ("below_runs", 56)]


def test_record_layouts():
    assert ctypes.sizeof(L.ChannelPair) == 8 and offsets(L.ChannelPair) == [("a", 0), ("b", 4)]
    assert ctypes.sizeof(L.PairEntry) == 32 and offsets(L.PairEntry) == SUMS + [("frames", 24), ("skipped", 28)]
    assert ctypes.sizeof(L.PairRegionConfig) == 24
    assert offsets(L.PairRegionConfig) == [("threshold", 0), ("power_floor", 8), ("min_run", 16), ("reserved", 20)]
    assert ctypes.sizeof(L.RegionPair) == 64 and offsets(L.RegionPair) == SUMS + REGION_TAIL
    assert ctypes.sizeof(L.GroupPair) == 64 and offsets(L.GroupPair) == SUMS + GROUP_TAIL
    assert ctypes.sizeof(L.LoudnessRegion) == 16         # the region record is what it was


def test_the_header_states_the_sizes():
    src = open(HEADER).read()
    for name, size in (("ss_channel_pair", 8), ("ss_pair_entry", 32), ("ss_pair_region_config", 24), ("ss_region_pair", 64),
                       ("ss_group_pair", 64)):
        assert re.search(r"\}\s*%s;\s*/\* %d bytes" % (name, size), src), name


def test_numpy_records_match_the_c_records():
    from soundscope_amd.batch import GROUP_PAIR_DTYPE, PAIR_ENTRY_DTYPE, REGION_PAIR_DTYPE
    for dt, struct, size in ((PAIR_ENTRY_DTYPE, L.PairEntry, 32), (REGION_PAIR_DTYPE, L.RegionPair, 64), (GROUP_PAIR_DTYPE, L.GroupPair, 64)):
        assert dt.itemsize == size == ctypes.sizeof(struct) and dtype_offsets(dt) == offsets(struct)
        for (name, ctype), n in zip(struct._fields_, dt.names):
            assert np.dtype(ctype) == dt.fields[n][0], (name, n)


def test_host_helpers_on_planted_records():
    from soundscope_amd.batch import PAIR_ENTRY_DTYPE, pair_balance_db, pair_correlation, pair_mono_loss_db
    rec = np.zeros(5, PAIR_ENTRY_DTYPE)
    rec["s_aa"], rec["s_bb"], rec["s_ab"] = [4, 4, 4, 0, 1], [4, 4, 1, 0, 100], [4, -4, 0, 0, 0]       # b = a, b = -a, unrelated, silent, b louder
    c, bal, loss = pair_correlation(rec), pair_balance_db(rec), pair_mono_loss_db(rec)
    assert c[0] == 1.0 and c[1] == -1.0 and c[2] == 0.0 and np.isnan(c[3])
    assert bal[0] == 0.0 and abs(bal[4] - 20.0) < 1e-12 and abs(bal[2] + 10 * np.log10(4)) < 1e-12
    assert loss[0] == 0.0 and loss[1] == -np.inf and abs(loss[2] + 10 * np.log10(2)) < 1e-12 and np.isnan(loss[3])


def test_abi_version_stays():
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2        # additive: the version stays


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int


def test_c99_pair_series_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_pair_series")
    assert kv["abi"] == "2"
    assert (kv["sizeof_pair"], kv["sizeof_entry"], kv["sizeof_config"], kv["sizeof_region_pair"], kv["sizeof_group_pair"]) == ("8", "32", "24", "64", "64")
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert (int(kv["cap"]), int(kv["entries"]), int(kv["pairs"])) == (50, 50, 2) and int(kv["tile"]) > 0
        assert int(kv["tail_frames"]) == 4700                                # the last entry is 100 frames short
        assert int(kv["same_power"]) == 1                                    # (1, 0)'s s_bb and (0, 0)'s s_ab are both the sum of x_0^2
        assert int(kv["item_frames"]) == 48000 and int(kv["album_frames"]) == 4 * (48000 * 5 - 100) and 0 < int(kv["album_active"]) <= 200
