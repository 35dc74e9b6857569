"""The loudness series' part of the C ABI without a GPU: the flag, the extremes record's layout, and a strict-C99 client of both new
entry points that compiles, links and fails loudly (SS_ERR_DEVICE) where there is no device."""
import ctypes

from soundscope_amd import _lib as L
from test_abi import build_c_client


def test_flag_value_and_all_unchanged():
    assert L.SS_BATCH_LOUDNESS_SERIES == 32
    assert L.SS_BATCH_ALL == 15 and not (L.SS_BATCH_ALL & L.SS_BATCH_LOUDNESS_SERIES)


def test_extremes_record_is_24_bytes():
    assert ctypes.sizeof(L.LoudnessExtremes) == 24
    assert L.LoudnessExtremes.max_momentary.offset == 0 and L.LoudnessExtremes.max_shortterm.offset == 8
    assert L.LoudnessExtremes.max_momentary_at.offset == 16 and L.LoudnessExtremes.max_shortterm_at.offset == 20


def test_entry_points_bound():
    lib = L.lib()
    for name in ("ss_batch_download_loudness_series", "ss_batch_loudness_extremes"):
        assert name in L.SYMBOLS and hasattr(lib, name)


def test_c99_loudness_series_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_loudness_series")
    assert kv["abi"] == "2" and kv["sizeof_extremes"] == "24" and kv["flag"] == "32"
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert 3 <= int(kv["at_m"]) < 30 and int(kv["at_s"]) == 29
