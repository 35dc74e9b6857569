"""The signal scan's part of the C ABI without a GPU: the four records' layouts and their numpy twins, the bound symbols, the
unchanged ABI version and batch config, a strict-C99 client of the five entry points that compiles, links and fails loudly
(SS_ERR_DEVICE) where there is no device, and the registers of the three kernels (ss_signal_scan.hip cross-compiled for gfx950 with
the resource-usage remark, as tests/test_peak_series_resources.py does): none of them uses scratch."""
import ctypes
import os
import re
import shutil

import pytest

from soundscope_amd import _lib as L
from soundscope_amd import batch as B
from test_abi import HEADER, build_c_client, declared_symbols, offsets
from test_kernel_resources import HIPCC, _resources

NEW = ("ss_batch_signal_scan", "ss_batch_signal_scan_plan", "ss_batch_download_stream_scans", "ss_batch_download_channel_scans",
       "ss_batch_download_signal_events")
KERNELS = ["k_signal_tiles", "k_signal_carry", "k_signal_events"]


def test_record_layouts():
    assert ctypes.sizeof(L.SignalScanConfig) == 24
    assert offsets(L.SignalScanConfig) == [("silence_threshold", 0), ("clip_level", 4), ("silence_min_frames", 8), ("clip_min_samples", 12),
                                           ("max_events", 16), ("reserved", 20)]
    assert ctypes.sizeof(L.StreamScan) == 56
    assert offsets(L.StreamScan) == [("silent_frames", 0), ("leading_silence", 8), ("trailing_silence", 16), ("longest_silence", 24),
                                     ("longest_silence_at", 32), ("silence_runs", 40), ("clip_runs", 48)]
    assert ctypes.sizeof(L.ChannelScan) == 64
    assert offsets(L.ChannelScan) == [("sum", 0), ("sum_sq", 8), ("nonfinite", 16), ("first_nonfinite", 24), ("clipped_samples", 32),
                                      ("longest_clip", 40), ("longest_clip_at", 48), ("clip_runs", 56)]
    assert ctypes.sizeof(L.SignalEvent) == 24
    assert offsets(L.SignalEvent) == [("first_frame", 0), ("frames", 8), ("channel", 16), ("reserved", 20)]


@pytest.mark.parametrize("dtype, struct", [("STREAM_SCAN_DTYPE", "StreamScan"), ("CHANNEL_SCAN_DTYPE", "ChannelScan"),
                                           ("SIGNAL_EVENT_DTYPE", "SignalEvent")])
def test_numpy_records_match_the_c_records(dtype, struct):
    dt, st = getattr(B, dtype), getattr(L, struct)
    assert dt.itemsize == ctypes.sizeof(st)
    assert [(n, dt.fields[n][1]) for n in dt.names] == offsets(st)
    for (n, ctype) in st._fields_:
        assert dt.fields[n][0] == {ctypes.c_double: "float64", ctypes.c_uint64: "uint64", ctypes.c_uint32: "uint32"}[ctype], n


def test_kinds():
    src = open(HEADER).read()
    assert re.search(r"SS_SIGNAL_SILENCE\s*=\s*0\s*,\s*SS_SIGNAL_CLIP\s*=\s*1", src)
    assert (B.SIGNAL_SILENCE, B.SIGNAL_CLIP) == (L.SS_SIGNAL_SILENCE, L.SS_SIGNAL_CLIP) == (0, 1)


def test_abi_version_and_batch_config_stay():
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2        # additive: the version stays
    assert ctypes.sizeof(L.BatchConfig) == 48


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int


def test_c99_signal_scan_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_signal_scan")
    assert kv["abi"] == "2"
    assert (kv["sizeof_config"], kv["sizeof_stream"], kv["sizeof_channel"], kv["sizeof_event"]) == ("24", "56", "64", "24")
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert (int(kv["tile"]), int(kv["cap"])) == (4096, 3)
        assert (int(kv["trailing"]), int(kv["silence_runs"]), int(kv["n_silence"]), int(kv["silence_at"])) == (9240, 1, 1, 1000)
        assert (int(kv["clip_runs"]), int(kv["n_clips"]), int(kv["clip_at"]), int(kv["clip_frames"]), int(kv["clip_channel"])) == (1, 1, 500, 5, 1)
        assert float(kv["sum0"]) == 0.25 * 10240 and int(kv["clean_runs"]) == 0


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_signal_scan.hip"))


@pytest.mark.parametrize("name", KERNELS)
def test_scan_kernels_use_no_scratch(kernels, name):
    assert name in kernels, sorted(kernels)
    assert int(kernels[name]["ScratchSize [bytes/lane]"]) == 0 and int(kernels[name]["VGPRs Spill"]) == 0, kernels[name]


def test_tile_kernels_leave_room_for_four_workgroups_a_cu(kernels):
    # 256 threads at no more than 128 VGPRs; the tile, the mask words and the sums are dynamic LDS (under 40 KB at every channel count)
    for name in ("k_signal_tiles", "k_signal_events"):
        assert int(kernels[name]["VGPRs"]) <= 128, kernels[name]
