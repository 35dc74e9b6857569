"""The meter banks' signal watch at the C boundary without a GPU: the two records' layouts (the batch scan's fields at the batch
offsets, then the live fields) and their numpy twins, the bound symbols, the unchanged ABI version and reading, a strict-C99 client
of the four entry points that compiles, links and fails loudly (SS_ERR_DEVICE) where there is no device, a NULL bank, and the
registers of the new kernels (ss_bank_signal_watch.hip cross-compiled for gfx950 with the resource-usage remark): no scratch, no
spilled VGPR, at most 128 VGPRs."""
import ctypes
import os
import re
import shutil

import pytest

from soundscope_amd import _lib as L
from soundscope_amd import batch as B
from soundscope_amd import meter_bank as M
from test_abi import HEADER, build_c_client, declared_symbols, offsets
from test_kernel_resources import HIPCC, _resources

NEW = ("ss_meter_bank_signal_watch_enable", "ss_meter_bank_signal_watch_plan", "ss_meter_bank_signal_watch_reset",
       "ss_meter_bank_signal_watch")
KERNELS = ["k_bank_signal_watch", "k_bank_signal_watch_reset"]


def test_record_layouts():
    assert ctypes.sizeof(L.StreamWatch) == 64 and ctypes.sizeof(L.ChannelWatch) == 80
    assert offsets(L.StreamWatch) == offsets(L.StreamScan) + [("frames", 56)]
    assert offsets(L.ChannelWatch) == offsets(L.ChannelScan) + [("trailing_clip", 64), ("last_clip_frame", 72)]
    src = open(HEADER).read()
    for name, size in (("ss_stream_watch", 64), ("ss_channel_watch", 80)):
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes\s*\*/" % (name, size), src), name


@pytest.mark.parametrize("dtype, struct, batch_dtype", [("STREAM_WATCH_DTYPE", "StreamWatch", "STREAM_SCAN_DTYPE"),
                                                        ("CHANNEL_WATCH_DTYPE", "ChannelWatch", "CHANNEL_SCAN_DTYPE")])
def test_numpy_records_match_the_c_records(dtype, struct, batch_dtype):
    dt, st, bt = getattr(M, dtype), getattr(L, struct), getattr(B, batch_dtype)
    assert dt.itemsize == ctypes.sizeof(st)
    assert [(n, dt.fields[n][1]) for n in dt.names] == offsets(st)
    for (n, ctype) in st._fields_:
        assert dt.fields[n][0] == {ctypes.c_double: "float64", ctypes.c_uint64: "uint64"}[ctype], n
    assert dt.names[:len(bt.names)] == bt.names                 # the batch record's fields first, at the batch record's offsets
    assert all(dt.fields[n] == bt.fields[n] for n in bt.names)


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes is not None
    for m in ("enable_signal_watch", "disable_signal_watch", "signal_watch_plan", "reset_signal_watch", "signal_watch"):
        assert callable(getattr(M.MeterBank, m)), m


def test_abi_version_and_reading_stay():
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2 == L.lib().ss_abi_version()       # additive
    assert ctypes.sizeof(L.MeterReading) == 72 and ctypes.sizeof(L.SignalScanConfig) == 24


def test_c99_meter_bank_watch_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_meter_bank_watch")
    assert kv["abi"] == "2" and (kv["sizeof_stream"], kv["sizeof_channel"]) == ("64", "80")
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK and int(kv["off"]) == L.SS_OK
        assert int(kv["before"]) == L.SS_ERR_INVALID_MODE == int(kv["after"]) and int(kv["events"]) == L.SS_ERR_INVALID_ARG
        assert (int(kv["tile"]), int(kv["frames"])) == (4096, 960)
        # stream 0 is silent on [100, 480) and [580, 960): the second run is open and counts
        assert (int(kv["trailing"]), int(kv["silence_runs"]), int(kv["longest_at"])) == (380, 2, 100)
        assert (int(kv["clip_runs"]), int(kv["last_clip"]), float(kv["sum0"])) == (2, 480 + 54, 0.25 * 200)
        assert int(kv["small"]) == L.SS_ERR_CAPACITY
        assert (int(kv["kept"]), int(kv["after_reset"])) == (960, 0)


def test_refusals_without_a_bank():
    """A NULL bank is SS_ERR_INVALID_ARG — behind the header's standing rule that without a device every compute entry point
    returns SS_ERR_DEVICE."""
    lib = L.lib()
    none = L.SS_ERR_DEVICE if lib.ss_device_count() == 0 else L.SS_ERR_INVALID_ARG
    cfg = L.SignalScanConfig(0.0, 1.0, 1, 1, 0, 0)
    t = ctypes.c_uint32(7)
    assert lib.ss_meter_bank_signal_watch_enable(None, ctypes.byref(cfg)) == none
    assert lib.ss_meter_bank_signal_watch_enable(None, None) == none
    assert lib.ss_meter_bank_signal_watch_plan(None, ctypes.byref(t)) == none and t.value == 7
    assert lib.ss_meter_bank_signal_watch_reset(None, None, 0) == none
    assert lib.ss_meter_bank_signal_watch(None, None, 0, None, 0) == none


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_bank_signal_watch.hip"))


def test_the_file_holds_the_two_kernels(kernels):
    assert sorted(kernels) == KERNELS


@pytest.mark.parametrize("name", KERNELS)
def test_watch_kernels_use_no_scratch(kernels, name):
    assert int(kernels[name]["ScratchSize [bytes/lane]"]) == 0 and int(kernels[name]["VGPRs Spill"]) == 0, kernels[name]
    assert int(kernels[name]["VGPRs"]) <= 128, kernels[name]    # 256 threads: room for four workgroups a CU beside the 40 KB of LDS


def test_the_reset_kernel_uses_no_lds(kernels):
    assert int(kernels["k_bank_signal_watch_reset"]["LDS Size [bytes/block]"]) == 0
