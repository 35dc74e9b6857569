"""Tracked meter-bank spectra at the C boundary (CPU): the five entry points are declared, exported and bound, the parameter
struct has the header's size, a strict-C99 client compiles, links and fails loudly (SS_ERR_DEVICE) where there is no device, a NULL
bank is refused, and the new kernels use no scratch — the update kernel no LDS either."""
import ctypes
import os
import shutil

import numpy as np
import pytest

from soundscope_amd import _lib as L
from soundscope_amd.meter_bank import MeterBank

from test_abi import build_c_client, declared_symbols
from test_kernel_resources import HIPCC, _resources

ENTRY_POINTS = ("ss_meter_bank_spectrum_track_enable", "ss_meter_bank_spectrum_track", "ss_meter_bank_spectrum_track_reset",
                "ss_meter_bank_spectrum_tracked", "ss_meter_bank_spectrum_tracked_columns")


def test_entry_points_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared and name in L.SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.ss_abi_version() == 2 == L.SS_ABI_VERSION      # entry points only: the version stays
    for m in ("enable_spectrum_tracking", "disable_spectrum_tracking", "track_spectrum", "tracked_spectrum",
              "tracked_spectrum_columns", "reset_spectrum_tracking"):
        assert callable(getattr(MeterBank, m)), m


def test_ballistics_struct_size():
    assert ctypes.sizeof(L.SpectrumBallistics) == 24
    assert [f[0] for f in L.SpectrumBallistics._fields_] == ["average_tau_s", "hold_s", "decay_db_per_s"]


def test_c99_meter_bank_track_client(tmp_path):
    """tests/cabi/cabi_meter_bank_track.c compiles as strict C99 and links; without a device the bank refuses with SS_ERR_DEVICE,
    with one it runs enable -> add -> track -> tracked and prints the update counts."""
    kv = build_c_client(tmp_path, "cabi_meter_bank_track")
    assert kv["abi"] == "2" and kv["sizeof_cfg"] == "24"
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK
        assert int(kv["no_history"]) == L.SS_ERR_INVALID_MODE and int(kv["before"]) == L.SS_ERR_INVALID_MODE
        assert int(kv["run"]) == L.SS_OK and int(kv["off"]) == L.SS_OK
        assert kv["rows"] == "2" and int(kv["bins"]) == 6820
        assert kv["updates0"] == "2" and kv["updates3"] == "2" and kv["hold_ge_avg"] == "1"
        assert kv["after_reset"] == "0"


def test_refusals_without_a_bank():
    """A NULL bank is SS_ERR_INVALID_ARG — behind the header's standing rule that without a device every compute entry point
    returns SS_ERR_DEVICE."""
    lib = L.lib()
    none = L.SS_ERR_DEVICE if lib.ss_device_count() == 0 else L.SS_ERR_INVALID_ARG
    cfg = L.SpectrumBallistics(0.125, 0.5, 16.0)
    f = np.zeros(4, np.float32)
    u = np.zeros(2, np.uint32)
    fp, up = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), u.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert lib.ss_meter_bank_spectrum_track_enable(None, ctypes.byref(cfg)) == none
    assert lib.ss_meter_bank_spectrum_track_enable(None, None) == none
    assert lib.ss_meter_bank_spectrum_track(None) == none
    assert lib.ss_meter_bank_spectrum_track_reset(None, None, 0) == none
    assert lib.ss_meter_bank_spectrum_tracked(None, fp, fp, 4, up, 2) == none
    assert lib.ss_meter_bank_spectrum_tracked_columns(None, 2, L.SS_GAIN_FIXED, 0.0, fp, fp, 4, up, 2) == none


def test_kernels_use_no_scratch_and_the_update_no_lds():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    ks = dict(_resources("ss_bank_spectrum_track.hip"))
    assert sorted(ks) == ["k_bank_spectrum_track", "k_bank_spectrum_track_reset", "k_bank_spectrum_tracked_columns",
                          "k_bank_spectrum_tracked_rows"]
    for name, x in ks.items():
        assert int(x["ScratchSize [bytes/lane]"]) == 0, (name, x)
    for name in ("k_bank_spectrum_track", "k_bank_spectrum_track_reset", "k_bank_spectrum_tracked_rows"):
        assert int(ks[name]["LDS Size [bytes/block]"]) == 0, (name, ks[name])
    # the update is a latency-hiding sweep: eight waves per SIMD, i.e. at most 64 VGPRs
    assert int(ks["k_bank_spectrum_track"]["VGPRs"]) <= 64 and int(ks["k_bank_spectrum_track"]["Occupancy [waves/SIMD]"]) == 8
    # two curves x 512 column accumulators
    assert int(ks["k_bank_spectrum_tracked_columns"]["LDS Size [bytes/block]"]) == 2 * 512 * 4
