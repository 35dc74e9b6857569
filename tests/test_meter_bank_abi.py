"""Meter banks at the C boundary (CPU): the record's layout, the bound symbols, a strict-C99 client, and the refusals that need
no device."""
import ctypes

import numpy as np

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.meter_bank import READING_DTYPE

from test_abi import build_c_client, declared_symbols

BANK_SYMBOLS = ["ss_meter_bank_create", "ss_meter_bank_destroy", "ss_meter_bank_add", "ss_meter_bank_add_device",
                "ss_meter_bank_add_pcm", "ss_meter_bank_reset", "ss_meter_bank_read", "ss_meter_bank_peaks",
                "ss_meter_bank_histograms"]


def test_reading_layout():
    """ss_meter_reading: 4 f64, 2 x 2 f64, u64 = 72 bytes; ctypes and numpy views agree with the header's offsets."""
    R = L.MeterReading
    assert ctypes.sizeof(R) == 72 == READING_DTYPE.itemsize
    want = {"momentary": 0, "shortterm": 8, "integrated": 16, "loudness_range": 24, "true_peak": 32, "sample_peak": 48,
            "frames": 64}
    for name, off in want.items():
        assert getattr(R, name).offset == off, name
        assert READING_DTYPE.fields[name][1] == off, name


def test_bank_symbols_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for s in BANK_SYMBOLS:
        assert s in declared and s in L.SYMBOLS, s
        assert getattr(lib, s) is not None
    assert L.SS_ABI_VERSION == 2 == lib.ss_abi_version()
    assert ssa.MeterBank is not None


def test_c99_meter_bank_client(tmp_path):
    """tests/cabi/cabi_meter_bank.c compiles as strict C99 and links; without a device the bank refuses with SS_ERR_DEVICE,
    with one the whole sequence succeeds (the reset stream counts its frames from the reset)."""
    kv = build_c_client(tmp_path, "cabi_meter_bank")
    assert kv["abi"] == "2" and kv["sizeof_reading"] == "72"
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert kv["frames0"] == "960" and kv["frames2"] == "480"


def test_refusals_without_a_bank():
    """A NULL bank: SS_ERR_DEVICE without a device, SS_ERR_INVALID_ARG with one; a NULL out pointer is refused first."""
    lib = L.lib()
    none = L.SS_ERR_DEVICE if lib.ss_device_count() == 0 else L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_create(1, 2, 48000, 0, None) == L.SS_ERR_INVALID_ARG
    x = np.zeros(4, np.float32)
    assert lib.ss_meter_bank_add(None, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2) == none
    assert lib.ss_meter_bank_add_device(None, None, 2, 4) == none
    assert lib.ss_meter_bank_add_pcm(None, None, 2, L.SS_PCM_S16) == none
    assert lib.ss_meter_bank_reset(None, None, 0) == none
    assert lib.ss_meter_bank_read(None, None, 0) == none
    assert lib.ss_meter_bank_peaks(None, 0, None, None, 0) == none
    assert lib.ss_meter_bank_histograms(None, 0, None) == none
    lib.ss_meter_bank_destroy(None)
    if lib.ss_device_count() == 0:
        h = ctypes.c_void_p()
        assert lib.ss_meter_bank_create(4, 2, 48000, 0, ctypes.byref(h)) == L.SS_ERR_DEVICE and not h.value
