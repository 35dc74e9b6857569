"""Meter-bank spectra at the C boundary (CPU): the bound symbols, a strict-C99 client, and the refusals that need no device."""
import ctypes

import numpy as np

from soundscope_amd import _lib as L
from soundscope_amd.meter_bank import MeterBank

from test_abi import build_c_client, declared_symbols

SPECTRUM_SYMBOLS = ["ss_meter_bank_spectrum_enable", "ss_meter_bank_spectrum_layout", "ss_meter_bank_spectrum",
                    "ss_meter_bank_spectrum_columns"]


def test_spectrum_symbols_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for s in SPECTRUM_SYMBOLS:
        assert s in declared and s in L.SYMBOLS, s
        assert getattr(lib, s) is not None
    assert L.SS_ABI_VERSION == 2 == lib.ss_abi_version()
    for m in ("enable_spectrum", "spectrum_layout", "spectrum", "spectrum_columns"):
        assert callable(getattr(MeterBank, m)), m


def test_c99_meter_bank_spectrum_client(tmp_path):
    """tests/cabi/cabi_meter_bank_spectrum.c compiles as strict C99 and links; without a device the bank refuses with
    SS_ERR_DEVICE, with one the layout is refused before the spectrum is enabled and the whole sequence succeeds after."""
    kv = build_c_client(tmp_path, "cabi_meter_bank_spectrum")
    assert kv["abi"] == "2" and kv["window"] == "16384"
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["before"]) == L.SS_ERR_INVALID_MODE
        assert int(kv["run"]) == L.SS_OK and kv["rows"] == "2" and int(kv["bins"]) > 6000 and kv["status0"] == "0"


def test_spectrum_refusals_without_a_bank():
    """A NULL bank: SS_ERR_DEVICE without a device, SS_ERR_INVALID_ARG with one."""
    lib = L.lib()
    none = L.SS_ERR_DEVICE if lib.ss_device_count() == 0 else L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_enable(None, 1) == none
    assert lib.ss_meter_bank_spectrum_enable(None, 0) == none
    assert lib.ss_meter_bank_spectrum_layout(None, None, None, None, None, 0) == none
    f = np.zeros(4, np.float32)
    st = np.zeros(2, np.int32)
    fp, sp = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert lib.ss_meter_bank_spectrum(None, fp, 4, sp, 2) == none
    assert lib.ss_meter_bank_spectrum_columns(None, 4, L.SS_GAIN_FIXED, 0.0, fp, 4, sp, 2) == none
