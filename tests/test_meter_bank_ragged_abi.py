"""Ragged meter-bank adds at the C boundary (CPU): the three symbols, a strict-C99 client, the refusals that need no device."""
import ctypes

import soundscope_amd as ssa
from soundscope_amd import _lib as L

from test_abi import build_c_client, declared_symbols

RAGGED_SYMBOLS = ["ss_meter_bank_add_ragged", "ss_meter_bank_add_ragged_pcm", "ss_meter_bank_add_ragged_device"]


def test_ragged_symbols_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for s in RAGGED_SYMBOLS:
        assert s in declared and s in L.SYMBOLS, s
        assert getattr(lib, s).argtypes is not None, s
    assert L.SS_ABI_VERSION == 2 == lib.ss_abi_version()
    for name in ("add_ragged", "add_ragged_pcm", "add_ragged_device"):
        assert callable(getattr(ssa.MeterBank, name))


def test_refusals_without_a_bank():
    """A NULL bank: SS_ERR_DEVICE without a device, SS_ERR_INVALID_ARG with one — whatever else is wrong with the call."""
    lib = L.lib()
    none = L.SS_ERR_DEVICE if lib.ss_device_count() == 0 else L.SS_ERR_INVALID_ARG
    frames = (ctypes.c_uint64 * 2)(4, 0)
    assert lib.ss_meter_bank_add_ragged(None, None, frames) == none
    assert lib.ss_meter_bank_add_ragged(None, None, None) == none
    assert lib.ss_meter_bank_add_ragged_pcm(None, None, frames, L.SS_PCM_S16) == none
    assert lib.ss_meter_bank_add_ragged_pcm(None, None, frames, 7) == none
    assert lib.ss_meter_bank_add_ragged_device(None, None, frames, 8) == none


def test_c99_ragged_client(tmp_path):
    """tests/cabi/cabi_meter_bank_ragged.c compiles as strict C99 and links; without a device the bank refuses with SS_ERR_DEVICE,
    with one every stream's frame count is the sum of what the two ragged calls gave it."""
    kv = build_c_client(tmp_path, "cabi_meter_bank_ragged")
    assert kv["abi"] == "2"
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert kv["frames0"] == "1440" and kv["frames1"] == "1000" and kv["frames2"] == "498"
