"""The batch resampler's part of the C ABI without a GPU: the plan record's layout against the header, the bound symbols, the
unchanged ABI version, and a strict-C99 client that compiles, links, gets the host functions' answers and fails loudly
(SS_ERR_DEVICE) where there is no device."""
import ctypes
import re

import numpy as np

from soundscope_amd import _lib as L
from soundscope_amd.batch import resample_host, resample_length, resample_plan, resample_taps
from test_abi import HEADER, build_c_client, declared_symbols, offsets

NEW = ("ss_resample_plan_make", "ss_resample_taps", "ss_resample_length", "ss_resample_host", "ss_batch_resample", "ss_batch_resample_plan")


def test_record_layout():
    assert ctypes.sizeof(L.ResamplePlan) == 56
    assert offsets(L.ResamplePlan) == [("in_rate", 0), ("out_rate", 4), ("up", 8), ("down", 12), ("taps", 16), ("reserved", 20),
                                       ("attenuation_db", 24), ("passband", 32), ("beta", 40), ("cutoff", 48)]
    assert re.search(r"\}\s*ss_resample_plan;\s*/\* 56 bytes", open(HEADER).read())


def test_abi_version_stays():
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", open(HEADER).read()) and L.SS_ABI_VERSION == 2      # additive: the version stays


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is (ctypes.c_uint64 if name == "ss_resample_length" else ctypes.c_int)


def test_c99_resample_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_resample")
    assert kv["abi"] == "2" and kv["sizeof_plan"] == "56"
    plan = resample_plan(32000, 48000)
    assert int(kv["make"]) == L.SS_OK and int(kv["make_equal"]) == L.SS_ERR_INVALID_ARG and int(kv["make_wide"]) == L.SS_ERR_UNSUPPORTED
    assert (int(kv["up"]), int(kv["down"]), int(kv["taps"])) == (plan.up, plan.down, plan.taps) == (3, 2, 72)
    assert int(kv["length"]) == resample_length(plan, 40) == 60
    # the host functions answer with or without a device: a ramp of 40 frames, stereo, the second channel negated
    x = np.arange(40, dtype=np.float32)[:, None] * np.array([0.25, -0.25], np.float32)[None, :]
    y = resample_host(plan, x, 2)
    assert int(kv["table"]) == L.SS_OK and int(kv["host"]) == L.SS_OK
    assert np.array([float(v) for v in kv["y"].split(",")], np.float32).tobytes() == y.reshape(-1).tobytes()
    assert float(kv["centre"]) == float(resample_taps(plan)[0, 35]) == 1.0
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["tile_out"]) % 3 == 0 and int(kv["tile_in"]) * 3 == int(kv["tile_out"]) * 2
        assert int(kv["frames"]) == resample_length(plan, 9001) and int(kv["passed"]) == 1
