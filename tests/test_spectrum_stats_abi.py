"""The batch spectrum statistics' part of the C ABI without a GPU: the entry points are exported and bound, a strict-C99 client of
them compiles, links and fails loudly (SS_ERR_DEVICE) where there is no device, and the new kernels use no scratch."""
import os
import shutil

import pytest

from soundscope_amd import _lib as L
from test_abi import build_c_client, declared_symbols
from test_kernel_resources import HIPCC, _resources

ENTRY_POINTS = ("ss_batch_spectrum_stats", "ss_batch_download_spectrum_stats", "ss_batch_corpus_spectrum", "ss_batch_spectrum_stats_plan")


def test_entry_points_declared_exported_and_bound():
    lib = L.lib()
    declared = declared_symbols()
    for name in ENTRY_POINTS:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.ss_abi_version() == 2                      # entry points only: the version stays


def test_c99_spectrum_stats_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_spectrum_stats")
    assert kv["abi"] == "2"
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["early"]) == L.SS_ERR_INVALID_MODE                    # a download before the first reduction
        # 1 s at 48 kHz, N = 4096, hop 1024: windows end at 5 * 1024 ... 46 * 1024
        assert int(kv["windows"]) == 42 == int(kv["counted_mid"]) == int(kv["counted_side"])
        assert int(kv["pooled_mid"]) == 84 == int(kv["pooled_side"])
        assert int(kv["chunks"]) >= 1 and int(kv["chunks"]) * int(kv["chunk_windows"]) >= 42
        assert float(kv["max0"]) >= float(kv["mean0"])


def test_kernels_use_no_scratch():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    ks = dict(_resources("ss_spectrum_stats.hip"))
    assert sorted(ks) == ["k_spectrum_stats", "k_spectrum_stats_combine", "k_spectrum_stats_corpus"]
    for name, x in ks.items():
        assert int(x["ScratchSize [bytes/lane]"]) == 0 and int(x["LDS Size [bytes/block]"]) == 0, (name, x)
    # the sweep is a latency-hiding kernel: eight waves per SIMD, i.e. at most 64 VGPRs
    assert int(ks["k_spectrum_stats"]["VGPRs"]) <= 64 and int(ks["k_spectrum_stats"]["Occupancy [waves/SIMD]"]) == 8
