"""The meter banks' pair watch at the C boundary without a GPU: the three records' layouts against the header, the "N bytes"
comments and the numpy twins, the bound symbols, the unchanged ABI version and pair entry, a NULL bank, a strict-C99 client of the
five entry points that compiles, links and fails loudly (SS_ERR_DEVICE) where there is no device — with one it feeds b = -a for two
entries and reads n_below == 2, trailing_below == 2 and correlation -1 — and the registers of the new kernels
(ss_bank_pair_watch.hip cross-compiled for gfx950 with the resource-usage remark): no scratch, no spilled VGPR, at most 128 VGPRs,
no LDS in the reset kernel."""
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

NEW = ("ss_meter_bank_pair_watch_enable", "ss_meter_bank_pair_watch_plan", "ss_meter_bank_pair_watch_reset",
       "ss_meter_bank_pair_watch", "ss_meter_bank_pair_watch_entries")
KERNELS = ["k_bank_pair_watch", "k_bank_pair_watch_reset"]
U64_FIELDS = ("entries", "n_active", "n_below", "first_below", "longest_below", "longest_below_at", "below_runs", "trailing_below")


def header_struct(name):
    """[(field, C type)] of `typedef struct name { ... } name;` in the header, in order (comments dropped, `a, b` lists split)"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s;" % (name, name), src, re.S).group(1)
    out = []
    for decl in body.split(";"):
        words = decl.split()
        if words:
            ctype, names = words[0], "".join(words[1:]).split(",")
            out += [(n, ctype) for n in names]
    return out


def test_record_layouts_against_the_header():
    assert (ctypes.sizeof(L.PairSums), ctypes.sizeof(L.PairWatchConfig), ctypes.sizeof(L.PairWatch)) == (40, 24, 160)
    assert offsets(L.PairSums) == [("s_aa", 0), ("s_bb", 8), ("s_ab", 16), ("frames", 24), ("skipped", 32)]
    assert offsets(L.PairWatchConfig) == [("threshold", 0), ("power_floor", 8), ("min_run", 16), ("window_entries", 20)]
    assert offsets(L.PairWatch) == [("window", 0), ("total", 40)] + [(n, 80 + 8 * i) for i, n in enumerate(U64_FIELDS)] + [
        ("open_frames", 144), ("window_count", 148), ("reserved", 152)]
    ctypes_of = {"double": ctypes.c_double, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "ss_pair_sums": L.PairSums}
    for name, struct in (("ss_pair_sums", L.PairSums), ("ss_pair_watch_config", L.PairWatchConfig), ("ss_pair_watch", L.PairWatch)):
        assert [(n, ctypes_of[t]) for n, t in header_struct(name)] == list(struct._fields_), name
    src = open(HEADER).read()
    for name, size in (("ss_pair_sums", 40), ("ss_pair_watch_config", 24), ("ss_pair_watch", 160)):
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes\s*\*/" % (name, size), src), name
    assert re.search(r"#define\s+SS_BANK_PAIR_WINDOW_MAX\s+600\b", src)


def test_numpy_records_match_the_c_records():
    assert M.PAIR_SUMS_DTYPE.itemsize == 40 and M.PAIR_WATCH_DTYPE.itemsize == 160
    assert [(n, M.PAIR_SUMS_DTYPE.fields[n][1]) for n in M.PAIR_SUMS_DTYPE.names] == offsets(L.PairSums)
    assert [(n, M.PAIR_WATCH_DTYPE.fields[n][1]) for n in M.PAIR_WATCH_DTYPE.names] == offsets(L.PairWatch)
    kinds = {ctypes.c_double: "float64", ctypes.c_uint64: "uint64", ctypes.c_uint32: "uint32"}
    for n, ctype in L.PairSums._fields_:
        assert M.PAIR_SUMS_DTYPE.fields[n][0] == kinds[ctype], n
    for n, ctype in L.PairWatch._fields_:
        assert M.PAIR_WATCH_DTYPE.fields[n][0] == (M.PAIR_SUMS_DTYPE if ctype is L.PairSums else kinds[ctype]), n
    # the nested records carry the pair entries' names: the batch helpers read rec["window"] directly
    assert M.PAIR_SUMS_DTYPE.names[:3] == B.PAIR_ENTRY_DTYPE.names[:3] == ("s_aa", "s_bb", "s_ab")
    import numpy as np
    rec = np.zeros(2, M.PAIR_WATCH_DTYPE)
    rec["window"]["s_aa"], rec["window"]["s_bb"], rec["window"]["s_ab"] = 4.0, 1.0, -2.0
    assert list(B.pair_correlation(rec["window"])) == [-1.0, -1.0]
    assert np.allclose(B.pair_balance_db(rec["window"]), 10 * np.log10(0.25)) and np.allclose(B.pair_mono_loss_db(rec["window"]), -10.0)


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes is not None
    for m in ("enable_pair_watch", "disable_pair_watch", "pair_watch_plan", "reset_pair_watch", "pair_watch", "pair_watch_entries"):
        assert callable(getattr(M.MeterBank, m)), m


def test_abi_version_and_pair_entry_stay():
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2 == L.lib().ss_abi_version()       # additive
    assert ctypes.sizeof(L.PairEntry) == 32 == B.PAIR_ENTRY_DTYPE.itemsize and ctypes.sizeof(L.ChannelPair) == 8
    assert ctypes.sizeof(L.MeterReading) == 72


def test_c99_meter_bank_pair_watch_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_meter_bank_pair_watch")
    assert kv["abi"] == "2"
    assert (kv["sizeof_sums"], kv["sizeof_config"], kv["sizeof_watch"], kv["sizeof_entry"]) == ("40", "24", "160", "32")
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK and int(kv["off"]) == L.SS_OK
        assert int(kv["before"]) == L.SS_ERR_INVALID_MODE == int(kv["after"])
        assert int(kv["wide"]) == L.SS_ERR_INVALID_ARG == int(kv["badpair"])
        assert (int(kv["lanes"]), int(kv["window"]), int(kv["pairs"])) == (256, 30, 1)
        # stream 0: b = -a over two complete entries, nothing open
        assert (int(kv["entries"]), int(kv["open"]), int(kv["n_below"]), int(kv["trailing"]), int(kv["first_below"])) == (2, 0, 2, 2, 0)
        assert float(kv["corr"]) == -1.0
        assert int(kv["same_below"]) == 0 and float(kv["same_corr"]) == 1.0
        assert (int(kv["ring"]), int(kv["first"]), int(kv["ring_frames"])) == (2, 0, 4800)
        assert int(kv["small"]) == L.SS_ERR_CAPACITY
        assert (int(kv["kept"]), int(kv["after_reset"])) == (2, 0)


def test_refusals_without_a_bank():
    """A NULL bank is SS_ERR_INVALID_ARG — behind the header's standing rule that without a device every compute entry point
    returns SS_ERR_DEVICE."""
    lib = L.lib()
    none = L.SS_ERR_DEVICE if lib.ss_device_count() == 0 else L.SS_ERR_INVALID_ARG
    cfg = L.PairWatchConfig(0.0, 0.0, 1, 30)
    a, b, c = ctypes.c_uint32(7), ctypes.c_uint32(8), ctypes.c_uint32(9)
    first, n = ctypes.c_uint64(5), ctypes.c_uint32(6)
    assert lib.ss_meter_bank_pair_watch_enable(None, None, 0, ctypes.byref(cfg)) == none
    assert lib.ss_meter_bank_pair_watch_enable(None, None, 0, None) == none
    assert lib.ss_meter_bank_pair_watch_plan(None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == none
    assert (a.value, b.value, c.value) == (7, 8, 9)
    assert lib.ss_meter_bank_pair_watch_reset(None, None, 0) == none
    assert lib.ss_meter_bank_pair_watch(None, None, 0) == none
    assert lib.ss_meter_bank_pair_watch_entries(None, 0, None, 0, ctypes.byref(first), ctypes.byref(n)) == none
    assert (first.value, n.value) == (5, 6)


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.skip("no hipcc / c++filt in this environment")
    return dict(_resources("ss_bank_pair_watch.hip"))


def test_the_file_holds_the_two_kernels(kernels):
    assert sorted(kernels) == KERNELS


@pytest.mark.parametrize("name", KERNELS)
def test_pair_watch_kernels_use_no_scratch(kernels, name):
    assert int(kernels[name]["ScratchSize [bytes/lane]"]) == 0 and int(kernels[name]["VGPRs Spill"]) == 0, kernels[name]
    assert int(kernels[name]["VGPRs"]) <= 128, kernels[name]    # 256 threads: room for four workgroups a CU


def test_the_reset_kernel_uses_no_lds(kernels):
    assert int(kernels["k_bank_pair_watch_reset"]["LDS Size [bytes/block]"]) == 0
