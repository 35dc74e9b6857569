"""The batch limiter's part of the C ABI without a GPU: the three records' layouts against the header, the numpy dtypes, the bound
symbols, the unchanged ABI version, the host function ss_limit_curve bit for bit against a brute-force numpy statement of the
header's steps 2 to 4 (ref_curve, below: a sliding-window minimum, a cumulative sum of u64 and one division), the two inequalities
of step 4, every refusal of the host function, and a strict-C99 client that compiles, links, gets the host function's answers and
fails loudly (SS_ERR_DEVICE) where there is no device."""
import ctypes
import math
import re

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from soundscope_amd import _lib as L
from soundscope_amd.batch import GAIN_CHANNEL_DTYPE, LIMIT_ITEM_DTYPE, LIMIT_STREAM_DTYPE, limit_curve
from test_abi import HEADER, build_c_client, declared_symbols, dtype_offsets, offsets

NEW = ("ss_limit_curve", "ss_batch_limit", "ss_batch_limit_plan", "ss_batch_download_limit_stats")
ONE = 1 << 30
SETTINGS = [(0, 0, 0), (1, 0, 0), (72, 480, 11), (2048, 8192, 23)]         # (look-ahead, hold, advance)
GAINS = [1.0, -2.5, 0.0]


def test_record_layouts():
    assert ctypes.sizeof(L.LimitItem) == 8 and offsets(L.LimitItem) == [("stream", 0), ("gain", 4)]
    assert ctypes.sizeof(L.LimitConfig) == 40
    assert offsets(L.LimitConfig) == [("channel_mask", 0), ("ceiling", 8), ("clip_level", 12), ("lookahead", 16), ("hold", 20),
                                      ("detector", 24), ("reserved", 28), ("scratch_bytes", 32)]
    assert ctypes.sizeof(L.LimitStream) == 32
    assert offsets(L.LimitStream) == [("n_limited", 0), ("first_limited", 8), ("min_sum", 16), ("touched", 24), ("reserved", 28)]


def test_the_header_states_the_sizes():
    src = open(HEADER).read()
    for name, size in (("ss_limit_item", 8), ("ss_limit_config", 40), ("ss_limit_stream", 32)):
        assert re.search(r"\}\s*%s;\s*/\* %d bytes" % (name, size), src), name
    for name, value in (("SS_LIMIT_SAMPLE_PEAK", 0), ("SS_LIMIT_TRUE_PEAK", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), src) and getattr(L, name) == value, name
    for name, value in (("SS_LIMIT_LOOKAHEAD_MAX", 2048), ("SS_LIMIT_HOLD_MAX", 8192)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src) and getattr(L, name) == value, name


def test_numpy_records_match_the_c_records():
    for dt, struct, size in ((LIMIT_ITEM_DTYPE, L.LimitItem, 8), (LIMIT_STREAM_DTYPE, L.LimitStream, 32), (GAIN_CHANNEL_DTYPE, L.GainChannel, 32)):
        assert dt.itemsize == size == ctypes.sizeof(struct) and dtype_offsets(dt) == offsets(struct)
        for (name, ctype), n in zip(struct._fields_, dt.names):
            assert np.dtype(ctype) == dt.fields[n][0], (name, n)


def test_abi_version_stays():
    src = open(HEADER).read()
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", src) and L.SS_ABI_VERSION == 2        # additive: the version stays


def test_entry_points_declared_bound_and_exported():
    lib = L.lib()
    declared = declared_symbols()
    for name in NEW:
        assert name in declared and name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).restype is ctypes.c_int


# ---- ss_limit_curve ------------------------------------------------------------------------------------------------------------
def ref_curve(level, gain, ceiling, lookahead, hold, advance):
    """The header's steps 2 to 4 in numpy, by brute force: (r_q u32, S u64, c f64) of every frame of ONE stream's levels (f32)."""
    m, Lk, H, A = np.asarray(level, np.float32), int(lookahead), int(hold), int(advance)
    n, top = m.size, np.float64(np.float32(ceiling))
    with np.errstate(all="ignore"):
        v = m.astype(np.float64) * np.float64(abs(np.float32(gain)))                  # exact
        over = np.isfinite(v) & (v > top)
        r_q = np.where(over, np.floor(top / np.where(over, v, 1.0) * ONE), ONE).astype(np.uint32)
    # w[i] is w_q of frame k = i - L: the minimum over [k - H, k + L + A], frames outside [0, n) reading ONE
    padded = np.concatenate([np.full(Lk + H, ONE, np.uint32), r_q, np.full(Lk + A, ONE, np.uint32)])
    w = sliding_window_view(padded, H + Lk + A + 1).min(axis=1)
    assert w.size == n + Lk
    run = np.concatenate([np.zeros(1, np.uint64), np.cumsum(w.astype(np.uint64))])
    S = run[Lk + 1:Lk + 1 + n] - run[:n]
    return r_q, S, S.astype(np.float64) / np.float64((Lk + 1) * ONE)


def planted_levels(n, lookahead):
    """A bed of 0.1 with events of 0.9 at frames 0, 3 and n - 1, two closer together than the look-ahead, two further apart, a NaN
    level and an infinite level"""
    m = np.full(n, 0.1, np.float32)
    near = max(1, lookahead // 2)
    for at in (0, 3, n - 1, n // 3, n // 3 + near, n // 2, n // 2 + 3 * lookahead + 7):
        m[at] = 0.9
    m[n // 3 + near] = 0.7
    m[n // 4] = np.nan
    m[n // 4 + 2 * lookahead + 5] = np.inf
    return m


@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("setting", SETTINGS, ids=["L%d_H%d_A%d" % s for s in SETTINGS])
def test_limit_curve_equals_the_numpy_statement_in_bits(setting, gain):
    Lk, H, A = setting
    n = 3 * (Lk + H) + 1000
    m = planted_levels(n, Lk)
    got = limit_curve(m, gain, 0.5, Lk, H, A)
    ref = ref_curve(m, gain, 0.5, Lk, H, A)
    for name, g, r in zip(("r_q", "S", "curve"), got, ref):
        assert g.dtype == r.dtype and g.tobytes() == r.tobytes(), (name, setting, gain, np.flatnonzero(g != r)[:4])
    r_q, S, c = got
    full = (Lk + 1) * ONE
    # a NaN or infinite level never moves the gain; a gain of 0 or levels under the ceiling neither
    assert r_q[n // 4] == ONE and r_q[n // 4 + 2 * Lk + 5] == ONE
    if abs(gain) * 0.9 > 0.5:
        assert r_q[0] < ONE and S[0] < full and (S < full).any()
        if n // 4 - 3 > 3 * Lk + H + A:                 # the events' reaches leave frames between them alone
            assert (S == full).any()
        assert r_q[0] == math.floor(0.5 / (float(np.float32(0.9)) * abs(gain)) * ONE)
    else:
        assert (r_q == ONE).all() and (S == full).all()
    # c == 1 exactly where the sum is full, and below 1 elsewhere
    assert ((c == 1.0) == (S == full)).all() and (c <= 1.0).all() and (S <= full).all()
    # step 4's inequalities: c[n] <= r_q[n] / ONE, and c[m] <= r_q[n] / ONE for m in [n - A, n]
    bound = r_q.astype(np.float64) / ONE
    assert (c <= bound).all()
    for back in range(1, A + 1):
        assert (c[:-back] <= bound[back:]).all(), back


def test_limit_curve_outputs_are_optional_and_an_empty_stream_is_valid():
    lib = L.lib()
    cfg = L.LimitConfig(0, 0.5, 1.0, 4, 4, 0, 0, 0)
    m = planted_levels(200, 4)
    ptr = m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.ss_limit_curve(ptr, m.size, 1.0, ctypes.byref(cfg), 0, None, None, None) == L.SS_OK
    only = np.zeros(m.size, np.uint64)
    assert lib.ss_limit_curve(ptr, m.size, 1.0, ctypes.byref(cfg), 0, None, only.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None) == L.SS_OK
    assert only.tobytes() == ref_curve(m, 1.0, 0.5, 4, 4, 0)[1].tobytes()
    assert lib.ss_limit_curve(None, 0, 1.0, ctypes.byref(cfg), 0, None, None, None) == L.SS_OK
    assert all(a.size == 0 for a in limit_curve(np.zeros(0, np.float32), 1.0, 0.5, 4, 4))


def test_limit_curve_refusals():
    lib = L.lib()
    m = np.full(16, 0.1, np.float32)
    ptr = m.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def call(gain=1.0, ceiling=0.5, lookahead=4, hold=4, advance=0, level=ptr, n=16, cfg=True):
        c = L.LimitConfig(0, ceiling, 1.0, lookahead, hold, 0, 0, 0)
        return lib.ss_limit_curve(level, n, gain, ctypes.byref(c) if cfg else None, advance, None, None, None)

    INVALID = L.SS_ERR_INVALID_ARG
    assert call() == L.SS_OK
    assert call(cfg=False) == INVALID and call(level=None) == INVALID
    assert call(gain=math.nan) == INVALID and call(gain=math.inf) == INVALID and call(gain=-math.inf) == INVALID
    for ceiling in (math.nan, 0.0, -0.5, math.inf):
        assert call(ceiling=ceiling) == INVALID, ceiling
    assert call(lookahead=L.SS_LIMIT_LOOKAHEAD_MAX) == L.SS_OK and call(lookahead=L.SS_LIMIT_LOOKAHEAD_MAX + 1) == INVALID
    assert call(hold=L.SS_LIMIT_HOLD_MAX) == L.SS_OK and call(hold=L.SS_LIMIT_HOLD_MAX + 1) == INVALID
    assert call(advance=23) == L.SS_OK and call(advance=24) == INVALID


# ---- the C99 client ------------------------------------------------------------------------------------------------------------
def test_c99_limiter_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_limiter")
    assert kv["abi"] == "2" and (kv["sizeof_item"], kv["sizeof_config"], kv["sizeof_stream"]) == ("8", "40", "32")
    # the host function answers with or without a device: 0.1 everywhere, 0.9 at frame 6, ceiling 0.5, L = 2, H = 1
    m = np.full(12, 0.1, np.float32)
    m[6] = 0.9
    r_q, S, c = ref_curve(m, 1.0, 0.5, 2, 1, 0)
    assert int(kv["curve"]) == L.SS_OK and int(kv["curve_nan"]) == L.SS_ERR_INVALID_ARG
    assert [int(v) for v in kv["r_q"].split(",")] == list(r_q) and [int(v) for v in kv["sum"].split(",")] == list(S)
    assert [float(v) for v in kv["c"].split(",")] == list(c)
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["tile"]) > 0 and int(kv["group"]) == 2 and kv["touched"] == "1010" and int(kv["under"]) == 1
