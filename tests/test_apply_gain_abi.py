"""The batch gain's part of the C ABI without a GPU: the five records' layouts against the header, the numpy dtypes, the bound
symbols, the unchanged ABI version, the two host functions (ss_gain_envelope bit for bit against gain_envelope, ss_normalisation_gain
against normalisation_gain on planted cases) and a strict-C99 client that compiles, links, gets the host functions' answers and fails
loudly (SS_ERR_DEVICE) where there is no device."""
import ctypes
import math
import re

import numpy as np
import pytest

from soundscope_amd import _lib as L
from soundscope_amd.batch import GAIN_CHANNEL_DTYPE, GAIN_POINT_DTYPE, gain_envelope, normalisation_gain
from test_abi import HEADER, build_c_client, declared_symbols, dtype_offsets, offsets

NEW = ("ss_normalisation_gain", "ss_gain_envelope", "ss_batch_apply_gain", "ss_batch_apply_gain_plan", "ss_batch_download_gain_stats",
       "ss_batch_download_pcm")
INF = math.inf


def test_record_layouts():
    assert ctypes.sizeof(L.NormaliseTarget) == 32
    assert offsets(L.NormaliseTarget) == [("target_lufs", 0), ("max_true_peak_dbtp", 8), ("max_gain_db", 16), ("min_gain_db", 24)]
    assert ctypes.sizeof(L.GainPoint) == 16 and offsets(L.GainPoint) == [("frame", 0), ("stream", 8), ("gain", 12)]
    assert ctypes.sizeof(L.GainConfig) == 16 and offsets(L.GainConfig) == [("channel_mask", 0), ("clip_level", 8), ("reserved", 12)]
    assert ctypes.sizeof(L.GainChannel) == 32
    assert offsets(L.GainChannel) == [("sample_peak", 0), ("touched", 4), ("n_over", 8), ("first_over", 16), ("n_nonfinite", 24)]
    assert ctypes.sizeof(L.PcmDither) == 16 and offsets(L.PcmDither) == [("seed", 0), ("kind", 8), ("reserved", 12)]


def test_the_header_states_the_sizes():
    src = open(HEADER).read()
    for name, size in (("ss_normalise_target", 32), ("ss_gain_point", 16), ("ss_gain_config", 16), ("ss_gain_channel", 32),
                       ("ss_pcm_dither", 16)):
        assert re.search(r"\}\s*%s;\s*/\* %d bytes" % (name, size), src), name
    for name, value in (("SS_GAIN_LIMITED_PEAK", 1), ("SS_GAIN_LIMITED_MAX", 2), ("SS_GAIN_LIMITED_MIN", 4), ("SS_GAIN_UNMEASURED", 8),
                        ("SS_DITHER_NONE", 0), ("SS_DITHER_TPDF", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), src) and getattr(L, name) == value, name


def test_numpy_records_match_the_c_records():
    for dt, struct, size in ((GAIN_POINT_DTYPE, L.GainPoint, 16), (GAIN_CHANNEL_DTYPE, L.GainChannel, 32)):
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
        assert getattr(lib, name).restype is (ctypes.c_double if name == "ss_gain_envelope" else ctypes.c_int)


# ---- ss_gain_envelope ----------------------------------------------------------------------------------------------------------
def points(rows):
    p = np.zeros(len(rows), GAIN_POINT_DTYPE)
    for i, (frame, gain) in enumerate(rows):
        p[i] = (frame, 3, gain)                         # (the stream field is not read)
    return p


def c_envelope(p, frames):
    lib, ptr = L.lib(), p.ctypes.data_as(ctypes.POINTER(L.GainPoint))
    return np.array([lib.ss_gain_envelope(ptr, p.size, int(f)) for f in frames], np.float64)


M24, M33 = 1 << 24, 1 << 33
ENVELOPES = {
    "one point": ([(100, 0.7)], [0, 99, 100, 101, M33]),
    "two adjacent frames": ([(1000, 1.0), (1001, 0.25)], [0, 999, 1000, 1001, 1002]),
    "a ramp of 7 frames": ([(10, 0.1), (17, 0.9)], range(5, 22)),
    "before the first and behind the last": ([(5, -0.5), (50, 0.3), (51, 0.3), (90, 1.7)], [0, 4, 5, 6, 49, 50, 51, 52, 89, 90, 91, 1 << 40]),
    "around 2^24": ([(M24 - 3, 0.3), (M24 + 5, 1.1)], range(M24 - 5, M24 + 8)),
    "around 2^33": ([(M33 - 3, 1.0), (M33 + 6, 1e-3), (M33 + 1000, 3.0)], list(range(M33 - 5, M33 + 9)) + [M33 + 999, M33 + 1000]),
    "from a gain of -0": ([(4, -0.0), (8, 1.0), (12, -0.0), (16, -0.0)], range(0, 20)),
    "thirds that do not round": ([(0, 0.0), (3, 1.0), (1 << 51, 1 / 3)], [0, 1, 2, 3, 4, 12345678901, (1 << 51) - 1, 1 << 51]),
}


@pytest.mark.parametrize("name", sorted(ENVELOPES))
def test_gain_envelope_equals_the_python_expression_in_bits(name):
    rows, frames = ENVELOPES[name]
    p, frames = points(rows), np.array(list(frames), np.uint64)
    got, ref = c_envelope(p, frames), gain_envelope(p, frames)
    assert got.tobytes() == ref.tobytes(), (name, got, ref)
    # the ends are the points' own gains, widened
    assert got[frames <= p["frame"][0]].tobytes() == np.full((frames <= p["frame"][0]).sum(), np.float64(p["gain"][0])).tobytes()
    assert (got[frames >= p["frame"][-1]] == np.float64(p["gain"][-1])).all()


def test_gain_envelope_of_no_point_is_one():
    assert L.lib().ss_gain_envelope(None, 0, 5) == 1.0 and (gain_envelope(np.zeros(0, GAIN_POINT_DTYPE), [0, 9]) == 1.0).all()


def test_gain_envelope_rounds_every_operation():
    """The ramp value as exact rationals rounded step by step: the quotient, the product, the sum (fractions, then float())."""
    from fractions import Fraction as Fr
    p = points([(7, 0.1), (1007, 0.9)])
    g0, g1 = Fr(float(p["gain"][0])), Fr(float(p["gain"][1]))
    d = float(Fr(float(g1 - g0)) / 1000)
    for f in (8, 333, 1006):
        assert c_envelope(p, [f])[0] == float(g0 + Fr(float(Fr(f - 7) * Fr(d))))


# ---- ss_normalisation_gain -----------------------------------------------------------------------------------------------------
def c_gain(loudness, peak, target, ceiling=INF, g_max=INF, g_min=-INF):
    t = L.NormaliseTarget(target, ceiling, g_max, g_min)
    db, lin, why = ctypes.c_double(), ctypes.c_float(), ctypes.c_uint32()
    rc = L.lib().ss_normalisation_gain(ctypes.byref(t), loudness, peak, ctypes.byref(db), ctypes.byref(lin), ctypes.byref(why))
    return rc, db.value, np.float32(lin.value), why.value


PEAK, MAX, MIN, UNMEASURED = L.SS_GAIN_LIMITED_PEAK, L.SS_GAIN_LIMITED_MAX, L.SS_GAIN_LIMITED_MIN, L.SS_GAIN_UNMEASURED
#        name                  loudness peak  (target, ceiling, max, min)       limited_by
GAINS = [("unlimited",           -18.3, 0.40, (-23.0, INF, INF, -INF),           0),
         ("ceiling with room",   -30.0, 0.05, (-23.0, -1.0, INF, -INF),          0),
         ("peak-limited",        -30.0, 0.70, (-23.0, -1.0, INF, -INF),          PEAK),
         ("peak-limited down",   -10.0, 1.60, (-14.0, -1.0, INF, -INF),          PEAK),       # -4 dB wanted, -5.08 dB of headroom
         ("peak-limited loud",   -31.7, 0.93, (-14.0, -2.0, INF, -INF),          PEAK),
         ("max-clamped",         -40.0, 0.01, (-23.0, INF, 12.0, -INF),          MAX),
         ("min-clamped",          -5.0, 0.90, (-23.0, INF, INF, -10.0),          MIN),
         ("peak then max",       -50.0, 0.50, (-23.0, -1.0, 3.0, -INF),          PEAK | MAX),
         ("min breaks ceiling",  -30.0, 0.90, (-23.0, -1.0, INF, 2.0),           PEAK | MIN),
         ("L = -inf",            -INF,  0.50, (-23.0, -1.0, INF, -INF),          UNMEASURED),
         ("L = +inf",             INF,  0.50, (-23.0, -1.0, INF, -INF),          UNMEASURED),
         ("L = NaN",          math.nan, 0.50, (-23.0, -1.0, 6.0, -6.0),          UNMEASURED),
         ("peak = 0",            -30.0, 0.00, (-23.0, -1.0, INF, -INF),          0),
         ("peak = inf",          -30.0, INF,  (-23.0, -1.0, INF, -INF),          0)]


@pytest.mark.parametrize("case", GAINS, ids=[c[0] for c in GAINS])
def test_normalisation_gain_on_planted_cases(case):
    name, loudness, peak, target, why = case
    rc, db, lin, got_why = c_gain(loudness, peak, *target)
    ref_db, ref_lin, ref_why = normalisation_gain(loudness, peak, *target)
    assert rc == L.SS_OK and got_why == why == int(ref_why), (name, got_why, ref_why)
    assert abs(db - float(ref_db)) <= 1e-12, (name, db, ref_db)
    # (libm: the two pow may differ in the last bit, which can move the f32 by one)
    assert lin == ref_lin or lin in (np.nextafter(ref_lin, np.float32(-INF)), np.nextafter(ref_lin, np.float32(INF))), (name, lin, ref_lin)
    if why & UNMEASURED:
        assert db == 0.0 and lin == 1.0
    if why == PEAK:                                     # the ceiling bound: the rounding of the gain does not carry gain * peak above it
        ceiling = target[1]
        assert float(lin) * peak <= 10.0 ** (ceiling / 20.0) * (1.0 + 2.0 ** -50), (name, float(lin) * peak)
        assert float(np.nextafter(lin, np.float32(INF))) * peak > 10.0 ** (ceiling / 20.0) * (1.0 - 2.0 ** -50), name    # ... and is the last such f32
    if why == 0 and math.isfinite(loudness):
        assert db == target[0] - loudness


def test_normalisation_gain_takes_arrays():
    db, lin, why = normalisation_gain([-30.0, -INF, -18.0], [0.7, 0.5, 0.1], -23.0, -1.0)
    assert db.shape == lin.shape == why.shape == (3,) and lin.dtype == np.float32 and why.dtype == np.uint32
    assert list(why) == [PEAK, UNMEASURED, 0]
    for i, (lu, pk) in enumerate(((-30.0, 0.7), (-INF, 0.5), (-18.0, 0.1))):
        one = normalisation_gain(lu, pk, -23.0, -1.0)
        assert float(one[0]) == db[i] and one[1] == lin[i] and int(one[2]) == why[i]


@pytest.mark.parametrize("args", [(-20.0, 0.5, math.nan), (-20.0, 0.5, -23.0, math.nan), (-20.0, 0.5, -23.0, -1.0, math.nan),
                                  (-20.0, 0.5, -23.0, -1.0, INF, math.nan), (-20.0, math.nan, -23.0), (-20.0, 0.5, -23.0, INF, -3.0, 3.0)])
def test_normalisation_gain_refuses_invalid_targets(args):
    assert c_gain(*args)[0] == L.SS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        normalisation_gain(*args)


def test_normalisation_gain_outputs_are_optional():
    t = L.NormaliseTarget(-23.0, INF, INF, -INF)
    assert L.lib().ss_normalisation_gain(ctypes.byref(t), -20.0, 0.5, None, None, None) == L.SS_OK
    assert L.lib().ss_normalisation_gain(None, -20.0, 0.5, None, None, None) == L.SS_ERR_INVALID_ARG


# ---- the C99 client ------------------------------------------------------------------------------------------------------------
def test_c99_apply_gain_client(tmp_path):
    kv = build_c_client(tmp_path, "cabi_apply_gain")
    assert kv["abi"] == "2"
    assert (kv["sizeof_target"], kv["sizeof_point"], kv["sizeof_config"], kv["sizeof_channel"], kv["sizeof_dither"]) == ("32", "16", "16", "32", "16")
    # the host functions answer with or without a device
    assert int(kv["law"]) == L.SS_OK and float(kv["gain_db"]) == -3.0 and int(kv["limited_by"]) == 0
    assert np.float32(float(kv["gain"])) == np.float32(10.0 ** (-3.0 / 20.0)) and int(kv["law_nan"]) == L.SS_ERR_INVALID_ARG
    ramp = points([(100, 1.0), (108, 0.0)])
    assert [float(kv[k]) for k in ("env_mid", "env_before", "env_behind")] == list(gain_envelope(ramp, [102, 0, 5000]))
    if int(kv["devices"]) == 0:
        assert int(kv["create"]) == L.SS_ERR_DEVICE
    else:
        assert int(kv["create"]) == L.SS_OK and int(kv["run"]) == L.SS_OK
        assert int(kv["tile"]) > 0 and kv["touched"] == "1010" and int(kv["peak_ok"]) == 1
