"""The resampler's host arithmetic without a GPU (include/soundscope_hip.h, "Batch resampler"): the plan rule as the header states it,
the Kaiser-windowed-sinc table against the numpy design (np.sinc, np.i0), the prototype's measured response, the reference chain
ss_resample_host against the f64 polyphase sum within the worst-case bound of a T-step FMA chain, the length rule and the edges."""
import ctypes
import math
import re

import numpy as np
import pytest

from soundscope_amd import _lib as L
from soundscope_amd.batch import resample_host, resample_length, resample_plan, resample_taps
from test_abi import HEADER

# (in, out): L, M, T at the defaults — computed with numpy from the header's rule
PAIRS = {(44100, 48000): (160, 147, 72), (48000, 44100): (147, 160, 76), (96000, 48000): (1, 2, 140), (48000, 96000): (2, 1, 72),
         (88200, 48000): (80, 147, 128), (32000, 48000): (3, 2, 72), (44100, 96000): (320, 147, 72)}
IDS = ["%d_%d" % p for p in PAIRS]


def rule(in_rate, out_rate, A=100.0, pb=20000.0 / 22050.0):
    """the header's plan rule, each operation as written there"""
    g = math.gcd(in_rate, out_rate)
    up, down = out_rate // g, in_rate // g
    fc = 0.5 * min(1.0, up / down)
    delta = 2.0 * (1.0 - pb) * fc
    beta = 0.1102 * (A - 8.7)
    taps = (int(math.ceil((A - 7.95) / (14.36 * delta))) + 3) // 4 * 4
    return up, down, taps, beta, fc


def design(plan):
    """the table in numpy, f64: [L][T]"""
    up, down, T, beta, fc = int(plan.up), int(plan.down), int(plan.taps), float(plan.beta), float(plan.cutoff)
    k, p = np.arange(T)[None, :], np.arange(up)[:, None]
    t = ((k - T // 2 + 1) * up - p) / up
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * t / T) ** 2))) / np.i0(beta)
    return h / h.sum(axis=1, keepdims=True)


def test_the_header_states_the_rule():
    src = open(HEADER).read()
    for text in ("0 meaning 100", "20000.0 / 22050.0", "0.5 * min(1.0, (double)L / (double)M)", "2.0 * (1.0 - passband) * fc",
                 "0.1102 * (A - 8.7)", "ceil((A - 7.95) / (14.36 * delta))", "multiple of 4", "[40, 140]", "[0.5, 0.99]"):
        assert text in src, text
    assert re.search(r"#define\s+SS_RESAMPLE_TAPS_MAX\s+24576\b", src) and L.SS_RESAMPLE_TAPS_MAX == 24576


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_plan_of_the_seven_pairs(pair):
    plan = resample_plan(*pair)
    up, down, taps, beta, fc = rule(*pair)
    assert (plan.up, plan.down, plan.taps) == PAIRS[pair] == (up, down, taps)
    assert (plan.in_rate, plan.out_rate, plan.reserved) == (pair[0], pair[1], 0)
    assert (plan.attenuation_db, plan.passband, plan.beta, plan.cutoff) == (100.0, 20000.0 / 22050.0, beta, fc)
    assert plan.taps % 4 == 0 and plan.up * plan.taps <= L.SS_RESAMPLE_TAPS_MAX


def test_plan_refusals():
    lib = L.lib()
    out = L.ResamplePlan()

    def make(a=44100, b=48000, A=0.0, pb=0.0, ptr=True):
        return lib.ss_resample_plan_make(a, b, A, pb, ctypes.byref(out) if ptr else None)

    INVALID = L.SS_ERR_INVALID_ARG
    assert make() == L.SS_OK
    assert make(b=44100) == INVALID and make(a=0) == INVALID and make(b=0) == INVALID and make(ptr=False) == INVALID
    assert make(A=39.9) == INVALID and make(A=140.1) == INVALID and make(A=math.nan) == INVALID
    assert make(A=40.0) == L.SS_OK and make(A=140.0) == L.SS_OK
    assert make(pb=0.49) == INVALID and make(pb=0.991) == INVALID and make(pb=math.nan) == INVALID
    assert make(pb=0.5) == L.SS_OK and make(pb=0.99, a=48000, b=96000) == L.SS_OK
    assert make(b=192000) == L.SS_ERR_UNSUPPORTED                    # L = 640: 640 x 72 taps
    assert make(A=80.0) == L.SS_OK and (out.up, out.down, out.taps) == rule(44100, 48000, 80.0)[:3]
    assert make(A=120.0, pb=0.8) == L.SS_OK and (out.up, out.down, out.taps) == rule(44100, 48000, 120.0, 0.8)[:3]


def test_taps_refusals():
    lib = L.lib()
    plan = resample_plan(44100, 48000)
    buf = np.zeros(160 * 72, np.float32)
    ptr = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.ss_resample_taps(ctypes.byref(plan), ptr, buf.size) == L.SS_OK
    assert lib.ss_resample_taps(ctypes.byref(plan), ptr, buf.size - 1) == L.SS_ERR_CAPACITY
    assert lib.ss_resample_taps(None, ptr, buf.size) == L.SS_ERR_INVALID_ARG
    assert lib.ss_resample_taps(ctypes.byref(plan), None, buf.size) == L.SS_ERR_INVALID_ARG


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_table_is_the_numpy_design(pair):
    plan = resample_plan(*pair)
    taps = resample_taps(plan)
    ref = design(plan)
    assert taps.dtype == np.float32 and taps.shape == ref.shape == (plan.up, plan.taps)
    assert np.abs(taps.astype(np.float64) - ref).max() <= 1e-7
    assert np.abs(taps.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-6
    if plan.up >= plan.down:
        impulse = np.zeros(plan.taps, np.float32)
        impulse[plan.taps // 2 - 1] = 1.0
        assert taps[0].tobytes() == impulse.tobytes()               # phase 0 passes the input sample through, in bits


def response_db(plan):
    """|H| of the prototype — the table interleaved by time at the rate L x in_rate, unit gain at 0 Hz — on a 2^22-point grid, and
    the grid's frequencies in cycles per INPUT sample"""
    taps = resample_taps(plan).astype(np.float64)
    proto = taps[::-1].T.reshape(-1)                                # sample k L + (L - 1 - p) is tap k of phase p
    n = 1 << 22
    with np.errstate(divide="ignore"):
        mag = 20.0 * np.log10(np.abs(np.fft.rfft(proto, n)) / plan.up)
    return mag, np.arange(n // 2 + 1) / n * plan.up


CASES = [(p, 0.0) for p in PAIRS] + [((44100, 48000), 80.0), ((44100, 48000), 120.0)]


@pytest.mark.parametrize("pair,A", CASES, ids=["%d_%d_A%g" % (p[0], p[1], a) for p, a in CASES])
def test_response_of_the_prototype(pair, A):
    plan = resample_plan(pair[0], pair[1], A)
    mag, f = response_db(plan)
    nyq = plan.cutoff                                               # the lower Nyquist, in cycles per input sample
    ripple = np.abs(mag[f <= plan.passband * nyq]).max()
    stop = mag[f >= (2.0 - plan.passband) * nyq].max()
    print("%d -> %d, A = %g: passband ripple %.2e dB, stopband %.2f dB" % (pair[0], pair[1], plan.attenuation_db, ripple, stop))
    if A == 0.0:                                                    # the seven pairs at the defaults (at A = 80 the design itself ripples by 1.1e-3 dB)
        assert ripple <= 0.001
    assert stop <= -(plan.attenuation_db - 2.0)                     # (the 2 dB: the Kaiser formula's known slack)


def chain_reference(plan, taps, x):
    """one channel: (the f64 polyphase sum, sum |h_k x_k|) of every output"""
    up, down, T = int(plan.up), int(plan.down), int(plan.taps)
    n = np.arange(resample_length(plan, x.size), dtype=np.int64)
    base, ph = n * down // up, n * down % up
    idx = base[:, None] - T // 2 + 1 + np.arange(T)[None, :]
    ok = (idx >= 0) & (idx < x.size)
    xs = np.where(ok, x.astype(np.float64)[np.clip(idx, 0, max(x.size - 1, 0))], 0.0)
    prod = taps.astype(np.float64)[ph] * xs
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_host_chain_within_the_fma_bound_of_the_f64_sum(pair):
    """each of the T fused steps rounds once, by at most 2^-24 of a partial sum that |.| bounds by sum |h_k x_k| (to first order,
    hence T + 1), and the f64 reference's own y carries the last 2^-24 |y|: derived, not measured"""
    plan = resample_plan(*pair)
    taps = resample_taps(plan)
    rng = np.random.default_rng(pair[0])
    F = 3000
    x = (0.2 * rng.standard_normal(F) + 0.5 * np.sin(2 * np.pi * 997.0 * np.arange(F) / pair[0])).astype(np.float32)
    y = resample_host(plan, x, 1, taps=taps)[:, 0].astype(np.float64)
    ref, mass = chain_reference(plan, taps, x)
    bound = (plan.taps + 1) * 2.0 ** -24 * mass + 2.0 ** -24 * np.abs(ref)
    worst = (np.abs(y - ref) / bound).max()
    print("%d -> %d: largest error %.4f of the bound" % (pair[0], pair[1], worst))
    assert (np.abs(y - ref) <= bound).all()


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_lengths(pair):
    plan = resample_plan(*pair)
    up, down = plan.up, plan.down
    for F in (0, 1, down - 1, down, down + 1, 10 ** 9 + 7):
        want = -(-F * up // down)
        assert resample_length(plan, F) == want, F
        if F < 1000:                                                # the rule itself: the outputs n with n M < F L
            assert want == sum(1 for n in range(want + 2) if n * down < F * up), F


def test_windows_equal_slices_of_the_whole():
    plan = resample_plan(48000, 44100)
    x = np.random.default_rng(3).standard_normal((700, 3)).astype(np.float32)
    whole = resample_host(plan, x, 3)
    assert whole.shape == (resample_length(plan, 700), 3)
    for first, n in ((0, 0), (0, 1), (1, 100), (147, 147), (whole.shape[0] - 5, 5), (whole.shape[0], 0)):
        assert resample_host(plan, x, 3, first, n).tobytes() == whole[first:first + n].tobytes(), (first, n)
    lib, t, f32p = L.lib(), resample_taps(plan), ctypes.POINTER(ctypes.c_float)
    out = np.zeros(8, np.float32)
    args = (ctypes.byref(plan), t.ctypes.data_as(f32p), x.ctypes.data_as(f32p), 700, 3)
    assert lib.ss_resample_host(*args, whole.shape[0], 1, out.ctypes.data_as(f32p)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_resample_host(*args[:4], 0, 0, 1, out.ctypes.data_as(f32p)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_resample_host(args[0], None, *args[2:], 0, 1, out.ctypes.data_as(f32p)) == L.SS_ERR_INVALID_ARG


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_a_single_sample_gives_the_table_reversed_in_time(pair):
    plan = resample_plan(*pair)
    taps = resample_taps(plan)
    y = resample_host(plan, np.ones(1, np.float32), 1)[:, 0]
    n = np.arange(y.size)
    base, ph = n * plan.down // plan.up, n * plan.down % plan.up
    assert (base == 0).all() and y.size == resample_length(plan, 1)
    assert y.tobytes() == taps[ph, plan.taps // 2 - 1 - base].tobytes()     # x[0] meets tap T/2 - 1 - base of the output's phase
    # the same over a longer run of zeros behind it: output n reads column T/2 - 1 - base(n), later outputs earlier taps
    x = np.zeros(plan.taps, np.float32)
    x[0] = 1.0
    y = resample_host(plan, x, 1)[:, 0]
    n = np.arange(y.size)
    base, ph = n * plan.down // plan.up, n * plan.down % plan.up
    k = plan.taps // 2 - 1 - base
    want = np.where(k >= 0, taps[ph, np.clip(k, 0, plan.taps - 1)], 0.0).astype(np.float32)
    assert np.array_equal(y, want)


@pytest.mark.parametrize("pair", [p for p in PAIRS if p[1] > p[0]], ids=lambda p: "%d_%d" % p)
def test_upsampling_passes_the_input_samples_through(pair):
    plan = resample_plan(*pair)
    x = np.random.default_rng(9).standard_normal((501, 2)).astype(np.float32)
    y = resample_host(plan, x, 2)
    j = np.arange(-(-y.shape[0] // plan.up))
    assert y[j * plan.up].tobytes() == x[j * plan.down].tobytes()


def test_non_finite_samples_stay_in_their_window():
    plan = resample_plan(44100, 48000)
    x = np.random.default_rng(4).standard_normal(2000).astype(np.float32)
    bad = x.copy()
    bad[1000] = np.nan
    y, z = resample_host(plan, x)[:, 0], resample_host(plan, bad)[:, 0]
    base = np.arange(y.size) * plan.down // plan.up
    hit = (base - plan.taps // 2 + 1 <= 1000) & (1000 <= base + plan.taps // 2)
    assert y[~hit].tobytes() == z[~hit].tobytes() and np.isnan(z[hit]).all()
