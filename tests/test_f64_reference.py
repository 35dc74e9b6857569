"""The f64 yardstick of the time-domain tests (tests/_f64ref.py) pinned on the CPU before any GPU test leans on it: its designed
K-weighting against the oracle meter's coefficients, its true peak against the oracle meter's f32 interpolator, its series on
a closed-form case, and the event-window shortcut against the whole-channel convolution."""
import numpy as np
import pytest

import _f64ref as R


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000, 96000, 192000])
def test_kweight_design_equals_the_meter(oracle, rate):
    b, a = R.kweight_coeffs(rate)
    ob, oa = oracle.Meter(2, rate).coeffs()
    for mine, theirs in ((b, ob), (a, oa)):
        assert np.all(np.abs(mine - theirs) <= 1e-14 * np.abs(theirs)), (rate, mine, theirs)


@pytest.mark.parametrize("rate,factor", [(48000, 4), (44100, 4), (96000, 2), (48000, 2)])
def test_true_peak_agrees_with_the_meter(oracle, rate, factor):
    """f64 against the crate's f32 polyphase interpolator on short inputs: within 1e-6 of the peak."""
    rng = np.random.default_rng(rate + factor)
    for n in (7, 50, 333, 2001):
        x = (rng.standard_normal((n, 2)) * 0.3).astype(np.float32)
        x[n // 2, 1] = np.float32(0.9)                      # a lone impulse: the interpolator rings around it
        m = oracle.Meter(2, rate, force_tp_factor=factor)
        m.add_frames(x.reshape(-1))
        for c in range(2):
            want = R.true_peak(x[:, c], factor)
            got = max(m.true_peak(c), m.sample_peak(c))
            assert abs(got - want) <= 1e-6 * want, (n, c, got, want)
            assert m.sample_peak(c) == R.true_peak(x[:, c], 0)


@pytest.mark.parametrize("factor", [4, 2])
def test_event_window_true_peak_equals_the_whole_convolution(factor):
    """The windowed shortcut the GPU tests use: exact around the event, bounded elsewhere — equal to the whole-channel
    convolution wherever the bound lies below the event, at the stream's start, middle and end."""
    rng = np.random.default_rng(factor)
    n, span = 3000, 12
    starts = np.array([0, 1, 5, 11, 40, 1500, n - 60, n - span - 3, n - span])
    x = rng.standard_normal((starts.size, n)) * 1e-3
    t = np.arange(span)
    for k, s in enumerate(starts):
        x[k, s:s + span] += 0.7 * np.sin(np.pi / 2 * t + np.pi / 4) * np.hanning(span + 2)[1:-1]
    x = x.astype(np.float32).astype(np.float64)
    peak = R.event_true_peak(R.event_windows(x, starts, span), starts, n, span, factor)
    bg = x.copy()
    for k, s in enumerate(starts):
        bg[k, s:s + span] = 0.0
    for k in range(starts.size):
        assert R.tap_bound(factor) * np.abs(bg[k]).max() < peak[k]
        want = R.true_peak(x[k], factor)
        assert abs(max(peak[k], np.abs(x[k]).max()) - want) <= 1e-14 * want, k      # (the same products, summed in another order)


def test_997hz_sine_reads_minus_3_01_lufs():
    """BS.1770: a 997 Hz sine at 0 dBFS in one channel reads -3.01 LUFS momentary; identical in L and R, 0.00."""
    rate = 48000
    n = 4 * R.subblock_frames(rate) * 5
    s = np.sin(2 * np.pi * 997 * np.arange(n) / rate)
    for x, want in ((np.stack([s, np.zeros(n)], 1), -3.01), (np.stack([s, s], 1), 0.0)):
        sub = R.kweighted_subblocks(x.reshape(-1), rate, 2)
        mom, st = R.loudness_series(sub, rate, 2)
        assert abs(mom[-1] - want) <= 0.005, (mom[-1], want)
        assert np.isneginf(R.loudness_series(np.zeros((5, 2)), rate, 2)[0]).all()


def test_channel_weights():
    assert list(R.channel_weights(1)) == [1.0]
    assert list(R.channel_weights(4)) == [1.0, 1.0, 1.41, 1.41]
    assert list(R.channel_weights(5)) == [1.0, 1.0, 1.0, 1.41, 1.41]
    assert list(R.channel_weights(8)) == [1.0, 1.0, 1.0, 0.0, 1.41, 1.41, 0.0, 0.0]


# ---- the spectrum yardstick of tests/test_gpu_spectrum_forms.py

@pytest.mark.parametrize("rate", [40000, 40960, 44100, 48000, 50000, 96000, 192000, 384000])
def test_retained_bins_equal_the_product(rate):
    """The bin rule for N = 2 ... 32768: 40 kHz keeps its Nyquist bin, 40960 Hz puts 20 Hz and 20 kHz exactly on bins 2 and 2000
    (a rate with no bins at some N included)."""
    import ctypes as C
    from soundscope_amd import _lib as L
    n = 2
    while n <= 32768:
        fb, nb = C.c_uint32(), C.c_uint32()
        assert L.lib().ss_inspect_bins(rate, n, C.byref(fb), C.byref(nb)) == 0
        assert R.retained_bins(rate, n) == (fb.value, nb.value), (rate, n)
        assert R.pink_db(rate, n).size == nb.value
        n *= 2
    if rate == 40000:
        first, count = R.retained_bins(rate, 4096)
        assert first + count - 1 == 2048                    # the Nyquist bin
    if rate == 40960:
        assert R.retained_bins(rate, 4096) == (2, 1999)


@pytest.mark.parametrize("rate,n", [(48000, 4096), (48000, 16384), (40000, 4096), (40000, 4), (44100, 1024), (192000, 32768)])
def test_spectrum_row_closed_forms(rate, n):
    """A bin-centred sine of amplitude A reads 20 log10 A + pink in its bin (a cosine on the Nyquist bin, its own mirror, reads
    20 log10 2A), an all-zero window -150 + pink in every bin.  The Hann weights are rounded to f32 like the crate's: that moves
    the bin by up to 1.5e-8 dB (measured), so the bar is 5e-8 dB; in f64 weights the rest of the arithmetic is exact to 1e-12."""
    first, count = R.retained_bins(rate, n)
    pink = R.pink_db(rate, n)
    t = np.arange(n)
    for k in sorted({first, first + count - 1, first + count // 3}):
        for A in (1.0, 0.25, 1e-3):
            nyq = 2 * k == n
            x = A * np.cos(np.pi * t) if nyq else A * np.sin(2 * np.pi * k * t / n + 0.7)
            row = R.spectrum_row_f64(x, rate, n)
            want = 20 * np.log10(2 * A if nyq else A) + pink[k - first]
            assert abs(row[k - first] - want) <= 5e-8, (k, A, row[k - first] - want)
    assert np.array_equal(R.spectrum_row_f64(np.zeros(n, np.float32), rate, n), -150.0 + pink)


def test_mid_side_f32():
    lr = np.array([[1.0, 3.0], [np.float32(0.1), np.float32(0.2)], [1e-30, -1e-30]], np.float32)
    m, s = R.mid_side_f32(lr)
    assert m.dtype == np.float32 and s.dtype == np.float32
    assert np.array_equal(m, (lr[:, 0] + lr[:, 1]) / np.float32(2)) and np.array_equal(s, (lr[:, 0] - lr[:, 1]) / np.float32(2))


def test_row_error_metric():
    """row_error: relative to the row's own peak amplitude, pink out, the stored value's two ulps allowed."""
    rate, n = 48000, 4096
    pink = R.pink_db(rate, n)
    ref = np.full(pink.size, -100.0) + pink
    ref[10] = -20.0 + pink[10]
    got = ref.astype(np.float32).astype(np.float64)
    assert R.row_error(got, ref, pink) == 0.0                   # storing the row in f32 is not an error
    got = ref.copy()
    got[500] = 20 * np.log10(10 ** (-100 / 20) + 1e-6 * 10 ** (-20 / 20)) + pink[500]
    assert abs(R.row_error(got, ref, pink) - 1e-6) < 1e-9        # one bin off by 1e-6 of the peak
    got = ref + 20 * np.log10(1 + 1e-5)                          # every bin 1e-5 high: the peak's bin sets it, less its allowance
    assert 1e-5 - 5e-7 <= R.row_error(got, ref, pink) <= 1e-5
    assert R.floor_error(got, ref, pink) < 1e-9                  # ... and nothing in the bins 40 dB under it
    got = ref.copy()
    got[500] = 20 * np.log10(10 ** (-100 / 20) + 1e-6 * 10 ** (-20 / 20)) + pink[500]
    assert abs(R.floor_error(got, ref, pink) - 1e-6) < 1e-9


def test_oracle_get_fft_against_the_f64_row(oracle):
    """The oracle's f32 radix-2 get_fft on random windows (noise 0 ... 80 dB under a tone) against the f64 row: within db_close,
    and its worst row_error is 1.8e-7 of the row's peak (measured; bar 1e-6) — the size of an f32 transform's rounding."""
    from conftest import db_close
    rng = np.random.default_rng(7)
    worst = 0.0
    for rate in (40000, 44100, 48000, 96000):
        for n in (1024, 4096, 16384, 32768):
            for _ in range(3):
                x = (rng.standard_normal(n) * 10 ** rng.uniform(-4, 0)).astype(np.float32)
                x += (0.5 * np.sin(2 * np.pi * rng.uniform(20, 19000) * np.arange(n) / rate)).astype(np.float32)
                got = oracle.get_fft(rate, x)[:, 1]
                ref = R.spectrum_row_f64(x, rate, n)
                assert db_close(got, ref, 0.01), (rate, n)
                worst = max(worst, R.row_error(got, ref, R.pink_db(rate, n)))
    assert worst <= 1e-6, worst


# ---- the gate of tests/test_gpu_gating_forms.py

def test_histogram_tables_equal_the_product():
    """the reference's own bin energies and boundaries against the tables the kernels receive, at test_product_tables' bound"""
    import ctypes as C
    from soundscope_amd import _lib as L
    e, b = np.empty(1000), np.empty(1001)
    f64p = C.POINTER(C.c_double)
    assert L.lib().ss_inspect_histogram(e.ctypes.data_as(f64p), b.ctypes.data_as(f64p)) == 0
    en, bd = R.histogram_tables()
    assert en.shape == (1000,) and bd.shape == (1001,)
    assert np.allclose(en, e, rtol=1e-14, atol=0.0) and np.allclose(bd, b, rtol=1e-14, atol=0.0)
    assert np.all((en > bd[:-1]) & (en < bd[1:]))


def _random_histograms():
    """a few hundred histograms: sparse (one to six bins anywhere, or within a lane or two of each other) and dense (every bin,
    or a band), counts of 1 ... 2^40 spread over the magnitudes"""
    rng = np.random.default_rng(3342)
    for k in range(360):
        h = np.zeros(1000, np.uint64)
        top = int(rng.integers(1, 41))
        if k % 3 == 0:
            bins = rng.integers(0, 1000, int(rng.integers(1, 7)))
        elif k % 3 == 1:
            lo = int(rng.integers(0, 960))
            bins = lo + rng.integers(0, 40, int(rng.integers(1, 7)))
        else:
            lo = int(rng.integers(0, 700))
            bins = np.arange(lo, 1000 if k % 2 else lo + int(rng.integers(20, 300)))
        h[bins] = (2.0 ** rng.uniform(0, top, len(bins))).astype(np.uint64)
        yield h


def _close_lu(got, want, tol):
    return got == want if np.isinf(want) or want == 0.0 else abs(got - want) <= tol


def test_histogram_evaluation_agrees_with_the_oracle(oracle):
    """integrated_from_hist / lra_from_hist against the oracle's evaluation of the same histogram.  1e-11 LU is derived, not
    measured: either side adds at most 1000 positive f64 terms in some order (relative error at most 1000 x 2^-53 = 1.1e-13,
    4.8e-13 LU), which leaves a tenfold margin for the log10 and the tables' last bits."""
    import _gating_plants as P
    hists = list(_random_histograms()) + [np.zeros(1000, np.uint64)]
    for p in P.PLANTS:
        ref = P.reference(P.signal_of(p))
        hists += [ref.hb, ref.hs]
    seen = [0, 0]
    for k, h in enumerate(hists):
        gi, wi = R.integrated_from_hist(h), oracle.gated_loudness_hist(h)
        gl, wl = R.lra_from_hist(h), oracle.loudness_range_hist(h)
        assert _close_lu(gi, wi, 1e-11), (k, gi, wi)
        assert _close_lu(gl, wl, 1e-11), (k, gl, wl)
        seen[0] += np.isfinite(wi)
        seen[1] += wl > 0.0
    assert seen[0] > 300 and seen[1] > 200, seen
    assert R.integrated_from_hist(np.zeros(1000, np.uint64)) == -np.inf and R.lra_from_hist(np.zeros(1000, np.uint64)) == 0.0


def test_gate_reference_edges():
    """the reference's own rules on hand-made cases: the bins' half-open edges, the open top bin, what is never counted, the
    start-bin rule on either side of a bin's energy, the short-term phase of a range, the order of the additions"""
    en, bd = R.histogram_tables()
    e = np.array([bd[0], np.nextafter(bd[0], 0.0), bd[1], np.nextafter(bd[1], 0.0), bd[999], bd[1000], 1e30, np.inf, np.nan, 0.0, -1.0])
    assert list(R.hist_bins_of(e)) == [0, -1, 1, 0, 999, 999, 999, 999, -1, -1, -1]
    hb, hs = R.gate_histograms(e, e[:0])
    assert hb.sum() == 7 and hb[999] == 4 and hs.sum() == 0
    assert R.gate_start_bin(en[500]) == (500, 500) and R.gate_start_bin(np.nextafter(en[500], 1.0)) == (500, 501)
    assert R.gate_start_bin(bd[500]) == (500, 500) and R.gate_start_bin(np.nextafter(bd[0], 0.0)) == (0, 0)
    sub = np.arange(1.0, 61.0)[:, None] * np.array([[1.0, 0.5, 0.25, 1e6, 2.0, 4.0]])
    blocks, st = R.gate_blocks(sub, 8000, 6, first=7, n=40)
    w = np.array([1.0, 0.5, 0.25, 0.0, 2.82, 5.64]).sum()
    assert blocks.size == 37 and st.size == 2
    assert np.allclose(blocks, w * np.array([sum(range(j - 2, j + 2)) for j in range(10, 47)]) / 3200.0, rtol=1e-15)
    assert np.allclose(st, w * np.array([sum(range(j - 28, j + 2)) for j in (36, 46)]) / 24000.0, rtol=1e-15)
    assert [a.size for a in R.gate_blocks(sub, 8000, 6, first=3, n=3)] == [0, 0] and [a.size for a in R.gate_blocks(sub, 8000, 6, 0, 30)] == [27, 1]
    # the ranks floor((n - 1) p + 0.5): two entries are ranks 0 and 1, eleven 1 and 10
    h = np.zeros(1000, np.uint64); h[[300, 310]] = 1
    assert R.lra_entries_from_hist(h)[1:] == (2, 300, 310)
    h[:] = 0; h[400:411] = 1
    assert R.lra_entries_from_hist(h)[1:] == (11, 401, 410)
    y = np.ones((100, 2))
    assert R.window_reading(y, [1.0, 1.0], 10, 40) == 10.0 * np.log10(20.0 / 40.0) - 0.691
    assert R.window_reading(y, [1.0, 0.0], 100, 40) == -0.691 and R.window_reading(0 * y, [1.0, 1.0], 50, 40) == -np.inf


def _plants():
    import _gating_plants as P
    return P.PLANTS


@pytest.mark.parametrize("plant", _plants(), ids=[p.name for p in _plants()])
def test_planted_signals_against_the_meter(oracle, plant):
    """every planted signal of the gating forms test: its condition holds in the reference, no value of the reference lies within
    1e-5 LU of a bin edge, and gate_blocks over the f64 sub-blocks agrees with the oracle's meter fed the same samples — the same
    bins (hence block counts), integrated loudness and range within 1e-6 LU"""
    import _gating_plants as P
    x = P.signal_of(plant)
    ref = P.reference(x)
    plant.check(ref)
    assert ref.n_sub == sum(n for n, _ in plant.segments) and ref.blocks.size == ref.n_sub - 3
    assert P.edge_clearance(ref) >= 1e-5, P.edge_clearance(ref)
    m = oracle.Meter(1, P.RATE)
    m.add_frames(x)
    assert m.block_hist().sum() == ref.hb.sum() and m.st_hist().sum() == ref.hs.sum()
    assert np.array_equal(m.block_hist(), ref.hb) and np.array_equal(m.st_hist(), ref.hs)
    assert _close_lu(m.integrated(), ref.integrated, 1e-6), (m.integrated(), ref.integrated)
    assert _close_lu(m.loudness_range(), ref.lra, 1e-6), (m.loudness_range(), ref.lra)
