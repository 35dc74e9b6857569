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
