"""The radix-16 core with its constant twiddles fused into the butterflies' fmas (fft16, soundscope_amd/csrc/ss_fft_dev.h): every
launch form that runs it against the f64 rows of tests/_f64ref.py, on the smallest shapes that reach the form, at planted edges.

Shapes.  A window ends at (N / hop + 1 + w) hop, so three windows of N = 4096 at hop 1024 are 7168 frames (6144 hold two), and
k_fft16k_run is planned from eight windows up: 24576 frames at N = 16384 — 17408 frames are ONE window, which k_fft16k takes and
which is kept as a form of its own.  Every case asserts the kernel the plan names before it looks at a value.

  ms1            2 streams x 7168 frames, stereo, 48 kHz: three windows
  ms1 columns    the same three windows, columns-only, against the two-pass reduction of the stored rows, bit for bit
  pairw          mono, 2 streams x 7168 frames: windows (0, 1) on one transform, window 2 with an empty partner
  k_fft16k_run   one stereo stream x 24576 frames at 96 kHz: eight windows, mid and side rows
  k_fft16k       one stereo stream x 17408 frames at 96 kHz: one window

Planted edges.  A full-scale sine on a bin centre whose second row carries the same bin 120 dB under it (bin k of one row and
bin N - k of the other meet in one butterfly of the packed transform); a second row 20 dB OVER the first; a second row of exact
zeros, which must read -150 + pink to the bit (f32: the kernels' own expression of the floor); an onset inside a window, off the
hop grid.

Where the onsets stand.  The bounds are the transform's rounding noise as a fraction of a row's own peak.  Two things that are
none of the core's reach them when a row's whole content lies under the tail of the Hann weights, so the material keeps away:
  * k_fft16k_run rebuilds its window weights from twiddles, to about 2^-24 ABSOLUTE; a row that is silent up to the window's
    last 524 frames (weights under 0.01) sees that as 1e-6 of its peak.  Measured with such a side row: floor_error 1.07e-6
    with the 81-instruction core and 1.06e-6 with this one.  The N = 16384 onset is 808 ... 7976 frames into its windows.
  * k_fft4096_pairw matches its two windows by windowed ENERGY; a tenfold step 644 frames before the end of the second window
    leaves that window's largest windowed sample 2.25 times the first's, and the first row's floor doubles: 3.16e-7 with either
    core, to all digits.  Windows that overlap by three quarters cannot differ by 20 dB throughout, so pairw carries no such step.
Every tone stands on a RETAINED bin (20 Hz ... 20 kHz): a row's peak is then the window's strongest component, which is what any
f32 transform's noise is relative to (conftest.db_close, `peak`).

Bounds, those of tests/test_gpu_spectrum_forms.py: row_error <= 4e-6 of the row's peak amplitude, floor_error (the bins 40 dB and
more under the peak) <= 3e-7 of it, every strong bin within 0.01 dB (conftest.db_close with the pink term taken out)."""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import db_close
import _f64ref as R

pytestmark = pytest.mark.gpu

BOUND, FLOOR = 4e-6, 3e-7
ONSET = 5500                     # inside windows 1 and 2 of N = 4096 ([2048, 6144), [3072, 7168)), 380 frames off the hop grid


def _kernel(b):
    return L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT).decode()


def _sine(frames, k, n, amp, phase):
    return amp * np.sin(2.0 * np.pi * k * np.arange(frames, dtype=np.float64) / n + phase)


def _noise(seed, frames, amp):
    return amp * np.random.default_rng(seed).uniform(-1.0, 1.0, frames)


def _stereo(mid, side):
    return np.stack([mid + side, mid - side], 1).astype(np.float32)


def _zero_row_f32(pink, n):
    """-150 + pink as the kernels store it: N = 4096 reads pink back out of its (offset + pink) table, N = 16384 adds the f32 pink"""
    pf = pink.astype(np.float32)
    if n == 4096:
        off = np.float32(10.0 * np.log10(4.0 / (4096.0 * 4096.0)))
        return np.float32(-150.0) + ((off + pf).astype(np.float32) - off).astype(np.float32)
    return np.float32(-150.0) + pf


def _check(got, x, rate, n, what, zero=False):
    """one stored row against the f64 row of the mono window x"""
    pink = R.pink_db(rate, n)
    ref = R.spectrum_row_f64(x, rate, n)
    if zero:
        assert not np.any(x), what
        assert np.array_equal(got, _zero_row_f32(pink, n)), (what, "zero row", float(np.abs(got - (-150.0 + pink)).max()))
        return 0.0, 0.0
    assert np.any(x), what
    g = got.astype(np.float64)
    e, f = R.row_error(g, ref, pink), R.floor_error(g, ref, pink)
    print("%-28s row_error %.2e  floor_error %.2e" % (what, e, f))
    assert e <= BOUND, (what, e)
    assert f <= FLOOR, (what, "floor", f)
    assert db_close(g, ref, 0.01, pink=pink), what
    return e, f


def _ms1_streams():
    """stream 0: full-scale sine on bin 256 in mid, the same bin 120 dB under it in side.  Stream 1: mid -26 dB on bin 300, side
    exactly zero up to ONSET (window 0: a row of zeros), then 20 dB over mid on bin 257."""
    F = 7168
    s0 = _stereo(_sine(F, 256, 4096, 1.0, 0.3), _sine(F, 256, 4096, 1e-6, 1.1) + _noise(1, F, 1e-8))
    side = _sine(F, 257, 4096, 0.5, 0.7) + _noise(2, F, 1e-4)
    side[:ONSET] = 0.0
    s1 = _stereo(_sine(F, 300, 4096, 0.05, 0.1) + _noise(3, F, 1e-5), side)
    return [s0, s1]


def _window(x, n, hop, w):
    p0 = (n // hop + 1) * hop - n + w * hop
    return x[p0:p0 + n]


def test_ms1_against_f64():
    xs = _ms1_streams()
    b = ssa.Batch(48000, 2, 2, 7168, 4096, 1024, flags=L.SS_BATCH_FFT)
    try:
        assert _kernel(b) == "k_fft4096_ms1" and b.layout.n_windows == 3
        b.upload(0, np.concatenate([x.reshape(-1) for x in xs]))
        b.run(); b.sync()
        for i, x in enumerate(xs):
            got = b.fft(i)
            for w in range(3):
                seg = _window(x, 4096, 1024, w)
                for c, row in enumerate(R.mid_side_f32(seg)):
                    _check(got[w, c], row, 48000, 4096, ("ms1", i, w, c), zero=(i == 1 and c == 1 and w == 0))
    finally:
        b.close()


@pytest.mark.parametrize("cols", [64, 512])
def test_ms1_columns_equal_the_two_pass_reduction(cols):
    xs = np.concatenate([x.reshape(-1) for x in _ms1_streams()])
    two = ssa.Batch(48000, 2, 2, 7168, 4096, 1024, flags=L.SS_BATCH_ALL)
    one = ssa.Batch(48000, 2, 2, 7168, 4096, 1024, flags=L.SS_BATCH_ALL, spectrum_columns=cols)
    try:
        assert _kernel(two) == _kernel(one) == "k_fft4096_ms1" and one.layout.n_windows == 3
        two.upload(0, xs); two.run(); two.render_spectrum(cols, 6.0)
        one.upload(0, xs); one.set_columns_gain(6.0); one.run(); one.sync()
        for s in range(2):
            a, c = one.spectrum_columns(s), two.spectrum_columns(s)
            assert a.shape == c.shape == (3, 2, cols)
            assert np.array_equal(a, c, equal_nan=True), (cols, s, int(np.sum(~((a == c) | (np.isnan(a) & np.isnan(c))))))
            assert np.isfinite(a).any()
    finally:
        one.close(); two.close()


def test_pairw_against_f64():
    """stream 0: a full-scale bin-centred sine, the same bin in both windows of a pair (window 2 alone on its transform).
    Stream 1: exact zeros up to ONSET — window 0 is a row of zeros under window 1's onset."""
    F = 7168
    a = _sine(F, 256, 4096, 1.0, 0.3)
    z = _sine(F, 1703, 4096, 0.3, 0.9) + _noise(5, F, 1e-4)      # (bin 1703: in the row's last group of four)
    z[:ONSET] = 0.0
    xs = [a.astype(np.float32), z.astype(np.float32)]
    b = ssa.Batch(48000, 1, 2, F, 4096, 1024, flags=L.SS_BATCH_FFT)
    try:
        assert _kernel(b) == "k_fft4096_pairw" and b.layout.n_windows == 3
        b.upload(0, np.concatenate(xs))
        b.run(); b.sync()
        for i, x in enumerate(xs):
            got = b.fft(i)
            for w in range(3):
                _check(got[w, 0], _window(x, 4096, 1024, w), 48000, 4096, ("pairw", i, w), zero=(i == 1 and w == 0))
    finally:
        b.close()


ONSET16K = 9000                  # N = 16384: inside every window of either shape, 7976 frames into window 0, 808 into window 7


def _stereo16k(frames):
    """mid: nothing up to ONSET16K, then a full-scale sine on bin 1000 of N = 16384 and, 60 dB under it, one on bin 3413, the last
    retained bin at 96 kHz; side: exact zeros (l == r), a row of zeros in every window"""
    mid = _sine(frames, 1000, 16384, 1.0, 0.2) + _sine(frames, 3413, 16384, 1e-3, 0.5) + _noise(7, frames, 1e-5)
    mid[:ONSET16K] = 0.0
    return _stereo(mid, np.zeros(frames))


@pytest.mark.parametrize("kernel,frames,nw", [("k_fft16k_run", 24576, 8), ("k_fft16k", 17408, 1)])
def test_fft16k_against_f64(kernel, frames, nw):
    x = _stereo16k(frames)
    b = ssa.Batch(96000, 2, 1, frames, 16384, 1024, flags=L.SS_BATCH_FFT)
    try:
        assert _kernel(b) == kernel and b.layout.n_windows == nw
        b.upload(0, x.reshape(-1))
        b.run(); b.sync()
        got = b.fft(0)
        for w in range(nw):
            for c, row in enumerate(R.mid_side_f32(_window(x, 16384, 1024, w))):
                _check(got[w, c], row, 96000, 16384, (kernel, w, c), zero=(c == 1))
    finally:
        b.close()
