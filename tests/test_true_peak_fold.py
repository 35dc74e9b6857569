"""The folded factor-4 interpolator table the VALU true-peak forms run on (ss_inspect_true_peak_fold), against the crate's taps.

Branch 3 of the 49-tap interpolator is branch 1 reversed and branch 2 is its own reverse, so the kernels evaluate
s = (y1 + y3) / 2 and d = (y1 - y3) / 2 on sums and differences of mirrored samples and take max(|y1|, |y3|) = |s| + |d|.  No GPU
needed."""
import ctypes as C

import numpy as np

from soundscope_amd import _lib as L
import _f64ref as R

f32p = C.POINTER(C.c_float)


def _fold():
    f = np.zeros(18, np.float32)
    assert L.lib().ss_inspect_true_peak_fold(f.ctypes.data_as(f32p)) == 0
    return f.reshape(3, 6)


def _branches():
    h = R.interpolator_taps(4)
    return h[1::4], h[2::4], h[3::4]            # coefficient of x[n - k], k = 0 .. 11


def test_the_taps_mirror_exactly():
    a, b, c = _branches()
    assert np.array_equal(c, a[::-1])
    assert np.array_equal(b, b[::-1])
    h = R.interpolator_taps(4)
    assert np.count_nonzero(h[0::4]) == 1 and h[24] == 1.0     # branch 0: the sample itself


def test_folded_table_reproduces_the_branches():
    a, b, c = _branches()
    f = _fold()
    k = np.arange(6)
    # one f32 rounding of the sum or difference, then an exact halving
    assert np.array_equal(f[0], (np.float32(0.5) * (a[k].astype(np.float32) + c[k].astype(np.float32))))
    assert np.array_equal(f[1], (np.float32(0.5) * (a[k].astype(np.float32) - c[k].astype(np.float32))))
    assert np.array_equal(f[2].astype(np.float64), b[:6])
    # what the two folded halves rebuild of branches 1 and 3 (k < 6; the mirror gives k >= 6): within the two roundings
    f64 = f.astype(np.float64)
    sp = lambda t: np.spacing(np.abs(t).astype(np.float32)).astype(np.float64)
    bound = (sp(a[:6] + c[:6]) + sp(a[:6] - c[:6])) / 4
    assert np.all(np.abs(f64[0] + f64[1] - a[:6]) <= bound)
    assert np.all(np.abs(f64[0] - f64[1] - c[:6]) <= bound)
    assert L.lib().ss_inspect_true_peak_fold(None) == 0


def test_folded_form_replays_the_branches():
    """The folded evaluation in f64 with the product's f32 table against the three branches: the table's rounding is all it adds."""
    a, b, c = _branches()
    f = _fold().astype(np.float64)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(5000 + 11)
    win = np.lib.stride_tricks.sliding_window_view(x, 12)[:, ::-1]      # win[n, k] = x[n + 11 - k]
    y1, y2, y3 = win @ a, win @ b, win @ c
    u = win[:, :6] + win[:, 11:5:-1]
    v = win[:, :6] - win[:, 11:5:-1]
    s, d, y2f = u @ f[0], v @ f[1], u @ f[2]
    assert np.abs(y2f - y2).max() < 1e-14
    assert np.abs((np.abs(s) + np.abs(d)) - np.maximum(np.abs(y1), np.abs(y3))).max() < 1e-7
