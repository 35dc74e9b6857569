"""Batch spectrogram (ss_batch_spectrogram): every stream's time x frequency chart tiles against numpy on the rows Batch.fft(stream)
returned from the same pass, cut to the stream's own window count:  cell (r, t, c) = nanmax of f32 clip(v + gain, -100, 0) over
the windows w with floor((w - w_min) * t_cols / (w_max - w_min)) == t and the bins with floor(chart_x / 100 * f_cols) == c (the
last column closed), chart_x from Batch.bin_tables().  A maximum is exact in any order, so every comparison is equality of values
with equal NaN positions — there is no tolerance anywhere in this file.

Where a pass has rows and none of them is refused, each cell is also held against the maximum over its windows of
render_spectrum(f_cols, gain)'s columns.  (A refused window is the one case where the two differ by definition: render_spectrum
draws its NaN values at the chart's floor, the spectrogram skips them.)"""
import ctypes as C

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_multich, make_stereo
from oracle.render import chart_column_of

pytestmark = pytest.mark.gpu

RATE, N, HOP = 48000, 4096, 1024
FFT, LUFS = L.SS_BATCH_FFT, L.SS_BATCH_LUFS
NAN = np.float32(np.nan)


def frames_for(windows, fft_n=N, hop=HOP):
    """the shortest stream that holds `windows` windows: they end at (fft_n / hop + 1) * hop ... (frames // hop) * hop"""
    return (fft_n // hop + windows) * hop


def windows_holding(frame, n_windows, fft_n=N, hop=HOP):
    """window w covers the frames [first + w * hop, first + w * hop + fft_n), first = (fft_n / hop + 1) * hop - fft_n"""
    first = (fft_n // hop + 1) * hop - fft_n
    return [w for w in range(n_windows) if first + w * hop <= frame < first + w * hop + fft_n]


def fmax_over(a, axis):
    """nanmax without its warnings: NaN where nothing (or only NaN) is reduced"""
    if a.shape[axis] == 0:
        shape = list(a.shape)
        del shape[axis]
        return np.full(shape, NAN, np.float32)
    return np.fmax.reduce(a, axis=axis)


def time_fold(per_window, t_cols, w_min, w_max):
    """[windows][R][f_cols] -> [R][t_cols][f_cols]: the maximum over every time column's windows (the floor rule, Python integers)"""
    nw, span = per_window.shape[0], w_max - w_min
    owner = np.array([(w - w_min) * t_cols // span if w_min <= w < w_max else -1 for w in range(nw)], dtype=np.int64)
    return np.stack([fmax_over(per_window[owner == t], 0) for t in range(t_cols)], axis=1)


def reference(rows, chart_x, t_cols, f_cols, w_min, w_max, gain):
    """the yardstick, in numpy: rows[window][R][bin] f32 of one stream (its own windows only) -> [R][t_cols][f_cols] f32"""
    col = chart_column_of(chart_x, f_cols)
    assert (np.diff(col) >= 0).all()
    with np.errstate(invalid="ignore"):                          # (inf - inf, NaN: they stay NaN, which is what is wanted)
        y = np.clip(rows + np.float32(gain), np.float32(-100), np.float32(0))
    assert y.dtype == np.float32
    start = np.searchsorted(col, np.arange(f_cols + 1))
    chart = np.stack([fmax_over(y[:, :, start[c]:start[c + 1]], 2) for c in range(f_cols)], axis=2)
    return time_fold(chart, t_cols, w_min, w_max)


def own_rows(b, stream):
    return b.fft(stream)[:b.stream_shape(stream).n_windows]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a, b, equal_nan=True)


def where_differs(a, b):
    return np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:6].tolist()


def check_view(b, rows, t_cols, f_cols, w_min=0, w_max=None, gain_db=0.0, gains=None, render=False, tag=""):
    """One view of batch b against numpy on rows[stream]; gains: per-stream f32 gains (the reference rule) instead of gain_db.
    Returns the pictures [stream][R][t_cols][f_cols]."""
    hi = int(b.layout.n_windows) if w_max is None else w_max
    chart_x = b.bin_tables()[0]
    b.spectrogram(t_cols, f_cols, w_min, w_max, None if gains is not None else gain_db)
    got = b.spectrograms()
    assert got.shape == (len(rows), int(b.layout.fft_channels), t_cols, f_cols)
    if render:
        b.render_spectrum(f_cols, None if gains is not None else gain_db)
    for s, r in enumerate(rows):
        g = gains[s] if gains is not None else gain_db
        ref = reference(r, chart_x, t_cols, f_cols, w_min, hi, g)
        assert same(got[s], ref), (tag, s, t_cols, f_cols, w_min, hi, where_differs(got[s], ref))
        assert same(b.spectrogram_of(s), got[s])
        if render:
            assert not np.isnan(r).any()
            via_render = time_fold(b.spectrum_columns(s)[:r.shape[0]], t_cols, w_min, hi)
            assert same(got[s], via_render), (tag, s, "render", where_differs(got[s], via_render))
    return got


# ---------------------------------------------------------------- 1: ms1 rows, n_bins = 1705 in rows of 1708 floats
@pytest.fixture(scope="module")
def ms1():
    """three streams of 37 windows with the meter: digital silence; a loud one whose 3 kHz tone stands above 0 dB in the mid row
    (0.9 of full scale, and +4.8 dB of pink compensation); an ordinary one"""
    frames = frames_for(37)
    tone = (0.9 * np.sin(2 * np.pi * 3000.0 * np.arange(frames) / RATE)).astype(np.float32)
    loud = make_stereo(13, frames, RATE, level=0.4)
    loud[0::2] += tone
    loud[1::2] += tone
    b = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT | LUFS)
    b.upload(0, np.concatenate([np.zeros(2 * frames, np.float32), loud, make_stereo(14, frames, RATE, level=1.0)]))
    b.run()
    lay = b.layout
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft4096_ms1"
    assert (lay.n_windows, lay.fft_channels, lay.n_bins, lay.fft_bin_stride) == (37, 2, 1705, 1708)      # three padding floats per row
    rows = [own_rows(b, s) for s in range(3)]
    assert not any(np.isnan(r).any() for r in rows) and rows[1][:, 0].max() > 0.0
    yield b, rows
    b.close()


@pytest.mark.parametrize("f_cols", [1, 160, 512])
@pytest.mark.parametrize("t_cols", [1, 5, 37, 64])
def test_whole_view_of_ms1_rows(ms1, t_cols, f_cols):
    b, rows = ms1
    got = check_view(b, rows, t_cols, f_cols, render=True, tag="ms1")
    empty_bins = np.isnan(got[2][0, 0])                         # chart columns that own no bin: the low end of a fine chart
    assert (empty_bins.any() or f_cols != 512) and not empty_bins[-1]
    if t_cols == 64:                                            # more time columns than windows: 27 of them own none
        assert int(np.isnan(got[2][0, :, -1]).sum()) == 64 - 37
    else:
        assert not np.isnan(got[2][:, :, ~empty_bins]).any()
    # digital silence: every cell is the chart's floor, or NaN where numpy has none
    assert np.array_equal(got[0][~np.isnan(got[0])], np.full(int((~np.isnan(got[0])).sum()), -100, np.float32))


@pytest.mark.parametrize("w_min,w_max", [(3, 29), (30, 50)])
def test_views_inside_and_beyond_the_stream(ms1, w_min, w_max):
    b, rows = ms1
    got = check_view(b, rows, 5, 160, w_min, w_max, render=True, tag="part")
    if w_max == 50:                                             # windows 30 ... 36 exist: columns 0 (30 ... 33) and 1 (34 ... 37); the rest is empty
        assert not np.isnan(got[2][:, :2, -1]).any() and np.isnan(got[2][:, 2:]).all()
    check_view(b, rows, 4, 16, 36, 2 ** 32 - 1, tag="far")      # one window in column 0 of a view as wide as a view can be


def test_gains_and_both_clamps(ms1):
    b, rows = ms1
    up = check_view(b, rows, 5, 160, gain_db=6.0, render=True, tag="+6 dB")
    down = check_view(b, rows, 5, 160, gain_db=-40.0, render=True, tag="-40 dB")
    assert (up[1] == 0.0).any() and (down[1] == -100.0).any() and (down[2] == -100.0).any() and np.nanmax(down[1]) < 0.0
    # the reference's rule: -13 - (float)integrated per stream
    with np.errstate(all="ignore"):
        gains = [np.float32(-13.0) - np.float32(r.integrated_lufs) for r in b.results()]
    assert np.isfinite(gains[1]) and np.isfinite(gains[2]) and gains[1] != gains[2]
    ref_gain = check_view(b, rows, 5, 160, gains=gains, render=True, tag="reference gain")
    assert not same(ref_gain[2], check_view(b, rows, 5, 160, gain_db=0.0)[2])


def test_reference_gain_needs_the_meter_and_views_are_checked(ms1):
    lib = L.lib()
    b, _ = ms1
    fp = C.POINTER(C.c_float)
    frames = frames_for(6)
    plain = ssa.Batch(RATE, 2, 2, frames, N, HOP, flags=FFT)
    buf = np.empty(2 * 2 * 3 * 8 + 1, np.float32)
    ok = L.SpectrogramView(3, 8, 0, 6, L.SS_GAIN_FIXED, 0.0)
    assert lib.ss_batch_download_spectrogram(plain._h, 0, 2, buf.ctypes.data_as(fp), buf.size) == L.SS_ERR_INVALID_MODE       # before the first call
    assert lib.ss_batch_spectrogram(plain._h, C.byref(L.SpectrogramView(3, 8, 0, 6, L.SS_GAIN_REFERENCE, 0.0))) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_spectrogram(plain._h, 0, 2, buf.ctypes.data_as(fp), buf.size) == L.SS_ERR_INVALID_MODE       # a refused call queues nothing
    for bad in ((0, 8, 0, 6, 0), (4097, 8, 0, 6, 0), (3, 0, 0, 6, 0), (3, 513, 0, 6, 0), (3, 8, 6, 6, 0), (3, 8, 7, 6, 0), (3, 8, 0, 6, 2), (3, 8, 0, 6, -1)):
        v = L.SpectrogramView(*bad, 0.0)
        assert lib.ss_batch_spectrogram(plain._h, C.byref(v)) == L.SS_ERR_INVALID_ARG, bad
        assert lib.ss_batch_spectrogram_plan(plain._h, C.byref(v), None, None) == L.SS_ERR_INVALID_ARG, bad
    assert lib.ss_batch_spectrogram(None, C.byref(ok)) == L.SS_ERR_INVALID_ARG == lib.ss_batch_spectrogram(plain._h, None)
    assert lib.ss_batch_spectrogram_plan(None, C.byref(ok), None, None) == L.SS_ERR_INVALID_ARG
    no_fft = ssa.Batch(RATE, 2, 2, frames, N, HOP, flags=LUFS)
    assert lib.ss_batch_spectrogram(no_fft._h, C.byref(ok)) == L.SS_ERR_INVALID_MODE == lib.ss_batch_spectrogram_plan(no_fft._h, C.byref(ok), None, None)
    assert lib.ss_batch_download_spectrogram(no_fft._h, 0, 1, buf.ctypes.data_as(fp), buf.size) == L.SS_ERR_INVALID_MODE
    no_fft.close()
    # the largest views are views like any other
    assert lib.ss_batch_spectrogram_plan(plain._h, C.byref(L.SpectrogramView(4096, 512, 0, 6, 0, 0.0)), None, None) == L.SS_OK
    plain.upload(0, np.concatenate([make_stereo(71 + s, frames, RATE) for s in range(2)]))
    plain.run()
    plain.spectrogram(3, 8, 0, 6, gain_db=0.0)
    assert lib.ss_batch_download_spectrogram(plain._h, 0, 2, buf.ctypes.data_as(fp), buf.size - 2) == L.SS_ERR_CAPACITY     # one float short
    assert lib.ss_batch_download_spectrogram(plain._h, 1, 2, buf.ctypes.data_as(fp), buf.size) == L.SS_ERR_INVALID_ARG      # first + count > n_streams
    assert lib.ss_batch_download_spectrogram(plain._h, 0, 2, None, buf.size) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_spectrogram(plain._h, 2, 0, None, 0) == L.SS_OK                                            # nothing to copy: it waits
    buf[-1] = 7.0
    assert lib.ss_batch_download_spectrogram(plain._h, 0, 2, buf.ctypes.data_as(fp), buf.size - 1) == L.SS_OK and buf[-1] == 7.0
    # spectrograms() is the per-stream downloads stacked, and any part of them
    all_of_them = plain.spectrograms()
    assert same(all_of_them, buf[:-1].reshape(2, 2, 3, 8)) and same(all_of_them, np.stack([plain.spectrogram_of(s) for s in range(2)]))
    assert same(plain.spectrograms(1), all_of_them[1:]) and plain.spectrograms(0, 0).shape == (0, 2, 3, 8)
    plain.close()


# ---------------------------------------------------------------- 2: a refused window
@pytest.mark.parametrize("kind", [np.nan, np.inf])
def test_refused_window_drops_out_of_its_own_cells_only(kind):
    nw = 37
    frames = frames_for(nw)
    bad_at = 20000
    refused = windows_holding(bad_at, nw)
    assert len(refused) == N // HOP
    x = [make_stereo(41 + s, frames, RATE, level=1.0) for s in range(3)]
    clean = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT)
    clean.upload(0, np.concatenate(x))
    clean.run()
    x[1][2 * bad_at] = np.float32(kind)                         # L only: mid and side both hold it
    b = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT)
    b.upload(0, np.concatenate(x))
    b.run()
    rows = [own_rows(b, s) for s in range(3)]
    for w in range(nw):
        assert np.isfinite(rows[1][w]).all() == (w not in refused), w
    for t_cols in (37, 5, 1):
        got = check_view(b, rows, t_cols, 160, tag=f"refused {kind}")
        untouched = check_view(clean, [own_rows(clean, s) for s in range(3)], t_cols, 160, tag="clean")
        assert same(got[0], untouched[0]) and same(got[2], untouched[2]) and not np.isnan(untouched[..., -1]).any()
        if t_cols == 37 and np.isnan(rows[1][refused]).all():   # a column per window: the refused ones read NaN in mid and side alike
            assert np.isnan(got[1][:, refused]).all()
            kept = [w for w in range(nw) if w not in refused]
            assert same(got[1][:, kept], untouched[1][:, kept])
        if t_cols == 5:                                         # column 2 (15 ... 22) holds them beside others: it has values
            assert not np.isnan(got[1][..., -1]).any()
    b.close()
    clean.close()


# ---------------------------------------------------------------- 3: ragged batches, with loud stale rows behind every stream's own count
def test_ragged_batch_never_reads_the_stale_rows():
    slot_windows = 37
    frames = frames_for(slot_windows)
    loud = np.concatenate([make_stereo(51 + s, frames, RATE, level=3.0) for s in range(3)])
    b = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT)
    b.upload(0, loud)
    b.run()
    b.sync()
    pass_one = [b.fft(s).copy() for s in range(3)]
    b.set_lengths([frames, frames_for(5), N])
    b.upload(0, loud * np.float32(1e-3))                        # the same material 60 dB down
    b.run()
    counts = [int(b.stream_shape(s).n_windows) for s in range(3)]
    assert counts == [37, 5, 0]
    slot = np.empty((37, 2, 1705), np.float32)                  # the plant: the slot behind stream 1's own count still holds pass one's rows
    assert L.lib().ss_batch_download_fft(b._h, 1, slot.ctypes.data_as(C.POINTER(C.c_float)), slot.size) == L.SS_OK
    assert np.array_equal(slot[-1], pass_one[1][-1]) and np.median(slot[-1, 0]) - np.median(slot[:5, 0]) > 40
    rows = [own_rows(b, s) for s in range(3)]
    assert [r.shape[0] for r in rows] == counts
    for t_cols in (37, 5, 1):
        got = check_view(b, rows, t_cols, 160, 0, 37, tag="ragged")
        assert np.isnan(got[2]).all()
        if t_cols == 37:
            assert not np.isnan(got[1][:, :5, -1]).any() and np.isnan(got[1][:, 5:]).all()
        assert np.nanmax(got[1]) < pass_one[1][:5].max() - 55     # a stale row would put this at pass one's level
    b.close()


# ---------------------------------------------------------------- 4: other row shapes
def test_three_channels_one_row_per_channel():
    frames = frames_for(9)
    b = ssa.Batch(RATE, 3, 2, frames, N, HOP, flags=FFT)
    assert b.layout.fft_channels == 3
    b.upload(0, np.concatenate([make_multich(31 + s, frames, 3, RATE, level=0.8).ravel() for s in range(2)]))
    b.run()
    rows = [own_rows(b, s) for s in range(2)]
    for t_cols, f_cols in ((4, 160), (9, 33)):
        check_view(b, rows, t_cols, f_cols, render=True, tag="3ch")
    b.close()


@pytest.mark.parametrize("fft_n,hop,windows,f_cols", [(1024, 256, 21, 100), (16384, 1024, 6, 160), (32768, 1024, 3, 64)])
def test_other_transform_lengths(fft_n, hop, windows, f_cols):
    """N = 32768 at 48 kHz: 13 640 bins a row — the fold goes through the chart's column slots, so LDS does not grow with them"""
    frames = frames_for(windows, fft_n, hop)
    b = ssa.Batch(RATE, 2, 1, frames, fft_n, hop, flags=FFT)
    assert b.layout.n_windows == windows and (fft_n != 32768 or b.layout.n_bins > 13000)
    b.upload(0, make_stereo(61, frames, RATE, level=1.0))
    b.run()
    rows = [own_rows(b, 0)]
    for t_cols in (1, 2, windows):
        check_view(b, rows, t_cols, f_cols, gain_db=3.0, render=fft_n == 1024, tag=f"N = {fft_n}")
    b.close()


# ---------------------------------------------------------------- 5: both plans
def test_one_long_stream_is_cut_into_runs():
    frames = frames_for(1400)                                   # 30 s
    b = ssa.Batch(RATE, 2, 1, frames, N, HOP, flags=FFT)
    b.upload(0, make_stereo(21, frames, RATE, level=1.0, gap=True))
    b.run()
    rows = [own_rows(b, 0)]
    for t_cols in (1, 7):
        runs, run_windows = b.spectrogram_plan(t_cols, 160, gain_db=0.0)
        assert runs > 1 and run_windows >= 16 and (runs - 1) * run_windows < -(-1400 // t_cols) <= runs * run_windows, (runs, run_windows)
        first = check_view(b, rows, t_cols, 160, tag="runs")
        b.spectrogram(t_cols, 160, gain_db=0.0)
        assert first.tobytes() == b.spectrograms().tobytes()    # the same rows reduced twice: the same bytes
    got = check_view(b, rows, 3, 160, 700, 2 ** 32 - 1, tag="runs, far")      # a view whose columns reach far beyond the stream
    assert not np.isnan(got[0][:, 0, -1]).any() and np.isnan(got[0][:, 1:]).all()
    b.close()


def test_many_short_streams_are_one_launch():
    n, frames = 64, frames_for(12)
    b = ssa.Batch(RATE, 2, n, frames, N, HOP, flags=FFT)
    b.upload(0, np.concatenate([make_stereo(100 + s, frames, RATE, level=0.2 + 0.05 * s) for s in range(n)]))
    b.run()
    rows = [own_rows(b, s) for s in range(n)]
    assert b.spectrogram_plan(5, 160, gain_db=0.0) == (1, 3) and b.spectrogram_plan(12, 64, gain_db=0.0) == (1, 1)
    first = check_view(b, rows, 5, 160, tag="64 streams")
    b.spectrogram(5, 160, gain_db=0.0)
    assert first.tobytes() == b.spectrograms().tobytes()
    check_view(b, rows, 12, 64, tag="64 streams")
    b.close()


# ---------------------------------------------------------------- 6: columns-only batches
@pytest.mark.parametrize("gain_db", [-3.0, None])
def test_columns_only_batch_equals_full_rows(gain_db):
    lib = L.lib()
    frames = frames_for(37)
    x = np.concatenate([make_stereo(81 + s, frames, RATE, level=0.5 + s) for s in range(3)])
    full = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT | LUFS)
    cols = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT | LUFS, spectrum_columns=160)
    cols.set_columns_gain(gain_db)
    for b in (full, cols):
        b.upload(0, x)
        b.run()
    for t_cols, w_min, w_max in ((1, 0, None), (5, 0, None), (64, 0, None), (4, 3, 29), (5, 30, 50)):
        full.spectrogram(t_cols, 160, w_min, w_max, gain_db)
        cols.spectrogram(t_cols, 160, w_min, w_max, 123.0)      # (the view's gain is not read)
        a, c = full.spectrograms(), cols.spectrograms()
        assert same(a, c), (t_cols, w_min, w_max, where_differs(a, c))
        assert np.isnan(a[..., -1]).any() == (t_cols == 64 or w_max == 50)
        stored = time_fold(cols.spectrum_columns(1), t_cols, w_min, 37 if w_max is None else w_max)
        assert same(c[1], stored)
    for f_cols in (159, 161, 1, 512):
        assert lib.ss_batch_spectrogram(cols._h, C.byref(L.SpectrogramView(5, f_cols, 0, 37, 0, 0.0))) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_spectrogram(cols._h, C.byref(L.SpectrogramView(5, 160, 0, 37, 99, 0.0))) == L.SS_OK     # nor is its gain mode
    full.close()
    cols.close()


# ---------------------------------------------------------------- 7: nothing of the pass is written
def test_nothing_else_moved():
    frames = frames_for(9)
    x = np.concatenate([make_stereo(91 + s, frames, RATE) for s in range(2)])
    b = ssa.Batch(RATE, 2, 2, frames, N, HOP)                   # every output of a pass: rows, decimation bins, sub-block energies
    b.upload(0, x)
    b.run()
    checks, results = b.checksums(), bytes(b.results())
    assert checks[:, 0].all()
    b.render_spectrum(160, -3.0)
    rendered = [b.spectrum_columns(s).copy() for s in range(2)]
    for view in ((1, 160), (9, 512), (4, 7)):
        b.spectrogram(*view, gain_db=-3.0)
        b.spectrograms()
    assert all(np.array_equal(b.spectrum_columns(s), rendered[s], equal_nan=True) for s in range(2))     # render_spectrum's own buffer
    assert np.array_equal(b.checksums(), checks) and bytes(b.results()) == results
    b.run()
    b.spectrogram(3, 160)                                       # (the reference's gain: it reads the meter's results)
    b.render_spectrum(160, -3.0)
    assert all(b.spectrum_columns(s).tobytes() == rendered[s].tobytes() for s in range(2))
    assert np.array_equal(b.checksums(), checks) and bytes(b.results()) == results
    b.close()


def test_no_window_at_all_is_valid():
    empty = ssa.Batch(RATE, 2, 2, N, N, HOP, flags=FFT)
    assert empty.layout.n_windows == 0
    empty.upload(0, np.concatenate([make_stereo(95 + s, N, RATE) for s in range(2)]))
    empty.run()
    empty.spectrogram(3, 16, 0, 5, gain_db=0.0)
    got = empty.spectrograms()
    assert got.shape == (2, 2, 3, 16) and np.isnan(got).all()
    assert empty.spectrogram_plan(3, 16, 0, 5, gain_db=0.0) == (1, 1)
    empty.close()


def test_windows_between_is_the_window_geometry():
    b = ssa.Batch(RATE, 2, 1, frames_for(37), N, HOP, flags=FFT)
    inside = lambda f0, f1: [w for w in range(37) if (w + 1) * HOP >= f0 and (w + 1) * HOP + N <= f1]
    for f0, f1 in ((0, frames_for(37)), (HOP, HOP + N), (HOP + 1, 3 * HOP + N), (7000, 20000), (7000, 7000 + N - 1), (0, 100), (30000, 10 ** 7)):
        ws = inside(f0, f1)
        lo, hi = b.windows_between(f0 / RATE, f1 / RATE)
        assert (list(range(lo, hi)) == ws) and (ws or lo == hi), (f0, f1, lo, hi, ws)
        for w in ws:                                            # ... as windows_holding states it
            assert w in windows_holding((w + 1) * HOP, 37) and w in windows_holding((w + 1) * HOP + N - 1, 37)
    b.close()
