"""Chart columns, one map for three paths ("Chart columns"): for the same material, column count and gain
  A  render_spectrum(cols, gain) on a full-row batch                      (k_render_spectrum, the column starts),
  B  the columns of a columns-only batch                                   (the spectrum kernel's fused fold, the column tables),
  C  spectrogram(t_cols = windows, cols, 0, windows, gain) of the rows     (k_spectrogram_rows, one window per time column)
are the same f32 values with NaN (a column that owns no bin) at the same places.  A and C clamp differently where a row value is
NaN; the rows here hold none, which the test asserts first."""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_stereo

pytestmark = pytest.mark.gpu

RATE, N, HOP, STREAMS, WINDOWS = 48000, 4096, 1024, 2, 6
FRAMES = N + WINDOWS * HOP + 17


@pytest.fixture(scope="module")
def material():
    return np.concatenate([make_stereo(500 + s, FRAMES, rate=RATE, level=0.2 + 0.1 * s) for s in range(STREAMS)])


@pytest.fixture(scope="module")
def full_rows(material):
    b = ssa.Batch(RATE, 2, STREAMS, FRAMES, N, HOP, flags=L.SS_BATCH_ALL)
    b.upload(0, material)
    b.run()
    assert b.layout.n_windows == WINDOWS and b.layout.fft_channels == 2
    for s in range(STREAMS):
        assert not np.isnan(b.fft(s)).any()                      # the condition under which A and C agree
    yield b
    b.close()


@pytest.mark.parametrize("cols", [1, 7, 512])
def test_three_paths_one_map(material, full_rows, cols):
    one = ssa.Batch(RATE, 2, STREAMS, FRAMES, N, HOP, flags=L.SS_BATCH_ALL, spectrum_columns=cols)
    one.upload(0, material)
    for gain in (7.5, None):                                     # fixed, and the reference's -13 - integrated
        full_rows.render_spectrum(cols, gain)
        full_rows.spectrogram(WINDOWS, cols, 0, WINDOWS, gain)
        pictures = full_rows.spectrograms()                      # [stream][row][window][cols]
        one.set_columns_gain(gain)
        one.run(); one.sync()
        for s in range(STREAMS):
            a, b, c = full_rows.spectrum_columns(s), one.spectrum_columns(s), pictures[s].transpose(1, 0, 2)
            assert a.shape == b.shape == c.shape == (WINDOWS, 2, cols) and a.dtype == b.dtype == c.dtype == np.float32
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(a), np.isnan(c)), (cols, gain, s)
            assert np.array_equal(a, b, equal_nan=True), (cols, gain, s)
            assert np.array_equal(a, c, equal_nan=True), (cols, gain, s)
            empty = np.isnan(a[0, 0])
            assert np.array_equal(np.isnan(a), np.broadcast_to(empty, a.shape))      # the map is the row's, whatever the window
            assert empty.any() == (cols == 512) and not empty.all()                  # 512 columns at this rate: some own no bin
    one.close()
