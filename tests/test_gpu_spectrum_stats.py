"""Batch spectrum statistics (ss_batch_spectrum_stats): every stream's long-term average (power mean) and peak-hold spectrum, and
the batch pooled, against numpy in f64 over the rows Batch.fft(stream) returned from the same pass, limited to the stream's own
window count:  max_db = nanmax, mean_db = 10 log10(nanmean(10^(v / 10))), windows_counted = the non-NaN values at bin 0.

max_db, the counts and the NaN positions are exact.  mean_db is within 1e-4 dB at EVERY bin, however quiet — the sum has only
positive terms, so nothing cancels and no level threshold is needed.  The bound is derived, not measured: the f32 exponent argument
rounds to at most 6e-6 dB at |v| <= 170, exp2f at 1-2 ulp is 1e-6 dB, the f32 result rounds to at most 8e-6 dB — under 2e-5 dB, and
1e-4 leaves a factor of five for the device's exp2f.  Every test prints its worst deviation (pytest -rA)."""
import ctypes as C
import warnings

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_multich, make_stereo

pytestmark = pytest.mark.gpu

TOL_DB = 1e-4
RATE, N, HOP = 48000, 4096, 1024
FFT = L.SS_BATCH_FFT


def frames_for(windows, fft_n=N, hop=HOP):
    """the shortest stream that holds `windows` windows: they end at (fft_n / hop + 1) * hop ... (frames // hop) * hop"""
    return (fft_n // hop + windows) * hop


def windows_holding(frame, n_windows, fft_n=N, hop=HOP):
    """window w covers the frames [(w + 1) * hop, (w + 1) * hop + fft_n)"""
    return [w for w in range(n_windows) if (w + 1) * hop <= frame < (w + 1) * hop + fft_n]


def reference(rows):
    """(mean_db f64, max_db f32, counted) of rows[window][fft_channel][bin] f32: the yardstick, in numpy"""
    R, nb = rows.shape[1], rows.shape[2]
    if rows.shape[0] == 0:
        return np.full((R, nb), np.nan), np.full((R, nb), np.nan, np.float32), np.zeros(R, np.uint64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # (all-NaN slices: the result is NaN, which is what is wanted)
        mean = 10.0 * np.log10(np.nanmean(10.0 ** (rows.astype(np.float64) / 10.0), axis=0))
        mx = np.nanmax(rows, axis=0)
    return mean, mx, (~np.isnan(rows[:, :, 0])).sum(axis=0).astype(np.uint64)


def own_rows(b, stream):
    return b.fft(stream)[:b.stream_shape(stream).n_windows]


def assert_matches(got, ref, tag):
    """got = (mean f32, max f32, counts) of the device, ref = reference(...); returns the worst |mean_db| deviation"""
    (mean, mx, cnt), (rmean, rmx, rcnt) = got, ref
    assert mean.dtype == np.float32 and mx.dtype == np.float32 and mean.shape == rmean.shape == mx.shape, tag
    assert np.array_equal(cnt.astype(np.uint64), rcnt), (tag, cnt, rcnt)
    assert np.array_equal(mx, rmx, equal_nan=True), (tag, np.argwhere(~((mx == rmx) | (np.isnan(mx) & np.isnan(rmx))))[:8])
    assert np.array_equal(np.isnan(mean), np.isnan(rmean)), (tag, np.argwhere(np.isnan(mean) != np.isnan(rmean))[:8])
    inf = np.isinf(rmean)
    assert np.array_equal(mean[inf].astype(np.float64), rmean[inf]), tag
    fin = np.isfinite(rmean)
    worst = float(np.abs(mean[fin].astype(np.float64) - rmean[fin]).max()) if fin.any() else 0.0
    print(f"{tag}: worst |mean_db - numpy| = {worst:.3g} dB over {int(fin.sum())} bins")
    assert worst <= TOL_DB, (tag, worst)
    return worst


def check_stream(b, stream, tag):
    rows = own_rows(b, stream)
    assert_matches(b.spectrum_stats_of(stream), reference(rows), f"{tag} stream {stream}")
    return rows


def check_corpus(b, tag):
    pooled = np.concatenate([own_rows(b, s) for s in range(int(b.cfg.n_streams))], axis=0)
    first, again = b.corpus_spectrum(), b.corpus_spectrum()
    assert_matches(first, reference(pooled), tag + " pooled")
    per_stream = sum(b.spectrum_stats_of(s)[2].astype(np.uint64) for s in range(int(b.cfg.n_streams)))
    assert np.array_equal(first[2], per_stream), (tag, first[2], per_stream)
    for a, c in zip(first, again):
        assert a.tobytes() == c.tobytes(), tag              # two calls: bit-identical, mean_db included


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------- 1: ms1 rows, n_bins = 1705 in rows of 1708 floats
@pytest.fixture(scope="module")
def ms1_batch():
    frames = frames_for(7)
    assert frames == 11264
    rng = np.random.default_rng(11)
    quiet = make_stereo(12, frames, RATE, level=0.9) * np.float32(1e-3)                     # 60 dB down ...
    quiet[2 * 1100:2 * 1900] = rng.uniform(-1, 1, 1600).astype(np.float32)               # ... with a full-scale burst that only window 0 holds
    assert windows_holding(1100, 7) == [0] == windows_holding(1899, 7)
    b = ssa.Batch(RATE, 2, 3, frames, N, HOP, flags=FFT)
    b.upload(0, np.concatenate([np.zeros(2 * frames, np.float32), make_stereo(13, frames, RATE, level=3.5), quiet]))
    b.run()
    b.spectrum_stats()
    yield b
    b.close()


def test_ms1_rows_with_padded_stride(ms1_batch):
    b = ms1_batch
    lay = b.layout
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft4096_ms1"
    assert (lay.n_windows, lay.fft_channels, lay.n_bins, lay.fft_bin_stride) == (7, 2, 1705, 1708)      # three padding floats per row
    assert b.spectrum_stats_plan == (1, 7)
    silence, loud, burst = (check_stream(b, s, "ms1") for s in range(3))
    mean, mx, cnt = b.spectrum_stats_of(0)
    # digital silence: every window's row is the -150 dB floor plus the pink compensation, and the mean of equal values is that value
    assert np.array_equal(silence, np.broadcast_to(silence[0], silence.shape)) and np.array_equal(mx, silence[0])
    assert np.abs(mean.astype(np.float64) - mx).max() <= TOL_DB and list(cnt) == [7, 7]
    assert np.abs(silence[0, 0].astype(np.float64) - (-150.0 + b.bin_tables()[2])).max() < 1e-3
    # one loud window among seven: the peak-hold is that window, the power mean 10 log10(7) = 8.45 dB below it
    mean, mx, cnt = b.spectrum_stats_of(2)
    # (but for the few bins where the burst has a null, or the quiet sine stands)
    hold = (mx - mean).astype(np.float64)
    assert (mx == burst[0]).mean() > 0.99 and (hold > 3.0).mean() > 0.99 and 8.3 < np.median(hold) < 8.46, np.median(hold)


def test_corpus_form_ms1(ms1_batch):
    check_corpus(ms1_batch, "ms1")


# ---------------------------------------------------------------- 2: generic kernel, one stream: the windows are cut into chunks
def test_generic_kernel_chunked_windows():
    frames = 8 * RATE
    b = ssa.Batch(RATE, 2, 1, frames, 1024, 256, flags=FFT)
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft_generic"
    nw = int(b.layout.n_windows)
    assert nw == frames // 256 - 4 and b.layout.fft_channels == 2
    chunks, chunk_windows = b.spectrum_stats_plan
    assert chunks > 1 and chunk_windows >= 16 and (chunks - 1) * chunk_windows < nw <= chunks * chunk_windows, (chunks, chunk_windows)
    b.upload(0, make_stereo(21, frames, RATE, level=1.0, gap=True))
    b.run()
    b.spectrum_stats()
    first = b.spectrum_stats_of(0)
    b.spectrum_stats()
    assert same_bits(first, b.spectrum_stats_of(0))                 # the same rows reduced twice: bit-identical, mean_db included
    check_stream(b, 0, "generic chunked")
    b.upload(0, make_stereo(22, frames, RATE, level=0.3))
    b.run()
    b.spectrum_stats()
    other = b.spectrum_stats_of(0)
    assert not np.array_equal(other[0], first[0]) and not np.array_equal(other[1], first[1])
    check_stream(b, 0, "generic chunked, other input")
    b.close()


# ---------------------------------------------------------------- 3: one row per channel, a NaN in one channel only
def test_per_channel_rows_refused_in_one_channel():
    nw, ch = 50, 3
    frames = frames_for(nw)
    bad_at = RATE                                          # 1 s: windows 42 ... 45
    b = ssa.Batch(RATE, ch, 2, frames, N, HOP, flags=FFT)
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft4096_pairw" and b.layout.fft_channels == 3
    x = [make_multich(31 + s, frames, ch, RATE, level=0.8) for s in range(2)]
    x[1][ch * bad_at + 1] = np.float32(np.nan)
    b.upload(0, np.concatenate(x))
    b.run()
    b.spectrum_stats()
    clean, holed = check_stream(b, 0, "per channel"), check_stream(b, 1, "per channel")
    refused = windows_holding(bad_at, nw)
    assert len(refused) == N // HOP
    nan_rows = np.isnan(holed).all(axis=2)                 # [window][channel]
    assert np.array_equal(nan_rows, np.isnan(holed).any(axis=2))
    assert np.flatnonzero(nan_rows[:, 1]).tolist() == refused and not nan_rows[:, [0, 2]].any() and not np.isnan(clean).any()
    assert list(b.spectrum_stats_of(0)[2]) == [nw, nw, nw]
    assert list(b.spectrum_stats_of(1)[2]) == [nw, nw - len(refused), nw]          # the count differs between the channels of one stream
    b.close()


# ---------------------------------------------------------------- 4: stereo refusals
@pytest.mark.parametrize("kind", [np.inf, -np.inf])
def test_stereo_refusals_leave_the_other_streams_alone(kind):
    nw = 12
    frames = frames_for(nw)
    bad_at = 7000
    x = [make_stereo(41 + s, frames, RATE, level=1.0) for s in range(4)]
    x[1][2 * bad_at] = np.float32(kind)                    # L only: mid and side are both infinite there
    x[2][0::2 * 512] = np.float32(np.nan)                  # a NaN in L twice per hop: every window of the stream is refused
    b = ssa.Batch(RATE, 2, 4, frames, N, HOP, flags=FFT)
    b.upload(0, np.concatenate(x))
    b.run()
    b.spectrum_stats()
    rows = [check_stream(b, s, f"stereo {kind}") for s in range(4)]
    refused = windows_holding(bad_at, nw)
    assert len(refused) == 4
    for w in range(nw):
        assert np.isfinite(rows[1][w]).all() == (w not in refused) and np.isfinite(rows[1][w]).any() == (w not in refused), w
    mean, mx, cnt = b.spectrum_stats_of(2)
    assert np.isnan(rows[2]).all() and np.isnan(mean).all() and np.isnan(mx).all() and list(cnt) == [0, 0]
    for s in (0, 3):
        assert np.isfinite(rows[s]).all() and list(b.spectrum_stats_of(s)[2]) == [nw, nw]
    # the refused windows drop out of stream 1 (NaN rows) or count as values (rows of infinities): either way what numpy says of the rows
    assert list(b.spectrum_stats_of(1)[2]) == [int((~np.isnan(rows[1][:, r, 0])).sum()) for r in range(2)]
    b.close()


def test_all_nan_stream_gives_nan_with_count_zero():
    """A stream whose every sample is NaN: every window is refused, so the results are NaN with count 0, and the stream beside it is
    unaffected.  (k_fft4096_ms1 takes a hop's level with fmaxf, which skips NaN: a window of nothing but NaN — or of zeros and NaN —
    has level 0 like digital silence, and used to be stored as the floor row, -166.30 ... -136.99 dB, where the reference refuses
    it.  The floor now goes only over a transform that is not NaN.)"""
    nw = 12
    frames = frames_for(nw)
    b = ssa.Batch(RATE, 2, 2, frames, N, HOP, flags=FFT)
    b.upload(0, np.concatenate([np.full(2 * frames, np.nan, np.float32), make_stereo(45, frames, RATE, level=1.0)]))
    b.run()
    b.spectrum_stats()
    rows = [check_stream(b, s, "all NaN") for s in range(2)]
    mean, mx, cnt = b.spectrum_stats_of(0)
    assert np.isnan(rows[0]).all()
    assert np.isfinite(rows[1]).all() and list(b.spectrum_stats_of(1)[2]) == [nw, nw]
    assert np.isnan(mean).all() and np.isnan(mx).all() and list(cnt) == [0, 0]
    b.close()


# ---------------------------------------------------------------- 5: ragged batches, with loud stale rows behind every stream's own count
@pytest.fixture(scope="module")
def ragged_batch():
    slot_windows = 12
    frames = frames_for(slot_windows)
    loud = np.concatenate([make_stereo(51 + s, frames, RATE, level=3.0) for s in range(4)])      # about -1 dBFS at the peaks
    assert 0.8 < np.abs(loud).max() <= 1.0
    b = ssa.Batch(RATE, 2, 4, frames, N, HOP, flags=FFT)
    b.upload(0, loud)
    b.run()
    b.sync()
    pass_one = [b.fft(s).copy() for s in range(4)]
    b.set_lengths([frames, frames_for(5), N + HOP, N])
    b.upload(0, loud * np.float32(1e-3))                   # the same material 60 dB down
    b.run()
    b.spectrum_stats()
    yield b, pass_one
    b.close()


def test_ragged_batch_never_reads_the_stale_rows(ragged_batch):
    b, pass_one = ragged_batch
    lay = b.layout
    counts = [int(b.stream_shape(s).n_windows) for s in range(4)]
    assert counts == [12, 5, 1, 0] and lay.n_windows == 12
    quiet_level = np.median(b.fft(0)[:, 0])
    for s in range(4):
        # the plant: rows of the slot behind the stream's own count still hold pass one's values, 60 dB above this pass's
        slot = np.empty((lay.n_windows, lay.fft_channels, lay.n_bins), np.float32)
        assert L.lib().ss_batch_download_fft(b._h, s, slot.ctypes.data_as(C.POINTER(C.c_float)), slot.size) == L.SS_OK
        stale = slot[counts[s]:]
        assert s == 0 or (np.array_equal(stale[-1], pass_one[s][-1]) and np.median(stale[-1, 0]) - quiet_level > 40)
        rows = check_stream(b, s, "ragged")
        assert rows.shape[0] == counts[s]
        mean, mx, cnt = b.spectrum_stats_of(s)
        assert list(cnt) == [counts[s]] * 2
        if counts[s]:
            assert np.median(mx[0] - pass_one[s][:counts[s], 0].max(axis=0)) < -55         # a stale row would put this near 0
    mean, mx, cnt = b.spectrum_stats_of(3)
    assert np.isnan(mean).all() and np.isnan(mx).all()


def test_corpus_form_ragged(ragged_batch):
    check_corpus(ragged_batch[0], "ragged")


# ---------------------------------------------------------------- 6: the reference's window, N = 16384 mid/side
def test_fft16k_run_rows():
    frames = 3 * RATE
    b = ssa.Batch(RATE, 2, 1, frames, 16384, HOP, flags=FFT)
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft16k_run" and b.layout.n_windows == frames // HOP - 16
    b.upload(0, make_stereo(61, frames, RATE, level=1.0, gap=False))
    b.run()
    b.spectrum_stats()
    check_stream(b, 0, "fft16k_run")
    b.close()


# ---------------------------------------------------------------- 8: modes, capacities, and nothing of the pass is written
def test_modes_capacity_and_untouched_outputs():
    lib = L.lib()
    fp, up, qp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    frames = frames_for(9)
    x = np.concatenate([make_stereo(81 + s, frames, RATE) for s in range(2)])

    columns_only = ssa.Batch(RATE, 2, 2, frames, N, HOP, flags=FFT, spectrum_columns=64)
    no_fft = ssa.Batch(RATE, 2, 2, frames, N, HOP, flags=L.SS_BATCH_LUFS)
    buf, cnt, cnt64 = np.empty(2 * 1705, np.float32), np.empty(2, np.uint32), np.empty(2, np.uint64)
    for other in (columns_only, no_fft):
        other.upload(0, x); other.run()
        assert lib.ss_batch_spectrum_stats(other._h) == L.SS_ERR_INVALID_MODE
        assert lib.ss_batch_download_spectrum_stats(other._h, 0, buf.ctypes.data_as(fp), None, buf.size, None, 0) == L.SS_ERR_INVALID_MODE
        assert lib.ss_batch_corpus_spectrum(other._h, buf.ctypes.data_as(fp), None, buf.size, None, 0) == L.SS_ERR_INVALID_MODE
        other.close()

    b = ssa.Batch(RATE, 2, 2, frames, N, HOP)              # every output of a pass: rows, decimation bins, sub-block energies
    assert b.layout.n_bins == 1705
    b.upload(0, x); b.run()
    args = (buf.ctypes.data_as(fp), buf.ctypes.data_as(fp), buf.size, cnt.ctypes.data_as(up), 2)
    assert lib.ss_batch_download_spectrum_stats(b._h, 0, *args) == L.SS_ERR_INVALID_MODE         # before the first reduction
    assert lib.ss_batch_corpus_spectrum(b._h, buf.ctypes.data_as(fp), None, buf.size, cnt64.ctypes.data_as(qp), 2) == L.SS_ERR_INVALID_MODE
    before = b.checksums()
    b.spectrum_stats()
    b.corpus_spectrum()
    assert np.array_equal(b.checksums(), before) and before[:, 0].all()
    assert lib.ss_batch_spectrum_stats(None) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_spectrum_stats(b._h, 2, *args) == L.SS_ERR_INVALID_ARG            # no such stream
    assert lib.ss_batch_download_spectrum_stats(b._h, 1, buf.ctypes.data_as(fp), None, buf.size - 1, None, 0) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_spectrum_stats(b._h, 1, None, None, buf.size, cnt.ctypes.data_as(up), 1) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_corpus_spectrum(b._h, buf.ctypes.data_as(fp), None, buf.size - 1, None, 0) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_spectrum_stats(b._h, 1, None, buf.ctypes.data_as(fp), buf.size, None, 0) == L.SS_OK    # either may be NULL
    assert np.array_equal(buf.reshape(2, 1705), b.spectrum_stats_of(1)[1])
    b.close()

    empty = ssa.Batch(RATE, 2, 2, N, N, HOP, flags=FFT)    # no window at all: valid, every result NaN with count 0
    assert empty.layout.n_windows == 0
    empty.upload(0, x[:4 * N]); empty.run()
    empty.spectrum_stats()
    for mean, mx, counted in (empty.spectrum_stats_of(1), empty.corpus_spectrum()):
        assert np.isnan(mean).all() and np.isnan(mx).all() and not counted.any()
    empty.close()
