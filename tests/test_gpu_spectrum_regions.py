"""Batch spectrum regions (ss_batch_spectrum_regions): the average (power mean) and peak-hold spectrum of time ranges of the streams
and of groups of them, against numpy in f64 over the rows Batch.fft(stream)[w_first:w_end] of the same pass — reference() of
tests/test_gpu_spectrum_stats.py, restated here:  max_db = nanmax, mean_db = 10 log10(nanmean(10^(v / 10))), windows_counted = the
non-NaN values at bin 0.  A group is checked against the pooled rows of its members, a region listed twice counted twice.

max_db, the counts and the NaN positions are exact.  mean_db is within 1e-4 dB at EVERY finite bin: the bound that
tests/test_gpu_spectrum_stats.py derives (f32 exponent argument 6e-6 dB, exp2f 1e-6 dB, f32 result 8e-6 dB: under 2e-5 dB, a factor
of five left for the device's exp2f) holds unchanged, because the arithmetic is the same — f32 powers, f64 sums, an f64 logarithm.
Every parity case prints its worst deviation (pytest -rA) and asserts that the bins it compared number fft_channels x n_bins for
every region that holds an unrefused window, so none passes by comparing nothing.

[w_first, w_end) is Batch.region_windows: ss_region_windows — the arithmetic the device path runs on, checked against an enumeration
of the windows in tests/test_spectrum_regions_abi.py — cut to the stream's own window count; the worked cases are pinned below.
Unless said otherwise: 48 kHz, fft_n 4096, hop 1024, stereo streams of 96 000 frames: 89 windows, 20 entries of 4800 frames."""
import ctypes as C
import warnings

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_multich, make_stereo

pytestmark = pytest.mark.gpu

TOL_DB = 1e-4
RATE, N, HOP, S = 48000, 4096, 1024, 4800
FRAMES, WINDOWS, ENTRIES = 96000, 89, 20
FFT = L.SS_BATCH_FFT
NO_GROUP = L.SS_REGION_NO_GROUP
FP, UP, QP = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


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
    """got = (mean f32, max f32, counts) of the device, ref = reference(...); returns (worst |mean_db| deviation, finite bins compared)"""
    (mean, mx, cnt), (rmean, rmx, rcnt) = got, ref
    assert mean.dtype == np.float32 and mx.dtype == np.float32 and mean.shape == rmean.shape == mx.shape, tag
    assert np.array_equal(cnt.astype(np.uint64), rcnt), (tag, cnt, rcnt)
    assert np.array_equal(mx, rmx, equal_nan=True), (tag, np.argwhere(~((mx == rmx) | (np.isnan(mx) & np.isnan(rmx))))[:8])
    assert np.array_equal(np.isnan(mean), np.isnan(rmean)), (tag, np.argwhere(np.isnan(mean) != np.isnan(rmean))[:8])
    inf = np.isinf(rmean)
    assert np.array_equal(mean[inf].astype(np.float64), rmean[inf]), tag
    fin = np.isfinite(rmean)
    worst = float(np.abs(mean[fin].astype(np.float64) - rmean[fin]).max()) if fin.any() else 0.0
    assert worst <= TOL_DB, (tag, worst)
    return worst, int(fin.sum())


def check_list(b, regions, n_groups, tag, rows_of=None):
    """The last list's regions and groups against numpy; returns ((mean, max, counts) of the regions, of the groups, the windows of
    every region)."""
    lay = b.layout
    full = int(lay.fft_channels) * int(lay.n_bins)
    rows_of = rows_of or {}
    regs, grps = b.region_spectra(), b.group_spectra()
    assert regs[0].shape == (len(regions), lay.fft_channels, lay.n_bins) and regs[2].shape == (len(regions), lay.fft_channels)
    assert grps[0].shape == (n_groups, lay.fft_channels, lay.n_bins) and grps[2].dtype == np.uint64 and regs[2].dtype == np.uint32
    worst, compared, windows, members = 0.0, 0, [], {g: [] for g in range(n_groups)}
    for i, r in enumerate(regions):
        s = int(r[0])
        if s not in rows_of:
            rows_of[s] = own_rows(b, s)
        lo, hi = b.region_windows(r)
        assert 0 <= lo <= hi <= rows_of[s].shape[0], (tag, i, lo, hi)
        rows = rows_of[s][lo:hi]
        w, n = assert_matches(tuple(a[i] for a in regs), reference(rows), f"{tag} region {i} {tuple(r)}")
        if (~np.isnan(rows)).all(axis=2).any(axis=0).all():         # every fft channel has an unrefused window
            assert n == full, (tag, i, n, full)
        worst, compared = max(worst, w), compared + n
        windows.append((lo, hi))
        if r[3] != NO_GROUP:
            members[int(r[3])].append(rows)
    for g, parts in members.items():
        pooled = np.concatenate(parts, axis=0) if parts else np.empty((0, lay.fft_channels, lay.n_bins), np.float32)
        w, n = assert_matches(tuple(a[g] for a in grps), reference(pooled), f"{tag} group {g}")
        if (~np.isnan(pooled)).all(axis=2).any(axis=0).all():
            assert n == full, (tag, g, n, full)
        worst, compared = max(worst, w), compared + n
    print(f"{tag}: worst |mean_db - numpy| = {worst:.3g} dB over {compared} finite bins of {len(regions)} regions and {n_groups} groups")
    return regs, grps, windows


def all_bytes(b):
    return tuple(a.tobytes() for a in b.region_spectra() + b.group_spectra())


def region_array(rows):
    return (L.LoudnessRegion * max(len(rows), 1))(*rows)


@pytest.fixture(scope="module")
def three():
    """three streams of different material after one pass, and their rows (computed once, left alone)"""
    b = ssa.Batch(RATE, 2, 3, FRAMES, N, HOP, flags=FFT)
    assert (b.layout.n_windows, b.layout.fft_channels, b.layout.n_bins, b.layout.fft_bin_stride) == (WINDOWS, 2, 1705, 1708)
    b.upload(0, np.concatenate([make_stereo(101 + s, FRAMES, RATE, level=(0.2, 1.0, 3.0)[s], gap=(s == 1)) for s in range(3)]))
    b.run()
    rows = {s: own_rows(b, s) for s in range(3)}
    yield b, rows
    b.close()


# ---------------------------------------------------------------- 1: one-chunk plan, every kind of region in one list
ONE_CHUNK = [(0, 2, 3, 0),                       # short regions of different streams in one group
             (1, 5, 6, 0),
             (2, 16, 1, 1),                      # owns window 74 alone
             (0, 16, 1, NO_GROUP),
             (1, 0, 1, 1),                       # owns no window although n > 0
             (2, 7, 0, 1),                       # n = 0
             (0, 15, 5, 2),                      # reaches the tail entry
             (1, 3, 4, 2), (1, 5, 4, 2),         # overlap
             (2, 9, 2, 3), (2, 9, 2, 3),         # listed twice: counted twice
             (0, 0, 6, NO_GROUP)]                # group 4 is named by nothing


def test_one_chunk_plan_mixed_list(three):
    b, rows = three
    b.spectrum_regions(ONE_CHUNK, 5)
    assert b.spectrum_regions_plan[0] == 1
    regs, grps, windows = check_list(b, ONE_CHUNK, 5, "one chunk", dict(rows))
    assert windows[2] == (74, 75) == windows[3] and windows[4] == (0, 0) and windows[5][0] == windows[5][1]
    assert windows[6][1] == WINDOWS and all(hi - lo < 32 for lo, hi in windows)
    assert windows[7][0] < windows[8][0] < windows[7][1] < windows[8][1]                                 # they do overlap
    assert list(regs[2][2]) == [1, 1] and np.array_equal(regs[1][2], rows[2][74]) and np.array_equal(regs[1][3], rows[0][74])
    assert np.abs(regs[0][2].astype(np.float64) - rows[2][74]).max() <= TOL_DB                          # one window: its own mean
    for i in (4, 5):
        assert np.isnan(regs[0][i]).all() and np.isnan(regs[1][i]).all() and not regs[2][i].any()
    assert list(grps[2][1]) == [1, 1] and np.array_equal(grps[1][1], regs[1][2])                       # one window and two empty regions
    assert list(grps[2][3]) == [2 * int(regs[2][9][0])] * 2 and regs[2][9][0] == windows[9][1] - windows[9][0] > 0
    assert np.array_equal(grps[1][3], regs[1][9]) and np.array_equal(regs[0][9], regs[0][10])
    assert list(grps[2][2]) == [int(regs[2][6][0]) + int(regs[2][7][0]) + int(regs[2][8][0])] * 2
    assert np.isnan(grps[0][4]).all() and np.isnan(grps[1][4]).all() and not grps[2][4].any()
    # a part of the list by first / count
    mean, mx, cnt = b.region_spectra(6, 3)
    assert mean.tobytes() == regs[0][6:9].tobytes() and mx.tobytes() == regs[1][6:9].tobytes() and cnt.tobytes() == regs[2][6:9].tobytes()
    mean, mx, cnt = b.group_spectra(2, 2)
    assert mean.tobytes() == grps[0][2:4].tobytes() and mx.tobytes() == grps[1][2:4].tobytes() and cnt.tobytes() == grps[2][2:4].tobytes()


# ---------------------------------------------------------------- 2: chunked plan: one stream, a long and a short region
def test_chunked_plan_and_two_calls_agree_byte_for_byte():
    b = ssa.Batch(RATE, 2, 1, FRAMES, N, HOP, flags=FFT)
    b.upload(0, make_stereo(111, FRAMES, RATE, level=1.0, gap=True))
    b.run()
    regions = [(0, 0, 20, 0), (0, 16, 1, 0)]
    b.spectrum_regions(regions, 1)
    assert b.spectrum_regions_plan == (5, 18)            # plan_spectrum_stats(4 pairs, 1708, 89): chunks > 1
    first = all_bytes(b)
    regs, grps, windows = check_list(b, regions, 1, "chunked")
    assert windows == [(0, WINDOWS), (74, 75)]           # the short region's chunks 1 .. 4 hold nothing
    assert list(regs[2][0]) == [WINDOWS] * 2 and list(regs[2][1]) == [1, 1] and list(grps[2][0]) == [WINDOWS + 1] * 2
    b.spectrum_regions(regions, 1)
    assert all_bytes(b) == first                          # all three arrays of regions and groups, mean_db included
    b.close()


# ---------------------------------------------------------------- 3: whole-stream regions against the existing reductions
def test_whole_streams_equal_spectrum_stats_and_the_corpus_form(three):
    b, rows = three
    regions = [(s, 0, ENTRIES, 0) for s in range(3)]
    b.spectrum_regions(regions, 1)
    regs, grps, windows = check_list(b, regions, 1, "whole streams", dict(rows))
    assert windows == [(0, WINDOWS)] * 3
    b.spectrum_stats()
    for s in range(3):
        mean, mx, cnt = b.spectrum_stats_of(s)
        assert np.array_equal(regs[1][s], mx, equal_nan=True) and np.array_equal(regs[2][s], cnt)
    mean, mx, cnt = b.corpus_spectrum()
    assert np.array_equal(grps[1][0], mx, equal_nan=True) and np.array_equal(grps[2][0], cnt) and list(cnt) == [3 * WINDOWS] * 2


# ---------------------------------------------------------------- 4: refusals
def test_refused_windows_drop_out_of_their_own_regions_only():
    bad_at = 40000
    refused = windows_holding(bad_at, WINDOWS)
    assert refused == [35, 36, 37, 38]
    regions = [(0, 7, 3, 0), (1, 7, 3, 0), (1, 8, 2, 1), (1, 8, 1, 1), (2, 8, 1, NO_GROUP), (2, 0, 20, 0), (1, 0, 20, NO_GROUP)]
    x = [make_stereo(121 + s, FRAMES, RATE, level=1.0) for s in range(3)]
    b = ssa.Batch(RATE, 2, 3, FRAMES, N, HOP, flags=FFT)
    b.upload(0, np.concatenate(x))
    b.run()
    b.spectrum_regions(regions, 2)
    clean = b.region_spectra()
    assert list(clean[2][:, 0]) == [10, 10, 5, 1, 1, WINDOWS, WINDOWS]
    x[1][2 * bad_at] = np.float32(np.nan)                 # L only: mid and side are both NaN there
    b.upload(0, np.concatenate(x))
    b.run()
    b.spectrum_regions(regions, 2)
    regs, grps, windows = check_list(b, regions, 2, "refusals")
    assert windows[:5] == [(32, 42), (32, 42), (37, 42), (37, 38), (37, 38)]
    assert np.isnan(b.fft(1)[refused]).all() and not np.isnan(b.fft(1)[[34, 39]]).any()
    # a region that holds some of the refused windows counts that many fewer; one that holds only refused windows reads NaN with 0
    assert list(regs[2][1]) == [10 - 4] * 2 and list(regs[2][2]) == [5 - 2] * 2 and list(regs[2][6]) == [WINDOWS - 4] * 2
    assert np.isnan(regs[0][3]).all() and np.isnan(regs[1][3]).all() and list(regs[2][3]) == [0, 0]
    assert np.isfinite(regs[0][1]).all() and np.isfinite(regs[0][2]).all()
    assert list(grps[2][1]) == [3, 3] and list(grps[2][0]) == [10 + 6 + WINDOWS] * 2
    for i in (0, 4, 5):                                   # the other streams' regions: as in the run without the NaN
        for a, c in zip(regs, clean):
            assert a[i].tobytes() == c[i].tobytes(), i
    b.close()


def test_refusal_in_one_channel_of_per_channel_rows():
    nw, ch = 50, 3
    frames = (N // HOP + nw) * HOP
    bad_at = RATE                                          # 1 s: windows 42 ... 45
    refused = windows_holding(bad_at, nw)
    assert refused == [42, 43, 44, 45]
    b = ssa.Batch(RATE, ch, 1, frames, N, HOP, flags=FFT)
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft4096_pairw" and b.layout.fft_channels == 3 and b.layout.n_windows == nw
    x = make_multich(131, frames, ch, RATE, level=0.8)
    x[ch * bad_at + 1] = np.float32(np.nan)
    b.upload(0, x)
    b.run()
    regions = [(0, 9, 3, 0), (0, 0, 9, 0)]                # the first reaches the tail entry and is cut at the stream's 50 windows
    b.spectrum_regions(regions, 1)
    regs, grps, windows = check_list(b, regions, 1, "per channel")
    assert windows == [(42, 50), (0, 38)]
    assert list(regs[2][0]) == [8, 8 - len(refused), 8] and list(regs[2][1]) == [38, 38, 38]      # the other channels' counts are untouched
    assert list(grps[2][0]) == [46, 42, 46]
    b.close()


# ---------------------------------------------------------------- 5: ragged batches, with loud stale rows behind every stream's own count
def test_ragged_batch_never_shows_the_stale_rows():
    lengths = [FRAMES, 30000, 5200, N]
    loud = np.concatenate([make_stereo(141 + s, FRAMES, RATE, level=3.0) for s in range(4)])       # about -1 dBFS at the peaks
    b = ssa.Batch(RATE, 2, 4, FRAMES, N, HOP, flags=FFT)
    b.upload(0, loud)
    b.run()
    b.sync()
    pass_one = [b.fft(s).copy() for s in range(4)]
    b.set_lengths(lengths)
    b.upload(0, loud * np.float32(1e-3))                   # the same material 60 dB down
    b.run()
    counts = [int(b.stream_shape(s).n_windows) for s in range(4)]
    assert counts == [WINDOWS, 25, 1, 0]
    regions = [(0, 0, 20, 0), (1, 0, 7, 0), (2, 0, 2, 1), (3, 0, 1, 1), (1, 4, 3, NO_GROUP)]     # each up to its stream's own E_s
    b.spectrum_regions(regions, 2)
    regs, grps, windows = check_list(b, regions, 2, "ragged")
    # without the cut at the stream's own count (1, 0, 7) would own 28 windows and (2, 0, 2) five: three and four stale rows
    assert windows == [(0, WINDOWS), (0, 25), (0, 1), (0, 0), (18, 25)]
    lay = b.layout
    for i, s in ((1, 1), (2, 2), (4, 1)):
        slot = np.empty((lay.n_windows, lay.fft_channels, lay.n_bins), np.float32)
        assert L.lib().ss_batch_download_fft(b._h, s, slot.ctypes.data_as(FP), slot.size) == L.SS_OK
        assert np.array_equal(slot[-1], pass_one[s][-1]) and np.median(slot[counts[s]:, 0]) - np.median(slot[:counts[s], 0]) > 40     # the plant: loud rows behind the count
        assert list(regs[2][i]) == [windows[i][1] - windows[i][0]] * 2
        assert np.median(regs[1][i][0] - pass_one[s][windows[i][0]:windows[i][1], 0].max(axis=0)) < -55      # a stale row would put this near 0
    assert np.isnan(regs[0][3]).all() and list(grps[2][1]) == [1, 1]
    before = all_bytes(b)
    lib = L.lib()
    for beyond in ((1, 0, 8, 0), (1, 7, 1, 0), (2, 2, 1, 0), (3, 1, 1, 0), (3, 0, 2, 0)):                # beyond the stream's own E_s
        assert lib.ss_batch_spectrum_regions(b._h, region_array([beyond]), 1, 1) == L.SS_ERR_INVALID_ARG, beyond
    assert lib.ss_batch_spectrum_regions(b._h, region_array([(0, 19, 1, 0)]), 1, 1) == L.SS_OK          # stream 0 keeps its own
    b.spectrum_regions(regions, 2)
    assert all_bytes(b) == before
    b.close()


# ---------------------------------------------------------------- 6: another row shape: N = 16384 mid/side
def test_fft16k_rows():
    frames = (16384 // HOP + 40) * HOP
    b = ssa.Batch(RATE, 2, 1, frames, 16384, HOP, flags=FFT)
    lay = b.layout
    assert L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT) == b"k_fft16k_run" and lay.n_windows == 40
    assert lay.fft_bin_stride != 1708 and (lay.fft_bin_stride // 4 + 63) // 64 > 7                 # longer rows, more slices
    b.upload(0, make_stereo(151, frames, RATE, level=1.0, gap=False))
    b.run()
    regions = [(0, 0, 12, 0), (0, 4, 6, 0)]
    b.spectrum_regions(regions, 1)
    regs, grps, windows = check_list(b, regions, 1, "fft16k_run")
    assert windows == [(0, 40), (18, 30)] and list(grps[2][0]) == [52, 52]
    b.close()


# ---------------------------------------------------------------- 7: the status ladder, and nothing is written or replaced by a refused call
def test_status_ladder_and_untouched_outputs():
    lib = L.lib()
    x = np.concatenate([make_stereo(161 + s, FRAMES, RATE) for s in range(2)])
    some = region_array([(0, 0, 20, 0), (1, 3, 4, 1)])
    cnt32, cnt64 = np.zeros(8, np.uint32), np.zeros(8, np.uint64)
    buf = np.zeros(2 * 2 * 1705, np.float32)

    columns_only = ssa.Batch(RATE, 2, 2, FRAMES, N, HOP, flags=FFT, spectrum_columns=64)
    no_fft = ssa.Batch(RATE, 2, 2, FRAMES, N, HOP, flags=L.SS_BATCH_LUFS)
    for other in (columns_only, no_fft):
        other.upload(0, x); other.run()
        assert lib.ss_batch_spectrum_regions(other._h, some, 2, 2) == L.SS_ERR_INVALID_MODE
        assert lib.ss_batch_download_region_spectra(other._h, 0, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_MODE
        assert lib.ss_batch_download_group_spectra(other._h, 0, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_MODE
        assert lib.ss_batch_spectrum_regions_plan(other._h, None, None) == L.SS_ERR_INVALID_MODE
        other.close()

    assert lib.ss_batch_spectrum_regions(None, some, 2, 2) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_region_spectra(None, 0, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_group_spectra(None, 0, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_spectrum_regions_plan(None, None, None) == L.SS_ERR_INVALID_ARG

    b = ssa.Batch(RATE, 2, 2, FRAMES, N, HOP, flags=FFT)  # without SS_BATCH_LUFS: the grid comes from the rate alone
    b.upload(0, x); b.run()
    # before the first call
    assert lib.ss_batch_download_region_spectra(b._h, 0, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_group_spectra(b._h, 0, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_spectrum_regions_plan(b._h, None, None) == L.SS_ERR_INVALID_MODE
    before = b.checksums()
    assert lib.ss_batch_spectrum_regions(b._h, some, 2, 2) == L.SS_OK
    b._listed["spectrum"] = (2, 2)
    assert lib.ss_batch_spectrum_regions_plan(b._h, None, None) == L.SS_OK                              # either pointer may be NULL
    check_list(b, [(0, 0, 20, 0), (1, 3, 4, 1)], 2, "ladder")
    assert np.array_equal(b.checksums(), before) and before[:, 0].all()                                # nothing of the pass is written
    kept = all_bytes(b)

    def refused(rows, n, n_groups, status):
        assert lib.ss_batch_spectrum_regions(b._h, rows, n, n_groups) == status, (n, n_groups, status)
        assert all_bytes(b) == kept                        # the previous list and results as they were
    refused(None, 2, 2, L.SS_ERR_INVALID_ARG)
    refused(region_array([(0, 0, 20, 0), (2, 0, 1, 0)]), 2, 2, L.SS_ERR_INVALID_ARG)                    # no such stream
    refused(region_array([(0, 0, 20, 0), (1, 20, 1, 0)]), 2, 2, L.SS_ERR_INVALID_ARG)                   # beyond E_s
    refused(region_array([(0, 0, 20, 0), (1, 0xFFFFFFFF, 2, 0)]), 2, 2, L.SS_ERR_INVALID_ARG)           # ... in 64 bits
    refused(region_array([(0, 0, 20, 0), (1, 0, 1, 2)]), 2, 2, L.SS_ERR_INVALID_ARG)                    # no such group
    refused(some, 2, 0xFFFFFFFE, L.SS_ERR_UNSUPPORTED)                                                  # a grid of groups beyond one launch
    # the downloads: ranges, capacities, and nothing written
    f = lambda a: a.ctypes.data_as(FP)
    assert lib.ss_batch_download_region_spectra(b._h, 1, 2, f(buf), None, buf.size, None, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_region_spectra(b._h, 3, 0, None, None, 0, None, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_region_spectra(b._h, 0xFFFFFFFF, 2, None, None, 0, None, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_group_spectra(b._h, 2, 1, f(buf), None, buf.size, None, 0) == L.SS_ERR_INVALID_ARG
    buf[:], cnt32[:], cnt64[:] = -7.0, 77, 77
    other = buf.copy()
    assert lib.ss_batch_download_region_spectra(b._h, 0, 2, f(buf), f(other), buf.size - 1, cnt32.ctypes.data_as(UP), 4) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_region_spectra(b._h, 0, 2, f(buf), f(other), buf.size, cnt32.ctypes.data_as(UP), 3) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_group_spectra(b._h, 0, 2, None, f(other), buf.size - 1, cnt64.ctypes.data_as(QP), 4) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_group_spectra(b._h, 0, 2, f(buf), None, buf.size, cnt64.ctypes.data_as(QP), 3) == L.SS_ERR_CAPACITY
    assert (buf == -7.0).all() and (other == -7.0).all() and (cnt32 == 77).all() and (cnt64 == 77).all()
    # any of the three may be NULL; the exact capacities are taken
    regs = b.region_spectra()
    assert lib.ss_batch_download_region_spectra(b._h, 1, 1, None, f(buf), 2 * 1705, None, 0) == L.SS_OK
    assert np.array_equal(buf[:2 * 1705].reshape(2, 1705), regs[1][1]) and (buf[2 * 1705:] == -7.0).all()
    assert lib.ss_batch_download_region_spectra(b._h, 0, 2, None, None, 0, cnt32.ctypes.data_as(UP), 4) == L.SS_OK
    assert np.array_equal(cnt32[:4].reshape(2, 2), regs[2]) and (cnt32[4:] == 77).all()
    assert lib.ss_batch_download_group_spectra(b._h, 1, 1, None, None, 0, cnt64.ctypes.data_as(QP), 2) == L.SS_OK
    assert list(cnt64[:2]) == list(regs[2][1]) and (cnt64[2:] == 77).all()
    assert all_bytes(b) == kept
    # n_regions == 0 is valid: no region, and groups that nothing names
    assert lib.ss_batch_spectrum_regions(b._h, None, 0, 2) == L.SS_OK
    b._listed["spectrum"] = (0, 2)
    assert lib.ss_batch_download_region_spectra(b._h, 0, 0, None, None, 0, None, 0) == L.SS_OK
    assert lib.ss_batch_download_region_spectra(b._h, 0, 1, f(buf), None, buf.size, None, 0) == L.SS_ERR_INVALID_ARG
    assert b.region_spectra()[0].shape == (0, 2, 1705)
    mean, mx, cnt = b.group_spectra()
    assert np.isnan(mean).all() and np.isnan(mx).all() and not cnt.any() and mean.shape == (2, 2, 1705)
    assert lib.ss_batch_spectrum_regions(b._h, None, 0, 0) == L.SS_OK
    assert lib.ss_batch_download_group_spectra(b._h, 0, 0, None, None, 0, None, 0) == L.SS_OK
    assert lib.ss_batch_download_group_spectra(b._h, 0, 1, f(buf), None, buf.size, None, 0) == L.SS_ERR_INVALID_ARG
    b.close()
