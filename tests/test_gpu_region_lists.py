"""A loudness list (ss_batch_loudness_regions) and a peak list (ss_batch_peak_regions) held by one batch at once: each keeps its own
device list, staging, counts and results, whatever is done to the other.

Everything is compared byte for byte: the records of a batch that holds both lists against those of a twin batch that only ever
held the one list (same input, same pass), so there is no tolerance.  What the records themselves must be is pinned by
test_gpu_loudness_regions.py and test_gpu_peak_series.py."""
import ctypes

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L

pytestmark = pytest.mark.gpu

RATE, CHANNELS, STREAMS, S = 48000, 2, 2, 4800
FRAMES = 30 * S + 9                                      # 30 sub-blocks, 31 entries
NO_GROUP = L.SS_REGION_NO_GROUP
INF = float("inf")
CEILING = 0.5
LOUD = [(0, 0, 30, 0), (1, 5, 20, 0), (0, 10, 7, NO_GROUP)]                                      # 3 regions, 1 group
PEAK = [(0, 0, 31, 0), (1, 0, 31, 1), (0, 30, 1, 1), (1, 12, 6, NO_GROUP), (0, 3, 0, 0)]         # 5 regions, 2 groups
LOUD_40 = [(i % 2, i % 20, 5 + i % 6, i % 3) for i in range(40)]                                 # 3 groups
PEAK_40 = [(i % 2, i % 29, 1 + i % 3, i % 2) for i in range(40)]                                 # 2 groups


def corpus():
    x = (0.1 * np.random.default_rng(2024).uniform(-1, 1, (STREAMS, FRAMES, CHANNELS))).astype(np.float32)
    for s, n, c, v in [(0, 12345, 1, 0.7), (0, 30 * S + 4, 0, 0.9), (1, 12 * S, 0, -0.8), (1, 29 * S + 17, 1, 0.6)]:
        x[s, n, c] = v
    return x.reshape(-1)


def batch(x):
    """the corpus resident, one pass and one peak series queued"""
    b = ssa.Batch(RATE, CHANNELS, STREAMS, FRAMES, 4096, 1024, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    b.upload(0, x)
    b.run()
    b.peak_series()
    return b


def loud_bytes(b):
    return bytes(b.region_results()), bytes(b.group_results())


def peak_bytes(b):
    ch = b.region_channel_peaks()
    return bytes(b.region_peaks()), bytes(b.group_peaks()), ch[0].tobytes(), ch[1].tobytes()


def only_loud(x, rows, n_groups):
    b = batch(x)
    b.loudness_regions(rows, n_groups)
    out = loud_bytes(b)
    b.close()
    return out


def only_peak(x, rows, n_groups):
    b = batch(x)
    b.peak_regions(rows, n_groups, CEILING)
    out = peak_bytes(b)
    b.close()
    return out


@pytest.fixture(scope="module")
def world():
    """the corpus and, computed once and left alone, the records of the twin batches that only ever held one list"""
    x = corpus()
    return {"x": x, "loud": only_loud(x, LOUD, 1), "peak": only_peak(x, PEAK, 2)}


def both(x, loud_first=True):
    b = batch(x)
    for kind in ("loud", "peak") if loud_first else ("peak", "loud"):
        if kind == "loud":
            b.loudness_regions(LOUD, 1)
        else:
            b.peak_regions(PEAK, 2, CEILING)
    return b


def counts_are(b, loud, peak):
    """the library's own counts: the exact capacity is taken, one less is refused"""
    lib = L.lib()
    for call, record, n in [(lib.ss_batch_download_region_results, L.RegionResult, loud[0]), (lib.ss_batch_download_group_results, L.GroupResult, loud[1]),
                            (lib.ss_batch_download_region_peaks, L.RegionPeaks, peak[0]), (lib.ss_batch_download_group_peaks, L.GroupPeaks, peak[1])]:
        arr = (record * max(n, 1))()
        assert call(b._h, arr, n) == L.SS_OK, (call.__name__, n)
        if n:
            assert call(b._h, arr, n - 1) == L.SS_ERR_CAPACITY, (call.__name__, n)


def test_twins_are_not_trivial(world):
    b = both(world["x"])
    res, pk, grp = b.region_results(), b.region_peaks(), b.group_peaks()
    assert res[0].n_gating_blocks == 27 and np.isfinite(res[0].integrated_lufs) and res[2].n_gating_blocks == 4
    top = float(np.float32(0.9))                         # the planted sample of the tail entry
    assert pk[0].sample_peak == top and pk[0].sample_peak_frame == 30 * S + 4 and pk[0].true_peak >= top
    assert pk[2].first_over == 30 and pk[4].true_peak == 0.0
    assert grp[1].sample_peak == top and grp[1].sample_peak_region == 2 and grp[1].n_over == pk[1].n_over + pk[2].n_over >= 3
    b.close()


def test_results_do_not_depend_on_the_other_list_or_the_order(world):
    b1, b2 = both(world["x"], True), both(world["x"], False)
    for b in (b1, b2):
        assert loud_bytes(b) == world["loud"] and peak_bytes(b) == world["peak"]
        counts_are(b, (3, 1), (5, 2))
        b.close()


def test_refusals_leave_both_lists_intact(world):
    b = both(world["x"])
    lib = L.lib()
    bad_stream = (L.LoudnessRegion * 2)((0, 0, 4, 0), (2, 0, 1, 0))
    bad_group = (L.LoudnessRegion * 2)((0, 0, 4, 0), (1, 0, 4, 1))
    assert lib.ss_batch_peak_regions(b._h, bad_stream, 2, 1, INF) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_loudness_regions(b._h, bad_group, 2, 1) == L.SS_ERR_INVALID_ARG
    counts_are(b, (3, 1), (5, 2))
    assert loud_bytes(b) == world["loud"] and peak_bytes(b) == world["peak"]
    b.close()


def test_growing_one_list_does_not_touch_the_other(world):
    x = world["x"]
    b = both(x)
    b.peak_regions(PEAK_40, 2, CEILING)                  # the peak side's buffers grow
    assert loud_bytes(b) == world["loud"]
    assert peak_bytes(b) == only_peak(x, PEAK_40, 2)
    counts_are(b, (3, 1), (40, 2))
    b.close()
    b = both(x)
    b.loudness_regions(LOUD_40, 3)                       # the mirror image
    assert peak_bytes(b) == world["peak"]
    assert loud_bytes(b) == only_loud(x, LOUD_40, 3)
    counts_are(b, (40, 3), (5, 2))
    b.close()


def test_each_feature_keeps_its_own_bound(world):
    lib = L.lib()
    b = batch(world["x"])

    def status(stream, first, n):
        one = (L.LoudnessRegion * 1)((stream, first, n, NO_GROUP))
        return lib.ss_batch_peak_regions(b._h, one, 1, 0, INF), lib.ss_batch_loudness_regions(b._h, one, 1, 0)
    assert status(0, 30, 1) == (L.SS_OK, L.SS_ERR_INVALID_ARG)       # the tail entry is no sub-block
    assert status(0, 29, 1) == (L.SS_OK, L.SS_OK)
    assert status(0, 31, 1) == (L.SS_ERR_INVALID_ARG, L.SS_ERR_INVALID_ARG)
    b.set_lengths([30 * S + 9, 12 * S + 1])
    b.run()
    b.peak_series()
    assert status(1, 12, 1) == (L.SS_OK, L.SS_ERR_INVALID_ARG)       # stream 1: 12 sub-blocks, 13 entries
    assert status(1, 11, 1) == (L.SS_OK, L.SS_OK)
    assert status(1, 13, 1) == (L.SS_ERR_INVALID_ARG, L.SS_ERR_INVALID_ARG)
    assert status(0, 30, 1) == (L.SS_OK, L.SS_ERR_INVALID_ARG)       # stream 0 keeps its own
    b.close()


def test_an_empty_list_of_one_kind_leaves_the_other(world):
    lib = L.lib()
    b = both(world["x"])
    assert lib.ss_batch_peak_regions(b._h, None, 0, 0, INF) == L.SS_OK
    counts_are(b, (3, 1), (0, 0))
    assert loud_bytes(b) == world["loud"]
    b.close()
    b = both(world["x"])
    assert lib.ss_batch_loudness_regions(b._h, None, 0, 0) == L.SS_OK
    counts_are(b, (0, 0), (5, 2))
    assert peak_bytes(b) == world["peak"]
    b.close()
