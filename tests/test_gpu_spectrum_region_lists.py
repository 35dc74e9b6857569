"""A loudness list (ss_batch_loudness_regions), a peak list (ss_batch_peak_regions) and a spectrum list (ss_batch_spectrum_regions)
held by one batch at once: each keeps its own device list, staging, counts and results, whatever is done to the other two.

Everything is compared byte for byte: the downloads of a batch that holds all three lists against those of a twin batch that only
ever held the one list (same input, same pass), so there is no tolerance.  What the results themselves must be is pinned by
test_gpu_loudness_regions.py, test_gpu_peak_series.py and test_gpu_spectrum_regions.py."""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L

pytestmark = pytest.mark.gpu

RATE, CHANNELS, STREAMS, S = 48000, 2, 2, 4800
FRAMES = 30 * S + 9                                      # 30 sub-blocks, 31 entries, 136 windows
NO_GROUP = L.SS_REGION_NO_GROUP
INF = float("inf")
CEILING = 0.5
LOUD = [(0, 0, 30, 0), (1, 5, 20, 0), (0, 10, 7, NO_GROUP)]                                      # 3 regions, 1 group
PEAK = [(0, 0, 31, 0), (1, 0, 31, 1), (0, 30, 1, 1), (1, 12, 6, NO_GROUP), (0, 3, 0, 0)]         # 5 regions, 2 groups
SPEC = [(0, 0, 31, 0), (1, 4, 15, 1), (1, 16, 1, 1), (0, 0, 1, NO_GROUP)]                        # 4 regions, 2 groups
SPEC_40 = [(i % 2, i % 25, 2 + i % 5, i % 3) for i in range(40)]                                 # 3 groups
LOUD_40 = [(i % 2, i % 20, 5 + i % 6, i % 3) for i in range(40)]
PEAK_40 = [(i % 2, i % 29, 1 + i % 3, i % 2) for i in range(40)]


def corpus():
    x = (0.1 * np.random.default_rng(2025).uniform(-1, 1, (STREAMS, FRAMES, CHANNELS))).astype(np.float32)
    for s, n, c, v in [(0, 12345, 1, 0.7), (0, 30 * S + 4, 0, 0.9), (1, 12 * S, 0, -0.8), (1, 29 * S + 17, 1, 0.6)]:
        x[s, n, c] = v
    return x.reshape(-1)


def batch(x):
    """the corpus resident, one pass and one peak series queued"""
    b = ssa.Batch(RATE, CHANNELS, STREAMS, FRAMES, 4096, 1024, flags=L.SS_BATCH_FFT | L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    b.upload(0, x)
    b.run()
    b.peak_series()
    return b


def loud_bytes(b):
    return bytes(b.region_results()), bytes(b.group_results())


def peak_bytes(b):
    ch = b.region_channel_peaks()
    return bytes(b.region_peaks()), bytes(b.group_peaks()), ch[0].tobytes(), ch[1].tobytes()


def spec_bytes(b):
    return tuple(a.tobytes() for a in b.region_spectra() + b.group_spectra())


SET = {"loud": lambda b, rows=LOUD, g=1: b.loudness_regions(rows, g),
       "peak": lambda b, rows=PEAK, g=2: b.peak_regions(rows, g, CEILING),
       "spec": lambda b, rows=SPEC, g=2: b.spectrum_regions(rows, g)}
GET = {"loud": loud_bytes, "peak": peak_bytes, "spec": spec_bytes}


def only(x, kind, *list_and_groups):
    b = batch(x)
    SET[kind](b, *list_and_groups)
    out = GET[kind](b)
    b.close()
    return out


@pytest.fixture(scope="module")
def world():
    """the corpus and, computed once and left alone, the downloads of the twin batches that only ever held one list"""
    x = corpus()
    return {"x": x, "loud": only(x, "loud"), "peak": only(x, "peak"), "spec": only(x, "spec")}


def all_three(x, order=("loud", "peak", "spec")):
    b = batch(x)
    for kind in order:
        SET[kind](b)
    return b


def as_twins(b, world, kinds=("loud", "peak", "spec")):
    return all(GET[k](b) == world[k] for k in kinds)


def test_twins_are_not_trivial(world):
    b = all_three(world["x"])
    assert b.layout.n_windows == 136
    mean, mx, cnt = b.region_spectra()
    gmean, gmx, gcnt = b.group_spectra()
    assert list(cnt[:, 0]) == [136, b.region_windows(SPEC[1])[1] - b.region_windows(SPEC[1])[0], 1, 0] and cnt[1, 0] > 30
    assert np.isfinite(mean[:3]).all() and np.isnan(mean[3]).all() and (mx[1] >= mx[2]).all()      # window 74 lies inside region 1
    assert list(gcnt[:, 0]) == [136, int(cnt[1, 0]) + 1] and np.isfinite(gmean).all()
    assert b.region_results()[0].n_gating_blocks == 27 and b.region_peaks()[2].first_over == 30
    b.close()


@pytest.mark.parametrize("order", [("loud", "peak", "spec"), ("spec", "peak", "loud"), ("peak", "spec", "loud")])
def test_results_do_not_depend_on_the_other_lists_or_the_order(world, order):
    b = all_three(world["x"], order)
    assert as_twins(b, world)
    b.close()


def test_what_is_done_to_the_spectrum_list_leaves_the_other_two(world):
    x, lib = world["x"], L.lib()
    b = all_three(x)
    # refused: a bad stream, a bad group, a bound beyond the entries
    for rows, n_groups in (([(0, 0, 4, 0), (2, 0, 1, 0)], 1), ([(0, 0, 4, 0), (1, 0, 4, 1)], 1), ([(0, 30, 2, 0)], 1)):
        assert lib.ss_batch_spectrum_regions(b._h, (L.LoudnessRegion * len(rows))(*rows), len(rows), n_groups) == L.SS_ERR_INVALID_ARG
        assert as_twins(b, world)
    # replaced and grown
    b.spectrum_regions(SPEC_40, 3)
    assert as_twins(b, world, ("loud", "peak")) and spec_bytes(b) == only(x, "spec", SPEC_40, 3)
    assert b.region_spectra()[0].shape[0] == 40 and b.group_spectra()[0].shape[0] == 3
    # replaced by a shorter one again
    b.spectrum_regions(SPEC, 2)
    assert as_twins(b, world)
    # emptied
    assert lib.ss_batch_spectrum_regions(b._h, None, 0, 0) == L.SS_OK
    b._listed["spectrum"] = (0, 0)
    assert as_twins(b, world, ("loud", "peak")) and b.region_spectra()[0].shape[0] == 0
    b.close()


def test_what_is_done_to_the_other_two_leaves_the_spectrum_list(world):
    x, lib = world["x"], L.lib()
    b = all_three(x)
    bad_stream = (L.LoudnessRegion * 2)((0, 0, 4, 0), (2, 0, 1, 0))
    bad_group = (L.LoudnessRegion * 2)((0, 0, 4, 0), (1, 0, 4, 1))
    assert lib.ss_batch_peak_regions(b._h, bad_stream, 2, 1, INF) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_loudness_regions(b._h, bad_group, 2, 1) == L.SS_ERR_INVALID_ARG
    assert as_twins(b, world)
    b.peak_regions(PEAK_40, 2, CEILING)                  # the peak side's buffers grow
    assert as_twins(b, world, ("loud", "spec")) and peak_bytes(b) == only(x, "peak", PEAK_40, 2)
    b.loudness_regions(LOUD_40, 3)                       # ... and the loudness side's
    assert as_twins(b, world, ("spec",)) and loud_bytes(b) == only(x, "loud", LOUD_40, 3)
    assert lib.ss_batch_peak_regions(b._h, None, 0, 0, INF) == L.SS_OK
    assert lib.ss_batch_loudness_regions(b._h, None, 0, 0) == L.SS_OK
    assert as_twins(b, world, ("spec",))
    b.close()


def test_the_spectrum_list_takes_the_peak_lists_bound(world):
    """every list the peak regions accept is accepted here (the tail entry included), so also every list the loudness regions accept"""
    lib = L.lib()
    b = batch(world["x"])

    def status(stream, first, n):
        one = (L.LoudnessRegion * 1)((stream, first, n, NO_GROUP))
        return (lib.ss_batch_spectrum_regions(b._h, one, 1, 0), lib.ss_batch_peak_regions(b._h, one, 1, 0, INF),
                lib.ss_batch_loudness_regions(b._h, one, 1, 0))
    assert status(0, 30, 1) == (L.SS_OK, L.SS_OK, L.SS_ERR_INVALID_ARG)       # the tail entry is no sub-block
    assert status(0, 29, 1) == (L.SS_OK, L.SS_OK, L.SS_OK)
    assert status(0, 31, 1) == (L.SS_ERR_INVALID_ARG,) * 3
    b.close()
