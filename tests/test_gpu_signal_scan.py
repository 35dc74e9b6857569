"""Batch signal scan (ss_batch_signal_scan): silence runs per stream, clip runs, sums and non-finite samples per channel, and the
lists of the runs.

The reference is numpy, in this file: the two predicates as f32 comparisons on single samples, runs from the differences of a
boolean sequence.  Every integer result must be EQUAL: the stream records and the lists are compared as whole structured arrays, the
channel records field by field.  The two f64 sums are held to the worst-case bound of recursive f64 summation in any order against
math.fsum of the f64-widened samples: |got - ref| <= g * sum|x| (g * sum x^2), g = (N - 1) u / (1 - (N - 1) u), u = 2^-53, N the
channel's finite samples.  Streams are about three tiles long (2 T + 71 frames, T read from the plan call)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import CHANNEL_SCAN_DTYPE, SIGNAL_CLIP, SIGNAL_EVENT_DTYPE, SIGNAL_SILENCE, STREAM_SCAN_DTYPE

pytestmark = pytest.mark.gpu

U64 = 0xFFFFFFFFFFFFFFFF
NO_CHANNEL = 0xFFFFFFFF
INT_FIELDS = ("nonfinite", "first_nonfinite", "clipped_samples", "longest_clip", "longest_clip_at", "clip_runs")
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))


def make_batch(rate, channels, streams, frames, flags=L.SS_BATCH_TRUE_PEAK):
    return ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=flags)


@functools.lru_cache(None)
def tile_frames(channels):
    b = make_batch(48000, channels, 1, 64)
    t = b.signal_scan_plan()[0]
    b.close()
    assert t % 64 == 0 and 0 < t * channels <= 8192
    return t


# ------------------------------------------------------------------------------------------------------------ reference
def runs_of(mask):
    """(first frames, lengths) of the maximal runs of a boolean sequence"""
    d = np.diff(np.concatenate(([0], np.asarray(mask, np.int8), [0])))
    first, end = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return first, end - first


def longest(first, n):
    if not n.size:
        return 0, U64
    i = int(np.argmax(n))                                    # the first of equals
    return int(n[i]), int(first[i])


def reference(x, thr, lvl, smin, cmin):
    """one stream x [frames][channels] f32 -> (stream record, channel records [C], silence list, clip list, (sum|x|, sum x^2, N) [C])"""
    x = np.asarray(x, np.float32)
    F, C = x.shape
    with np.errstate(invalid="ignore"):
        a = np.abs(x)
        silent = (a <= np.float32(thr)).all(axis=1)
        clipped = a >= np.float32(lvl)
    st, ch = np.zeros((), STREAM_SCAN_DTYPE), np.zeros(C, CHANNEL_SCAN_DTYPE)
    first, n = runs_of(silent)
    st["silent_frames"] = int(silent.sum())
    st["leading_silence"] = int(n[0]) if n.size and first[0] == 0 else 0
    st["trailing_silence"] = int(n[-1]) if n.size and first[-1] + n[-1] == F else 0
    st["longest_silence"], st["longest_silence_at"] = longest(first, n)
    keep = n >= smin
    st["silence_runs"] = int(keep.sum())
    sil_list = np.zeros(int(keep.sum()), SIGNAL_EVENT_DTYPE)
    sil_list["first_frame"], sil_list["frames"], sil_list["channel"] = first[keep], n[keep], NO_CHANNEL
    clip_lists, bounds = [], []
    for c in range(C):
        first, n = runs_of(clipped[:, c])
        keep = n >= cmin
        ev = np.zeros(int(keep.sum()), SIGNAL_EVENT_DTYPE)
        ev["first_frame"], ev["frames"], ev["channel"] = first[keep], n[keep], c
        clip_lists.append(ev)
        fin = np.isfinite(x[:, c])
        v = x[fin, c].astype(np.float64)
        ch[c]["sum"], ch[c]["sum_sq"] = math.fsum(v), math.fsum(v * v)
        ch[c]["nonfinite"] = int((~fin).sum())
        ch[c]["first_nonfinite"] = int(np.flatnonzero(~fin)[0]) if (~fin).any() else U64
        ch[c]["clipped_samples"] = int(clipped[:, c].sum())
        ch[c]["longest_clip"], ch[c]["longest_clip_at"] = longest(first, n)
        ch[c]["clip_runs"] = int(keep.sum())
        bounds.append((math.fsum(np.abs(v)), math.fsum(v * v), int(fin.sum())))
    st["clip_runs"] = int(ch["clip_runs"].sum())
    return st, ch, sil_list, np.concatenate(clip_lists) if C else np.zeros(0, SIGNAL_EVENT_DTYPE), bounds


def gamma(n):
    u = 2.0 ** -53
    return (n - 1) * u / (1 - (n - 1) * u) if n > 1 else 0.0


def check(b, streams, tag, max_events=256, **cfg):
    """scan the batch and hold every result against reference() of `streams` (each its own [frames][channels])"""
    thr, lvl = cfg.get("silence_threshold", 0.0), cfg.get("clip_level", 1.0)
    smin = cfg.get("silence_min_frames")
    smin = (int(b.cfg.sample_rate) + 5) // 10 if smin is None else smin
    cmin = cfg.get("clip_min_samples", 3)
    b.signal_scan(max_events=max_events, **cfg)
    got_st, got_ch = b.stream_scans(), b.channel_scans()
    for s, x in enumerate(streams):
        st, ch, sil, clip, bounds = reference(x, thr, lvl, smin, cmin)
        assert got_st[s] == st, (tag, s, got_st[s], st)
        for f in INT_FIELDS:
            assert np.array_equal(got_ch[s][f], ch[f]), (tag, s, f, got_ch[s][f], ch[f])
        for c, (sum_abs, sum_sq, n) in enumerate(bounds):
            assert abs(got_ch[s][c]["sum"] - ch[c]["sum"]) <= gamma(n) * sum_abs, (tag, s, c, "sum", got_ch[s][c]["sum"], ch[c]["sum"])
            assert abs(got_ch[s][c]["sum_sq"] - ch[c]["sum_sq"]) <= gamma(n) * sum_sq, (tag, s, c, "sum_sq")
        for kind, ref in ((SIGNAL_SILENCE, sil), (SIGNAL_CLIP, clip)):
            got = b.signal_events(s, kind)
            assert got.shape == ref[:max_events].shape and np.array_equal(got, ref[:max_events]), (tag, s, kind, got[:8], ref[:8])
    return got_st, got_ch


def loud(rng, frames, channels):
    """never silent at thresholds up to 0.05, never clipped at levels from 0.5"""
    return (rng.uniform(0.1, 0.4, (frames, channels)) * rng.choice([-1.0, 1.0], (frames, channels))).astype(np.float32)


def upload(b, streams):
    slot, C = int(b.cfg.frames_per_stream), int(b.cfg.channels)
    pcm = np.zeros((len(streams), slot, C), np.float32)
    for s, x in enumerate(streams):
        pcm[s, :len(x)] = x
    b.upload(0, pcm)


# ------------------------------------------------------------------------------------------------------------ 1. planted runs
def planted_intervals(T, L):
    """per stream the [first, end) intervals of its planted runs: every edge the kernels have"""
    F = 2 * T + 71
    seams = []                                               # runs at the mask-word seams of tile 1
    for j in range(1, T // 64):
        m = T + 64 * j
        seams.append([(m - 4, m), (m - 2, m + 2), (m - 1, m + 3), (m + 1, m + 5), (m, m + 4), (m - 3, m + 1)][j % 6])
    straddle = [(T - k, T - k + n) for n in (L - 1, L, L + 1) for k in range(1, n)]          # every split of every length
    assert len(straddle) == 6 or L != 3
    return F, [
        [(0, 7), (T, T + 6), (2 * T - 6, 2 * T), (F - 7, F)],                   # from frame 0, from T, to 2T - 1, to F - 1
        [(185, 191), (192, 198), (252, 256), (257, 261), (T - 9, T), (T + 1, T + 8)] + seams,       # one false frame at a seam
        [straddle[0], (straddle[1][0] + T, straddle[1][1] + T)],
        [straddle[2], (straddle[3][0] + T, straddle[3][1] + T)],
        [straddle[4], (straddle[5][0] + T, straddle[5][1] + T)],
        [(T, 2 * T)],                                                           # exactly one whole tile
        [(0, 2 * T)],                                                           # exactly two
        [(0, F)],                                                               # the whole stream
    ]


@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_planted_runs_at_every_edge(channels, rate):
    T, L = tile_frames(channels), 3
    F, plan = planted_intervals(T, L)
    rng = np.random.default_rng(channels * 7 + rate)
    b = make_batch(rate, channels, len(plan), F)
    assert b.signal_scan_plan() == (T, 3)
    silent, clipped = [], []
    for s, intervals in enumerate(plan):
        x, y = loud(rng, F, channels), loud(rng, F, channels)
        for (lo, hi) in intervals:
            x[lo:hi] = 0.0
            y[lo:hi, (s + lo) % channels] = rng.choice([-1.0, 1.0, 1.5], hi - lo)
        if s < 5:                                            # (frame 100 lies outside their runs)
            x[100] = 0.0
            x[100, s % channels] = 0.25                      # every channel but one is silent: not a silent frame
        silent.append(x)
        clipped.append(y)
    upload(b, silent)
    st, _ = check(b, silent, "silence", silence_min_frames=L, clip_min_samples=L)
    assert int(st[7]["leading_silence"]) == int(st[7]["trailing_silence"]) == F and int(st[0]["leading_silence"]) == 7
    check(b, silent, "silence, 100 ms")                      # the default minimum follows the rate
    upload(b, clipped)
    check(b, clipped, "clips", silence_min_frames=L, clip_min_samples=L)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 2. random masks
THRESHOLDS = {
    # name: (threshold, silent values, just not silent, clip level, clipped values, just not clipped)
    "digital": (0.0, [0.0, -0.0], [1e-45, -1e-45, 1e-39], 1.0, [1.0, -1.0, 1.5], [ONE_BELOW, -ONE_BELOW]),
    "at-threshold": (1e-3, [np.float32(1e-3), -np.float32(1e-3), 0.0, 5e-4], [np.nextafter(np.float32(1e-3), np.float32(1))], 0.5,
                     [0.5, -0.5, 0.75], [np.nextafter(np.float32(0.5), np.float32(0))]),
    "at-ceiling": (0.0, [0.0], [1e-45], 1.0, [1.0, -1.0], [ONE_BELOW, -ONE_BELOW]),
}


@pytest.mark.parametrize("case", sorted(THRESHOLDS))
@pytest.mark.parametrize("p", [0.02, 0.5, 0.98])
def test_random_masks(p, case):
    thr, quiet, near_quiet, lvl, hot, near_hot = THRESHOLDS[case]
    channels = {0.02: 1, 0.5: 2, 0.98: 3}[p] if case != "at-ceiling" else {0.02: 6, 0.5: 1, 0.98: 2}[p]
    T = tile_frames(channels)
    F = 2 * T + 71
    rng = np.random.default_rng(int(p * 100) + len(case))
    streams = []
    for _ in range(3):
        x = loud(rng, F, channels)
        r = rng.random((F, channels))
        for vals, sel in ((near_quiet, r < 0.05), (near_hot, (r >= 0.05) & (r < 0.1))):
            x[sel] = rng.choice(np.asarray(vals, np.float32), int(sel.sum()))
        is_quiet = rng.random((F, channels)) < p
        is_hot = ~is_quiet & (rng.random((F, channels)) < p)
        x[is_quiet] = rng.choice(np.asarray(quiet, np.float32), int(is_quiet.sum()))
        x[is_hot] = rng.choice(np.asarray(hot, np.float32), int(is_hot.sum()))
        streams.append(x)
    b = make_batch(48000, channels, 3, F)
    upload(b, streams)
    for least in (1, 3, 64, T + 5):
        check(b, streams, (case, p, least), max_events=64, silence_threshold=thr, clip_level=lvl, silence_min_frames=least, clip_min_samples=least)
    b.close()


def test_sixty_four_channels():
    """65 sequences: the carry's wave takes them in two rounds, and the clip list runs through both"""
    channels = 64
    T = tile_frames(channels)
    F = 2 * T + 71
    rng = np.random.default_rng(64)
    streams = []
    for _ in range(3):
        x = loud(rng, F, channels)
        x[rng.random(F) < 0.5] = 0.0
        x[rng.random((F, channels)) < 0.3] = -1.0
        streams.append(x)
    b = make_batch(48000, channels, 3, F)
    upload(b, streams)
    for cap in (256, 4096):                                  # the list ends inside an early channel's runs, or holds channel 63's too
        st, _ = check(b, streams, ("64 channels", cap), max_events=cap, silence_min_frames=2, clip_min_samples=2)
        assert 256 < int(st[0]["clip_runs"]) < 4096
    b.close()


# ------------------------------------------------------------------------------------------------------------ 3. ragged lengths
@pytest.mark.parametrize("channels", [2, 3])
def test_ragged_lengths_and_isolation(channels):
    T = tile_frames(channels)
    lengths = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7]
    slot = 2 * T + 7
    rng = np.random.default_rng(channels)
    b = make_batch(48000, channels, len(lengths), slot)
    pcm = np.tile(np.array([0.0, 2.0], np.float32), len(lengths) * slot * channels // 2 + 1)[:len(lengths) * slot * channels]
    pcm = pcm.reshape(len(lengths), slot, channels).copy()   # behind every stream's own length, and next to it: silent and clipped samples
    streams = []
    for s, n in enumerate(lengths):
        x = loud(rng, n, channels)
        x[n // 2:] = 0.0                                     # silence up to the stream's own last frame
        x[:n // 3, s % channels] = 1.0                       # a clip run from its frame 0
        pcm[s, :n] = x
        streams.append(x)
    b.upload(0, pcm)
    b.set_lengths(lengths)
    st, ch = check(b, streams, "ragged", silence_min_frames=1, clip_min_samples=1)
    assert st[0].tobytes() == np.array((0, 0, 0, 0, U64, 0, 0), STREAM_SCAN_DTYPE).tobytes()      # F_s == 0: zero or none
    assert (ch[0]["first_nonfinite"] == U64).all() and (ch[0]["longest_clip_at"] == U64).all() and (ch[0]["sum"] == 0).all()
    b.close()
    if channels == 2:                                        # ... and the same streams scanned alone, on the device
        for s, n in enumerate(lengths):
            if n:
                one = make_batch(48000, channels, 1, n)
                one.upload(0, streams[s])
                one.signal_scan(silence_min_frames=1, clip_min_samples=1)
                assert one.stream_scans()[0] == st[s] and one.channel_scans()[0].tobytes() == ch[s].tobytes(), (s, n)
                for kind in (SIGNAL_SILENCE, SIGNAL_CLIP):
                    assert np.array_equal(one.signal_events(0, kind), reference(streams[s], 0.0, 1.0, 1, 1)[2 + kind])
                one.close()


# ------------------------------------------------------------------------------------------------------------ 4. non-finite samples
@pytest.mark.parametrize("threshold", [0.0, float("inf")])
def test_nonfinite_samples(threshold):
    channels = 2
    T = tile_frames(channels)
    F = 2 * T + 71
    streams = []
    for bad in (np.nan, np.inf, -np.inf):
        x = np.zeros((F, channels), np.float32)
        x[:, 0] = 0.125
        x[:T // 2, 0] = 0.0                                  # silence from frame 0 ...
        x[T - 10:T + 10] = 0.0                               # ... across the tile seam ...
        x[F - 20:] = 0.0                                     # ... and to the last frame
        x[0:5, 1] = x[T - 10:T + 10, 1] = x[F - 20:, 1] = 1.0
        x[T - 10:T + 10, 0] = x[F - 20:, 0] = -1.0           # both channels clip across the seam and at the end
        x[0, 1] = x[T, 1] = x[F - 1, 1] = bad
        streams.append(x)
    b = make_batch(48000, channels, 3, F)
    upload(b, streams)
    st, ch = check(b, streams, ("nonfinite", threshold), silence_threshold=threshold, silence_min_frames=1, clip_min_samples=1)
    assert (ch[:, 1]["nonfinite"] == 3).all() and (ch[:, 1]["first_nonfinite"] == 0).all() and (ch[:, 0]["nonfinite"] == 0).all()
    assert (ch[:, 1]["sum"] == 5 - 1 + 20 - 1 + 20 - 1).all() and (ch[:, 1]["sum_sq"] == 42).all()      # the finite samples alone
    # a NaN is neither silent nor clipped: it splits the run across the seam; an infinity is clipped and, at +inf only, silent
    assert int(ch[0, 1]["clip_runs"]) == 4 and int(ch[0, 1]["longest_clip"]) == 19 and int(ch[1, 1]["longest_clip"]) == 20
    if threshold == 0.0:
        assert int(st[0]["leading_silence"]) == 0 and int(st[1]["trailing_silence"]) == 0
    else:
        assert int(st[0]["silent_frames"]) == F - 3 and int(st[1]["silent_frames"]) == int(st[2]["silent_frames"]) == F
    b.close()


# ------------------------------------------------------------------------------------------------------------ 5. sums
def test_sums():
    channels = 2
    T = tile_frames(channels)
    F = 2 * T + 71
    rng = np.random.default_rng(5)
    streams = [rng.uniform(-1, 1, (F, channels)).astype(np.float32), (0.3 + 0.1 * rng.standard_normal((F, channels))).astype(np.float32),
               np.full((F, channels), 0.25, np.float32)]
    b = make_batch(48000, channels, 3, F)
    upload(b, streams)
    _, ch = check(b, streams, "sums")                        # (the bound is check()'s)
    assert (ch[2]["sum"] == 0.25 * F).all() and (ch[2]["sum_sq"] == 0.0625 * F).all()
    b.close()


# ------------------------------------------------------------------------------------------------------------ 6. lists and the cap
def test_event_lists_and_the_cap():
    channels = 3
    T = tile_frames(channels)
    F = 2 * T + 71
    assert F > 5000
    rng = np.random.default_rng(6)
    x = loud(rng, F, channels)
    for i in range(40):
        x[50 + 100 * i:56 + 100 * i] = 0.0                   # 40 runs of 6 silent frames ...
        x[80 + 100 * i:82 + 100 * i] = 0.0                   # ... and 40 too short to count
    for c in range(channels):
        for i in range(25):
            x[10 + 200 * i + 7 * c:14 + 200 * i + 7 * c, c] = 1.0       # 25 runs of 4 clipped samples per channel
    streams = [x, loud(rng, F, channels), x[::-1].copy()]
    b = make_batch(48000, channels, 3, F)
    upload(b, streams)
    for cap in (0, 1, 39, 40, 65536):
        st, ch = check(b, streams, ("cap", cap), max_events=cap, silence_min_frames=5, clip_min_samples=3)
        assert int(st[0]["silence_runs"]) == 40 and int(st[0]["clip_runs"]) == 75 and (ch[0]["clip_runs"] == 25).all()       # the true totals
        n = ctypes.c_uint32(12345)
        out = np.zeros(max(cap, 1), SIGNAL_EVENT_DTYPE)
        for kind, total in ((SIGNAL_SILENCE, 40), (SIGNAL_CLIP, 75)):
            rc = L.lib().ss_batch_download_signal_events(b._h, 0, kind, out.ctypes.data_as(ctypes.POINTER(L.SignalEvent)), cap, ctypes.byref(n))
            assert rc == L.SS_OK and n.value == min(total, cap)
        assert b.signal_events(1, SIGNAL_SILENCE).size == 0 and b.signal_events(1, SIGNAL_CLIP).size == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------ 7. replacing, determinism
def downloads(b):
    out = [b.stream_scans().tobytes(), b.channel_scans().tobytes()]
    for s in range(int(b.cfg.n_streams)):
        out += [b.signal_events(s, SIGNAL_SILENCE).tobytes(), b.signal_events(s, SIGNAL_CLIP).tobytes()]
    return out


def test_replacing_and_determinism():
    channels = 2
    T = tile_frames(channels)
    F = 2 * T + 71
    rng = np.random.default_rng(7)

    def corpus():
        streams = []
        for _ in range(3):
            x = rng.uniform(-1.2, 1.2, (F, channels)).astype(np.float32)
            x[rng.random((F, channels)) < 0.4] = 0.0
            streams.append(x)
        return streams

    streams = corpus()
    b = make_batch(48000, channels, 3, F)
    upload(b, streams)
    b.signal_scan(silence_min_frames=2, clip_min_samples=1)
    first = downloads(b)
    b.signal_scan(silence_min_frames=2, clip_min_samples=1)
    assert downloads(b) == first                             # byte for byte
    check(b, streams, "second config", max_events=16, silence_threshold=0.5, clip_level=0.9, silence_min_frames=4, clip_min_samples=2)
    assert downloads(b) != first
    b.signal_scan(silence_min_frames=2, clip_min_samples=1)
    assert downloads(b) == first
    streams = corpus()
    upload(b, streams)
    check(b, streams, "new input", silence_min_frames=2, clip_min_samples=1)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 8. nothing else moves
def test_a_scan_moves_nothing_else():
    b = make_batch(48000, 2, 2, 48000, flags=L.SS_BATCH_ALL)
    b.synthesize(11)
    b.run()
    before = (b.checksums().tobytes(), bytes(b.results()), b.download_input(0).tobytes(), b.download_input(1).tobytes())
    b.signal_scan(silence_threshold=0.01, clip_level=0.5, silence_min_frames=1, clip_min_samples=1)
    x = [b.download_input(s).reshape(-1, 2) for s in range(2)]
    check(b, x, "behind a pass", silence_threshold=0.01, clip_level=0.5, silence_min_frames=1, clip_min_samples=1)
    assert (b.checksums().tobytes(), bytes(b.results()), b.download_input(0).tobytes(), b.download_input(1).tobytes()) == before
    b.close()
    b = make_batch(48000, 2, 2, 48000, flags=L.SS_BATCH_ALL)            # a batch that never ran a pass
    b.synthesize(11)
    check(b, x, "no pass", silence_threshold=0.01, clip_level=0.5, silence_min_frames=1, clip_min_samples=1)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_previous_results():
    channels = 2
    T = tile_frames(channels)
    F = 2 * T + 71
    rng = np.random.default_rng(9)
    x = rng.uniform(-1.2, 1.2, (F, channels)).astype(np.float32)
    x[rng.random((F, channels)) < 0.5] = 0.0
    lib = L.lib()
    b = make_batch(48000, channels, 2, F)
    upload(b, [x, x[::-1].copy()])
    st, ch, ev = np.zeros(2, STREAM_SCAN_DTYPE), np.zeros((2, channels), CHANNEL_SCAN_DTYPE), np.zeros(8, SIGNAL_EVENT_DTYPE)
    p_st, p_ch = st.ctypes.data_as(ctypes.POINTER(L.StreamScan)), ch.ctypes.data_as(ctypes.POINTER(L.ChannelScan))
    p_ev, n = ev.ctypes.data_as(ctypes.POINTER(L.SignalEvent)), ctypes.c_uint32(777)
    # a download before the first scan
    assert lib.ss_batch_download_stream_scans(b._h, p_st, 2) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_channel_scans(b._h, p_ch, 2 * channels) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_signal_events(b._h, 0, SIGNAL_SILENCE, p_ev, 8, ctypes.byref(n)) == L.SS_ERR_INVALID_MODE
    b.signal_scan(silence_min_frames=2, clip_min_samples=1, max_events=8)
    good = downloads(b)
    assert int(b.stream_scans()[0]["silence_runs"]) > 8      # (the lists are full)
    nan, inf = float("nan"), float("inf")
    bad = [(nan, 1.0, 1, 1, 8, 0), (-1e-9, 1.0, 1, 1, 8, 0), (0.0, nan, 1, 1, 8, 0), (0.0, 0.0, 1, 1, 8, 0), (0.0, -1.0, 1, 1, 8, 0),
           (0.0, 1.0, 0, 1, 8, 0), (0.0, 1.0, 1, 0, 8, 0), (0.0, 1.0, 1, 1, 65537, 0), (0.0, 1.0, 1, 1, 8, 1)]
    assert lib.ss_batch_signal_scan(b._h, None) == L.SS_ERR_INVALID_ARG
    for fields in bad:
        cfg = L.SignalScanConfig(*fields)
        assert lib.ss_batch_signal_scan(b._h, ctypes.byref(cfg)) == L.SS_ERR_INVALID_ARG, fields
        assert downloads(b) == good, fields
    assert lib.ss_batch_signal_scan(b._h, ctypes.byref(L.SignalScanConfig(inf, inf, 1, 1, 8, 0))) == L.SS_OK      # both are allowed
    b.signal_scan(silence_min_frames=2, clip_min_samples=1, max_events=8)
    assert downloads(b) == good
    # the downloads' own refusals write nothing
    for kind in (2, -1):
        assert lib.ss_batch_download_signal_events(b._h, 0, kind, p_ev, 8, ctypes.byref(n)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_signal_events(b._h, 2, SIGNAL_CLIP, p_ev, 8, ctypes.byref(n)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_signal_events(b._h, 0, SIGNAL_SILENCE, p_ev, 7, ctypes.byref(n)) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_stream_scans(b._h, p_st, 1) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_channel_scans(b._h, p_ch, 2 * channels - 1) == L.SS_ERR_CAPACITY
    assert n.value == 777 and not st.tobytes().strip(b"\0") and not ch.tobytes().strip(b"\0") and not ev.tobytes().strip(b"\0")
    assert downloads(b) == good
    b.close()
