"""Batch peak series and peak regions (ss_batch_peak_series, ss_batch_peak_regions): the true and sample peak of every 100 ms entry
of every stream, the frame that attains each, and their maxima over ranges and groups.

Reference for true_peak: the f64 polyphase sum over tests/_f64ref.interpolator_taps — y_f[n] = sum_d taps[d factor + f] x[n - d],
x[n] = 0 for n < 0, branch 0 the sample itself — with the crate's capture from 0 (a NaN output is skipped, an infinity counts, the
first frame wins).  Each entry must satisfy |got - ref| <= 1e-4 ref (rel_close, the bar the pass's true peak is held to);
sample_peak and its frame must be exact; true_peak_frame must be exact wherever the reference's maximum is unambiguous (every other
frame of the entry at least 1 % below it) and wherever the input makes the arithmetic exact (impulses on silence).  The worst
observed ratio is printed (run with -s)."""
import ctypes

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from _f64ref import interpolator_taps, subblock_frames

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NO_GROUP = L.SS_REGION_NO_GROUP
REL = 1e-4
WORST = {"ratio": 0.0}


def factor_of(rate, forced=0):
    return forced if forced else (4 if rate < 96000 else 2 if rate < 192000 else 0)


def frame_maxima(x, factor):
    """[frames][channels] f64: max over the branches of every frame (NaN branches skipped; NaN where all are), x [frames][channels]"""
    x = np.asarray(x, np.float32).astype(np.float64)
    v = np.abs(x)
    if factor:
        taps = interpolator_taps(factor)
        nt = 12 if factor == 4 else 24
        with np.errstate(invalid="ignore", over="ignore"):
            for f in range(1, factor):
                y = np.zeros_like(x)
                for d in range(nt - 1, -1, -1):
                    sh = np.zeros_like(x)
                    sh[d:] = x[:x.shape[0] - d] if d else x
                    y = y + taps[d * factor + f] * sh
                v = np.fmax(v, np.abs(y))
    return v


def capture(v, S):
    """per (entry, channel) of per-frame values v [frames][channels]: (max from 0, first frame attaining it or NONE, unambiguous)"""
    F, C = v.shape
    E = (F + S - 1) // S
    val, at, clear = np.zeros((E, C)), np.full((E, C), NONE, np.int64), np.ones((E, C), bool)
    for j in range(E):
        seg = v[j * S:(j + 1) * S]
        m = np.where(np.isnan(seg), 0.0, seg)
        best = m.max(axis=0)
        for c in range(C):
            if best[c] > 0.0:
                val[j, c] = best[c]
                at[j, c] = int(np.flatnonzero(m[:, c] == best[c])[0])
                others = np.delete(m[:, c], at[j, c])
                clear[j, c] = (not others.size) or others.max() <= 0.99 * best[c]
    return val, at, clear


def reference(x, channels, rate, factor, frames=None):
    x = np.asarray(x, np.float32).reshape(-1, channels)
    if frames is not None:
        x = x[:frames]
    S = subblock_frames(rate)
    tp = capture(frame_maxima(x, factor), S)
    sp = capture(np.abs(x.astype(np.float64)), S)
    return tp, sp


def check_series(got, ref, tag, exact=False):
    """one stream's downloaded series [entries][channels] against reference(); exact: the input makes every sum exact"""
    (tv, ta, tclear), (sv, sa, _) = ref
    assert got.shape == tv.shape, (tag, got.shape, tv.shape)
    assert np.array_equal(got["sample_peak"], sv.astype(np.float32)), (tag, "sample_peak")
    assert np.array_equal(got["sample_peak_frame"].astype(np.int64), sa), (tag, "sample_peak_frame")
    g = got["true_peak"].astype(np.float64)
    fin = np.isfinite(tv)
    assert np.array_equal(g[~fin], tv[~fin]), (tag, "non-finite true_peak")
    err = np.abs(g[fin] - tv[fin])
    if fin.any() and (tv[fin] > 0).any():
        WORST["ratio"] = max(WORST["ratio"], float((err[tv[fin] > 0] / tv[fin][tv[fin] > 0]).max()))
    assert (err <= REL * tv[fin]).all(), (tag, "true_peak", float((err / np.maximum(tv[fin], 1e-300)).max()))
    if exact:
        assert np.array_equal(got["true_peak"], tv.astype(np.float32)), (tag, "exact true_peak")
    sure = np.ones_like(tclear) if exact else tclear
    assert np.array_equal(got["true_peak_frame"].astype(np.int64)[sure], ta[sure]), (tag, "true_peak_frame")
    print(f"{tag}: worst |got - ref| / ref so far {WORST['ratio']:.3e}")
    return int(sure.sum())


def noise(seed, frames, channels, level=0.1):
    return (level * np.random.default_rng(seed).uniform(-1, 1, (frames, channels))).astype(np.float32)


def plant(x, rng, S, every=2, gain=0.9):
    """isolated events: in every `every`-th entry one sample of one channel at +-gain, at the entry's first, last or a random frame.
    Over noise of 0.03 the frames beside it reach at most 0.9 gain + 0.05 (the largest tap and the noise's own ringing), more than
    1 % below it"""
    F, C = x.shape
    for j in range(0, (F + S - 1) // S, every):
        lo, hi = j * S, min((j + 1) * S, F)
        n = [lo, hi - 1, int(rng.integers(lo, hi))][int(rng.integers(0, 3))]
        x[n, int(rng.integers(0, C))] = gain * (1 if rng.integers(0, 2) else -1)
    return x


def make_batch(rate, channels, streams, frames, forced=0, flags=L.SS_BATCH_TRUE_PEAK):
    return ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=flags, true_peak_factor=forced)


# ------------------------------------------------------------------------------------------------------------ shapes
SHAPES = [(44100, 0, 1), (48000, 0, 2), (48000, 0, 3), (96000, 0, 8), (192000, 0, 2), (96000, 4, 3), (96000, 4, 8)]


@pytest.mark.parametrize("rate,forced,channels", SHAPES)
def test_noise_and_events_against_f64_oracle_and_pass(oracle, rate, forced, channels):
    S, factor = subblock_frames(rate), factor_of(rate, forced)
    frames, streams = int(0.37 * rate) + 13, 3
    rng = np.random.default_rng(rate + 7 * channels + forced)
    xs = [plant(noise(100 * s + channels, frames, channels, level=0.03), rng, S) for s in range(streams)]
    b = make_batch(rate, channels, streams, frames, forced, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    b.upload(0, np.concatenate([x.reshape(-1) for x in xs]))
    tile, cap = b.peak_series_plan()
    assert cap == (frames + S - 1) // S == 4 and 0 < tile <= S and tile * channels <= 8192
    b.peak_series()
    series = [b.peak_series_of(s) for s in range(streams)]
    sure = 0
    for s in range(streams):
        sure += check_series(series[s], reference(xs[s], channels, rate, factor), f"{rate}/{factor}/{channels}ch stream {s}")
    assert sure >= streams * 2                           # the planted entries are position-checked
    # the running maximum of stream 0's entries against the crate's meter fed sub-block by sub-block
    m = oracle.Meter(channels, rate, forced)
    run = np.zeros(channels)
    for j in range(frames // S):
        m.add_frames(xs[0][j * S:(j + 1) * S].reshape(-1))
        run = np.maximum(run, series[0]["true_peak"][j].astype(np.float64))
        for c in range(channels):
            want = m.true_peak(c)
            assert abs(run[c] - want) <= REL * want, (j, c, run[c], want)
    # the pass: its sample peak bit for bit, its true peak within the bar; and it does not notice the series
    b.run()
    res_a, sums_a = bytes(b.results()), b.checksums().tobytes()
    for s in range(streams):
        tp, sp = b.peaks(s)
        assert np.array_equal(series[s]["sample_peak"].max(axis=0).astype(np.float64), sp), (s, "sample peak of the pass")
        mine = series[s]["true_peak"].max(axis=0).astype(np.float64)
        assert (np.abs(mine - tp) <= REL * tp).all(), (s, mine, tp)
    b.peak_series()
    b.run()
    b.peak_series()
    assert bytes(b.results()) == res_a and b.checksums().tobytes() == sums_a
    for s in range(streams):
        assert b.peak_series_of(s).tobytes() == series[s].tobytes()
    b.close()


# ------------------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("rate,forced,channels", [(48000, 0, 2), (96000, 0, 1), (96000, 4, 8)])
def test_impulses_at_entry_tile_and_stream_edges(rate, forced, channels):
    S, factor = subblock_frames(rate), factor_of(rate, forced)
    H = 11 if factor == 4 else 23
    frames = 2 * S + 7
    probe = make_batch(rate, channels, 1, frames, forced)
    tile, _ = probe.peak_series_plan()
    probe.close()
    at = [0, S - 1, tile - 1, tile, tile + H, S + tile - 1, S + tile, frames - 1]
    xs = np.zeros((len(at), frames, channels), np.float32)
    for s, n in enumerate(at):
        xs[s, n, s % channels] = 1.0
    b = make_batch(rate, channels, len(at), frames, forced)
    b.upload(0, xs.reshape(-1))
    b.peak_series()
    taps = interpolator_taps(factor)
    ring = np.float32(max(np.abs(taps[f::factor][:H + 1]).max() for f in range(1, factor)))
    for s, n in enumerate(at):
        got = b.peak_series_of(s)
        check_series(got, reference(xs[s], channels, rate, factor), f"impulse at {n}", exact=True)
        c, j, off = s % channels, n // S, n % S
        assert (got["true_peak"][j, c], got["sample_peak"][j, c]) == (1.0, 1.0)
        assert (got["true_peak_frame"][j, c], got["sample_peak_frame"][j, c]) == (off, off)
        silent = np.delete(got[:, :], c, axis=1)
        assert not silent["true_peak"].any() and (silent["true_peak_frame"] == NONE).all()
    # the impulse at the last frame of entry 0: entry 1 holds its ringing alone
    got = b.peak_series_of(1)
    assert got["sample_peak"][1, 1 % channels] == 0.0 and got["sample_peak_frame"][1, 1 % channels] == NONE
    assert got["true_peak"][1, 1 % channels] == ring and 0 < ring < 1
    b.close()


# ------------------------------------------------------------------------------------------------------------ isolation
def test_stream_isolation_and_ragged_lengths():
    rate, channels = 48000, 3
    S = subblock_frames(rate)
    lengths = [0, 1, S - 1, S, S + 1, 2 * S + 7, S + 5, 2 * S]
    slot = 2 * S + 40
    xs = np.empty((len(lengths), slot, channels), np.float32)
    for s, n in enumerate(lengths):
        xs[s] = noise(40 + s, slot, channels)
        xs[s, n:] = np.where(np.arange(slot - n)[:, None] % 2, -1.0, 1.0)       # full-scale garbage behind the stream's own length
    xs[6, :40] = 0.0                                     # a silent head behind stream 5's garbage ...
    xs[7, :S] = 0.0                                      # ... and a silent first entry behind full-scale samples of stream 6
    b = make_batch(rate, channels, len(lengths), slot)
    b.upload(0, xs.reshape(-1))
    b.set_lengths(lengths)
    b.peak_series()
    for s, n in enumerate(lengths):
        got = b.peak_series_of(s)
        assert got.shape == ((n + S - 1) // S, channels)
        check_series(got, reference(xs[s], channels, rate, 4, n), f"ragged stream {s} of {n} frames")
        if n:
            assert got["sample_peak"].max() <= 0.1       # the garbage is never seen
            tail = n - (got.shape[0] - 1) * S
            assert (got["sample_peak_frame"][-1] < tail).all()
    got = b.peak_series_of(7)
    assert not got["true_peak"][0].any() and (got["true_peak_frame"][0] == NONE).all() and (got["sample_peak_frame"][0] == NONE).all()
    b.close()
    # full-length streams: full scale in the last 24 frames of stream 0, a silent head of stream 1
    x = np.stack([noise(1, slot, channels), noise(2, slot, channels)])
    x[0, -24:] = 1.0
    x[1, :S] = 0.0
    b = make_batch(rate, channels, 2, slot)
    b.upload(0, x.reshape(-1))
    b.peak_series()
    got = b.peak_series_of(1)
    assert not got["true_peak"][0].any() and not got["sample_peak"][0].any()
    assert (got["true_peak_frame"][0] == NONE).all() and (got["sample_peak_frame"][0] == NONE).all()
    check_series(got, reference(x[1], channels, rate, 4), "stream behind a loud tail")
    b.close()


# ------------------------------------------------------------------------------------------------------------ non-finite
@pytest.fixture(scope="module")
def clean():
    rate, channels, streams = 48000, 2, 3
    frames = 2 * subblock_frames(rate) + 300
    xs = np.stack([noise(70 + s, frames, channels) for s in range(streams)])
    b = make_batch(rate, channels, streams, frames)
    b.upload(0, xs.reshape(-1))
    b.peak_series()
    base = [b.peak_series_of(s) for s in range(streams)]
    yield rate, channels, xs, b, base
    b.close()


S48 = 4800
PLANTS = {"nan": [(S48 + 100, np.nan)], "nan at an entry's end": [(S48 - 3, np.nan)], "+inf": [(S48 + 100, np.inf)],
          "+inf in an entry's last frames": [(S48 - 5, np.inf)], "+inf and -inf": [(S48 - 8, np.inf), (S48 - 3, -np.inf)]}


@pytest.mark.parametrize("kind", list(PLANTS))
def test_non_finite_samples(clean, kind):
    rate, channels, xs, b, base = clean
    x = xs.copy()
    for n, v in PLANTS[kind]:
        x[1, n, 0] = v
    b.upload(0, x.reshape(-1))
    b.peak_series()
    got = b.peak_series_of(1)
    check_series(got, reference(x[1], channels, rate, 4), kind)
    if "nan" in kind:
        n = PLANTS[kind][0][0]
        want = np.abs(np.delete(x[1, (n // S48) * S48:(n // S48 + 1) * S48, 0], n % S48)).max()
        assert got["sample_peak"][n // S48, 0] == want                # its own sample peak ignores it
    if kind == "+inf in an entry's last frames":
        assert np.isinf(got["true_peak"][0, 0]) and np.isinf(got["sample_peak"][0, 0]) and np.isinf(got["true_peak"][1, 0])
        assert got["true_peak_frame"][0, 0] == S48 - 5 == got["sample_peak_frame"][0, 0] and got["true_peak_frame"][1, 0] == 0
        assert np.isfinite(got["sample_peak"][1, 0])
    # the other channel and the other streams: byte for byte what they were without the plant
    assert got[:, 1].tobytes() == base[1][:, 1].tobytes()
    for s in (0, 2):
        assert b.peak_series_of(s).tobytes() == base[s].tobytes()
    b.upload(0, xs.reshape(-1))


# ------------------------------------------------------------------------------------------------------------ ties and regions
def region_ref(series, S, a, n, ceiling):
    """a region's record from the stream's downloaded series, on the host: the tie rule spelled out"""
    out = {}
    for key in ("true_peak", "sample_peak"):
        best, where = 0.0, (None, None)
        for j in range(a, a + n):
            for c in range(series.shape[1]):
                v, f = float(series[key][j, c]), j * S + int(series[key + "_frame"][j, c])
                if v > best or (v == best and v > 0 and (f, c) < where):
                    best, where = v, (f, c)
        out[key] = (best, where[0] if best > 0 else 0xFFFFFFFFFFFFFFFF, where[1] if best > 0 else NONE)
    over = [j for j in range(a, a + n) if (series["true_peak"][j].astype(np.float64) > ceiling).any()]
    out["over"] = (len(over), over[0] if over else NONE)
    ch = series[a:a + n]
    out["channels"] = (ch["true_peak"].max(axis=0, initial=0), ch["sample_peak"].max(axis=0, initial=0))
    return out


def check_regions(b, rows, series, S, ceiling, n_groups):
    res = b.region_peaks()
    ch_t, ch_s = b.region_channel_peaks()
    assert len(res) == len(rows) and ch_t.shape == (len(rows), series[0].shape[1])
    groups = [dict(t=(0.0, NONE), s=(0.0, NONE), over=0) for _ in range(n_groups)]
    for i, (s, a, n, g) in enumerate(rows):
        want, r = region_ref(series[s], S, a, n, ceiling), res[i]
        assert (r.true_peak, r.true_peak_frame, r.true_peak_channel) == want["true_peak"], (i, rows[i])
        assert (r.sample_peak, r.sample_peak_frame, r.sample_peak_channel) == want["sample_peak"], (i, rows[i])
        assert (r.n_over, r.first_over) == want["over"], (i, rows[i], ceiling)
        assert np.array_equal(ch_t[i], want["channels"][0]) and np.array_equal(ch_s[i], want["channels"][1])
        if g != NO_GROUP:
            if r.true_peak > groups[g]["t"][0]:
                groups[g]["t"] = (r.true_peak, i)
            if r.sample_peak > groups[g]["s"][0]:
                groups[g]["s"] = (r.sample_peak, i)
            groups[g]["over"] += r.n_over
    got = b.group_peaks()
    assert len(got) == n_groups
    for g in range(n_groups):
        assert (got[g].true_peak, got[g].true_peak_region) == groups[g]["t"], g
        assert (got[g].sample_peak, got[g].sample_peak_region) == groups[g]["s"], g
        assert got[g].n_over == groups[g]["over"], g
    return res, got


def test_ties_go_to_the_lowest_frame_channel_entry_and_region():
    rate, channels, S = 48000, 2, 4800
    frames = 4 * S
    x = np.zeros((3, frames, channels), np.float32)
    x[0, 700, 0] = x[0, 3100, 0] = 0.5                   # one entry, two equal samples: the lower frame
    x[0, S + 50, 1] = x[0, S + 50, 0] = 0.5              # the same frame on both channels: channel 0 ...
    x[0, 2 * S + 90, 0] = 0.5
    x[0, 2 * S + 60, 1] = 0.5                            # ... but the lower frame on channel 1 comes first
    x[1, 3 * S + 5, 1] = 0.5
    x[2, 10, 0] = 0.25
    b = make_batch(rate, channels, 3, frames)
    b.upload(0, x.reshape(-1))
    b.peak_series()
    series = [b.peak_series_of(s) for s in range(3)]
    for s in range(3):
        check_series(series[s], reference(x[s], channels, rate, 4), f"ties stream {s}", exact=True)
    assert series[0]["true_peak_frame"][0, 0] == 700 == series[0]["sample_peak_frame"][0, 0]
    rows = [(0, 0, 4, 0), (0, 1, 1, 1), (0, 2, 1, 1), (0, 1, 3, NO_GROUP), (1, 0, 4, 0), (0, 0, 1, 0), (2, 0, 4, 2), (2, 1, 3, 2)]
    b.peak_regions(rows, 4, 0.3)
    res, grp = check_regions(b, rows, series, S, 0.3, 4)
    assert (res[0].sample_peak_frame, res[0].sample_peak_channel) == (700, 0)             # lowest entry
    assert (res[1].sample_peak_frame, res[1].sample_peak_channel) == (S + 50, 0)          # lowest channel
    assert (res[2].sample_peak_frame, res[2].sample_peak_channel) == (2 * S + 60, 1)      # lowest frame before lowest channel
    assert (res[3].sample_peak_frame, res[3].sample_peak_channel) == (S + 50, 0)
    assert grp[0].sample_peak_region == 0 and grp[1].sample_peak_region == 1              # lowest region among equals
    assert (grp[3].true_peak, grp[3].true_peak_region, grp[3].n_over) == (0.0, NONE, 0)   # a group nobody names
    assert (res[7].true_peak, res[7].true_peak_frame, res[7].true_peak_channel) == (0.0, 0xFFFFFFFFFFFFFFFF, NONE)
    b.close()


def test_regions_groups_overs_and_changing_lists():
    rate, channels = 48000, 3
    S = subblock_frames(rate)
    lengths = [6 * S + 17, 5 * S, 3 * S + 1, 0]
    slot = 6 * S + 17
    rng = np.random.default_rng(5)
    xs = np.stack([noise(90 + s, slot, channels) for s in range(len(lengths))])
    for s, j, c, v in [(0, 1, 0, 0.5), (0, 4, 2, 0.8), (0, 6, 1, 0.3), (1, 0, 1, 0.5), (1, 3, 0, 0.9), (2, 3, 2, 0.7)]:
        xs[s, min(j * S + int(rng.integers(0, S)), lengths[s] - 1), c] = v
    b = make_batch(rate, channels, len(lengths), slot)
    b.upload(0, xs.reshape(-1))
    b.set_lengths(lengths)
    b.peak_series()
    series = [b.peak_series_of(s) for s in range(len(lengths))]
    entries = [(n + S - 1) // S for n in lengths]
    assert [x.shape[0] for x in series] == entries == [7, 5, 4, 0]
    whole = [(s, 0, entries[s], 0) for s in range(4)]
    sliding = [(0, a, 3, 1) for a in range(5)] + [(1, a, 2, 2) for a in range(4)]
    rows = whole + sliding + [(0, 6, 1, NO_GROUP), (2, 2, 2, 1), (1, 2, 0, 2), (0, 7, 0, 0), (0, 0, 7, 0), (1, 0, 5, 1)]
    for ceiling in (0.6, np.inf, 0.0):                   # between two planted peaks; nothing over; every entry with a sample
        b.peak_regions(rows, 3, ceiling)
        res, _ = check_regions(b, rows, series, S, ceiling, 3)
        assert res[0].true_peak == float(series[0]["true_peak"].max()) and res[0].n_over == {0.6: 1, np.inf: 0, 0.0: 7}[ceiling]
    short = rows[:2]
    b.peak_regions(short, 1)                             # a shorter list, then a longer one than any before
    check_regions(b, short, series, S, np.inf, 1)
    longer = rows + rows[::-1] + sliding
    b.peak_regions(np.array(longer, np.uint32), 5, 0.45)
    check_regions(b, longer, series, S, 0.45, 5)
    b.peak_regions([], 0)
    assert len(b.region_peaks()) == 0 and len(b.group_peaks()) == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------ refusals, determinism
def test_refusals():
    rate, channels, S = 48000, 2, 4800
    frames = 2 * S + 9                                   # three entries, two sub-blocks
    lib = L.lib()
    b = make_batch(rate, channels, 2, frames)
    b.upload(0, noise(3, 2 * frames, channels).reshape(-1))
    rows = (L.LoudnessRegion * 2)((0, 0, 3, 0), (1, 1, 2, NO_GROUP))
    ent, rp, gp = (L.PeakEntry * (3 * channels))(), (L.RegionPeaks * 2)(), (L.GroupPeaks * 1)()
    f = (ctypes.c_float * (2 * channels))()
    n = ctypes.c_uint32()
    inf = float("inf")
    # before the first computation
    assert lib.ss_batch_download_peak_series(b._h, 0, ent, 3, ctypes.byref(n)) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_peak_regions(b._h, rows, 2, 1, inf) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_peak_series(b._h) == L.SS_OK
    assert lib.ss_batch_download_region_peaks(b._h, rp, 2) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_group_peaks(b._h, gp, 1) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_region_channel_peaks(b._h, f, f, 2 * channels) == L.SS_ERR_INVALID_MODE
    # the series' download
    assert lib.ss_batch_download_peak_series(b._h, 2, ent, 3, None) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_peak_series(b._h, 0, ent, 2, None) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_peak_series(b._h, 0, ent, 3, ctypes.byref(n)) == L.SS_OK and n.value == 3
    # the list
    assert lib.ss_batch_peak_regions(b._h, rows, 2, 1, inf) == L.SS_OK
    for bad in [(2, 0, 1, 0), (0, 3, 1, 0), (0, 0, 4, 0), (0, 0xFFFFFFFF, 2, 0), (0, 0, 1, 1), (0, 0, 1, 0xFFFFFFFE)]:
        one = (L.LoudnessRegion * 1)(bad)
        assert lib.ss_batch_peak_regions(b._h, one, 1, 1, inf) == L.SS_ERR_INVALID_ARG, bad
    for ceiling in (float("nan"), -1.0, -inf):
        assert lib.ss_batch_peak_regions(b._h, rows, 2, 1, ceiling) == L.SS_ERR_INVALID_ARG, ceiling
    assert lib.ss_batch_peak_regions(b._h, None, 1, 0, inf) == L.SS_ERR_INVALID_ARG
    # a refused call leaves the previous list; small caps
    assert lib.ss_batch_download_region_peaks(b._h, rp, 1) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_group_peaks(b._h, gp, 0) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_region_channel_peaks(b._h, f, None, 2 * channels - 1) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_region_peaks(b._h, rp, 2) == L.SS_OK and rp[0].true_peak > 0 and rp[1].first_over == NONE
    assert lib.ss_batch_download_region_channel_peaks(b._h, None, f, 2 * channels) == L.SS_OK and f[0] > 0
    assert lib.ss_batch_download_region_channel_peaks(b._h, f, None, 2 * channels) == L.SS_OK
    # the tail entry is a valid region; an empty list and an empty region are valid
    tail = (L.LoudnessRegion * 2)((0, 2, 1, 0), (1, 3, 0, 0))
    assert lib.ss_batch_peak_regions(b._h, tail, 2, 1, 0.0) == L.SS_OK
    assert lib.ss_batch_download_region_peaks(b._h, rp, 2) == L.SS_OK
    assert rp[0].n_over == 1 and rp[0].first_over == 2 and 2 * S <= rp[0].sample_peak_frame < frames
    assert (rp[1].true_peak, rp[1].true_peak_channel, rp[1].n_over) == (0.0, NONE, 0)
    assert lib.ss_batch_peak_regions(b._h, None, 0, 0, inf) == L.SS_OK
    assert lib.ss_batch_download_region_peaks(b._h, None, 0) == L.SS_OK and lib.ss_batch_download_group_peaks(b._h, None, 0) == L.SS_OK
    b.close()


def test_two_calls_agree_byte_for_byte():
    rate, channels, streams = 44100, 2, 4
    S = subblock_frames(rate)
    frames = 5 * S + 100
    b = make_batch(rate, channels, streams, frames)
    b.upload(0, noise(11, streams * frames, channels).reshape(-1))
    rows = [(s, a, n, (s + a) % 3) for s in range(streams) for a, n in ((0, 6), (1, 3), (2, 4), (5, 1))]

    def everything():
        b.peak_series()
        b.peak_regions(rows, 3, 0.099)
        ch = b.region_channel_peaks()
        return [b.peak_series_of(s).tobytes() for s in range(streams)] + [bytes(b.region_peaks()), bytes(b.group_peaks()),
                                                                           ch[0].tobytes(), ch[1].tobytes()]
    first = everything()
    assert everything() == first
    assert any(g.n_over for g in b.group_peaks())
    b.close()
