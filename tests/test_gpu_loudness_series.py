"""Batch loudness series (SS_BATCH_LOUDNESS_SERIES): every stream's momentary and short-term loudness after each 100 ms sub-block,
and their maxima, against the crate's meter restated in the oracle — fed the stream s100 frames at a time, read after every call —
and against the product's own streaming handle.

Entry j is EbuR128::loudness_momentary() / loudness_shortterm() after the first (j + 1) s100 frames, the partial readings of the
first 0.3 s / 2.9 s included (the crate's ring starts zeroed); a non-finite sample poisons every window behind its sub-block.  The
maxima run over the full windows only (j >= 3, j >= 29), skip NaN, count infinities and take the first j of a tie.  Every
full-window energy is the one k_finalize fed its histograms, so the histograms are re-derived from the series bin for bin."""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_multich, make_stereo

pytestmark = pytest.mark.gpu

TOL_LU = 1e-6
AUTO, RUN_IN, WHOLE = L.SS_TD_AUTO, L.SS_TD_RUN_IN, L.SS_TD_WHOLE_STREAMS
SERIES = L.SS_BATCH_ALL | L.SS_BATCH_LOUDNESS_SERIES
NONE = 0xFFFFFFFF
BAD = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}


def s100_of(rate):
    return (rate + 5) // 10


def signal(seed, frames, channels, rate, level=0.4):
    return make_stereo(seed, frames, rate, level=level) if channels == 2 else make_multich(seed, frames, channels, rate, level=level)


def oracle_series(oracle, rate, channels, x, frames=None):
    """(momentary, shortterm) of the crate's meter after every whole sub-block of the first `frames` frames"""
    frames = x.size // channels if frames is None else frames
    s = s100_of(rate)
    n = frames // s
    m = oracle.Meter(channels, rate)
    mom, st = np.empty(n), np.empty(n)
    for j in range(n):
        m.add_frames(x[j * s * channels:(j + 1) * s * channels])
        mom[j], st[j] = m.momentary(), m.shortterm()
    return mom, st


def assert_same_series(got, ref, tag, tol=TOL_LU):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (tag, np.flatnonzero(np.isnan(got) != np.isnan(ref))[:8])
    assert np.array_equal(np.isinf(got), np.isinf(ref)), (tag, np.flatnonzero(np.isinf(got) != np.isinf(ref))[:8])
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), tag
    fin = np.isfinite(ref)
    if fin.any():
        d = np.abs(got[fin] - ref[fin])
        assert d.max() <= tol, (tag, float(d.max()), int(np.flatnonzero(fin)[d.argmax()]))


def expected_extreme(series, first):
    """numpy max and first argmax over the full windows j >= first, NaN skipped; (-inf, NONE) if there is no value"""
    v = np.asarray(series, np.float64)[first:]
    ok = ~np.isnan(v)
    if not ok.any():
        return -np.inf, NONE
    best = v[ok].max()
    return float(best), int(first + np.flatnonzero(ok & (v == best))[0])


def assert_extremes(e, mom, st, tag):
    vm, am = expected_extreme(mom, 3)
    vs, as_ = expected_extreme(st, 29)
    assert (e.max_momentary, e.max_momentary_at) == (vm, am), (tag, e.max_momentary, e.max_momentary_at, vm, am)
    assert (e.max_shortterm, e.max_shortterm_at) == (vs, as_), (tag, e.max_shortterm, e.max_shortterm_at, vs, as_)


def run_and_check(oracle, b, rate, channels, xs, tag):
    b.run(); b.sync()
    ext = b.loudness_extremes()
    for s, x in xs.items():
        mom, st = b.loudness_series(s)
        rm, rs = oracle_series(oracle, rate, channels, x, b.stream_shape(s).frames)
        assert_same_series(mom, rm, (tag, s, "momentary"))
        assert_same_series(st, rs, (tag, s, "shortterm"))
        assert_extremes(ext[s], mom, st, (tag, s))
    return ext


# ---------------------------------------------------------------- 1. rates x channel counts
@pytest.mark.parametrize("channels", [1, 2, 6, 8])
@pytest.mark.parametrize("rate", [44100, 48000, 96000])
def test_series_matches_the_crate(oracle, rate, channels):
    """4.35 s streams (not a whole number of sub-blocks): every entry of both series, partial readings included.  Six channels:
    index 3 is weight 0 (its samples are loud and must not count), the surrounds 1.41."""
    frames, ns = int(rate * 4.35), 3
    b = ssa.Batch(rate, channels, ns, frames, 4096, 1024, flags=SERIES)
    xs = {}
    for s in range(ns):
        x = signal(100 * channels + s, frames, channels, rate)
        if channels == 6:
            x.reshape(frames, 6)[:, 3] = np.float32(0.9)
        xs[s] = x
        b.upload(s, x)
    assert b.layout.n_subblocks == frames // s100_of(rate)
    run_and_check(oracle, b, rate, channels, xs, (rate, channels))


# ---------------------------------------------------------------- 1b. time-domain modes x overlap modes, the one-stream path
@pytest.mark.parametrize("overlap", [0, 1, 2])
@pytest.mark.parametrize("td_mode,channels", [(AUTO, 2), (RUN_IN, 2), (WHOLE, 2), (AUTO, 8), (RUN_IN, 8), (WHOLE, 8)])
def test_series_in_every_time_domain_and_overlap_mode(oracle, td_mode, channels, overlap):
    rate, frames, ns = 48000, 48000 * 12, 4
    b = ssa.Batch(rate, channels, ns, frames, 4096, 1024, flags=SERIES)
    b.set_time_domain_mode(td_mode)
    b.set_overlap(overlap)
    g = b.geometry
    if td_mode == WHOLE:
        assert (g.td_split, g.td_segments) == (1, 1)
    else:
        assert g.td_split != 1 and g.td_segments > 1, (g.td_split, g.td_segments)
    xs = {}
    for s in range(ns):
        xs[s] = signal(7000 + s, frames, channels, rate, level=0.2 + 0.1 * s)
        b.upload(s, xs[s])
    run_and_check(oracle, b, rate, channels, xs, (td_mode, channels, overlap))


def test_series_one_stream_batch(oracle):
    """one file: the time-domain kernel's td_split == 2 path (segments on eight waves) and the SMALL gating form"""
    rate, frames = 48000, 48000 * 10
    b = ssa.Batch(rate, 2, 1, frames, 4096, 1024, flags=SERIES)
    assert b.geometry.td_split == 2
    x = make_stereo(31, frames, rate, gap=True)
    b.upload(0, x)
    run_and_check(oracle, b, rate, 2, {0: x}, "one stream")


@pytest.mark.parametrize("ns,seconds", [(2, 65), (70, 110)])
def test_series_long_streams_loop(oracle, ns, seconds):
    """more sub-blocks than threads in a workgroup: 650 per stream in the SMALL form (256 threads), 1100 per stream in the
    big-grid form (1024 threads) — a thread walks several.  The meter alone (no spectrum, no peaks' flag)."""
    rate = 16000
    frames = rate * seconds
    b = ssa.Batch(rate, 1, ns, frames, 4096, 1024, flags=L.SS_BATCH_LUFS | L.SS_BATCH_LOUDNESS_SERIES)
    xs = {s: make_multich(90 + s, frames, 1, rate) for s in sorted({0, ns // 2, ns - 1})}
    buf = np.zeros((ns, frames), np.float32)
    for s, x in xs.items():
        buf[s] = x
    b.upload(0, buf.reshape(-1))
    run_and_check(oracle, b, rate, 1, xs, ("long", ns, seconds))


def test_series_with_columns_only_reference_gain(oracle):
    """columns-only spectrum with the reference's per-file gain: the whole meter chain runs first, the spectrum kernel last"""
    rate, frames, ns = 48000, 48000 * 6, 4
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=SERIES, spectrum_columns=64)
    xs = {}
    for s in range(ns):
        xs[s] = make_stereo(500 + s, frames, rate)
        b.upload(s, xs[s])
    run_and_check(oracle, b, rate, 2, xs, "columns")


# ---------------------------------------------------------------- 2. the product's streaming handle
@pytest.mark.parametrize("rate,channels", [(48000, 2), (44100, 6)])
def test_series_matches_the_streaming_handle(rate, channels):
    """ssa.Analyzer fed 100 ms per call: its momentary / short-term getters after every call are the series"""
    frames = int(rate * 4.2)
    s = s100_of(rate)
    x = signal(4242 + channels, frames, channels, rate)
    b = ssa.Batch(rate, channels, 1, frames, 4096, 1024, flags=SERIES)
    b.upload(0, x)
    b.run(); b.sync()
    mom, st = b.loudness_series(0)
    a = ssa.Analyzer()
    a.create_loudness_meter(channels, rate)
    hm, hs = np.empty(mom.size), np.empty(st.size)
    for j in range(mom.size):
        a.add_samples(x[j * s * channels:(j + 1) * s * channels])
        hm[j], hs[j] = a.get_momentary_lufs(), a.get_shortterm_lufs()
    assert_same_series(mom, hm, "handle momentary")
    assert_same_series(st, hs, "handle shortterm")


# ---------------------------------------------------------------- 3. ragged batches
def test_ragged_lengths(oracle):
    rate, slot = 48000, 48000 * 5
    lengths = [slot, int(0.35 * rate), int(2.55 * rate), int(4.567 * rate) + 13, 2000, 0, 30 * 4800, 4 * 4800 - 1]
    ns = len(lengths)
    b = ssa.Batch(rate, 2, ns, slot, 4096, 1024, flags=SERIES)
    b.set_lengths(lengths)
    xs = {}
    for s, f in enumerate(lengths):
        x = np.zeros(2 * slot, np.float32)
        x[:2 * f] = make_stereo(60 + s, slot, rate)[:2 * f]
        x[2 * f:] = np.float32(0.9)                 # the slot's tail is not part of the stream
        xs[s] = x
        b.upload(s, x)
    ext = run_and_check(oracle, b, rate, 2, xs, "ragged")
    for s, f in enumerate(lengths):
        n = f // 4800
        mom, st = b.loudness_series(s)
        assert b.stream_shape(s).n_subblocks == n and mom.size == n and st.size == n
        if n < 4:
            assert (ext[s].max_momentary, ext[s].max_momentary_at) == (-np.inf, NONE), (s, n)
        else:
            assert np.isfinite(ext[s].max_momentary) and 3 <= ext[s].max_momentary_at < n
        if n < 30:
            assert (ext[s].max_shortterm, ext[s].max_shortterm_at) == (-np.inf, NONE), (s, n)
        else:
            assert np.isfinite(ext[s].max_shortterm) and 29 <= ext[s].max_shortterm_at < n


# ---------------------------------------------------------------- 4. non-finite samples
@pytest.mark.parametrize("td_mode", [AUTO, RUN_IN, WHOLE])
def test_nonfinite_samples(oracle, td_mode):
    """The bench geometry (1024 x 10 s stereo: four segments of 25 sub-blocks, or whole streams).  One non-finite sample per
    stream at 1 s, at a segment boundary (last frame of segment 0, first frame of segment 1), in a sub-block's last frame (the
    +Inf window that holds a value) and in the last segment; the programme gets 21.6 dB louder behind the sample, so a window
    wrongly read behind it would raise the maxima."""
    rate, frames, ns = 48000, 480000, 1024
    seg = 25 * 4800
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=SERIES)
    b.synthesize(0x5EED0000, 0)
    b.set_time_domain_mode(td_mode)
    g = b.geometry
    if td_mode == WHOLE:
        assert (g.td_split, g.td_segments) == (1, 1)
    else:
        assert g.td_split == 0 and g.td_segments == 4 and g.td_segment_subblocks == seg // 4800
    cases = [(3, "nan", 48000, 0), (4, "+inf", 48000, 1), (5, "-inf", 48000, 0),
             (100, "nan", seg - 1, 1), (101, "+inf", seg - 1, 0), (102, "-inf", seg, 1), (103, "nan", seg, 0),
             (200, "+inf", 3 * seg + 4800 * 7 - 1, 1), (201, "nan", 3 * seg + 12345, 0)]
    xs = {}
    for s, kind, f, c in cases:
        x = make_stereo(1000 + s, frames, rate, level=1.0).reshape(frames, 2)
        step = min(f + 2400, frames - 1)
        x[:step] *= np.float32(0.05)
        x[step:] *= np.float32(0.6)
        x = x.reshape(-1).copy()
        x[2 * f + c] = BAD[kind]
        xs[s] = x
        b.upload(s, x)
    ext = run_and_check(oracle, b, rate, 2, xs, ("nonfinite", td_mode))
    for s, kind, f, c in cases:
        mom, st = b.loudness_series(s)
        bad = f // 4800
        assert np.isnan(mom[bad + 1:]).all() and np.isnan(st[bad + 1:]).all(), (s, kind)
        vm, am = expected_extreme(mom[:bad + 1], 3)
        assert (ext[s].max_momentary, ext[s].max_momentary_at) == (vm, am), (s, kind)
        if bad >= 29:
            vs, as_ = expected_extreme(st[:bad + 1], 29)
            assert (ext[s].max_shortterm, ext[s].max_shortterm_at) == (vs, as_), (s, kind)
        else:
            assert (ext[s].max_shortterm, ext[s].max_shortterm_at) == (-np.inf, NONE), (s, kind)


# ---------------------------------------------------------------- 5. extremes, and the histograms re-derived from the series
def test_extremes_ties_and_silence(oracle):
    """a silent stream reads -inf everywhere: an infinity counts as a value and every full window ties, so the maxima are -inf at
    the FIRST full window (not "none"); beside it a programme and the same 400 ms over and over (near-ties)"""
    rate, frames, ns = 48000, 48000 * 8, 3
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=SERIES)
    xs = {0: np.zeros(2 * frames, np.float32), 1: make_stereo(3, frames, rate)}
    period = make_stereo(4, 4 * 4800, rate)
    xs[2] = np.tile(period, frames // (4 * 4800))
    for s, x in xs.items():
        b.upload(s, x)
    ext = run_and_check(oracle, b, rate, 2, xs, "ties")
    assert (ext[0].max_momentary, ext[0].max_momentary_at, ext[0].max_shortterm, ext[0].max_shortterm_at) == (-np.inf, 3, -np.inf, 29)
    assert np.isfinite(ext[1].max_momentary) and np.isfinite(ext[1].max_shortterm)


def bins_of(values):
    """histogram bin of each LUFS value (ebur128: bin i holds [-70 + i/10, -70 + (i+1)/10), the top bin open above), and the values
    within 1e-9 LU of an edge (either neighbour is right for them)"""
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v) & (v >= -70.0 - 1e-9)]
    g = (v + 70.0) * 10.0
    near = np.abs(g - np.round(g)) < 1e-8
    idx = np.clip(np.floor(g), 0, 999).astype(np.int64)
    return idx[~near & (v >= -70.0)], v[near]


def assert_hist_from_series(hist, values, tag):
    idx, near = bins_of(values)
    want = np.bincount(idx, minlength=1000).astype(np.int64)
    diff = hist.astype(np.int64) - want
    assert (diff >= 0).all() and diff.sum() <= near.size, (tag, np.flatnonzero(diff)[:8], near)


@pytest.mark.parametrize("rate,channels", [(48000, 2), (44100, 6)])
def test_extremes_and_histograms_of_one_stream(oracle, rate, channels):
    frames = rate * 40
    b = ssa.Batch(rate, channels, 1, frames, 4096, 1024, flags=SERIES)
    x = signal(77 + channels, frames, channels, rate).reshape(frames, channels)
    x *= np.exp(np.linspace(np.log(0.02), np.log(1.0), frames, dtype=np.float32))[:, None]        # a slow fade-in: many bins
    x = x.reshape(-1).copy()
    b.upload(0, x)
    ext = run_and_check(oracle, b, rate, channels, {0: x}, ("hist", rate, channels))
    mom, st = b.loudness_series(0)
    assert_extremes(ext[0], mom, st, "one stream")
    hb, hs = b.histograms()
    assert_hist_from_series(hb, mom[3:], "block histogram")
    assert_hist_from_series(hs, st[29::10], "short-term histogram")
    assert hb.sum() > 300 and hs.sum() > 30


# ---------------------------------------------------------------- 6. the bench shape: nothing else moves
def test_bench_shape_outputs_unchanged(oracle):
    rate, frames, ns = 48000, 480000, 1024
    outs = []
    for flags in (L.SS_BATCH_ALL, SERIES):
        b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=flags)
        b.synthesize(0x5EED0000, 0)
        b.run(); b.sync()
        outs.append((bytes(b.results()), b.checksums().copy()))
        if flags == SERIES:
            ext = b.loudness_extremes()
            for s in range(0, ns, 127):
                x = b.download_input(s)
                mom, st = b.loudness_series(s)
                rm, rs = oracle_series(oracle, rate, 2, x)
                assert_same_series(mom, rm, (s, "momentary"))
                assert_same_series(st, rs, (s, "shortterm"))
                assert_extremes(ext[s], mom, st, s)
        b.close()
    assert outs[0][0] == outs[1][0], "ss_batch_results"
    assert np.array_equal(outs[0][1], outs[1][1]), "ss_batch_checksums"


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    lib = L.lib()
    with pytest.raises(ssa.AnalyzerError) as e:
        ssa.Batch(48000, 2, 2, 48000 * 2, 4096, 1024, flags=L.SS_BATCH_FFT | L.SS_BATCH_TRUE_PEAK | L.SS_BATCH_LOUDNESS_SERIES)
    assert e.value.code == L.SS_ERR_INVALID_ARG
    dp = ctypes_double_p()
    plain = ssa.Batch(48000, 2, 2, 48000 * 2, 4096, 1024, flags=L.SS_BATCH_ALL)
    plain.synthesize(); plain.run(); plain.sync()
    buf = np.empty(64, np.float64)
    assert lib.ss_batch_download_loudness_series(plain._h, 0, buf.ctypes.data_as(dp), None, 64) == L.SS_ERR_INVALID_MODE
    ext = (L.LoudnessExtremes * 2)()
    assert lib.ss_batch_loudness_extremes(plain._h, ext, 2) == L.SS_ERR_INVALID_MODE
    b = ssa.Batch(48000, 2, 2, 48000 * 2, 4096, 1024, flags=SERIES)
    b.synthesize(); b.run(); b.sync()
    assert lib.ss_batch_download_loudness_series(b._h, 0, buf.ctypes.data_as(dp), None, 19) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_loudness_series(b._h, 0, None, buf.ctypes.data_as(dp), 20) == L.SS_OK
    assert lib.ss_batch_download_loudness_series(b._h, 2, buf.ctypes.data_as(dp), None, 64) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_loudness_extremes(b._h, ext, 1) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_loudness_extremes(b._h, ext, 2) == L.SS_OK
    assert np.array_equal(buf[:20], b.loudness_series(0)[1])


def ctypes_double_p():
    import ctypes
    return ctypes.POINTER(ctypes.c_double)
