"""Batch gain (ss_batch_apply_gain, Batch.normalise): the resident corpus times a gain curve per stream, in place, and the records
the sweep leaves.

The reference is numpy, in this file: the curve is gain_envelope(points, arange(F)) (held in bits against the library's
ss_gain_envelope by tests/test_apply_gain_abi.py), the samples are (x.astype(f64) * g[:, None]).astype(f32) — one rounded f64
multiplication and one round-to-nearest conversion, what the header defines — and the records are a few lines of integer numpy.
Everything must be EQUAL: corpora byte for byte where the reference is finite and NaN for NaN elsewhere (a NaN's payload is
unspecified in touched frames), records byte for byte.  Frames behind a stream's own length, unselected channels and streams without
a point must come back as the bytes that were uploaded, signalling NaNs and negative zeros included."""
import ctypes
import math

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import GAIN_CHANNEL_DTYPE, GAIN_POINT_DTYPE, gain_envelope, normalisation_gain

pytestmark = pytest.mark.gpu

U64_MAX = 0xFFFFFFFFFFFFFFFF
FILL = 0.5                                  # what lies behind a stream's own length in its slot


def make_batch(rate, channels, streams, frames, flags=L.SS_BATCH_TRUE_PEAK):
    return ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=flags)


@pytest.fixture(scope="module")
def tile():
    b = make_batch(48000, 2, 1, 64)
    t = b.apply_gain_plan()
    b.close()
    assert t > 0
    return t


def noise(rng, frames, channels, level=1.0):
    return (level * rng.uniform(-1.0, 1.0, (frames, channels))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ reference
def ref_samples(x, pts, mask):
    """x [F][C] f32, pts [(frame, gain)] of this stream -> the product, unselected channels as they are"""
    F, C = x.shape
    p = np.zeros(len(pts), GAIN_POINT_DTYPE)
    for i, (frame, gain) in enumerate(pts):
        p[i] = (frame, 0, gain)
    g = gain_envelope(p, np.arange(F, dtype=np.uint64))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = (x.astype(np.float64) * g[:, None]).astype(np.float32)
    out = x.copy()
    for c in range(C):
        if mask == 0 or mask >> c & 1:
            out[:, c] = y[:, c]
    return out


def ref_records(y, clip, touched):
    """the records of one stream's frames y [F][C] as they are behind the call"""
    F, C = y.shape
    rec = np.zeros(C, GAIN_CHANNEL_DTYPE)
    rec["first_over"] = U64_MAX
    if not touched:
        return rec
    rec["touched"] = 1
    bits = y.view(np.uint32) & 0x7FFFFFFF                                       # |y| as integers: they order as the values do
    clip_bits = int(np.float32(clip).view(np.uint32))
    for c in range(C):
        a = bits[:, c]
        finite, over = a < 0x7F800000, (a >= clip_bits) & (a <= 0x7F800000) & (not math.isinf(clip))
        rec[c]["sample_peak"] = np.uint32(a[finite].max() if finite.any() else 0).view(np.float32)
        rec[c]["n_over"] = int(over.sum())
        rec[c]["first_over"] = int(np.argmax(over)) if over.any() else U64_MAX
        rec[c]["n_nonfinite"] = int((~finite).sum())
    return rec


def same_corpus(got, ref, tag):
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN positions")
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~nan
    assert not bad.any(), (tag, np.argwhere(bad)[:4], got[bad][:4], ref[bad][:4])


def apply_and_check(b, streams, points, tag, mask=0, clip=1.0, lengths=None):
    """Upload `streams` (their own frames; the rest of a slot is FILL), apply points {stream: [(frame, gain)]} and hold the whole
    corpus and every record against the reference.  Returns (corpus bytes, record bytes)."""
    slot, C = int(b.cfg.frames_per_stream), int(b.cfg.channels)
    pcm = np.full((len(streams), slot, C), FILL, np.float32)
    for s, x in enumerate(streams):
        pcm[s, :len(x)] = x
    b.upload(0, pcm)
    if lengths is not None:
        b.set_lengths(lengths)
    rows = [(s, frame, gain) for s, pts in points.items() for frame, gain in pts]
    b.apply_gain(rows, mask, clip)
    stats = b.gain_stats()
    corpus = []
    for s, x in enumerate(streams):
        F = len(x)
        want = pcm[s].copy()
        if s in points:
            want[:F] = ref_samples(np.ascontiguousarray(pcm[s, :F]), points[s], mask)
        got = b.download_input(s).reshape(slot, C)
        same_corpus(got[:F], want[:F], (tag, s))
        assert got[F:].tobytes() == want[F:].tobytes(), (tag, s, "frames behind the stream's length")
        if s not in points:
            assert got.tobytes() == pcm[s].tobytes(), (tag, s, "a stream without a point")
        for c in range(C):
            if mask and not mask >> c & 1:
                assert got[:, c].tobytes() == pcm[s, :, c].tobytes(), (tag, s, c, "an unselected channel")
        ref = ref_records(want[:F], clip, s in points)
        assert stats[s].tobytes() == ref.tobytes(), (tag, s, stats[s], ref)
        corpus.append(got)
    return np.stack(corpus).tobytes(), stats.tobytes()


# ------------------------------------------------------------------------------------------------------------ 1. ragged lengths
def test_ragged_lengths_and_untouched_bytes(tile):
    """Slot of 9001 frames (odd: streams 1 and 3 start 8-byte aligned only), lengths 9001, 0, 1, tile + 1; stream 2 has no point and
    carries a signalling NaN and a negative zero."""
    rng = np.random.default_rng(1)
    lengths = [9001, 0, 1, tile + 1]
    assert lengths[3] <= 9001
    streams = [noise(rng, F, 2) for F in lengths]
    streams[2] = np.array([[0x7FA00000, 0x80000000]], np.uint32).view(np.float32)
    b = make_batch(48000, 2, 4, 9001)
    apply_and_check(b, streams, {0: [(0, 0.5)], 1: [(7, 2.0)], 3: [(100, -1.25)]}, "ragged", lengths=lengths)
    # ... and with lengths set, a ramp across the short streams' ends
    apply_and_check(b, streams, {0: [(4000, 0.5), (9000, 0.25)], 3: [(tile - 1, 1.0), (tile + 1, 0.0)]}, "ragged ramp", lengths=lengths)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 2. envelope plants
def test_envelope_plants(tile):
    rng = np.random.default_rng(2)
    F = 3 * tile + 17
    x = noise(rng, F, 2)
    b = make_batch(48000, 2, 1, F)
    dense = [(5, 1.0)] + [(tile + 50 + 3 * i, float(g)) for i, g in enumerate(rng.uniform(-2.0, 2.0, 1000).astype(np.float32))]
    assert dense[-1][0] < 2 * tile
    plants = {
        "a point on every tile boundary": [(5, 0.25), (tile, 0.75), (2 * tile, 0.75), (3 * tile, -1.5), (F + 100, 0.5)],
        "steps, one across a tile boundary": [(5, 1.0), (100, 1.0), (101, 0.5), (tile - 1, 0.5), (tile, 2.0), (F + 100, 2.0)],
        "a ramp from inside tile 0 to inside tile 2": [(tile - 1000, 0.2), (2 * tile + 777, 1.9)],
        "1000 points inside one tile": dense,
        "fades": [(5, 0.0), (500, 1.0), (F - 400, 1.0), (F - 1, 0.0)],
        "first and last frame": [(0, 2.0), (F - 1, 0.5)],
        "all of it behind the end": [(F + 1, 0.3), (F + 100, 3.0)],
    }
    for tag, pts in plants.items():
        apply_and_check(b, [x], {0: pts}, tag)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 3. long index
def test_frame_index_beyond_f32(tile):
    """Mono, 2^24 + 64 frames, a ramp from 2^24 - 3 to 2^24 + 5: an f32 frame index (or offset) goes wrong here."""
    M = 1 << 24
    F = M + 64
    rng = np.random.default_rng(3)
    x = np.tile(noise(rng, 1 << 16, 1), (F // (1 << 16) + 1, 1))[:F].copy()
    x[M - 8:M + 16] = noise(rng, 24, 1)
    b = make_batch(48000, 1, 1, F)
    apply_and_check(b, [x], {0: [(M - 3, 0.3), (M + 5, 1.1)]}, "2^24")
    b.close()


# ------------------------------------------------------------------------------------------------------------ 4. channels and mask
@pytest.mark.parametrize("channels", [1, 3, 6])
def test_channel_counts(tile, channels):
    rng = np.random.default_rng(40 + channels)
    F = tile + 904
    streams = [noise(rng, F, channels), noise(rng, F - 1, channels)]
    b = make_batch(48000, channels, 2, F)
    apply_and_check(b, streams, {0: [(0, 0.7)], 1: [(10, 0.1), (F - 10, 1.3)]}, ("channels", channels), lengths=[F, F - 1])
    b.close()


@pytest.mark.parametrize("channels", [2, 6])
def test_mask_flips_one_channel(tile, channels):
    from test_gpu_pair_series import exact_noise
    rng = np.random.default_rng(50 + channels)
    F = tile + 904
    x = exact_noise(rng, F, channels)
    b = make_batch(48000, channels, 1, F)
    b.upload(0, x)
    b.pair_series([(0, 1)])
    before = b.pair_entries(0)
    apply_and_check(b, [x], {0: [(0, -1.0)]}, ("mask", channels), mask=0b10)
    b.pair_series([(0, 1)])
    after = b.pair_entries(0)
    # (multiples of 2^-8: every sum is exact, so the flipped channel negates s_ab exactly and leaves the powers)
    assert np.array_equal(after["s_ab"], -before["s_ab"]) and (before["s_ab"] != 0).any()
    assert np.array_equal(after["s_aa"], before["s_aa"]) and np.array_equal(after["s_bb"], before["s_bb"])
    # the same mask along a ramp (the f64 form)
    apply_and_check(b, [x], {0: [(3, -1.0), (F - 3, 1.0)]}, ("mask ramp", channels), mask=0b10)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 5. values
VALUE_FORMS = {"constant": lambda g, F: [(0, g)], "ramp": lambda g, F: [(0, g), (1 << 40, g * 0.5)]}


@pytest.mark.parametrize("form", sorted(VALUE_FORMS))
@pytest.mark.parametrize("channels", [1, 2])
def test_values(tile, channels, form):
    rng = np.random.default_rng(5)
    F = 2 * tile + 3
    b = make_batch(48000, channels, 1, F)
    pts = VALUE_FORMS[form]
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1e-30, -1e-30, 1e-38, 1e-45], np.float32)
    x = noise(rng, F, channels)
    x[7:7 + special.size, 0] = special
    x[tile + 1:tile + 1 + special.size, channels - 1] = special[::-1]
    # gain 0 (signed zeros as numpy has them; inf * 0 is NaN), gain 2 (3e38 overflows to inf), a gain that makes subnormals
    for g in (0.0, -0.0, 2.0, 1e-10):
        _, stats = apply_and_check(b, [x], {0: pts(g, F)}, ("values", channels, form, g))
        rec = np.frombuffer(stats, GAIN_CHANNEL_DTYPE)
        if g == 2.0:
            assert rec[0]["n_nonfinite"] >= 5 and rec[0]["n_over"] >= 4           # NaN, +-inf, +-3e38 -> +-inf; the infinities are over
    # clip_level exactly at a sample's magnitude (>=), first_over in the second tile
    y = (0.9 * noise(rng, F, channels)).astype(np.float32)
    y[tile + 7, channels - 1] = 1.0
    y[tile + 9, 0] = -1.0
    y[tile + 5, 0] = np.nextafter(np.float32(1.0), np.float32(0.0))           # just under: not over
    _, stats = apply_and_check(b, [y], {0: [(0, 0.5)]}, ("clip", channels), clip=0.5)
    rec = np.frombuffer(stats, GAIN_CHANNEL_DTYPE)
    assert rec[channels - 1]["first_over"] == tile + 7 and rec[0]["first_over"] == (tile + 7 if channels == 1 else tile + 9)
    assert int(rec["n_over"].sum()) == 2
    _, stats = apply_and_check(b, [y], {0: [(0, 4.0)]}, ("clip at inf", channels), clip=math.inf)
    assert int(np.frombuffer(stats, GAIN_CHANNEL_DTYPE)["n_over"].sum()) == 0
    b.close()


# ------------------------------------------------------------------------------------------------------------ 6. determinism
def test_two_calls_leave_the_same_bytes(tile):
    rng = np.random.default_rng(6)
    F = 5 * tile + 1
    streams = [noise(rng, F, 2, 1.2) for _ in range(3)]
    streams[1][100, 1] = np.nan
    points = {0: [(0, 1.5)], 2: [(17, 0.0), (3 * tile, 2.0), (3 * tile + 1, 0.5), (F, 0.1)]}
    b = make_batch(48000, 2, 3, F)
    first = apply_and_check(b, streams, points, "first", clip=0.8)
    again = apply_and_check(b, streams, points, "again", clip=0.8)
    assert first == again
    b.close()


# ------------------------------------------------------------------------------------------------------------ 7. queue order
def test_a_pass_queued_behind_the_gain_reads_the_product():
    rng = np.random.default_rng(7)
    F = 48000
    x = np.stack([noise(rng, F, 2, 0.3), noise(rng, F, 2, 0.05)])
    points = {0: [(0, 0.5)], 1: [(1000, 1.0), (40000, 3.0)]}
    b = make_batch(48000, 2, 2, F, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    b.upload(0, x)
    b.apply_gain([(s, f, g) for s, pts in points.items() for f, g in pts])
    b.run()                                                     # (no sync between the two)
    got = [[getattr(r, n) for n, _ in L.StreamResult._fields_ if n not in ("true_peak", "sample_peak")] + list(r.true_peak) + list(r.sample_peak)
           for r in b.results()]
    b.upload(0, np.stack([ref_samples(x[s], points[s], 0) for s in range(2)]))
    b.run()
    ref = [[getattr(r, n) for n, _ in L.StreamResult._fields_ if n not in ("true_peak", "sample_peak")] + list(r.true_peak) + list(r.sample_peak)
           for r in b.results()]
    assert np.array_equal(np.array(got, np.float64), np.array(ref, np.float64), equal_nan=True), (got, ref)
    assert all(math.isfinite(r[0]) for r in got)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 8. status codes
def test_status_codes(tile):
    lib = L.lib()
    b = make_batch(48000, 2, 3, 1000)
    h = b._h
    ok_cfg = L.GainConfig(0, 1.0, 0)

    def call(rows, cfg=ok_cfg, n=None, null=False):
        p = np.zeros(len(rows), GAIN_POINT_DTYPE)
        for i, (s, f, g) in enumerate(rows):
            p[i] = (f, s, g)
        ptr = None if null else p.ctypes.data_as(ctypes.POINTER(L.GainPoint))
        return lib.ss_batch_apply_gain(h, ptr, len(rows) if n is None else n, ctypes.byref(cfg) if cfg is not None else None)

    rec = (L.GainChannel * 6)()
    assert lib.ss_batch_download_gain_stats(h, rec, 6) == L.SS_ERR_INVALID_MODE          # before the first call
    INVALID = L.SS_ERR_INVALID_ARG
    assert call([], n=2, null=True) == INVALID                                             # points == NULL with n_points > 0
    assert call([(0, 0, 1.0), (1, 0, 1.0), (0, 5, 1.0)]) == INVALID                        # not grouped by stream
    assert call([(0, 5, 1.0), (0, 5, 2.0)]) == INVALID and call([(0, 6, 1.0), (0, 5, 2.0)]) == INVALID     # not strictly ascending
    assert call([(3, 0, 1.0)]) == INVALID                                                  # stream >= n_streams
    assert call([(0, 0, math.nan)]) == INVALID and call([(0, 0, math.inf)]) == INVALID and call([(0, 0, -math.inf)]) == INVALID
    assert call([(0, 1 << 52, 1.0)]) == INVALID and call([(0, (1 << 52) - 1, 1.0)]) == L.SS_OK
    assert call([(0, 0, 1.0)], L.GainConfig(0b100, 1.0, 0)) == INVALID                     # a mask bit at or above the channel count
    for clip in (math.nan, 0.0, -1.0):
        assert call([(0, 0, 1.0)], L.GainConfig(0, clip, 0)) == INVALID
    assert call([(0, 0, 1.0)], L.GainConfig(0, 1.0, 1)) == INVALID and call([(0, 0, 1.0)], None) == INVALID
    assert lib.ss_batch_apply_gain(None, None, 0, ctypes.byref(ok_cfg)) == INVALID
    # none of the refused calls touched anything; n_points == 0 is valid and reads all untouched
    x = noise(np.random.default_rng(8), 1000, 2)
    b.upload(0, np.stack([x, x, x]))
    assert call([]) == L.SS_OK and call([], null=True) == L.SS_OK
    assert lib.ss_batch_download_gain_stats(h, rec, 5) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_gain_stats(h, None, 6) == INVALID
    stats = b.gain_stats()
    assert (stats["touched"] == 0).all() and (stats["first_over"] == U64_MAX).all() and (stats["n_over"] == 0).all()
    assert (stats["sample_peak"] == 0).all() and (stats["n_nonfinite"] == 0).all()
    assert b.download_input(1).tobytes() == x.tobytes()
    # the streams in any order, negative and zero gains, points behind the end
    assert call([(2, 0, -1.0), (0, 5000, 0.0), (0, 6000, 1.0)]) == L.SS_OK
    assert list(b.gain_stats()["touched"][:, 0]) == [1, 0, 1]
    b.close()


# ------------------------------------------------------------------------------------------------------------ 9. normalise
RATE, SECONDS, TARGET = 48000, 5, -23.0


def normalise_material():
    """Three stereo streams of uniform noise at different levels; the quiet third carries one loud sample, so a ceiling binds for it
    alone (the target wants x 1.51 of it, which would take the 0.7 to 1.06).  On the CPU oracle the three read -3.05, -18.63 and
    -26.57 LUFS and, multiplied by their f32 gains to -23, -23.009, -22.977 and -23.020: inside the 0.1 LU of a histogram bin."""
    rng = np.random.default_rng(9)
    F = RATE * SECONDS
    x = np.stack([noise(rng, F, 2, 0.6), noise(rng, F, 2, 0.1), noise(rng, F, 2, 0.04)])
    x[2, F // 2, 0] = 0.7
    return x


def readings(b, n):
    S = (RATE + 5) // 10
    E = (int(b.cfg.frames_per_stream) + S - 1) // S
    b.peak_regions([(s, 0, E) for s in range(n)])
    return np.array([r.integrated_lufs for r in b.results()]), np.array([r.true_peak for r in b.region_peaks()])


@pytest.mark.parametrize("ceiling", [math.inf, -1.0])
def test_normalise(ceiling):
    x = normalise_material()
    n, F = x.shape[0], x.shape[1]
    b = make_batch(RATE, 2, n, F, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    b.upload(0, x)
    out = b.normalise(TARGET, max_true_peak_dbtp=ceiling)
    # the gains are the law applied to the batch's own readings (no pass has run since: they describe the corpus before the call)
    loudness, peak = readings(b, n)
    assert np.array_equal(out["loudness"], loudness) and np.array_equal(out["peak"], peak) and (peak > 0).all()
    db, lin, why = normalisation_gain(loudness, peak, TARGET, ceiling)
    assert np.array_equal(out["gain_db"], db) and np.array_equal(out["gain"], lin) and np.array_equal(out["limited_by"], why)
    assert list(why) == ([0, 0, 0] if math.isinf(ceiling) else [0, 0, L.SS_GAIN_LIMITED_PEAK])
    # the corpus is numpy times those gains
    for s in range(n):
        same_corpus(b.download_input(s).reshape(F, 2), (x[s].astype(np.float64) * np.float64(lin[s])).astype(np.float32), ("normalise", s))
    stats = b.gain_stats()
    assert (stats["touched"] == 1).all()
    # a second pass reads the target within one histogram bin, the limited stream's true peak stays under the ceiling
    b.run()
    b.peak_series()
    after = b.results()
    for s in range(n):
        if why[s] == 0:
            print("stream %d: %.4f LUFS behind the gain" % (s, after[s].integrated_lufs))
            assert abs(after[s].integrated_lufs - TARGET) <= 0.1, (s, after[s].integrated_lufs)
        else:
            top = float(b.peak_series_of(s)["true_peak"].max())
            print("stream %d: true peak %.6f against %.6f" % (s, top, 10.0 ** (ceiling / 20.0)))
            assert top <= 10.0 ** (ceiling / 20.0) * (1.0 + 1e-4), (s, top)
            assert after[s].integrated_lufs < TARGET
    b.close()


def test_normalise_album():
    x = normalise_material()
    n, F = x.shape[0], x.shape[1]
    b = make_batch(RATE, 2, n, F, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    b.upload(0, x)
    out = b.normalise(TARGET, max_true_peak_dbtp=-1.0, album=True)
    S = (RATE + 5) // 10
    b.loudness_regions([(s, 0, F // S, 0) for s in range(n)], 1)
    b.peak_regions([(s, 0, (F + S - 1) // S, 0) for s in range(n)], 1)
    loudness, peak = b.group_results()[0].integrated_lufs, b.group_peaks()[0].true_peak
    db, lin, why = normalisation_gain(loudness, peak, TARGET, -1.0)
    assert (out["loudness"] == loudness).all() and (out["peak"] == peak).all() and math.isfinite(loudness) and peak >= 0.7
    assert (out["gain"] == lin).all() and (out["gain_db"] == db).all() and (out["limited_by"] == why).all()
    for s in range(n):
        same_corpus(b.download_input(s).reshape(F, 2), (x[s].astype(np.float64) * np.float64(lin)).astype(np.float32), ("album", s))
    b.close()


def test_normalise_needs_the_loudness_pass():
    b = make_batch(RATE, 2, 1, 4800)
    with pytest.raises(ValueError):
        b.normalise(TARGET)
    b.close()
