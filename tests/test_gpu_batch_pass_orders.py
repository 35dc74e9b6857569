"""The orders a batch pass can be queued in, and the ways its input can arrive, must not change a bit.

ss_batch_run puts the spectrum kernel in one of three places (first, behind the time-domain kernel, last), on one stream or
two, with or without the event marks of per-kernel timing; the time-domain launch is one launch or a launch and its fix-up.
Every combination of overlap 0 / 1 / 2 and timing on / off is held against a sequential pass with timing off, on small shapes
whose geometry is asserted first:

  * stereo, three streams: segments on eight waves with the run-in inside the one launch (td_split 2).  That form wants
    0.8 x 4 waves per stream to lose against 0.556 x segments of two sub-blocks, so six segments: 1.1 s (52800 frames, 11
    sub-blocks) is the shortest stream that takes it — at 0.7 s (7 sub-blocks) three stereo streams are whole-stream workgroups;
  * the same batch with ragged lengths (52800, 20000 and 4799 frames: the last under one sub-block and under one window): the
    split is off, one wave per segment, the run-in stays (few streams never reach the fix-up: eight waves per shortest segment
    fit the chip);
  * ragged stereo WITH the fix-up launch needs 8 x streams x 6 segments above the 4096 waves the chip holds: 86 streams;
  * mono, three streams of 0.7 s (33600 frames, 7 sub-blocks), uniform and ragged (33600, 20000, 4799): no whole-stream form
    for one channel, so segments hand over through the fix-up launch;
  * a columns-only stereo batch under the fixed gain and under the reference's per-file gain (spectrum last).

The uploads: the same material through every entry point gives the same bits in the batch's input.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.analyzer import AnalyzerError
from conftest import make_multich, make_stereo

pytestmark = pytest.mark.gpu

RATE, FFT_N, HOP = 48000, 4096, 1024
FLAGS = L.SS_BATCH_ALL | L.SS_BATCH_LOUDNESS_SERIES
STEREO_FRAMES, MONO_FRAMES = 52800, 33600
RAGGED_TAIL = (20000, 4799)
KERNELS = (L.SS_KERNEL_FFT, L.SS_KERNEL_TIME_DOMAIN, L.SS_KERNEL_FINALIZE, L.SS_KERNEL_WAVEFORM)


@functools.lru_cache(maxsize=None)
def _material(channels, frames, kinds=3):
    """[kinds][frames * channels] f32, made once per shape and never written to"""
    if channels == 2:
        x = np.stack([make_stereo(11 + i, frames, RATE, level=0.5 / (1 + i)) for i in range(kinds)])
    else:
        x = np.stack([make_multich(23 + i, frames, channels, RATE, level=0.4 / (1 + i)) for i in range(kinds)])
    x.setflags(write=False)
    return x


def _lengths(longest, n_streams):
    cycle = (longest,) + RAGGED_TAIL
    return [cycle[i % 3] for i in range(n_streams)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])      # bit patterns: -inf, -0 and NaN compare like any value


def _snapshot(b, columns=False):
    n = int(b.cfg.n_streams)
    snap = {
        "checksums": b.checksums(),
        "results": np.array([(r.integrated_lufs, r.loudness_range, r.true_peak[0], r.true_peak[1], r.sample_peak[0],
                              r.sample_peak[1], float(r.n_gating_blocks), float(r.n_st_blocks)) for r in b.results()], np.float64),
        "histograms": np.concatenate(b.histograms()),
        "series": np.concatenate([np.concatenate(b.loudness_series(i)) for i in range(n)]),
        "extremes": np.array([(e.max_momentary, e.max_shortterm, float(e.max_momentary_at), float(e.max_shortterm_at))
                              for e in b.loudness_extremes()], np.float64),
    }
    if columns:
        snap["columns"] = np.stack([b.spectrum_columns(i) for i in range(n)])
    return snap


def _cross(b, what, columns=False):
    """every overlap x timing combination against the sequential untimed pass; returns that reference"""
    b.set_overlap(0)
    b.timing_enable(False)
    b.run(); b.sync()
    ref = _snapshot(b, columns)
    assert ref["checksums"][:, 2].any(), "sub-block checksums must not all be zero"
    bad = []
    for overlap in (0, 1, 2):
        for timed in (False, True):
            b.set_overlap(overlap)
            assert b.geometry.overlap == overlap
            b.timing_enable(timed)
            b.run(); b.sync()
            if timed:
                counts = [b.timing_read(k)[1] for k in KERNELS]
                if counts != [1, 1, 1, 1]:
                    bad.append((overlap, timed, "launches per kernel", counts))
            got = _snapshot(b, columns)
            for key, want in ref.items():
                if not np.array_equal(_bits(got[key]), _bits(want)):
                    bad.append((overlap, timed, key, int((_bits(got[key]) != _bits(want)).sum())))
    b.set_overlap(0)
    b.timing_enable(False)
    assert not bad, f"{what}: passes that differ from the sequential untimed pass (overlap, timing, what, how many): {bad}"
    return ref


def _geo(b):
    g = b.geometry
    return g.td_split, g.td_segments, g.td_segment_subblocks, g.td_warm_subblocks, g.td_fixup_subblocks


def test_stereo_eight_wave_segments_uniform_then_ragged():
    x = _material(2, STEREO_FRAMES)
    b = ssa.Batch(RATE, 2, 3, STEREO_FRAMES, FFT_N, HOP, flags=FLAGS)
    b.upload(0, x)
    assert _geo(b) == (2, 6, 2, 2, 0), _geo(b)
    uniform = _cross(b, "stereo, uniform")
    assert uniform["checksums"].all()
    b.set_lengths(_lengths(STEREO_FRAMES, 3))
    assert _geo(b) == (0, 6, 2, 2, 0), _geo(b)
    assert [b.stream_shape(i).n_subblocks for i in range(3)] == [11, 4, 0] and b.stream_shape(2).n_windows == 0
    _cross(b, "stereo, ragged")
    b.close()


def test_stereo_ragged_with_the_fixup_launch():
    ns = 86
    x = _material(2, STEREO_FRAMES)
    b = ssa.Batch(RATE, 2, ns, STEREO_FRAMES, FFT_N, HOP, flags=FLAGS)
    b.upload(0, x[np.arange(ns) % 3])
    b.set_lengths(_lengths(STEREO_FRAMES, ns))
    g = _geo(b)
    assert g[0] == 0 and g[1] == 6 and g[3] == 0 and g[4] == 2, g
    _cross(b, "stereo, 86 streams, ragged")
    b.close()


def test_mono_fixup_launch_uniform_then_ragged():
    x = _material(1, MONO_FRAMES)
    b = ssa.Batch(RATE, 1, 3, MONO_FRAMES, FFT_N, HOP, flags=FLAGS)
    b.upload(0, x)
    assert _geo(b) == (0, 4, 2, 0, 2), _geo(b)
    uniform = _cross(b, "mono, uniform")
    assert uniform["checksums"].all()
    b.set_lengths(_lengths(MONO_FRAMES, 3))
    assert _geo(b) == (0, 4, 2, 0, 2), _geo(b)
    assert [b.stream_shape(i).n_subblocks for i in range(3)] == [7, 4, 0]
    _cross(b, "mono, ragged")
    b.close()


def test_columns_only_fixed_and_reference_gain():
    x = _material(2, STEREO_FRAMES)
    b = ssa.Batch(RATE, 2, 3, STEREO_FRAMES, FFT_N, HOP, flags=FLAGS, spectrum_columns=64)
    b.upload(0, x)
    b.set_columns_gain(-3.0)
    fixed = _cross(b, "columns-only, fixed gain", columns=True)
    b.set_columns_gain(None)                     # -13 - integrated of each stream: the spectrum kernel runs last
    reference = _cross(b, "columns-only, reference gain", columns=True)
    for snap in (fixed, reference):
        assert snap["columns"].shape == (3, b.layout.n_windows, b.layout.fft_channels, 64)
        assert np.isfinite(snap["columns"]).any()
    assert not np.array_equal(_bits(fixed["columns"]), _bits(reference["columns"])), "the gain mode must show in the columns"
    assert np.array_equal(_bits(fixed["results"]), _bits(reference["results"]))
    b.close()


def _special_floats(n, rng):
    """f32 bit patterns that a conversion or an arithmetic copy would not keep: signed zeros, subnormals, infinities, quiet and
    signalling NaNs with payloads, among ordinary values"""
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFBFFFFF, 0x7FC12345, 0x7FA54321], np.uint32)
    bits[:special.size] = special
    bits[-special.size:] = special[::-1]
    bits[n // 2:n // 2 + special.size] = special
    return bits.view(np.float32)


def test_every_upload_entry_point_gives_the_same_input():
    frames, ns = 4099, 3
    b = ssa.Batch(RATE, 2, ns, frames, FFT_N, HOP, flags=L.SS_BATCH_LUFS)        # uploaded and downloaded only, never analysed
    per = b.samples_per_stream
    lib, vp = L.lib(), C.c_void_p
    rng = np.random.default_rng(5)
    x = np.concatenate([make_stereo(3, frames, RATE), make_stereo(4, frames, RATE), _special_floats(per, rng)])
    s16 = rng.integers(-32768, 32768, ns * per).astype(np.int16)
    s16[:4] = (-32768, 32767, 0, -1)
    zeros = np.zeros(ns * per, np.float32)

    def downloaded():
        return np.concatenate([b.download_input(i) for i in range(ns)])

    def upload_pcm(a, fmt):
        assert lib.ss_batch_upload_pcm(b._h, 0, ns, a.ctypes.data_as(vp), fmt) == 0

    def upload_pcm_async(a, fmt):
        assert lib.ss_batch_upload_pcm_async(b._h, 0, ns, a.ctypes.data_as(vp), fmt) == 0
        b.sync()

    def upload_samples(a, fmt):
        for i in range(ns):
            assert lib.ss_batch_upload_samples(b._h, i, a[i * per:(i + 1) * per].ctypes.data_as(vp), per, fmt) == 0
        b.sync()

    forms = {"upload_pcm": upload_pcm, "upload_pcm_async": upload_pcm_async, "upload_samples": upload_samples}
    b.upload(0, x)
    assert np.array_equal(_bits(downloaded()), _bits(x)), "ss_batch_upload"
    for name, form in forms.items():
        b.upload(0, zeros)
        form(x, L.SS_PCM_F32)
        assert np.array_equal(_bits(downloaded()), _bits(x)), f"{name}, f32"
    want = s16.astype(np.float32) / np.float32(32768.0)                          # (the scale is a power of two: exact)
    for name, form in forms.items():
        b.upload(0, zeros)
        form(s16, L.SS_PCM_S16)
        assert np.array_equal(_bits(downloaded()), _bits(want)), f"{name}, s16"
    # a range that does not start at stream 0, and the head of one slot: the rest of the input stays as it was
    b.upload(0, zeros)
    assert lib.ss_batch_upload_pcm_async(b._h, 1, 2, s16[per:].ctypes.data_as(vp), L.SS_PCM_S16) == 0
    b.sync()
    got = downloaded()
    assert not got[:per].any() and np.array_equal(_bits(got[per:]), _bits(want[per:]))
    assert lib.ss_batch_upload_samples(b._h, 0, s16.ctypes.data_as(vp), 1001, L.SS_PCM_S16) == 0
    b.sync()
    got = downloaded()
    assert np.array_equal(_bits(got[:1001]), _bits(want[:1001])) and not got[1001:per].any()
    assert np.array_equal(_bits(got[per:]), _bits(want[per:]))
    b.close()


def test_refused_set_lengths_leaves_the_batch_as_it_was():
    x = _material(1, MONO_FRAMES)
    b = ssa.Batch(RATE, 1, 3, MONO_FRAMES, FFT_N, HOP, flags=FLAGS)
    b.upload(0, x)
    b.set_lengths(_lengths(MONO_FRAMES, 3))
    b.run(); b.sync()
    before = _snapshot(b)
    shapes = [tuple(getattr(b.stream_shape(i), f) for f in ("frames", "n_windows", "n_subblocks", "n_wave_points")) for i in range(3)]
    geo = _geo(b)
    with pytest.raises(AnalyzerError) as err:
        b.set_lengths([1000, MONO_FRAMES + 1, 2000])
    assert err.value.code == L.SS_ERR_INVALID_ARG
    assert shapes == [tuple(getattr(b.stream_shape(i), f) for f in ("frames", "n_windows", "n_subblocks", "n_wave_points")) for i in range(3)]
    assert geo == _geo(b)
    b.run(); b.sync()
    after = _snapshot(b)
    for key, want in before.items():
        assert np.array_equal(_bits(after[key]), _bits(want)), key
    b.close()
