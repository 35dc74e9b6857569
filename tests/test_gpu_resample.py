"""The batch resampler on the device (ss_batch_resample, soundscope_amd/csrc/ss_resample.hip): every output equals ss_resample_host —
the definition, one fmaf chain per output — in bits.  Five rate pairs x four channel counts on a ragged batch whose lengths sit at
the edges of the kernel's tiles (taken from ss_batch_resample_plan), every length at both 16-byte alignments of its slot; impulses
at a stream's first and last frame, a NaN and an infinity (outputs whose window misses them keep the clean run's bits), subnormal
products; sentinels behind every source length (never heard) and behind every output length (never touched).  Then what does not
depend on where a stream lies, the refusals, a sine's true peak and loudness across the conversion, and the ordering against a gain
queued on the source straight behind the call.  Mono and stereo take the register-taps kernel where T <= 128, three and six
channels and 96 -> 48 kHz (T = 140) the LDS-taps kernel, 64 channels of a wide table the direct one: each against the same host
chain.  88.2 -> 48 kHz (T = 128) runs the register form's larger instantiation, a 160 x 148 table the LDS form with every phase
in mono and stereo, and a -DSS_TUNING build made by the test runs the register and the LDS form on the same plans."""
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_forms_child as child
import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import resample_host, resample_length, resample_plan, resample_taps

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 48000), (48000, 44100), (96000, 48000), (48000, 96000), (32000, 48000)]
CHANNELS = [1, 2, 3, 6]
FLAGS = L.SS_BATCH_TRUE_PEAK                # no spectrum, no decimation: the corpus is all these tests need


def material(rng, frames, channels, rate):
    n = np.arange(frames)[:, None]
    x = 0.1 * rng.standard_normal((frames, channels)) + 0.3 * np.sin(2 * np.pi * 997.0 * n / rate + np.arange(channels)[None, :])
    return x.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_or_both_nan(got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(ref)[~nan])


def tiles_of(plan, channels):
    probe = ssa.Batch(int(plan.in_rate), channels, 1, 1, flags=FLAGS)
    try:
        return probe.resample_tiles(plan)
    finally:
        probe.close()


def fill(batch, streams, sentinel):
    """streams: [frames_s][channels] arrays; the slot behind each is `sentinel`"""
    fps, ch = int(batch.cfg.frames_per_stream), int(batch.cfg.channels)
    slab = np.full((len(streams), fps, ch), sentinel, np.float32)
    for s, x in enumerate(streams):
        slab[s, :x.shape[0]] = x
    batch.upload(0, slab)
    batch.set_lengths([x.shape[0] for x in streams])


def pattern(n_streams, fps, ch):
    """what lies in a destination before the call: finite floats, no two neighbours alike"""
    return (np.arange(n_streams * fps * ch, dtype=np.uint32) * np.uint32(2654435761) >> np.uint32(9) | np.uint32(0x3F000000)).view(np.float32).reshape(n_streams, fps, ch)


def convert(streams, plan, channels, slack=5, twice=False):
    """the streams through resample_into: (outputs per stream, what lies behind them, dst's reported frames) and the pattern's tails"""
    fps = max(x.shape[0] for x in streams) | 1
    src = ssa.Batch(int(plan.in_rate), channels, len(streams), fps, flags=FLAGS)
    lens = [resample_length(plan, x.shape[0]) for x in streams]
    fps_out = (max(lens) + slack) | 1
    dst = ssa.Batch(int(plan.out_rate), channels, len(streams), fps_out, flags=FLAGS)
    try:
        fill(src, streams, 0.5)
        before = pattern(len(streams), fps_out, channels)
        dst.upload(0, before)
        runs = []
        for _ in range(2 if twice else 1):
            src.resample_into(dst, plan)
            slots = [dst.download_input(s).reshape(fps_out, channels) for s in range(len(streams))]
            runs.append(slots)
        for s in range(len(streams)):
            assert int(dst.stream_shape(s).frames) == lens[s], s
            assert runs[0][s][lens[s]:].tobytes() == before[s, lens[s]:].tobytes(), ("behind the output of stream", s)
        if twice:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs)), "two calls, two results"
        # src is read only
        for s, x in enumerate(streams):
            back = src.download_input(s).reshape(fps, channels)
            assert back[:x.shape[0]].tobytes() == x.tobytes() and (back[x.shape[0]:] == 0.5).all(), s
        return [runs[0][s][:lens[s]] for s in range(len(streams))]
    finally:
        src.close()
        dst.close()


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("pair", PAIRS, ids=["%d_%d" % p for p in PAIRS])
def test_every_output_equals_the_host_chain(pair, channels):
    plan = resample_plan(*pair)
    taps = resample_taps(plan)
    T, M = int(plan.taps), int(plan.down)
    tile_out, tile_in = tiles_of(plan, channels)
    assert tile_out % int(plan.up) == 0 and tile_in == tile_out // int(plan.up) * M
    rng = np.random.default_rng(pair[0] + channels)
    lengths = [0, 1, T // 2 - 1, T // 2, M, tile_in - 1, tile_in, tile_in + 1, 2 * tile_in + 71]
    streams = [material(rng, F, channels, pair[0]) for F in lengths for _ in range(2)]      # odd slots: both alignments of each
    F = tile_in + 71
    impulses = np.zeros((F, channels), np.float32)
    impulses[0] = impulses[F - 1] = 1.0
    clean = material(rng, F, channels, pair[0])
    dirty = clean.copy()
    planted = [(F // 2, 0, np.nan), (F // 2 + T + 5, channels - 1, np.inf)]
    for f, c, v in planted:
        dirty[f, c] = v
    tiny = (clean.astype(np.float64) * 2.0 ** -120).astype(np.float32)
    streams += [impulses, clean, dirty, tiny]
    got = convert(streams, plan, channels, twice=True)
    for s, x in enumerate(streams):
        ref = resample_host(plan, x, channels, taps=taps)
        assert same_bits_or_both_nan(got[s], ref), (pair, channels, "stream", s, "frames", x.shape[0])
    # outputs whose window [base - T/2 + 1, base + T/2] misses the planted samples keep the clean run's bits
    i_clean, i_dirty = len(streams) - 3, len(streams) - 2
    base = np.arange(got[i_clean].shape[0], dtype=np.int64) * M // int(plan.up)
    hit = np.zeros(got[i_clean].shape, bool)
    for f, c, _ in planted:
        hit[:, c] |= (base - T // 2 + 1 <= f) & (f <= base + T // 2)
    assert hit.any() and (~hit).any()
    assert np.array_equal(bits(got[i_dirty])[~hit], bits(got[i_clean])[~hit])
    assert not np.isfinite(got[i_dirty][hit]).all()
    # the subnormal stream is no row of zeros
    assert np.count_nonzero(got[-1]) > got[-1].size // 2 and np.abs(got[-1]).max() < 2.0 ** -118


def test_upsampled_frames_are_the_input_frames():
    plan = resample_plan(32000, 48000)
    x = material(np.random.default_rng(5), 4001, 2, 32000)
    y = convert([x], plan, 2)[0]
    assert np.array_equal(bits(y[::3]), bits(x[::2][:y[::3].shape[0]]))


def test_the_direct_form_equals_the_host_chain():
    """64 channels beside a 160 x 148 table fit neither staged form: 23840 floats of table (rows of 149) and the 18824 of one period's
    run are 42664, over the 38912 the LDS form takes"""
    plan = resample_plan(44100, 48000, 112.0, 0.95)
    assert (int(plan.up), int(plan.down), int(plan.taps)) == (160, 147, 148)
    rng = np.random.default_rng(64)
    tile_out, tile_in = tiles_of(plan, 64)
    assert (tile_out, tile_in) == (160, 147)                        # the direct form's tile: ceil(8192 / 64 / 160) = 1 period
    streams = [material(rng, F, 64, 44100) for F in (0, 1, 69, tile_in + 1, 2 * tile_in + 71)]
    got = convert(streams, plan, 64)
    taps = resample_taps(plan)
    for s, x in enumerate(streams):
        assert np.array_equal(bits(got[s]), bits(resample_host(plan, x, 64, taps=taps))), s


def edge_streams(rng, plan, channels):
    tile_out, tile_in = tiles_of(plan, channels)
    T = int(plan.taps)
    lengths = [0, 1, T // 2 - 1, T // 2, int(plan.down), tile_in - 1, tile_in, tile_in + 1, 2 * tile_in + 71]
    return [material(rng, F, channels, int(plan.in_rate)) for F in lengths for _ in range(2)]


@pytest.mark.parametrize("channels", [1, 2])
def test_128_taps_in_registers_equal_the_host_chain(channels):
    """88.2 -> 48 kHz is 80 / 147 with 128 taps per phase: the register form's second instantiation (80 < T <= 128)"""
    plan = resample_plan(88200, 48000)
    assert (int(plan.up), int(plan.down), int(plan.taps)) == (80, 147, 128)
    streams = edge_streams(np.random.default_rng(128 + channels), plan, channels)
    got = convert(streams, plan, channels)
    taps = resample_taps(plan)
    for s, x in enumerate(streams):
        assert np.array_equal(bits(got[s]), bits(resample_host(plan, x, channels, taps=taps))), (s, x.shape[0])


@pytest.mark.parametrize("channels", [1, 2])
def test_many_phases_through_the_lds_form_equal_the_host_chain(channels):
    """160 phases of 148 taps are more than a lane holds, so mono and stereo take the LDS form here — with every phase in use, where
    96 -> 48 kHz has one"""
    plan = resample_plan(44100, 48000, 112.0, 0.95)
    assert (int(plan.up), int(plan.down), int(plan.taps)) == (160, 147, 148)
    streams = edge_streams(np.random.default_rng(148 + channels), plan, channels)
    got = convert(streams, plan, channels)
    taps = resample_taps(plan)
    for s, x in enumerate(streams):
        assert np.array_equal(bits(got[s]), bits(resample_host(plan, x, channels, taps=taps))), (s, x.shape[0])


def test_register_and_lds_forms_agree_in_the_tuning_build(tmp_path):
    """The release library has no switch for the kernel form; the -DSS_TUNING build reads SS_RESAMPLE_FORM.  That build is made here,
    once (every translation unit of the Makefile: this is the one slow test of the file, the compile is its cost), and a fresh
    child process per form converts 44.1 -> 48 kHz and 48 -> 44.1 kHz, mono and stereo (tests/resample_forms_child.py): the two
    forms' bytes equal each other and ss_resample_host."""
    csrc = os.path.join(os.path.dirname(L.LIB_PATH), "..", "csrc")
    lib = str(tmp_path / "libsoundscope_hip_tuning.so")
    subprocess.run(["make", "-j", str(max(1, min(16, os.cpu_count() or 1))), "-C", csrc, "OBJDIR=" + str(tmp_path / "obj"), "OUT=" + lib,
                    "EXTRA=-DSS_TUNING"], check=True, stdout=subprocess.DEVNULL, timeout=600)
    outs = {}
    for form in (1, 2):
        d = tmp_path / ("form%d" % form)
        d.mkdir()
        env = dict(os.environ, SOUNDSCOPE_HIP_LIB=lib, SS_RESAMPLE_FORM=str(form))
        r = subprocess.run([sys.executable, child.__file__, str(d)], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[form] = {case: np.load(str(d / ("%d_%d_%d.npz" % case))) for case in child.CASES}
    for case in child.CASES:
        plan = resample_plan(case[0], case[1])
        taps = resample_taps(plan)
        a, b = outs[1][case], outs[2][case]
        if case[2] == 2:                                            # the knob took: in stereo the two forms cut the streams differently
            assert tuple(a["tiles"]) != tuple(b["tiles"]), case
        for s, x in enumerate(child.streams_of(case)):
            ref = resample_host(plan, x, case[2], taps=taps).reshape(-1)
            assert a["s%d" % s].tobytes() == b["s%d" % s].tobytes() == ref.tobytes(), (case, s, x.shape[0])


def test_bits_do_not_depend_on_slot_or_batch():
    plan = resample_plan(44100, 48000)
    rng = np.random.default_rng(11)
    x = material(rng, 9000, 2, 44100)
    alone = convert([x], plan, 2)[0]
    others = [material(rng, F, 2, 44100) for F in (10001, 3, 777, 9000, 4410)]
    crowd = convert(others + [x, others[0][:500]], plan, 2, slack=40)
    assert crowd[5].tobytes() == alone.tobytes()


def test_refusals_leave_the_destination_alone():
    plan = resample_plan(44100, 48000)
    src = ssa.Batch(44100, 2, 3, 1001, flags=FLAGS)
    need = resample_length(plan, 1001)
    good = ssa.Batch(48000, 2, 3, need, flags=FLAGS)
    small = ssa.Batch(48000, 2, 3, need - 1, flags=FLAGS)
    mono = ssa.Batch(48000, 1, 3, need, flags=FLAGS)
    fewer = ssa.Batch(48000, 2, 2, need, flags=FLAGS)
    rate = ssa.Batch(96000, 2, 3, need, flags=FLAGS)
    lib = L.lib()
    try:
        src.upload(0, material(np.random.default_rng(2), 3 * 1001, 2, 44100))
        for dst, want in ((small, L.SS_ERR_CAPACITY), (mono, L.SS_ERR_INVALID_ARG), (fewer, L.SS_ERR_INVALID_ARG), (rate, L.SS_ERR_INVALID_ARG)):
            n, fps, ch = int(dst.cfg.n_streams), int(dst.cfg.frames_per_stream), int(dst.cfg.channels)
            before = pattern(n, fps, ch)
            dst.upload(0, before)
            assert lib.ss_batch_resample(src._h, dst._h, plan) == want
            assert all(int(dst.stream_shape(s).frames) == fps for s in range(n))
            assert all(dst.download_input(s).tobytes() == before[s].tobytes() for s in range(n))
        assert lib.ss_batch_resample(src._h, src._h, plan) == L.SS_ERR_INVALID_ARG
        assert lib.ss_batch_resample(good._h, src._h, plan) == L.SS_ERR_INVALID_ARG         # the rates the wrong way round
        assert lib.ss_batch_resample(src._h, good._h, None) == L.SS_ERR_INVALID_ARG
        bad = resample_plan(44100, 48000)
        bad.reserved = 1
        assert lib.ss_batch_resample(src._h, good._h, bad) == L.SS_ERR_INVALID_ARG
        bad = resample_plan(44100, 48000)
        bad.taps += 4
        assert lib.ss_batch_resample(src._h, good._h, bad) == L.SS_ERR_INVALID_ARG
        assert lib.ss_batch_resample(src._h, good._h, plan) == L.SS_OK
        assert all(int(good.stream_shape(s).frames) == need for s in range(3))
    finally:
        for b in (src, good, small, mono, fewer, rate):
            b.close()


def test_a_sine_keeps_its_peak_and_its_loudness():
    """997 Hz at half of full scale, one second at 44.1 kHz, to 48 kHz: the true peak within 0.01 dB of -6.02, the integrated loudness within
    0.01 LU of the source's"""
    n = np.arange(44100)
    x = (0.5 * np.sin(2 * np.pi * 997.0 * n / 44100.0)).astype(np.float32)
    src = ssa.Batch(44100, 2, 1, 44100, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK)
    try:
        src.upload(0, np.repeat(x[:, None], 2, axis=1))
        dst = src.resample(48000)
        try:
            assert int(dst.cfg.sample_rate) == 48000 and int(dst.stream_shape(0).frames) == 48000 == int(dst.cfg.frames_per_stream)
            dst.peak_series()
            peak = float(dst.peak_series_of(0)["true_peak"].max())
            assert abs(20.0 * np.log10(peak) - 20.0 * np.log10(0.5)) < 0.01, peak        # 20 log10(0.5) = -6.02
            src.run()
            dst.run()
            a, b = src.results()[0].integrated_lufs, dst.results()[0].integrated_lufs
            print("true peak %.4f dBTP, loudness %.4f -> %.4f LUFS" % (20.0 * np.log10(peak), a, b))
            assert abs(a - b) < 0.01
        finally:
            dst.close()
    finally:
        src.close()


def test_a_gain_queued_on_the_source_does_not_overtake_the_read():
    plan = resample_plan(48000, 44100)
    rng = np.random.default_rng(21)
    n_streams, F = 64, 48000
    x = material(rng, n_streams * F, 2, 48000).reshape(n_streams, F, 2)
    src = ssa.Batch(48000, 2, n_streams, F, flags=FLAGS)
    dst = ssa.Batch(44100, 2, n_streams, resample_length(plan, F), flags=FLAGS)
    try:
        src.upload(0, x)
        src.resample_into(dst, plan)
        src.apply_gain([(s, 0, 0.0) for s in range(n_streams)])
        taps = resample_taps(plan)
        for s in (0, n_streams // 2, n_streams - 1):
            assert np.array_equal(bits(dst.download_input(s).reshape(-1, 2)), bits(resample_host(plan, x[s], 2, taps=taps))), s
        assert not src.download_input(0).any()
    finally:
        src.close()
        dst.close()
