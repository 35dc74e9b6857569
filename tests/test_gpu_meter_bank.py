"""Meter banks on the MI355X: every stream of a bank against its own oracle meter fed the same blocks (read behind every call),
against the product's own handles (bit for bit where the arithmetic is the same), under a selective reset, with non-finite
samples, through every input form, at the scale of 1024 live stereo inputs, and the refusal codes of every entry point."""
import ctypes as C

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.analyzer import AnalyzerError

from conftest import make_multich, make_stereo

pytestmark = pytest.mark.gpu

TOL_LU = 1e-6                     # as tests/test_gpu_loudness_series.py holds the series
IRREGULAR = [1, 127, 4801, 48000, 0, 480, 1, 4800]


def material(seed, frames, channels, rate, level=0.5):
    if channels == 2:
        return make_stereo(seed, frames, rate, level=level)
    return make_multich(seed, frames, channels, rate, level=level)


def same_lufs(got, ref, tol=TOL_LU):
    if np.isnan(ref) or np.isinf(ref):
        return (np.isnan(got) and np.isnan(ref)) or got == ref
    return abs(got - ref) <= tol


def close9(a, b):
    return a == b or abs(a - b) <= 1e-9


def same_peak(a, b, rel=1e-4):
    if np.isinf(a) or np.isinf(b) or np.isnan(b):
        return a == b or (np.isnan(a) and np.isnan(b))
    return abs(a - b) <= rel * max(abs(b), 1e-30)


def oracle_shortterm(po, m):
    try:
        return m.shortterm()
    except po.OracleError:                     # thirty sub-blocks exceed the crate's 3 s ring: its call fails
        return float("nan")


def check_against_oracle(po, bank, meters, rec, tag, peaks=True):
    for s, m in enumerate(meters):
        r = rec[s]
        assert same_lufs(r["momentary"], m.momentary()), (tag, s, "M", r["momentary"], m.momentary())
        assert same_lufs(r["shortterm"], oracle_shortterm(po, m)), (tag, s, "S", r["shortterm"], oracle_shortterm(po, m))
        assert same_lufs(r["integrated"], m.integrated()), (tag, s, "I", r["integrated"], m.integrated())
        assert same_lufs(r["loudness_range"], m.loudness_range()), (tag, s, "LRA", r["loudness_range"], m.loudness_range())
        if not peaks:
            continue
        tp, sp = bank.peaks(s)
        for c in range(bank.channels):
            assert sp[c] == m.sample_peak(c), (tag, s, c, sp[c], m.sample_peak(c))
            assert same_peak(tp[c], max(m.true_peak(c), m.sample_peak(c))), (tag, s, c, tp[c], m.true_peak(c))
        for c in range(2):
            if c < bank.channels:
                assert r["sample_peak"][c] == sp[c] and r["true_peak"][c] == tp[c], (tag, s, c)
            else:
                assert np.isnan(r["sample_peak"][c]) and np.isnan(r["true_peak"][c]), (tag, s, c)


def feed_blocks(bank, xs, blocks, C_, after=None):
    """feed every stream its own material block by block ([n][frames * C]); after(i, pos, block) behind every call"""
    pos = 0
    for i, f in enumerate(blocks):
        bank.add(np.stack([x[pos * C_:(pos + f) * C_] for x in xs]))
        if after:
            after(i, pos, f)
        pos += f
    return pos


SHAPES = [(48000, 2), (44100, 2), (96000, 2), (16, 2), (48000, 1), (48000, 3), (48000, 6), (48000, 8)]


@pytest.mark.parametrize("rate,channels", SHAPES)
def test_every_stream_matches_its_oracle_meter(oracle, rate, channels):
    """Three streams of different material, blocks of 1 frame, 480 (one wave per stream), 4 800 (eight-wave workgroups), and an
    irregular mix with calls longer than 32 sub-blocks (pieces) and an empty call; every reading behind every call."""
    n = 3
    blocks = [1, 480, 480, 4800] + IRREGULAR + [4800] * 3
    total = sum(blocks)
    xs = [material(100 + 7 * s + channels, total, channels, rate, level=0.3 + 0.2 * s) for s in range(n)]
    bank = ssa.MeterBank(n, channels, rate)
    meters = [oracle.Meter(channels, rate) for _ in range(n)]

    def after(i, pos, f):
        for s in range(n):
            meters[s].add_frames(xs[s][pos * channels:(pos + f) * channels])
        rec = bank.read()
        assert (rec["frames"] == pos + f).all()
        check_against_oracle(oracle, bank, meters, rec, (rate, channels, i, f))

    feed_blocks(bank, xs, blocks, channels, after)
    for s in range(n):
        hb, hs = bank.histograms(s)
        assert np.array_equal(hb, meters[s].block_hist()) and np.array_equal(hs, meters[s].st_hist()), s


def test_bank_equals_handles_bit_for_bit():
    """Eight streams and eight handles fed the same block sequences: integrated loudness, range, peaks bit for bit; momentary and
    short-term within 1e-9 LU (the handle sums the 3 s ring itself, the bank decomposes the window)."""
    n, rate, channels = 8, 48000, 2
    blocks = [480] * 12 + [4800] * 3 + [1, 127, 4801, 48000, 480] + [4800] * 7
    total = sum(blocks)
    xs = [material(300 + s, total, channels, rate, level=0.1 + 0.1 * s) for s in range(n)]
    bank = ssa.MeterBank(n, channels, rate)
    handles = []
    for _ in range(n):
        a = ssa.Analyzer()
        a.create_loudness_meter(channels, rate)
        handles.append(a)

    def after(i, pos, f):
        for s in range(n):
            handles[s].add_samples(xs[s][pos * channels:(pos + f) * channels])
        rec = bank.read()
        for s, h in enumerate(handles):
            r = rec[s]
            assert r["integrated"] == h.get_integrated_lufs() and r["loudness_range"] == h.get_loudness_range(), (i, s)
            assert close9(r["momentary"], h.get_momentary_lufs()) and close9(r["shortterm"], h.get_shortterm_lufs()), (i, s)
            tp, sp = bank.peaks(s)
            for c in range(channels):
                assert sp[c] == h.get_sample_peak_channel(c) and tp[c] == h.get_true_peak_channel(c), (i, s, c)
                assert r["sample_peak"][c] == sp[c] and r["true_peak"][c] == tp[c], (i, s, c)

    feed_blocks(bank, xs, blocks, channels, after)


def test_selective_reset(oracle):
    """Stream 1 is reset at a frame count that is not a multiple of the sub-block: the other streams stay bit-identical to a bank
    that was never reset, stream 1 matches a fresh oracle meter fed what came behind the reset."""
    n, rate, channels = 4, 48000, 2
    before = [4800, 4800, 127, 480, 4801]
    after_blocks = [480] * 5 + [4800] * 40 + [1, 48000]
    blocks = before + after_blocks
    total = sum(blocks)
    xs = [material(500 + s, total, channels, rate) for s in range(n)]
    a, b = ssa.MeterBank(n, channels, rate), ssa.MeterBank(n, channels, rate)
    fresh = oracle.Meter(channels, rate)
    cut = sum(before)
    assert cut % 4800 != 0
    feed_blocks(a, xs, before, channels)
    feed_blocks(b, xs, before, channels)
    a.reset([1])
    pos = cut
    for f in after_blocks:
        blk = np.stack([x[pos * channels:(pos + f) * channels] for x in xs])
        a.add(blk)
        b.add(blk)
        fresh.add_frames(xs[1][pos * channels:(pos + f) * channels])
        pos += f
        ra, rb = a.read(), b.read()
        for s in (0, 2, 3):
            assert ra[s].tobytes() == rb[s].tobytes(), (pos, s)
        assert ra[1]["frames"] == pos - cut
        check_against_oracle(oracle, a, [fresh], ra[1:2], ("reset", pos), peaks=False)
    for s in (0, 2, 3):
        assert all(np.array_equal(u, v) for u, v in zip(a.histograms(s), b.histograms(s))), s
        assert all(np.array_equal(u, v) for u, v in zip(a.peaks(s), b.peaks(s))), s
    tp, sp = a.peaks(1)
    for c in range(channels):
        assert sp[c] == fresh.sample_peak(c) and same_peak(tp[c], max(fresh.true_peak(c), fresh.sample_peak(c)))
    hb, hs = a.histograms(1)
    assert np.array_equal(hb, fresh.block_hist()) and np.array_equal(hs, fresh.st_hist())
    a.reset()
    assert (a.read()["frames"] == 0).all() and (a.read()["momentary"] == -np.inf).all()


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_nonfinite_sample_poisons_its_own_stream_only(oracle, value):
    n, rate, channels = 3, 48000, 2
    blocks = [4800] * 6 + [480] * 10 + [4800] * 40
    total = sum(blocks)
    xs = [material(700 + s, total, channels, rate) for s in range(n)]
    bad = [x.copy() for x in xs]
    bad[1][2 * (4800 * 7 + 333)] = np.float32(value)
    dirty, clean = ssa.MeterBank(n, channels, rate), ssa.MeterBank(n, channels, rate)
    m = oracle.Meter(channels, rate)
    pos = 0
    for f in blocks:
        dirty.add(np.stack([x[pos * channels:(pos + f) * channels] for x in bad]))
        clean.add(np.stack([x[pos * channels:(pos + f) * channels] for x in xs]))
        m.add_frames(bad[1][pos * channels:(pos + f) * channels])
        pos += f
        rd, rc = dirty.read(), clean.read()
        assert rd[0].tobytes() == rc[0].tobytes() and rd[2].tobytes() == rc[2].tobytes(), pos
        check_against_oracle(oracle, dirty, [m], rd[1:2], (value, pos), peaks=False)
    for s in (0, 2):
        assert all(np.array_equal(u, v) for u, v in zip(dirty.histograms(s), clean.histograms(s)))


def test_input_forms(oracle):
    """add_pcm of s16, s24 and f64 equals add of the decoded f32; add_device equals add."""
    n, rate, channels = 3, 48000, 2
    blocks = [480, 4800, 127, 4801]
    total = sum(blocks)
    xs = np.stack([material(900 + s, total, channels, rate) for s in range(n)])      # [n][total * C]
    rng = np.random.default_rng(5)
    raws = {
        L.SS_PCM_S16: rng.integers(-32768, 32767, xs.shape, dtype=np.int16),
        L.SS_PCM_F64: xs.astype(np.float64) * 0.9,
    }
    s24 = rng.integers(-(1 << 23), (1 << 23) - 1, xs.shape, dtype=np.int32)
    raws[L.SS_PCM_S24] = np.stack([s24 & 0xFF, (s24 >> 8) & 0xFF, (s24 >> 16) & 0xFF], axis=-1).astype(np.uint8)   # [n][samples][3]
    for fmt, raw in raws.items():
        decoded = np.stack([oracle.pcm_to_f32(raw[s].tobytes(), fmt) for s in range(n)])
        a, b = ssa.MeterBank(n, channels, rate), ssa.MeterBank(n, channels, rate)
        pos = 0
        for f in blocks:
            a.add_pcm(np.ascontiguousarray(raw[:, pos * channels:(pos + f) * channels]), fmt)
            b.add(decoded[:, pos * channels:(pos + f) * channels])
            pos += f
            assert a.read().tobytes() == b.read().tobytes(), (fmt, pos)
    # device-resident input: a batch's input buffer (stream s at s * total * C floats: more than a call's frames)
    src = ssa.Batch(rate, channels, n, total, flags=L.SS_BATCH_LUFS)
    src.upload(0, xs)
    base = src.input_device_ptr()
    a, b = ssa.MeterBank(n, channels, rate), ssa.MeterBank(n, channels, rate)
    pos = 0
    for f in blocks:
        a.add_device(base + 4 * pos * channels, f, total * channels)
        b.add(xs[:, pos * channels:(pos + f) * channels])
        pos += f
        assert a.read().tobytes() == b.read().tobytes(), pos
    for s in range(n):
        assert all(np.array_equal(u, v) for u, v in zip(a.histograms(s), b.histograms(s)))
    src.close()


def test_staging_regrows_between_calls(oracle):
    """Six calls with nothing that waits for the stream between them: every call but the last grows or reuses the page-locked
    staging buffer while the previous call's copy may still be in flight (64 frames, 4 800: grown, 64 of s24: reused, a ragged
    call of (20 000, 0, 7): grown, a reset's list and 960 frames: reused).  Then one read: every stream equals a handle fed and
    reset the same way, as test_bank_equals_handles_bit_for_bit holds them."""
    n, rate, channels = 3, 48000, 2
    ragged = [20000, 0, 7]
    s24 = np.random.default_rng(11).integers(-(1 << 23), (1 << 23) - 1, (n, 64 * channels), dtype=np.int32)
    raw = np.stack([s24 & 0xFF, (s24 >> 8) & 0xFF, (s24 >> 16) & 0xFF], axis=-1).astype(np.uint8)          # [n][samples][3]
    decoded = [oracle.pcm_to_f32(raw[s].tobytes(), L.SS_PCM_S24) for s in range(n)]
    xs = [material(1100 + s, 64 + 4800 + ragged[s] + 960, channels, rate, level=0.2 + 0.2 * s) for s in range(n)]
    cut = [np.cumsum([0, 64, 4800, ragged[s], 960]) * channels for s in range(n)]
    part = lambda s, i: xs[s][cut[s][i]:cut[s][i + 1]]

    bank = ssa.MeterBank(n, channels, rate)
    bank.add(np.stack([part(s, 0) for s in range(n)]))
    bank.add(np.stack([part(s, 1) for s in range(n)]))
    bank.add_pcm(raw, L.SS_PCM_S24)
    bank.add_ragged([part(s, 2) if ragged[s] else None for s in range(n)])
    bank.reset([1])
    bank.add(np.stack([part(s, 3) for s in range(n)]))
    rec = bank.read()

    for s in range(n):
        h = ssa.Analyzer()
        h.create_loudness_meter(channels, rate)
        for blk in (part(s, 0), part(s, 1), decoded[s], part(s, 2)):
            h.add_samples(blk)
        if s == 1:
            h.reset()
        h.add_samples(part(s, 3))
        r = rec[s]
        assert r["frames"] == (960 if s == 1 else 64 + 4800 + 64 + ragged[s] + 960), s
        assert r["integrated"] == h.get_integrated_lufs() and r["loudness_range"] == h.get_loudness_range(), s
        assert close9(r["momentary"], h.get_momentary_lufs()) and close9(r["shortterm"], h.get_shortterm_lufs()), s
        tp, sp = bank.peaks(s)
        for c in range(channels):
            assert sp[c] == h.get_sample_peak_channel(c) and tp[c] == h.get_true_peak_channel(c), (s, c)
            assert r["sample_peak"][c] == sp[c] and r["true_peak"][c] == tp[c], (s, c)


def test_scale_1024_live_inputs(oracle):
    """1024 stereo 48 kHz streams fed 10 ms blocks for 5 s straight from device memory (a batch's synthesised input): 32
    sampled streams against the oracle, every stream's integrated loudness and range against the batch pass over the same
    material (not bit for bit: calls of different lengths take different time-domain forms)."""
    n, rate, channels, block, secs = 1024, 48000, 2, 480, 5
    frames = rate * secs
    b = ssa.Batch(rate, channels, n, frames, flags=L.SS_BATCH_LUFS)
    b.synthesize(seed=0xBA2C)
    b.run()
    b.sync()
    res = b.results()
    base = b.input_device_ptr()
    bank = ssa.MeterBank(n, channels, rate)
    sample = list(range(0, n, n // 32))
    xs = {s: b.download_input(s) for s in sample}
    meters = {s: oracle.Meter(channels, rate) for s in sample}
    for t in range(frames // block):
        pos = t * block
        bank.add_device(base + 4 * pos * channels, block, frames * channels)
        for s in sample:
            meters[s].add_frames(xs[s][pos * channels:(pos + block) * channels])
        if t % 50 == 49:
            rec = bank.read()
            check_against_oracle(oracle, bank, [meters[s] for s in sample], rec[sample], ("scale", t), peaks=False)
    rec = bank.read()
    assert (rec["frames"] == frames).all()
    for s in range(n):
        assert same_lufs(rec[s]["integrated"], res[s].integrated_lufs), (s, rec[s]["integrated"], res[s].integrated_lufs)
        assert same_lufs(rec[s]["loudness_range"], res[s].loudness_range), (s, rec[s]["loudness_range"], res[s].loudness_range)
    b.close()


def test_refusal_codes():
    lib = L.lib()
    h = C.c_void_p()
    for args, want in [((1, 0, 48000, 0), L.SS_ERR_NOMEM), ((1, 65, 48000, 0), L.SS_ERR_NOMEM), ((1, 2, 15, 0), L.SS_ERR_NOMEM),
                       ((1, 2, 2822401, 0), L.SS_ERR_NOMEM), ((0, 2, 48000, 0), L.SS_ERR_INVALID_ARG),
                       ((1, 2, 48000, 3), L.SS_ERR_INVALID_ARG)]:
        assert lib.ss_meter_bank_create(*args, C.byref(h)) == want, args
        assert not h.value
    bank = ssa.MeterBank(2, 2, 48000)
    x = np.zeros((2, 960), np.float32)
    bank.add(x)
    before = bank.read()
    hb = bank._h
    f32p = C.POINTER(C.c_float)
    assert lib.ss_meter_bank_add(hb, None, 4) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_add(hb, None, 0) == L.SS_OK                                    # frames == 0: a no-op
    assert lib.ss_meter_bank_add(hb, x.ctypes.data_as(f32p), 0) == L.SS_OK
    assert lib.ss_meter_bank_add_device(hb, None, 4, 8) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_add_device(hb, C.c_void_p(0x1000), 4, 7) == L.SS_ERR_INVALID_ARG   # stride < frames * channels
    assert lib.ss_meter_bank_add_device(hb, None, 0, 0) == L.SS_OK
    assert lib.ss_meter_bank_add_pcm(hb, x.ctypes.data, 4, 7) == L.SS_ERR_INVALID_ARG     # no such format
    assert lib.ss_meter_bank_add_pcm(hb, None, 4, L.SS_PCM_S16) == L.SS_ERR_INVALID_ARG
    assert bank.read().tobytes() == before.tobytes()
    idx = (C.c_uint32 * 1)(2)
    assert lib.ss_meter_bank_reset(hb, idx, 1) == L.SS_ERR_INVALID_ARG
    out = np.empty(2, ssa.meter_bank.READING_DTYPE)
    assert lib.ss_meter_bank_read(hb, out.ctypes.data, 1) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_read(hb, None, 2) == L.SS_ERR_INVALID_ARG
    pk = np.empty(2)
    dp = C.POINTER(C.c_double)
    assert lib.ss_meter_bank_peaks(hb, 0, pk.ctypes.data_as(dp), None, 1) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_peaks(hb, 2, pk.ctypes.data_as(dp), None, 2) == L.SS_ERR_INVALID_ARG
    hist = np.empty(2000, np.uint64)
    assert lib.ss_meter_bank_histograms(hb, 2, hist.ctypes.data_as(C.POINTER(C.c_uint64))) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_histograms(hb, 0, None) == L.SS_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        bank.add(np.zeros(3, np.float32))                                                  # a partial frame
    with pytest.raises(AnalyzerError):
        bank.reset([5])
