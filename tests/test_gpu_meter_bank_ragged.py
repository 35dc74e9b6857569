"""Ragged meter-bank adds on the MI355X (ss_meter_bank_add_ragged*): every stream its own frame count per call.  The contract is
the bank's, per stream: after a ragged call stream s is in the state an `Analyzer` is in after one add_samples of the same frames
— integrated loudness, range and every peak bit for bit, momentary and short-term within 1e-9 LU (the bound
tests/test_gpu_meter_bank.py holds a bank to against handles: the handle sums its 3 s ring, the bank decomposes the window).
The handle exposes no histograms; the bank's are held, bit for bit, to the oracle meter's fed the same blocks.

A stream takes the one-wave form of k_time_domain for a call of up to `tile_len` frames and the eight-wave workgroup beyond
(td_launch_c); tile_len = td_ring_tile_frames(channels, S), from the chunk-length model of ss_time_domain.hip:
    48 kHz stereo 960 (L = 30, five tiles per sub-block), 44.1 kHz stereo 1470 (L = 49), 48 kHz 5 channels 600 (L = 50)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.meter_bank import MeterBank

from conftest import make_multich, make_stereo
from oracle.render import spectrum_columns_f32

pytestmark = pytest.mark.gpu

TILE_LEN = {(48000, 2): 960, (44100, 2): 1470, (48000, 5): 600}
N = 16384


def material(seed, frames, channels, rate, level=0.5):
    """interleaved f32 [frames * channels]"""
    if channels == 2:
        return make_stereo(seed, frames, rate, level=level)
    return make_multich(seed, frames, channels, rate, level=level)


def new_handle(channels, rate):
    a = ssa.Analyzer()
    a.create_loudness_meter(channels, rate)
    return a


def same_bits(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def close9(a, b):
    return same_bits(a, b) or abs(a - b) <= 1e-9


def check_stream_against_handle(bank, s, r, h, fed, tag):
    assert int(r["frames"]) == fed, (tag, s, r["frames"], fed)
    print(tag, s, "I", r["integrated"], h.get_integrated_lufs(), "LRA", r["loudness_range"], h.get_loudness_range(),
          "M", r["momentary"] - h.get_momentary_lufs(), "S", r["shortterm"] - h.get_shortterm_lufs())
    assert same_bits(r["integrated"], h.get_integrated_lufs()), (tag, s, "I", r["integrated"], h.get_integrated_lufs())
    assert same_bits(r["loudness_range"], h.get_loudness_range()), (tag, s, "LRA", r["loudness_range"], h.get_loudness_range())
    assert close9(r["momentary"], h.get_momentary_lufs()), (tag, s, "M", r["momentary"], h.get_momentary_lufs())
    assert close9(r["shortterm"], h.get_shortterm_lufs()), (tag, s, "S", r["shortterm"], h.get_shortterm_lufs())
    tp, sp = bank.peaks(s)
    for c in range(bank.channels):
        assert same_bits(sp[c], h.get_sample_peak_channel(c)), (tag, s, c, "sample peak", sp[c], h.get_sample_peak_channel(c))
        assert same_bits(tp[c], h.get_true_peak_channel(c)), (tag, s, c, "true peak", tp[c], h.get_true_peak_channel(c))
        if c < 2:
            assert same_bits(r["sample_peak"][c], sp[c]) and same_bits(r["true_peak"][c], tp[c]), (tag, s, c)


def special_schedule(rate, channels, n=6, calls=12, seed=11):
    """[call][stream] frame counts: every length of the issue's list on some stream, different streams drawing different ones in
    the same call; the three lengths beyond 3 s once each, on different streams, so that every stream stays under 10 s"""
    S, tile = (rate + 5) // 10, TILE_LEN[(rate, channels)]
    small = [0, 1, S - 1, S, S + 1, tile, tile + 1, 2 * S + 3]
    rng = np.random.default_rng(seed)
    sched = []
    for i in range(calls):
        rot = rng.permutation(len(small))
        sched.append([small[(rot[s % len(small)])] for s in range(n)])
    # every small length appears: call i gives stream s small[(i + s) % 8] in the first eight calls' diagonal
    for i in range(len(small)):
        sched[i][i % n] = small[i]
    sched[3][0] = 70 * S + 11                               # three pieces: 32 S, 32 S, 6 S + 11
    sched[6][1] = 32 * S                                    # exactly one piece
    sched[8][2] = 32 * S + 1                                # a second piece of one frame
    sched[8][4] = 32 * S
    seen = {f for row in sched for f in row}
    assert seen >= set(small) | {70 * S + 11, 32 * S, 32 * S + 1}
    assert all(len(set(row)) > 1 for row in sched)
    assert all(sum(row[s] for row in sched) < 10 * rate for s in range(n))
    return sched


@pytest.mark.parametrize("rate,channels", [(48000, 2), (44100, 2), (48000, 5)])
def test_bank_equals_handles_bit_for_bit(oracle, rate, channels):
    """Six streams, six handles, twelve ragged calls whose lengths sit on both sides of tile_len, of the sub-block and of the
    32-sub-block piece; every reading behind every call, the histograms against the oracle meter's."""
    n = 6
    sched = special_schedule(rate, channels, n)
    total = [sum(row[s] for row in sched) for s in range(n)]
    xs = [material(40 + s + channels, total[s], channels, rate, level=0.2 + 0.1 * s) for s in range(n)]
    bank = MeterBank(n, channels, rate)
    handles = [new_handle(channels, rate) for _ in range(n)]
    meters = [oracle.Meter(channels, rate) for _ in range(n)]
    fed = [0] * n
    for i, row in enumerate(sched):
        blocks = [xs[s][fed[s] * channels:(fed[s] + f) * channels] if f else None for s, f in enumerate(row)]
        bank.add_ragged(blocks)
        for s, f in enumerate(row):
            if f:
                handles[s].add_samples(blocks[s])
                meters[s].add_frames(blocks[s])
            fed[s] += f
        rec = bank.read()
        for s in range(n):
            check_stream_against_handle(bank, s, rec[s], handles[s], fed[s], (rate, channels, i, row[s]))
            hb, hs = bank.histograms(s)
            assert np.array_equal(hb, meters[s].block_hist()) and np.array_equal(hs, meters[s].st_hist()), (i, s)


def snapshot(bank, s):
    return (bank.read()[s].tobytes(), [h.tobytes() for h in bank.histograms(s)], [p.tobytes() for p in bank.peaks(s)])


def test_untouched_streams():
    """A stream given no frames keeps its record, histograms and peaks byte for byte while the others advance, at every kind of
    call (one wave, eight waves, both in one call, several pieces); an all-zero call changes nothing for anyone."""
    n, rate, channels = 5, 48000, 2
    xs = [material(60 + s, 4 * rate, channels, rate) for s in range(n)]
    bank = MeterBank(n, channels, rate)
    bank.enable_spectrum()
    bank.add(np.stack([x[:2 * 7001] for x in xs]))          # everyone has a state worth keeping
    fed = [7001] * n
    rows0, _ = bank.spectrum()
    for k, row in enumerate([[480, 0, 480, 0, 1], [4801, 0, 0, 961, 960], [0, 0, 153601, 17, 0], [1, 0, 0, 0, 0]]):
        before = [snapshot(bank, s) for s in range(n)]
        spec_before, _ = bank.spectrum()
        bank.add_ragged([xs[s][fed[s] * 2:(fed[s] + f) * 2] if f else None for s, f in enumerate(row)])
        rec = bank.read()
        spec_after, _ = bank.spectrum()
        for s, f in enumerate(row):
            fed[s] += f
            assert int(rec[s]["frames"]) == fed[s]
            if f == 0:
                assert snapshot(bank, s) == before[s], (k, s)
                assert spec_after[s].tobytes() == spec_before[s].tobytes(), (k, s)
            else:
                assert rec[s].tobytes() != before[s][0], (k, s)
    assert fed[1] == 7001 and np.array_equal(bank.spectrum()[0][1], rows0[1])
    before = [snapshot(bank, s) for s in range(n)]
    spec_before, _ = bank.spectrum()
    bank.add_ragged([None] * n)
    bank.add_ragged([np.zeros(0, np.float32)] * n)
    zeros = (C.c_uint64 * n)()
    assert L.lib().ss_meter_bank_add_ragged(bank._h, None, zeros) == L.SS_OK
    assert L.lib().ss_meter_bank_add_ragged_device(bank._h, None, zeros, 0) == L.SS_OK
    assert [snapshot(bank, s) for s in range(n)] == before
    assert bank.spectrum()[0].tobytes() == spec_before.tobytes()


def test_uniform_equivalence():
    """add and add_ragged with equal lengths: records, histograms, spectrum rows and statuses identical after every call — one
    wave (480, 960 = tile_len), eight waves (961, 4801), several pieces (32 S + 7) — and uniform adds behind ragged ones keep
    every stream's window where its own frames put it."""
    n, rate, channels = 4, 48000, 2
    lengths = [480, 960, 961, 1, 4801, 32 * 4800 + 7, 127, 16384, 3]
    total = sum(lengths)
    xs = [material(80 + s, total, channels, rate, level=0.3 + 0.1 * s) for s in range(n)]
    a, b = MeterBank(n, channels, rate), MeterBank(n, channels, rate)
    a.enable_spectrum()
    b.enable_spectrum()
    pos = 0
    for i, f in enumerate(lengths):
        blk = [x[pos * 2:(pos + f) * 2] for x in xs]
        a.add(np.stack(blk))
        if i % 3 == 2:
            b.add(np.stack(blk))                             # a uniform add between ragged ones
        else:
            b.add_ragged(blk)
        pos += f
        assert a.read().tobytes() == b.read().tobytes(), (i, f)
        ra, sa = a.spectrum()
        rb, sb = b.spectrum()
        assert ra.tobytes() == rb.tobytes() and np.array_equal(sa, sb), (i, f)
    for s in range(n):
        assert all(np.array_equal(u, v) for u, v in zip(a.histograms(s), b.histograms(s))), s
    ca, _ = a.spectrum_columns(160, "reference")
    cb, _ = b.spectrum_columns(160, "reference")
    assert ca.tobytes() == cb.tobytes()


def test_selective_reset_between_ragged_calls():
    """Stream 1 is reset between ragged calls, off the sub-block grid: it equals a fresh handle fed what came after; the other
    streams equal a twin bank that was never reset."""
    n, rate, channels = 4, 48000, 2
    before = [[4800, 127, 961, 0], [480, 4801, 1, 333], [0, 960, 4800, 4800]]
    after = [[480, 4801, 0, 17], [961, 0, 4800, 480], [32 * 4800 + 1, 480, 959, 0], [1, 4799, 480, 9600]]
    xs = [material(90 + s, 5 * rate, channels, rate) for s in range(n)]
    a, b = MeterBank(n, channels, rate), MeterBank(n, channels, rate)
    fresh = new_handle(channels, rate)
    fed, since = [0] * n, 0
    for k, row in enumerate(before + after):
        if k == len(before):
            assert fed[1] % 4800 != 0
            a.reset([1])
        blocks = [xs[s][fed[s] * 2:(fed[s] + f) * 2] if f else None for s, f in enumerate(row)]
        a.add_ragged(blocks)
        b.add_ragged(blocks)
        for s, f in enumerate(row):
            fed[s] += f
        if k >= len(before):
            if row[1]:
                fresh.add_samples(blocks[1])
            since += row[1]
            ra, rb = a.read(), b.read()
            for s in (0, 2, 3):
                assert ra[s].tobytes() == rb[s].tobytes(), (k, s)
            check_stream_against_handle(a, 1, ra[1], fresh, since, ("reset", k))
    for s in (0, 2, 3):
        assert all(np.array_equal(u, v) for u, v in zip(a.histograms(s), b.histograms(s))), s
        assert all(np.array_equal(u, v) for u, v in zip(a.peaks(s), b.peaks(s))), s


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_nonfinite_sample_poisons_its_own_stream_only(value):
    """The planted stream reads as a handle fed the same samples; the others stay byte-equal to a clean twin bank."""
    n, rate, channels = 3, 48000, 2
    sched = [[4800, 480, 961], [480, 4801, 0], [961, 4800, 4800], [0, 480, 32 * 4800 + 5], [4800, 9600, 480], [480, 4800, 4800]]
    xs = [material(700 + s, 5 * rate, channels, rate) for s in range(n)]
    bad = [x.copy() for x in xs]
    bad[1][2 * (480 + 333) + 1] = np.float32(value)          # inside call 1's eight-wave block of stream 1
    dirty, clean = MeterBank(n, channels, rate), MeterBank(n, channels, rate)
    h = new_handle(channels, rate)
    fed = [0] * n
    for k, row in enumerate(sched):
        dirty.add_ragged([bad[s][fed[s] * 2:(fed[s] + f) * 2] if f else None for s, f in enumerate(row)])
        clean.add_ragged([xs[s][fed[s] * 2:(fed[s] + f) * 2] if f else None for s, f in enumerate(row)])
        h.add_samples(bad[1][fed[1] * 2:(fed[1] + row[1]) * 2])
        for s, f in enumerate(row):
            fed[s] += f
        rd, rc = dirty.read(), clean.read()
        assert rd[0].tobytes() == rc[0].tobytes() and rd[2].tobytes() == rc[2].tobytes(), k
        check_stream_against_handle(dirty, 1, rd[1], h, fed[1], (value, k))
    for s in (0, 2):
        assert all(np.array_equal(u, v) for u, v in zip(dirty.histograms(s), clean.histograms(s)))


def test_input_forms(oracle):
    """One ragged schedule as f32, as s16 and s24 (material pre-quantised) and from device memory: byte-equal banks."""
    n, rate, channels = 4, 48000, 2
    sched = [[480, 0, 961, 17], [4801, 480, 0, 960], [1, 32 * 4800 + 3, 333, 0], [0, 0, 0, 5], [127, 4800, 4799, 9601]]
    total = [sum(row[s] for row in sched) for s in range(n)]
    rng = np.random.default_rng(9)
    for fmt in (L.SS_PCM_S16, L.SS_PCM_S24):
        if fmt == L.SS_PCM_S16:
            raw = [rng.integers(-20000, 20000, total[s] * channels, dtype=np.int16).view(np.uint8) for s in range(n)]
            sb = 2
        else:
            q = [rng.integers(-(1 << 22), 1 << 22, total[s] * channels, dtype=np.int32) for s in range(n)]
            raw = [np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=-1).astype(np.uint8).reshape(-1) for v in q]
            sb = 3
        xs = [oracle.pcm_to_f32(raw[s].tobytes(), fmt) for s in range(n)]
        cap = max(max(row) for row in sched)
        src = ssa.Batch(rate, channels, n, cap, flags=L.SS_BATCH_LUFS)      # a device buffer: stream s at s * cap * C floats
        f32, pcm, dev = MeterBank(n, channels, rate), MeterBank(n, channels, rate), MeterBank(n, channels, rate)
        fed = [0] * n
        for k, row in enumerate(sched):
            f32.add_ragged([xs[s][fed[s] * 2:(fed[s] + f) * 2] if f else None for s, f in enumerate(row)])
            pcm.add_ragged_pcm([raw[s][fed[s] * 2 * sb:(fed[s] + f) * 2 * sb] if f else None for s, f in enumerate(row)], fmt)
            padded = np.zeros((n, cap * channels), np.float32)
            for s, f in enumerate(row):
                padded[s, :f * 2] = xs[s][fed[s] * 2:(fed[s] + f) * 2]
            src.upload(0, padded)
            src.sync()
            dev.add_ragged_device(src.input_device_ptr(), row, cap * channels)
            want = f32.read().tobytes()
            assert pcm.read().tobytes() == want, (fmt, k)
            assert dev.read().tobytes() == want, (fmt, k)          # (waits: the buffer may be overwritten now)
            for s, f in enumerate(row):
                fed[s] += f
        assert [int(v) for v in f32.read()["frames"]] == total
        for s in range(n):
            for other in (pcm, dev):
                assert all(np.array_equal(u, v) for u, v in zip(f32.histograms(s), other.histograms(s))), (fmt, s)
        src.close()


# ---- spectra ----------------------------------------------------------------------------------------------------------------------
class History:
    """The host's copy of every stream's input, as tests/test_gpu_meter_bank_spectrum.py keeps it: the newest N frames of a
    stream with zeros in front."""

    def __init__(self, n, channels):
        self.blocks = [[] for _ in range(n)]
        self.channels = channels

    def add(self, s, block):
        self.blocks[s].append(np.asarray(block, np.float32).reshape(-1, self.channels))

    def fed(self, s):
        return sum(b.shape[0] for b in self.blocks[s])

    def window(self, s):
        x = np.concatenate([np.zeros((N, self.channels), np.float32)] + self.blocks[s], axis=0)
        return x[-N:]


def signals(win):
    from oracle import pyoracle as po
    if win.shape[1] == 2:
        return list(po.mid_side(win.reshape(-1)))
    return [np.ascontiguousarray(win[:, c]) for c in range(win.shape[1])]


def handle_fft(an, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty((N // 2 + 1, 2), np.float64)
    n = C.c_size_t(0)
    rc = L.lib().ss_get_fft(an._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, out.ctypes.data_as(C.POINTER(C.c_double)),
                            out.shape[0], C.byref(n))
    return rc, out[:n.value].copy()


def check_rows_against_handle(bank, hist, an, streams, tag, columns=True):
    rows, st = bank.spectrum()
    pink = bank.spectrum_pink()
    _, _, chart_x = bank.spectrum_layout()
    integ = bank.read()["integrated"]
    cols, cst = bank.spectrum_columns(160, "reference") if columns else (None, st)
    assert np.array_equal(cst, st)
    for s in streams:
        for r, sig in enumerate(signals(hist.window(s))):
            rc, ref = handle_fft(an, sig)
            assert st[s, r] == rc, (tag, s, r, st[s, r], rc)
            if rc:
                assert np.isnan(rows[s, r]).all(), (tag, s, r)
                continue
            got = rows[s, r].astype(np.float64) + pink
            assert np.array_equal(ref[:, 0], chart_x) and np.array_equal(got, ref[:, 1]), (tag, s, r, hist.fed(s))
            if columns:
                g = np.float32(-13.0) - np.float32(integ[s])
                assert np.array_equal(cols[s, r], spectrum_columns_f32(got.astype(np.float32), chart_x, g, 160), equal_nan=True), (tag, s, r)
    return st


@pytest.mark.parametrize("channels", [2, 5])
def test_spectra_per_stream(channels):
    """Every stream's window follows its own frame counter: totals that end on an odd start (stream 0), on a multiple of 16384
    (stream 1), under 16384 frames (stream 2), behind one call of more than 16384 frames (stream 3), and a stream that never got
    a frame (stream 4); rows bit-equal to ss_get_fft of the stream's own window, the columns to the host reduction."""
    rate, n = 48000, 5
    sched = [[1001, 480, 100, 0, 0], [4801, 16384 - 480, 0, 20001, 0], [0, 16384, 481, 3, 0], [12345, 0, 1, 480, 0], [480, 16384, 0, 0, 0]]
    bank = MeterBank(n, channels, rate)
    bank.enable_spectrum()
    an = ssa.Analyzer(2, rate)
    hist = History(n, channels)
    for k, row in enumerate(sched):
        blocks = [material(13 * k + s, f, channels, rate) if f else None for s, f in enumerate(row)]
        bank.add_ragged(blocks)
        for s, f in enumerate(row):
            if f:
                hist.add(s, blocks[s])
        st = check_rows_against_handle(bank, hist, an, range(n), (channels, k))
        assert (st == L.SS_OK).all()
    fed = [hist.fed(s) for s in range(n)]
    assert fed[0] > N and fed[0] % 2 == 1 and fed[1] % N == 0 and fed[1] > N and 0 < fed[2] < N and fed[3] > N and fed[4] == 0
    # a uniform add behind the ragged ones moves every stream's own window
    blocks = [material(200 + s, 777, channels, rate) for s in range(n)]
    bank.add(np.stack(blocks))
    for s in range(n):
        hist.add(s, blocks[s])
    check_rows_against_handle(bank, hist, an, range(n), (channels, "uniform"))
    # enabling again zeroes ring and counters
    bank.enable_spectrum()
    rows, st = bank.spectrum()
    assert (st == 0).all() and (rows == np.float32(-150.0)).all()


def test_spectrum_nan_leaves_with_its_own_streams_frames():
    """A NaN in stream 1: its rows read SS_ERR_NAN until stream 1 ALONE has moved 16384 frames past it, however far the others
    move meanwhile; their statuses stay SS_OK."""
    rate, n = 48000, 3
    bank = MeterBank(n, 2, rate)
    bank.enable_spectrum()
    an = ssa.Analyzer(2, rate)
    hist = History(n, 2)
    first = [material(s, 5000, 2, rate) for s in range(n)]
    first[1][2 * 4000] = np.nan                               # 999 frames behind it in this call
    sched = [[5000, 5000, 5000], [16384, 8000, 0], [20000, 7384, 480], [480, 1, 16384]]
    for k, row in enumerate(sched):
        blocks = first if k == 0 else [material(31 * k + s, f, 2, rate) if f else None for s, f in enumerate(row)]
        bank.add_ragged(blocks)
        for s, f in enumerate(row):
            if f:
                hist.add(s, blocks[s])
        st = check_rows_against_handle(bank, hist, an, range(n), ("nan", k), columns=False)
        inside = hist.fed(1) - 4000 <= N                       # the NaN is frame 4000 of stream 1
        assert (st[1] == (L.SS_ERR_NAN if inside else L.SS_OK)).all(), (k, st[1])
        assert (st[0] == L.SS_OK).all() and (st[2] == L.SS_OK).all(), k
    assert hist.fed(1) - 4000 == N + 1                         # the last call moved it out by one frame


def test_refusals():
    """Every check of the ragged calls; a refused call leaves the bank as it was."""
    lib = L.lib()
    n = 3
    bank = MeterBank(n, 2, 48000)
    x = np.zeros(2 * 960, np.float32)
    bank.add_ragged([x, x[:480], None])
    before = bank.read().tobytes()
    hb = bank._h
    ptrs = (C.c_void_p * n)(x.ctypes.data, x.ctypes.data, x.ctypes.data)
    frames = (C.c_uint64 * n)(4, 0, 4)
    assert lib.ss_meter_bank_add_ragged(hb, ptrs, None) == L.SS_ERR_INVALID_ARG                 # no frames array
    assert lib.ss_meter_bank_add_ragged_pcm(hb, ptrs, None, L.SS_PCM_S16) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_add_ragged_device(hb, C.c_void_p(0x1000), None, 64) == L.SS_ERR_INVALID_ARG
    holes = (C.c_void_p * n)(x.ctypes.data, None, None)
    assert lib.ss_meter_bank_add_ragged(hb, holes, frames) == L.SS_ERR_INVALID_ARG              # pcm[2] NULL with frames[2] > 0
    assert lib.ss_meter_bank_add_ragged(hb, None, frames) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_add_ragged_pcm(hb, holes, frames, L.SS_PCM_S16) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_add_ragged_pcm(hb, ptrs, frames, 7) == L.SS_ERR_INVALID_ARG        # no such format
    assert lib.ss_meter_bank_add_ragged_device(hb, C.c_void_p(0x1000), frames, 7) == L.SS_ERR_INVALID_ARG   # stride < 4 * 2
    assert lib.ss_meter_bank_add_ragged_device(hb, None, frames, 8) == L.SS_ERR_INVALID_ARG
    huge = (C.c_uint64 * n)(4, (1 << 40) + 1, 0)
    assert lib.ss_meter_bank_add_ragged(hb, ptrs, huge) == L.SS_ERR_NOMEM                       # no buffer holds it
    assert lib.ss_meter_bank_add_ragged_pcm(hb, ptrs, huge, L.SS_PCM_S16) == L.SS_ERR_NOMEM
    assert lib.ss_meter_bank_add_ragged_device(hb, C.c_void_p(0x1000), huge, 1 << 50) == L.SS_ERR_NOMEM
    summed = (C.c_uint64 * n)(1 << 38, 1 << 38, 1 << 38)                                        # each fits, together they do not
    assert lib.ss_meter_bank_add_ragged(hb, ptrs, summed) == L.SS_ERR_NOMEM
    assert lib.ss_meter_bank_add_ragged(None, ptrs, frames) == L.SS_ERR_INVALID_ARG             # a device is there
    assert bank.read().tobytes() == before
    with pytest.raises(ValueError):
        bank.add_ragged([x, x])                                                                  # a block per stream
    with pytest.raises(ValueError):
        bank.add_ragged([x, x[:3], None])                                                        # a partial frame
    with pytest.raises(ValueError):
        bank.add_ragged_device(0x1000, [1, 2], 8)
    assert bank.read().tobytes() == before


def test_scale_1024_jittered_streams():
    """1024 stereo 48 kHz streams, 60 ticks, each stream 432 ... 528 frames per tick and none with probability 1/20, spectrum on:
    eight sampled streams against their handles (meters and rows), every frame count against the stream's own sum."""
    rate, n, ticks = 48000, 1024, 60
    rng = np.random.default_rng(1024)
    lens = rng.integers(432, 529, (ticks, n))
    lens[rng.random((ticks, n)) < 0.05] = 0
    total = lens.sum(axis=0)
    base = np.stack([material(s, 530 * ticks, 2, rate) for s in range(16)])          # sixteen programmes at 1024 gains
    gains = rng.uniform(0.1, 1.0, n).astype(np.float32)
    sample = [int(s) for s in rng.choice(n, 8, replace=False)]
    bank = MeterBank(n, 2, rate)
    bank.enable_spectrum()
    handles = {s: new_handle(2, rate) for s in sample}
    hist = History(n, 2)
    an = ssa.Analyzer(2, rate)
    fed = np.zeros(n, np.int64)
    for t in range(ticks):
        blocks = [base[s % 16, fed[s] * 2:(fed[s] + lens[t, s]) * 2] * gains[s] if lens[t, s] else None for s in range(n)]
        bank.add_ragged(blocks)
        for s in sample:
            if lens[t, s]:
                handles[s].add_samples(blocks[s])
                hist.add(s, blocks[s])
        fed += lens[t]
        if t % 20 == 19:
            rec = bank.read()
            assert np.array_equal(rec["frames"].astype(np.int64), fed)
            for s in sample:
                check_stream_against_handle(bank, s, rec[s], handles[s], int(fed[s]), ("scale", t))
    assert np.array_equal(fed, total) and (total > N).all()
    rows, st = bank.spectrum()
    assert (st == 0).all()
    check_rows_against_handle(bank, hist, an, sample, "scale")


@pytest.mark.parametrize("seed", [3, 17, 42, 1009])
def test_randomised_ragged_programme(seed):
    """tools/fuzz_bank_ragged.py: random shape, stream count, schedule, resets, non-finite plants and input forms against handles."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_bank_ragged
    ok, msg = fuzz_bank_ragged.programme(seed)
    assert ok, msg
