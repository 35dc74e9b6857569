"""The decimation bins and the peaks of a batch, bit for bit against the oracle at planted inputs (48 kHz stereo, one bin per
millisecond: 48 frames = 96 samples a bin, twenty bins per 960-frame tile).

`k_time_domain` produces the bins inside its tile loop and the sample peak in its second filter pass; whichever phase
of the tile does that work, the (min, max) pairs of `Batch.waveform` and both values of `Batch.peaks` are the reference's: IEEE
minNum / maxNum over a bin (a NaN is ignored, a bin of nothing but NaN stays NaN, -0.0 < +0.0 is kept apart by sign), `if v > max`
for the peaks.  The planted positions are the ones at which a per-lane running minimum kept inside the true-peak trip (DESIGN 8:
considered, not built) would go wrong: the first and the last frame of a lane's run of fifteen frames, and of sixteen (three lanes
to a bin), of a bin, and the lanes on either side of a DPP row (15 | 16, 47 | 48) and of the wave's halves (31 | 32).

Material: +-1e-3 of noise under isolated single-sample spikes, so that the interpolated level stays under the largest sample
(the taps of the factor-4 branches are < 0.91) and `true_peak()` = max(interpolated, sample peak) is the sample peak itself — the
device's folded interpolator is within 1.1e-7 of the crate's chain, not bit-identical, and a bit-for-bit comparison of the true
peak needs material on which that does not show.  NaN payloads are not compared (both sides hold the default quiet NaN)."""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L

pytestmark = pytest.mark.gpu

RATE = 48000
TILE, BIN = 960, 48
FLAGS = L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK | L.SS_BATCH_WAVEFORM
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _noise(seed, frames, amp=1e-3):
    return np.random.default_rng(seed).uniform(-amp, amp, (frames, 2)).astype(np.float32)


def _same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    iv = np.uint32 if got.dtype == np.float32 else np.uint64
    return np.array_equal(got[~nan].view(iv), want[~nan].view(iv))


def _check(oracle, b, i, x, rate=RATE, tag=None):
    flat = np.ascontiguousarray(x.reshape(-1))
    want = np.ascontiguousarray(oracle.get_waveform(flat, x.shape[0] / rate)[:, 1]).astype(np.float32)     # window = duration
    got = np.ascontiguousarray(b.waveform(i).reshape(-1))[:want.size]
    if not _same_bits(got, want):
        bad = [k for k in range(want.size) if not _same_bits(got[k:k + 1], want[k:k + 1])]
        raise AssertionError((tag, i, "bins (2 bin + {0: min, 1: max})", bad[:10], got[bad[:10]], want[bad[:10]]))
    m = oracle.Meter(2, rate)
    m.add_frames(flat)
    tp, sp = b.peaks(i)
    ref_sp = np.array([m.sample_peak(c) for c in range(2)], np.float64)
    ref_tp = np.maximum(np.array([m.true_peak(c) for c in range(2)], np.float64), ref_sp)
    assert _same_bits(sp, ref_sp), (tag, i, "sample peak", sp, ref_sp)
    assert _same_bits(tp, ref_tp), (tag, i, "true peak", tp, ref_tp)


def _run(oracle, x, rate=RATE, tag=None, want_geo=None):
    ns, frames = x.shape[0], x.shape[1]
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=FLAGS)
    try:
        g = b.geometry
        assert g.waveform_fused == 1, g.waveform_fused
        if want_geo:
            want_geo(g)
        b.upload(0, x.reshape(-1))
        b.run(); b.sync()
        for i in range(ns):
            _check(oracle, b, i, x[i], rate, tag)
    finally:
        b.close()


def test_planted_extremes(oracle):
    """2 streams x 1.0 s.  Stream 0: the non-finite values and the signed zeros, each the only extreme of its bin, and a NaN eleven
    frames in front of a tile (inside the interpolator's reach of that tile, which takes the crate's loop).  Stream 1: finite
    spikes at the edges of lane runs, bins, DPP rows and wave halves; its largest sample is one isolated spike."""
    frames = RATE
    x = np.stack([_noise(1, frames), _noise(2, frames)])
    t = lambda k: TILE * k                                   # first frame of tile k (a sub-block is five tiles)
    s0 = x[0]
    s0[t(3) + 5 * BIN + 7, 0] = NAN                          # one NaN in a bin: ignored
    s0[t(4) + 2 * BIN:t(4) + 3 * BIN, :] = NAN               # a bin of nothing but NaN
    s0[t(6) + 9 * BIN + 47, 1] = INF                         # +Inf, the bin's last sample
    s0[t(8) + 0 * BIN, 0] = -INF                             # -Inf, a tile's (and a bin's, and a lane's) first sample
    s0[t(10) + 4 * BIN:t(10) + 5 * BIN, :] = np.abs(s0[t(10) + 4 * BIN:t(10) + 5 * BIN, :]) + np.float32(1e-6)
    s0[t(10) + 4 * BIN + 20, 1] = np.float32(-0.0)           # -0.0 the only non-positive sample: min = -0.0
    s0[t(12) + 7 * BIN:t(12) + 8 * BIN, :] = -np.abs(s0[t(12) + 7 * BIN:t(12) + 8 * BIN, :]) - np.float32(1e-6)
    s0[t(12) + 7 * BIN + 31, 0] = np.float32(0.0)            # +0.0 the only non-negative sample: max = +0.0
    s0[t(20) - 11, 1] = NAN                                  # eleven frames in front of tile 20
    s0[t(31) - 11, 0] = INF                                  # ... and of tile 31, an infinity
    s1 = x[1]
    amp = iter(np.float32(0.15 + 0.002 * k) * (1 if k % 2 else -1) for k in range(200))
    for lanes in (15, 16):                                   # frames per lane: today's trip, and a sixteen-frame one
        for k, lane in enumerate((0, 1, 14, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 49, 59, 63)):
            for edge in (0, lanes - 1):
                f = lane * lanes + edge
                if f < TILE:
                    tile = 2 + (3 * k + edge + lanes) % 40       # spread over the tiles, both channels
                    s1[t(tile) + f, (k + edge) & 1] = next(amp)
    for k, binq in enumerate((0, 5, 19)):                    # the first and the last frame of a bin, opposite signs
        s1[t(44 + k) + binq * BIN, k & 1] = next(amp)
        s1[t(44 + k) + binq * BIN + BIN - 1, k & 1] = -next(amp)
    s1[t(47) + 333, 0] = np.float32(0.9)                     # the stream's largest sample, isolated
    s1[t(48) + 777, 1] = np.float32(-0.85)

    def geo(g):
        assert g.td_true_peak_factor == 4
    _run(oracle, x, tag="planted", want_geo=geo)


def test_short_last_tile(oracle):
    """1.0 s + 7 frames: the bins no longer hold whole frames and the last tile is seven frames long"""
    frames = RATE + 7
    x = np.stack([_noise(3, frames), _noise(4, frames)])
    x[0, frames - 3, 0] = np.float32(0.5)
    x[0, frames - 7, 1] = np.float32(-0.6)
    x[1, frames - 1, 1] = np.float32(0.7)
    x[1, 4800 * 9 + 959, 0] = np.float32(-0.4)
    _run(oracle, x, tag="short-last-tile")


def test_segmented_batch(oracle):
    """8 streams x 10 s cut into segments: a bin whose frames sit in the halo of a segment's first tile, spikes on either side of
    every segment boundary"""
    frames, ns = 10 * RATE, 8
    x = np.stack([_noise(10 + i, frames) for i in range(ns)])
    seg = None

    def geo(g):
        nonlocal seg
        assert g.td_segments > 1, g.td_segments
        seg = g.td_segment_subblocks * 4800
    b = ssa.Batch(RATE, 2, ns, frames, 4096, 1024, flags=FLAGS)
    try:
        geo(b.geometry)
        assert b.geometry.waveform_fused == 1
        for i in range(ns):
            for k, bnd in enumerate(range(seg, frames, seg)):
                d = (1 + 5 * i + 3 * k) % 47                 # 1 .. 47 frames in front of the boundary: inside the bin that ends there
                x[i, bnd - d, k & 1] = np.float32(0.2 + 0.01 * i + 0.001 * (k % 50))
                x[i, bnd + (d % 13), (k + 1) & 1] = np.float32(-0.25 - 0.01 * i)
            x[i, 4800 * 50 + 100 + i, i & 1] = np.float32(0.9)
        b.upload(0, x.reshape(-1))
        b.run(); b.sync()
        for i in range(ns):
            _check(oracle, b, i, x[i], tag="segmented")
    finally:
        b.close()


def test_general_bins_at_44k1(oracle):
    """44.1 kHz stereo x 1.0 s: 88.2 samples a bin, the general decimation path"""
    frames = 44100
    x = np.stack([_noise(20, frames), _noise(21, frames)])
    x[0, 4410 * 3 + 17, 0] = np.float32(0.5)
    x[0, 4410 * 5 - 1, 1] = np.float32(-0.6)
    x[1, 44099, 0] = np.float32(0.7)
    x[1, 0, 1] = np.float32(-0.3)
    x[1, 22050, 0] = NAN
    _run(oracle, x, rate=44100, tag="44k1")
