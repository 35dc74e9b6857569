"""Planted gate edges for the gating tests (a helper module, not a test file): mono 500 Hz tone programmes at 8 kHz whose gating
and short-term blocks land where the gate's integer logic can go wrong, and the condition each plant must meet, asserted from
the f64 reference (tests/_f64ref.py) alone before anything is compared with it.

500 Hz at 8 kHz is 16 samples a cycle and 50 cycles a sub-block, so every sub-block of a steady segment carries the same energy
(the filter's transient at a level step moves the first block of a segment by about 0.001 LU), and a level given in LUFS is the
level the blocks read: the tone's K-weighted gain is taken from the filter's response at 500 Hz.  Levels sit on bin centres
(x.x5 LUFS), 0.05 LU from either edge.  Only the counts per bin decide the relative gates and the percentile ranks; they were
chosen on the CPU with the reference and are asserted here, so a change of the reference or of a programme that loses an edge
fails as a test, not silently."""
import collections

import numpy as np

import _f64ref as R

RATE = 8000
S = R.subblock_frames(RATE)
TONE_HZ = 500.0


def tone_offset():
    """LUFS of a unit-amplitude 500 Hz sine through the K-weighting at RATE: -0.691 + 10 log10(|H|^2 / 2)"""
    b, a = R.kweight_coeffs(RATE)
    z = np.exp(-2j * np.pi * TONE_HZ / RATE * np.arange(5))
    return -0.691 + 10.0 * np.log10(abs((b @ z) / (a @ z)) ** 2 / 2.0)


def tone(segments, extra_frames=0):
    """mono f32: one phase-continuous 500 Hz sine, segment after segment of (sub-blocks, LUFS; None: digital silence); the last
    level runs on for `extra_frames` frames that complete no sub-block"""
    off = tone_offset()
    amps = [np.full(n * S, 0.0 if l is None else 10.0 ** ((l - off) / 20.0)) for n, l in segments]
    amps.append(np.full(extra_frames, amps[-1][-1]))
    amp = np.concatenate(amps)
    return (amp * np.sin(2.0 * np.pi * TONE_HZ * np.arange(amp.size) / RATE)).astype(np.float32)


Reference = collections.namedtuple("Reference", "n_sub blocks st hb hs integrated lra")


def reference_of_subblocks(sub, first=0, n=None):
    """what the gate must read from the sub-blocks [first, first + n) of one mono stream"""
    blocks, st = R.gate_blocks(sub, RATE, 1, first, n)
    hb, hs = R.gate_histograms(blocks, st)
    return Reference(sub.shape[0], blocks, st, hb, hs, R.integrated_from_hist(hb), R.lra_from_hist(hs))


def reference(x):
    """the same from the samples, through the sequential f64 K-weighting"""
    return reference_of_subblocks(R.kweighted_subblocks(x, RATE, 1))


def lufs(e):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(e, np.float64)) - 0.691


def edge_clearance(ref):
    """smallest distance in LU of a block or short-term value of `ref` from a bin edge (values that cannot reach a bin ignored)"""
    v = np.concatenate([lufs(ref.blocks), lufs(ref.st)])
    v = v[np.isfinite(v) & (v >= -71.0) & (v <= 31.0)]
    if not v.size:
        return np.inf
    g = (v + 70.0) * 10.0
    return float(np.abs(g - np.round(g)).min()) / 10.0


# ---- the conditions
def _quiet(ref):
    assert ref.blocks.size > 0 and ref.st.size > 0
    assert ref.hb.sum() == 0 and ref.hs.sum() == 0 and ref.integrated == -np.inf and ref.lra == 0.0


def _silent(ref):
    _quiet(ref)
    assert not ref.blocks.any() and not ref.st.any()


def _under_absolute_gate(ref):
    _quiet(ref)
    assert (lufs(ref.blocks) > -75.1).all() and (lufs(ref.blocks) < -74.9).all()


def _bin0(ref):
    assert ref.hb[0] == ref.blocks.size > 0 and ref.hs[0] == ref.st.size > 0
    assert abs(ref.integrated - -69.95) < 1e-9 and ref.lra == 0.0


def _top_bin(ref):
    assert (lufs(ref.blocks) > 49.9).all()                                   # twenty LU past the last boundary
    assert ref.hb[999] == ref.blocks.size > 0 and ref.hs[999] == ref.st.size > 0
    assert abs(ref.integrated - 29.95) < 1e-9 and ref.lra == 0.0


def _relative_gate(counted):
    def check(ref):
        cnt, mean = R.hist_moments(ref.hb)
        holding, start = R.gate_start_bin(0.1 * mean)
        quiet = int(R.hist_bins_of(ref.blocks[-1:])[0])
        assert quiet == holding and ref.hb[holding] >= 30, (quiet, holding)         # the quiet part lies in the threshold's own bin
        assert start == (holding if counted else holding + 1), (start, holding)
        assert abs(lufs(0.1 * mean) - lufs(R.histogram_tables()[0][holding])) > 0.01   # ... and the threshold is not on a knife's edge
        a, b = R.integrated_from_hist(ref.hb, holding), R.integrated_from_hist(ref.hb, holding + 1)
        assert b - a > 0.1, (a, b)                                                # the two readings of the rule are 2.6 LU apart
        assert ref.integrated == (a if counted else b)
    return check


def _range_gate(counted):
    def check(ref):
        cnt, mean = R.hist_moments(ref.hs)
        holding, start = R.gate_start_bin(0.01 * mean)
        quiet = int(R.hist_bins_of(ref.st[:1])[0])
        assert 60 * 10 <= ref.n_sub <= 90 * 10
        assert quiet == holding and ref.hs[holding] >= 20, (quiet, holding)         # the quiet part lies in the threshold's own bin
        assert start == (holding if counted else holding + 1), (start, holding)
        assert abs(lufs(0.01 * mean) - lufs(R.histogram_tables()[0][holding])) > 0.01
        a, b = R.lra_from_hist(ref.hs, holding), R.lra_from_hist(ref.hs, holding + 1)
        assert a > 20.0 and b == 0.0, (a, b)                                      # counted: the range spans both parts; dropped: none
        assert ref.lra == (a if counted else b)
    return check


def _percentile_lanes(ref):
    start, n, lo, hi = R.lra_entries_from_hist(ref.hs)
    cum = np.cumsum(ref.hs)
    rank_lo, rank_hi = int((n - 1) * 0.1 + 0.5), int((n - 1) * 0.95 + 0.5)
    assert 60 * 10 <= ref.n_sub <= 90 * 10
    assert lo % 16 == 15 and hi % 16 == 0 and hi > lo + 1, (lo, hi)                 # last bin of a lane, first bin of another
    assert cum[lo] == rank_lo + 1 and ref.hs[lo + 1] > 0                            # the 10 % entry is the last of its bin: the next rank is the next lane's
    assert cum[hi - 1] == rank_hi and ref.hs[hi - 1] > 0                            # the 95 % entry is the first of its bin: the rank before is the lane before's
    assert start < lo - 16


def _gate_inside_lane(ref):
    start, n, lo, hi = R.lra_entries_from_hist(ref.hs)
    lane = start // 16
    assert 60 * 10 <= ref.n_sub <= 90 * 10
    assert 0 < start % 16 < 15                                                    # strictly inside the lane's 16 bins
    assert ref.hs[16 * lane:start].sum() > 0                                       # entries under the gate in the same lane
    assert lo // 16 == lane and lo > start                                        # the 10 % entry is that lane's to find, from the gate bin on
    assert n == ref.hs.sum() - ref.hs[:start].sum() < ref.hs.sum()
    assert ref.lra > 20.0


def _st_blocks(k):
    def check(ref):
        assert ref.st.size == k == ref.hs.sum()
        assert (ref.lra == 0.0) == (k == 1) and (k == 1 or ref.lra > 2.0)
    return check


Plant = collections.namedtuple("Plant", "name segments extra check")
PLANTS = [
    Plant("silent", [(45, None)], 7, _silent),
    Plant("minus-75", [(45, -75.0)], 7, _under_absolute_gate),
    Plant("bin-0", [(45, -69.95)], 7, _bin0),
    Plant("top-bin", [(45, 50.0)], 7, _top_bin),
    # 40 loud sub-blocks (bin 499) and 41 / 40 quiet ones 12.8 LU under them (bin 371, where the threshold falls): the threshold
    # 0.039 LU under the bin's energy (the quiet blocks count, -22.89 LUFS) and 0.011 LU over it (they drop, -20.21 LUFS)
    Plant("relative-counted", [(40, -20.05), (41, -32.85)], 13, _relative_gate(True)),
    Plant("relative-dropped", [(40, -20.05), (40, -32.85)], 13, _relative_gate(False)),
    # 65 s: bins 415 x 7, 416 x 11, 422, 427, 431 x 39, 432 x 4; 63 entries, ranks 6 and 59
    Plant("percentile-lanes", [(80, -28.45), (120, -28.35), (400, -26.85), (50, -26.75)], 21, _percentile_lanes),
    # 64 s: bins 266 x 15 (under the gate), 270 x 15, 452 x 2, 481, 482, 499 x 28; the gate starts at bin 268 = 16 x 16 + 12
    Plant("gate-inside-lane", [(170, -43.35), (300, -20.05), (170, -42.95)], 21, _gate_inside_lane),
    # the same rule at the range's gate, 20 LU under the mean of the short-term values: 31 s (27 s) quiet in bin 272 (273), where
    # the threshold falls 0.025 LU under (0.038 LU over) the bin's energy, then 35 s (33 s) loud in bin 499
    Plant("range-gate-counted", [(310, -42.75), (350, -20.05)], 21, _range_gate(True)),
    Plant("range-gate-dropped", [(270, -42.65), (330, -20.05)], 21, _range_gate(False)),
    Plant("one-st-block", [(20, -30.05), (15, -22.05)], 3, _st_blocks(1)),
    Plant("two-st-blocks", [(20, -30.05), (25, -22.05)], 3, _st_blocks(2)),
]
PLANT_IDS = [p.name for p in PLANTS]


def signal_of(plant):
    return tone(plant.segments, plant.extra)
