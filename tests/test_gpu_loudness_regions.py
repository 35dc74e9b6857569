"""Batch loudness regions (ss_batch_loudness_regions): the gated loudness of runs of one stream's 100 ms sub-blocks and of groups of
such runs, against the crate's meter restated in the oracle.

Reference for region (a, n) of a stream: an oracle meter fed the stream s100 frames at a time and read after every call (the
series `mom`, `st`); the gating blocks are mom[a + 3 : a + n], the short-term blocks st[a + 29 : a + n : 10] (phase anchored at the
region's start), binned into the crate's 1000 bins of 0.1 LU from -70 LUFS and evaluated with the oracle's gated_loudness_hist /
loudness_range_hist.  A bin comparison is only valid while no reference value lies within 10 x TOL_LU of a bin edge (the product's
last bits could otherwise legitimately flip a bin): every comparison asserts that about its reference values first, and the
inputs are chosen (on the CPU, from the oracle alone) so that the assertion holds."""
import ctypes

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_multich, make_stereo

pytestmark = pytest.mark.gpu

TOL_LU = 1e-6
SERIES = L.SS_BATCH_ALL | L.SS_BATCH_LOUDNESS_SERIES
METER = L.SS_BATCH_LUFS | L.SS_BATCH_LOUDNESS_SERIES
NONE = 0xFFFFFFFF
NO_GROUP = L.SS_REGION_NO_GROUP
BAD = {"nan": np.float32(np.nan), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf)}


def s100_of(rate):
    return (rate + 5) // 10


def signal(seed, frames, channels, rate, level=0.4):
    return make_stereo(seed, frames, rate, level=level) if channels == 2 else make_multich(seed, frames, channels, rate, level=level)


def faded(seed, channels, rate, seconds=40):
    """the x0.02 -> x1.0 exponential fade of test_gpu_loudness_series::test_extremes_and_histograms_of_one_stream: many bins"""
    frames = rate * seconds
    x = signal(seed, frames, channels, rate).reshape(frames, channels)
    x *= np.exp(np.linspace(np.log(0.02), np.log(1.0), frames, dtype=np.float32))[:, None]
    return x.reshape(-1).copy()


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


def edge_distance(values):
    """smallest distance in LU of a binnable value (>= -70 LUFS or within reach of it) from a bin edge; inf if there is none"""
    v = np.asarray(values, np.float64)
    v = v[np.isfinite(v) & (v >= -70.0 - 1.0) & (v < 30.0)]
    if not v.size:
        return np.inf
    g = (v + 70.0) * 10.0
    return float(np.abs(g - np.round(g)).min()) / 10.0


def hist_of(values):
    """the crate's histogram of LUFS values: bin i holds [-70 + i / 10, -70 + (i + 1) / 10), the top bin open above; NaN and values
    under the absolute gate land nowhere"""
    v = np.asarray(values, np.float64)
    v = v[~np.isnan(v)]
    v = v[v >= -70.0]
    idx = np.clip(np.floor((np.minimum(v, 1e6) + 70.0) * 10.0), 0, 999).astype(np.int64)
    return np.bincount(idx, minlength=1000).astype(np.uint64)


def extreme(series, lo, hi):
    """max and first argmax (absolute index) over series[lo:hi], NaN skipped; (-inf, NONE) if there is no value"""
    v = np.asarray(series, np.float64)[lo:max(lo, hi)]
    ok = ~np.isnan(v)
    if not ok.any():
        return -np.inf, NONE
    best = v[ok].max()
    return float(best), int(lo + np.flatnonzero(ok & (v == best))[0])


class Ref:
    """what region (a, n) of a stream with the series (mom, st) must read"""
    def __init__(self, oracle, mom, st, a, n, st_on=True):
        self.mvals = mom[a + 3:a + n] if n > 3 else mom[:0]
        self.svals = st[a + 29:a + n:10] if (st_on and n >= 30) else st[:0]
        self.clear = min(edge_distance(self.mvals), edge_distance(self.svals))
        self.hb, self.hs = hist_of(self.mvals), hist_of(self.svals)
        self.nb, self.ns = self.mvals.size, self.svals.size
        self.integrated = oracle.gated_loudness_hist(self.hb)
        self.lra = oracle.loudness_range_hist(self.hs)
        self.max_m = extreme(mom, a + 3, a + n)
        self.max_s = extreme(st, a + 29, a + n) if st_on else (-np.inf, NONE)


def close(got, want, tol=TOL_LU):
    if np.isinf(want) or np.isnan(want):
        return got == want or (np.isnan(got) and np.isnan(want))
    return abs(got - want) <= tol


def check_region(res, ref, tag, hists=None):
    """one region's result (and, where it has a group of its own, that group's histogram pair) against the reference"""
    assert ref.clear >= 10 * TOL_LU, (tag, "a reference value lies on a bin edge", ref.clear)
    assert (res.n_gating_blocks, res.n_st_blocks) == (ref.nb, ref.ns), (tag, res.n_gating_blocks, res.n_st_blocks, ref.nb, ref.ns)
    if hists is not None:
        assert np.array_equal(hists[0], ref.hb), (tag, "block bins", np.flatnonzero(hists[0] != ref.hb)[:8])
        assert np.array_equal(hists[1], ref.hs), (tag, "short-term bins", np.flatnonzero(hists[1] != ref.hs)[:8])
    print(tag, "I", res.integrated_lufs, ref.integrated, "LRA", res.loudness_range, ref.lra, "edge", ref.clear)
    assert close(res.integrated_lufs, ref.integrated), (tag, res.integrated_lufs, ref.integrated)
    assert close(res.loudness_range, ref.lra), (tag, res.loudness_range, ref.lra)
    assert close(res.max_momentary, ref.max_m[0]) and close(res.max_shortterm, ref.max_s[0]), (tag, res.max_momentary, ref.max_m, res.max_shortterm, ref.max_s)
    if ref.max_m[1] == NONE:
        assert res.max_momentary_at == NONE, tag
    if ref.max_s[1] == NONE:
        assert res.max_shortterm_at == NONE, tag


def check_own_series(res, mom, st, a, n, tag, st_on=True):
    """maxima byte-equal to the product's own series restricted to the region"""
    vm, am = extreme(mom, a + 3, a + n)
    vs, as_ = extreme(st, a + 29, a + n) if st_on else (-np.inf, NONE)
    assert (res.max_momentary, res.max_momentary_at) == (vm, am), (tag, res.max_momentary, res.max_momentary_at, vm, am)
    assert (res.max_shortterm, res.max_shortterm_at) == (vs, as_), (tag, res.max_shortterm, res.max_shortterm_at, vs, as_)


def bits(x):
    return np.float64(x).tobytes()


# ---------------------------------------------------------------- 1. whole-stream regions, bit for bit
@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("rate", [44100, 48000, 96000])
def test_whole_stream_regions_are_the_pass_itself(rate, channels):
    frames, ns = int(rate * 6.35), 3
    b = ssa.Batch(rate, channels, ns, frames, 4096, 1024, flags=SERIES)
    for s in range(ns):
        b.upload(s, signal(300 * channels + s, frames, channels, rate, level=0.2 + 0.15 * s))
    b.run()
    b.corpus_gate_enqueue()
    n = b.layout.n_subblocks
    assert n == frames // s100_of(rate)
    b.loudness_regions([(s, 0, n, 0) for s in range(ns)], n_groups=1)
    res, grp = b.region_results(), b.group_results()
    sr, ext = b.results(), b.loudness_extremes()
    for s in range(ns):
        assert bits(res[s].integrated_lufs) == bits(sr[s].integrated_lufs), (s, res[s].integrated_lufs, sr[s].integrated_lufs)
        assert bits(res[s].loudness_range) == bits(sr[s].loudness_range), (s, res[s].loudness_range, sr[s].loudness_range)
        assert (res[s].n_gating_blocks, res[s].n_st_blocks) == (sr[s].n_gating_blocks, sr[s].n_st_blocks) == (n - 3, (n - 30) // 10 + 1)
        assert bits(res[s].max_momentary) == bits(ext[s].max_momentary) and bits(res[s].max_shortterm) == bits(ext[s].max_shortterm)
        assert (res[s].max_momentary_at, res[s].max_shortterm_at) == (ext[s].max_momentary_at, ext[s].max_shortterm_at)
        assert np.isfinite(res[s].integrated_lufs) and np.isfinite(res[s].max_shortterm)
    hb, hs = b.histograms()
    gb, gs = b.group_histograms(0)
    assert np.array_equal(gb, hb) and np.array_equal(gs, hs) and hb.sum() > 0 and hs.sum() > 0
    ci, cl = b.corpus_gate_read()
    assert bits(grp[0].integrated_lufs) == bits(ci) and bits(grp[0].loudness_range) == bits(cl), (grp[0].integrated_lufs, ci, grp[0].loudness_range, cl)
    assert (grp[0].n_gating_blocks, grp[0].n_st_blocks) == (ns * (n - 3), ns * ((n - 30) // 10 + 1))


# ---------------------------------------------------------------- 2. sub-ranges against the oracle
@pytest.mark.parametrize("rate,channels,seed", [(48000, 2, 79), (44100, 6, 84)])
def test_sub_ranges_against_the_oracle(oracle, rate, channels, seed):
    x = faded(seed, channels, rate)
    frames = x.size // channels
    b = ssa.Batch(rate, channels, 1, frames, 4096, 1024, flags=SERIES)
    b.upload(0, x)
    b.run()
    N = b.layout.n_subblocks
    assert N == 400
    spans = [(0, N), (7, 57), (13, 29), (13, 30), (13, 39), (13, 40), (100, 0), (100, 1), (100, 3), (100, 4), (5, 395), (200, 200), (N - 35, 35)]
    b.loudness_regions([(0, a, n, g) for g, (a, n) in enumerate(spans)], n_groups=len(spans))
    res, grp = b.region_results(), b.group_results()
    mom, st = oracle_series(oracle, rate, channels, x)
    pm, ps = b.loudness_series(0)
    assert edge_distance(mom[3:]) >= 10 * TOL_LU and edge_distance(st[29:]) >= 10 * TOL_LU      # every full window, any phase
    refs = {}
    for g, (a, n) in enumerate(spans):
        ref = refs[(a, n)] = Ref(oracle, mom, st, a, n)
        check_region(res[g], ref, (seed, a, n), b.group_histograms(g))
        check_own_series(res[g], pm, ps, a, n, (seed, a, n))
        assert (grp[g].n_gating_blocks, grp[g].n_st_blocks) == (ref.nb, ref.ns)
        assert bits(grp[g].integrated_lufs) == bits(res[g].integrated_lufs) and bits(grp[g].loudness_range) == bits(res[g].loudness_range)
    assert (refs[(13, 29)].nb, refs[(13, 29)].ns) == (26, 0) and (refs[(13, 30)].nb, refs[(13, 30)].ns) == (27, 1)
    assert (refs[(13, 39)].ns, refs[(13, 40)].ns) == (1, 2) and (refs[(100, 3)].nb, refs[(100, 4)].nb) == (0, 1)
    # the phase of the short-term blocks is the region's: for (5, 395) the stream-anchored blocks are others, and the reference tells
    stream_phase = hist_of(st[39:400:10])                       # j = 29 + 10 m >= 5 + 29
    assert edge_distance(st[39:400:10]) >= 10 * TOL_LU
    assert not np.array_equal(stream_phase, refs[(5, 395)].hs)
    assert not np.array_equal(b.group_histograms(spans.index((5, 395)))[1], stream_phase)


# ---------------------------------------------------------------- 3. groups
def test_groups_sum_their_regions(oracle):
    """an album over three streams of different levels, one region listed twice, two overlapping regions, an empty group and a
    region outside every group"""
    rate, frames, ns = 48000, 48000 * 8, 3
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=SERIES)
    series = []
    for s in range(ns):
        x = make_stereo(910 + s, frames, rate, level=0.1 * 3 ** s)
        b.upload(s, x)
        series.append(oracle_series(oracle, rate, 2, x))
    b.run()
    n = b.layout.n_subblocks
    regions = [(0, 0, n, 0), (1, 0, n, 0), (2, 0, n, 0),
               (0, 5, 60, 1), (0, 5, 60, 1),
               (1, 0, 50, 2), (1, 30, 50, 2),
               (2, 10, 40, NO_GROUP)]
    b.loudness_regions(regions, n_groups=4)
    res, grp = b.region_results(), b.group_results()
    refs = [Ref(oracle, *series[s], a, k) for s, a, k, _ in regions]
    for r, ref, rg in zip(res, refs, regions):
        check_region(r, ref, rg)
    for g in range(4):
        mine = [ref for ref, rg in zip(refs, regions) if rg[3] == g]
        hb = sum((m.hb for m in mine), np.zeros(1000, np.uint64))
        hs = sum((m.hs for m in mine), np.zeros(1000, np.uint64))
        gb, gs = b.group_histograms(g)
        assert np.array_equal(gb, hb) and np.array_equal(gs, hs), g
        assert (grp[g].n_gating_blocks, grp[g].n_st_blocks) == (sum(m.nb for m in mine), sum(m.ns for m in mine)), g
        assert close(grp[g].integrated_lufs, oracle.gated_loudness_hist(hb)), (g, grp[g].integrated_lufs)
        assert close(grp[g].loudness_range, oracle.loudness_range_hist(hs)), (g, grp[g].loudness_range)
    assert np.array_equal(b.group_histograms(1)[0], 2 * refs[3].hb) and refs[3].hb.sum() > 0          # listed twice: the bins double
    assert bits(grp[1].integrated_lufs) == bits(res[3].integrated_lufs)
    assert (grp[3].integrated_lufs, grp[3].loudness_range, grp[3].n_gating_blocks, grp[3].n_st_blocks) == (-np.inf, 0.0, 0, 0)
    # the album is not the mean of its streams: the louder stream's blocks carry the gate
    assert grp[0].integrated_lufs > np.mean([res[s].integrated_lufs for s in range(3)]) + 1.0


# ---------------------------------------------------------------- 4. silence and the absolute gate
def test_silence_counts_blocks_and_bins_none():
    rate, frames = 48000, 48000 * 5
    b = ssa.Batch(rate, 2, 2, frames, 4096, 1024, flags=SERIES)
    x = make_stereo(5, frames, rate)
    x[:2 * 2 * rate] = 0.0                                       # the first 2 s: digital silence (the filter is still at rest)
    b.upload(0, x)
    b.upload(1, np.zeros(2 * frames, np.float32))
    b.run()
    b.loudness_regions([(0, 2, 15, 0), (1, 3, 45, 1)], n_groups=2)
    res, grp = b.region_results(), b.group_results()
    for g, (a, n, nb, ns) in enumerate([(2, 15, 12, 0), (3, 45, 42, 2)]):
        assert (res[g].n_gating_blocks, res[g].n_st_blocks) == (nb, ns)
        gb, gs = b.group_histograms(g)
        assert gb.sum() == 0 and gs.sum() == 0
        assert res[g].integrated_lufs == -np.inf and res[g].loudness_range == 0.0 and grp[g].integrated_lufs == -np.inf
        assert (res[g].max_momentary, res[g].max_momentary_at) == (-np.inf, a + 3), (res[g].max_momentary, res[g].max_momentary_at)
    assert (res[0].max_shortterm, res[0].max_shortterm_at) == (-np.inf, NONE)
    assert (res[1].max_shortterm, res[1].max_shortterm_at) == (-np.inf, 3 + 29)


# ---------------------------------------------------------------- 5. ragged batches
def test_ragged_batch_bounds_follow_each_stream(oracle):
    rate, slot = 48000, 48000 * 5
    lengths = [slot, int(0.35 * rate), int(2.55 * rate), int(4.567 * rate) + 13, 2000, 0, 30 * 4800, 4 * 4800 - 1]
    ns = len(lengths)
    b = ssa.Batch(rate, 2, ns, slot, 4096, 1024, flags=SERIES)
    b.set_lengths(lengths)
    series = []
    for s, f in enumerate(lengths):
        x = np.zeros(2 * slot, np.float32)
        x[:2 * f] = make_stereo(60 + s, slot, rate)[:2 * f]
        x[2 * f:] = np.float32(0.9)                 # the slot's tail is not part of the stream
        b.upload(s, x)
        series.append(oracle_series(oracle, rate, 2, x, f))
    b.run()
    subs = [int(b.stream_shape(s).n_subblocks) for s in range(ns)]
    assert subs == [f // 4800 for f in lengths]
    regions = [(s, 0, k, NO_GROUP) for s, k in enumerate(subs)] + [(s, k // 2, k - k // 2, NO_GROUP) for s, k in enumerate(subs)] + \
              [(s, k, 0, NO_GROUP) for s, k in enumerate(subs)]
    b.loudness_regions(regions)
    res = b.region_results()
    sr = b.results()
    for r, (s, a, k, _) in zip(res, regions):
        check_region(r, Ref(oracle, *series[s], a, k), ("ragged", s, a, k))
        if a == 0 and k == subs[s]:
            assert bits(r.integrated_lufs) == bits(sr[s].integrated_lufs) and r.n_gating_blocks == sr[s].n_gating_blocks
    lib = L.lib()
    for s, k in enumerate(subs):
        for a, n in ((0, k + 1), (k, 1), (k + 1, 0)):
            one = (L.LoudnessRegion * 1)(L.LoudnessRegion(s, a, n, NO_GROUP))
            assert lib.ss_batch_loudness_regions(b._h, one, 1, 0) == L.SS_ERR_INVALID_ARG, (s, a, n)
    assert bytes(b.region_results()) == bytes(res)               # a refused call leaves the last list's results


# ---------------------------------------------------------------- 6. non-finite samples
def test_nonfinite_samples_follow_the_stream(oracle):
    rate, frames, ns = 48000, 48000 * 12, 4
    bad = 57
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=SERIES)
    assert b.geometry.td_segments > 1
    series = []
    for s, kind in enumerate(["nan", "+inf", "-inf", None]):
        x = make_stereo(1200 + s, frames, rate, level=0.3)
        if kind:
            x[2 * (bad * 4800 + 1234) + (s & 1)] = BAD[kind]
        b.upload(s, x)
        series.append(oracle_series(oracle, rate, 2, x))
    b.run()
    spans = [(10, 48), (20, 38), (40, 50), (60, 40), (58, 62)]    # ending with `bad`, ending with it, spanning it, behind it, right behind it
    regions = [(s, a, n, s * len(spans) + g) for s in range(ns) for g, (a, n) in enumerate(spans)]
    b.loudness_regions(regions, n_groups=len(regions))
    res = b.region_results()
    for r, (s, a, n, g) in zip(res, regions):
        ref = Ref(oracle, *series[s], a, n)
        gb, gs = b.group_histograms(g)
        check_region(r, ref, ("nonfinite", s, a, n), (gb, gs))
        pm, ps = b.loudness_series(s)
        check_own_series(r, pm, ps, a, n, ("nonfinite", s, a, n))
        assert (r.n_gating_blocks, r.n_st_blocks) == (n - 3, (n - 30) // 10 + 1)       # blocks behind `bad` count as well
        if s == 3:
            assert gb.sum() == n - 3 and np.isfinite(r.integrated_lufs)
            continue
        assert np.isnan(series[s][0][bad + 1:]).all()
        assert gb.sum() <= max(0, bad + 1 - (a + 3)) and gs.sum() <= len(range(a + 29, min(a + n, bad + 1), 10))
        if a + n <= bad + 1:
            assert gb.sum() >= n - 4 and np.isfinite(r.integrated_lufs)
        if a > bad:
            assert (r.integrated_lufs, r.loudness_range) == (-np.inf, 0.0) and gb.sum() == 0 and gs.sum() == 0
            assert (r.max_momentary, r.max_momentary_at, r.max_shortterm, r.max_shortterm_at) == (-np.inf, NONE, -np.inf, NONE)


# ---------------------------------------------------------------- 7. loops and the plan's threshold
@pytest.mark.parametrize("ns", [70, 2])
def test_long_streams_many_regions(oracle, ns):
    """2100 sub-blocks per stream.  A list whose longest region exceeds 2048 sub-blocks runs every workgroup on 1024 threads, a
    list of short regions on 256 (region_gate_threads: the plan's one threshold), 5000 regions or a handful; a thread walks
    several blocks either way.  40 regions of each list on the three reference streams against the oracle."""
    rate, seconds = 16000, 210
    frames = rate * seconds
    b = ssa.Batch(rate, 1, ns, frames, 4096, 1024, flags=METER)
    streams = sorted({0, ns // 2, ns - 1})
    buf = np.zeros((ns, frames), np.float32)
    series = {}
    for s in streams:
        buf[s] = make_multich(90 + s, frames, 1, rate)
        series[s] = oracle_series(oracle, rate, 1, buf[s])
    b.upload(0, buf.reshape(-1))
    b.run()
    N = b.layout.n_subblocks
    assert N == 2100
    rng = np.random.default_rng(20241)
    short = []
    for _ in range(5000):
        n = int(rng.integers(0, 301))
        short.append((int(rng.integers(0, ns)), int(rng.integers(0, N - n + 1)), n, int(rng.integers(0, 8))))
    long_one = [(streams[-1], 0, N, 3)]
    few = [r for r in short if r[0] in series][:50]
    sr = b.results()
    for name, regions in (("5000 + long", short + long_one), ("5000", short), ("few", few), ("few + long", few + long_one)):
        b.loudness_regions(regions, n_groups=8)
        res = b.region_results()
        first = (bytes(res), bytes(b.group_results()), [b.group_histograms(g) for g in (0, 3, 7)])
        checked = 0
        for r, (s, a, n, _) in zip(res, regions):
            if s not in series or checked == 40 or n == N:
                continue
            ref = Ref(oracle, *series[s], a, n)
            if ref.clear < 10 * TOL_LU:
                continue                                       # (the reference cannot decide a bin for this region)
            check_region(r, ref, (name, s, a, n))
            checked += 1
        assert checked == 40, (name, checked)
        if regions[-1][2] == N:                                  # the whole stream: the pass's own bits
            s = regions[-1][0]
            assert bits(res[len(regions) - 1].integrated_lufs) == bits(sr[s].integrated_lufs)
            assert bits(res[len(regions) - 1].loudness_range) == bits(sr[s].loudness_range)
            assert res[len(regions) - 1].n_gating_blocks == sr[s].n_gating_blocks == N - 3
        b.loudness_regions(regions, n_groups=8)                  # the whole call again: byte for byte
        again = (bytes(b.region_results()), bytes(b.group_results()), [b.group_histograms(g) for g in (0, 3, 7)])
        assert first[0] == again[0] and first[1] == again[1], name
        assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(first[2], again[2])), name


# ---------------------------------------------------------------- 8. nothing else moves
def test_the_pass_is_untouched():
    rate, frames, ns = 48000, 48000 * 4, 6
    b = ssa.Batch(rate, 2, ns, frames, 4096, 1024, flags=SERIES)
    b.synthesize(0x5EED0000, 0)
    b.run(); b.sync()
    before = (bytes(b.results()), b.checksums().copy(), b.histograms(), bytes((L.LoudnessExtremes * ns)(*b.loudness_extremes())))
    regions = [(s, s, 40 - s, s % 2) for s in range(ns)] + [(0, 0, 40, NO_GROUP)]
    b.loudness_regions(regions, n_groups=2)
    mine = (bytes(b.region_results()), bytes(b.group_results()), b.group_histograms(1))
    after = (bytes(b.results()), b.checksums().copy(), b.histograms(), bytes((L.LoudnessExtremes * ns)(*b.loudness_extremes())))
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[3] == after[3]
    assert np.array_equal(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
    b.run()
    b.loudness_regions(regions, n_groups=2)
    again = (bytes(b.region_results()), bytes(b.group_results()), b.group_histograms(1))
    assert mine[0] == again[0] and mine[1] == again[1] and np.array_equal(mine[2][0], again[2][0]) and np.array_equal(mine[2][1], again[2][1])
    assert bytes(b.results()) == before[0]
    assert mine[2][0].sum() > 0


# ---------------------------------------------------------------- 9. refusals
def test_refusals():
    lib = L.lib()
    RP, GP = L.RegionResult * 4, L.GroupResult * 4
    u64p = ctypes.POINTER(ctypes.c_uint64)
    hist = np.empty(2000, np.uint64)

    def regs(*rows):
        return (L.LoudnessRegion * len(rows))(*[L.LoudnessRegion(*r) for r in rows])

    plain = ssa.Batch(48000, 2, 2, 48000 * 2, 4096, 1024, flags=L.SS_BATCH_FFT | L.SS_BATCH_TRUE_PEAK)
    plain.synthesize(); plain.run(); plain.sync()
    assert lib.ss_batch_loudness_regions(plain._h, regs((0, 0, 10, NO_GROUP)), 1, 0) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_region_results(plain._h, RP(), 4) == L.SS_ERR_INVALID_MODE

    b = ssa.Batch(48000, 2, 2, 48000 * 2, 4096, 1024, flags=L.SS_BATCH_ALL)
    b.synthesize(); b.run(); b.sync()
    assert b.layout.n_subblocks == 20
    # downloads before the first call
    assert lib.ss_batch_download_region_results(b._h, RP(), 4) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_group_results(b._h, GP(), 4) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_group_histograms(b._h, 0, hist.ctypes.data_as(u64p)) == L.SS_ERR_INVALID_MODE
    for rows, n_groups in [([(2, 0, 10, NO_GROUP)], 0),                      # stream >= n_streams
                           ([(0, 0, 21, NO_GROUP)], 0), ([(0, 20, 1, NO_GROUP)], 0), ([(0, 21, 0, NO_GROUP)], 0),
                           ([(1, 0xFFFFFFFF, 2, NO_GROUP)], 0), ([(1, 2, 0xFFFFFFFF, NO_GROUP)], 0),      # a + n in 64 bits
                           ([(0, 0, 10, 0)], 0), ([(0, 0, 10, 2)], 2), ([(0, 0, 10, 0xFFFFFFFE)], 2),    # group >= n_groups
                           ([(0, 0, 10, 0), (0, 0, 10, 1), (1, 0, 30, 0)], 2)]:                          # a bad one behind good ones
        assert lib.ss_batch_loudness_regions(b._h, regs(*rows), len(rows), n_groups) == L.SS_ERR_INVALID_ARG, rows
    assert lib.ss_batch_loudness_regions(b._h, None, 1, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_loudness_regions(None, regs((0, 0, 10, NO_GROUP)), 1, 0) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_region_results(b._h, RP(), 4) == L.SS_ERR_INVALID_MODE      # every call so far was refused
    # an empty list is a list
    assert lib.ss_batch_loudness_regions(b._h, None, 0, 0) == L.SS_OK
    assert lib.ss_batch_download_region_results(b._h, None, 0) == L.SS_OK
    assert lib.ss_batch_download_group_results(b._h, None, 0) == L.SS_OK
    assert lib.ss_batch_group_histograms(b._h, 0, hist.ctypes.data_as(u64p)) == L.SS_ERR_INVALID_ARG
    # capacities
    assert lib.ss_batch_loudness_regions(b._h, regs((0, 0, 20, 0), (1, 0, 20, 1), (1, 20, 0, NO_GROUP)), 3, 2) == L.SS_OK
    assert lib.ss_batch_download_region_results(b._h, RP(), 2) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_group_results(b._h, GP(), 1) == L.SS_ERR_CAPACITY
    out, grp = RP(), GP()
    assert lib.ss_batch_download_region_results(b._h, out, 3) == L.SS_OK and lib.ss_batch_download_group_results(b._h, grp, 2) == L.SS_OK
    assert lib.ss_batch_group_histograms(b._h, 1, hist.ctypes.data_as(u64p)) == L.SS_OK
    assert lib.ss_batch_group_histograms(b._h, 2, hist.ctypes.data_as(u64p)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_group_histograms(b._h, 1, None) == L.SS_ERR_INVALID_ARG
    sr = b.results()
    assert bits(out[1].integrated_lufs) == bits(sr[1].integrated_lufs) == bits(grp[1].integrated_lufs)
    assert (out[2].n_gating_blocks, out[2].integrated_lufs, out[2].max_momentary_at) == (0, -np.inf, NONE)
    assert 0 < hist[:1000].sum() <= 17 and hist[1000:].sum() == 0
