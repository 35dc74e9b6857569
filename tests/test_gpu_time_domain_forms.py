"""Every launch form of `k_time_domain` against the f64 restatements of tests/_f64ref.py, at planted edges.

Each case of the table names a shape and the geometry it must reach — (td_split, td_segments, td_segment_subblocks,
td_warm_subblocks, td_fixup_subblocks, td_true_peak_factor, waveform_fused) — and asserts that tuple before anything else, so
that a change of choose_td_geometry fails here instead of quietly testing another form.  The register build (three or four
waves per SIMD, td_three_waves) is not part of the geometry: the grids are picked clearly on either side of its threshold of
3 x 256 four-wave workgroups, and each case names the build it means.

Material.  Every (stream, channel) carries one planted burst — twelve Hann-tapered frames at fs / 4, phased so that its peak falls
between samples (its true peak 2.6 dB over its sample peak) — over quiet noise whose interpolated level is provably under the
burst (event_true_peak's bound); the bursts walk every frame within 64 of each boundary class (stream start and end, the first
segment boundary, a sub-block boundary behind it) and the rest of that sub-block in steps of 7 frames, one position per
(stream, channel) and run, the batch re-uploaded between runs; channel c's burst sits at its own position with its own
amplitude, so a swapped channel or packed half reads the other's peak.  The first streams of a run carry the hand-over's worst
material instead: a DC offset and a 7 Hz component (ss_host.h) with a level step k frames in front of every segment (or
sub-block) boundary, k swept over ten values.

Checks per run: every channel's true peak within 1e-6 of the f64 value (relative), its sample peak bit for bit, the decimation
bins bit for bit where the flag is on; every sub-block energy of the checked streams within the case's bound of a sequential f64
K-weighting, divided by the sub-block's own energy; with SS_BATCH_LOUDNESS_SERIES, the momentary and short-term series within
1e-6 LU of the f64 series and their maxima in value and place.  Bounds: the measured worst value with at most 10x margin, next
to each case."""
import collections
import zlib

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
import _f64ref as R
from _td_plants import STEP_K, burst as _burst, torture as _torture      # (shared with the streaming forms' tests)

pytestmark = pytest.mark.gpu

AUTO, RUN_IN, WHOLE = L.SS_TD_AUTO, L.SS_TD_RUN_IN, L.SS_TD_WHOLE_STREAMS
F32, F16X3 = L.SS_TP_ARITH_F32, L.SS_TP_ARITH_F16X3
LTW = L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK | L.SS_BATCH_WAVEFORM
LT = L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK
SERIES = L.SS_BATCH_LOUDNESS_SERIES

SPAN = 12
TP_REL = 1e-6
SERIES_LU = 1e-6
N_TORTURE = 10

Case = collections.namedtuple("Case", "name rate ch ns frames mode flags factor arith geo build e_bound ragged")
Case.__new__.__defaults__ = (None,)


def _e(rate):
    """energy bounds of the exact forms on the burst material, per rate: within test_kweighting_is_f64_accurate_at_every_rate's
    bars and at most 10x the worst case of the rate below (48 kHz 1.6e-11, 44.1 kHz 1.4e-11, 96 kHz 7.5e-11, 192 kHz 2.6e-10)"""
    return {44100: 1e-10, 48000: 1e-10, 96000: 5e-10, 192000: 2e-9}[rate]


# name, rate, channels, streams, frames, mode, flags, factor, arith, geometry, register build, energy bound (, ragged lengths)
CASES = [
    # the benchmark's form: fix-up launch, four-waves build (1024 four-wave workgroups; bench.py's own shape)
    #   measured: energy 1.7e-12, hand-over material 1.4e-09, true peak 2.7e-07
    Case("bench", 48000, 2, 1024, 480000, AUTO, LTW | SERIES, 0, F32, (0, 4, 25, 0, 2, 4, 1), "4w", _e(48000)),
    # fix-up launch, three-waves build (250 workgroups); waveform fast path (WAVE 2) and off (WAVE 0)
    #   measured: energy 3.0e-12, hand-over material 1.3e-09, true peak 2.4e-07
    Case("fixup-3w", 48000, 2, 100, 96000, AUTO, LTW | SERIES, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 5.2e-12, hand-over material 1.3e-09, true peak 2.3e-07
    Case("fixup-3w-nowave", 48000, 2, 100, 96000 + 23, AUTO, LT, 0, F32, (0, 10, 2, 0, 2, 4, 0), "3w", _e(48000)),
    # 44.1 kHz: the general decimation path (WAVE 1), factor 4
    #   measured: energy 1.4e-11, hand-over material 7.1e-10, true peak 2.1e-07
    Case("fixup-44k", 44100, 2, 100, 88200 + 29, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(44100)),
    # a decimation window of 1 s over 2 s of stereo: 192 samples per bin (WAVE 3)
    #   measured: energy 7.3e-12, hand-over material 1.3e-09, true peak 2.0e-07
    Case("fixup-wave3", 48000, 2, 100, 96000, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    # run-in (0.1 s from zero in front of every segment > 0): its truncation is the bound
    #   measured: energy 4.2e-12, hand-over material 3.2e-09, true peak 2.0e-07
    Case("run-in", 48000, 2, 100, 96000 + 31, RUN_IN, LTW, 0, F32, (0, 20, 1, 1, 0, 4, 1), "3w", None),
    # one segment per stream: enough streams that nseg == 1 wins (1024 workgroups); mono has no whole-stream form
    #   measured: energy 5.8e-12, hand-over material 9.0e-10, true peak 2.3e-07
    Case("one-segment", 48000, 1, 4096, 24000 + 37, AUTO, LTW, 0, F32, (0, 1, 0, 0, 0, 4, 1), "4w", _e(48000)),
    # whole-stream workgroups, both builds, stereo and eight channels
    #   measured: energy 4.9e-12, hand-over material 9.9e-10, true peak 2.4e-07
    Case("whole-2-3w", 48000, 2, 300, 96000 + 3, WHOLE, LTW, 0, F32, (1, 1, 0, 0, 0, 4, 1), "3w", _e(48000)),
    #   measured: energy 5.5e-12, hand-over material 7.9e-10, true peak 2.3e-07
    Case("whole-2-4w", 48000, 2, 1100, 24000 + 5, WHOLE, LTW, 0, F32, (1, 1, 0, 0, 0, 4, 1), "4w", _e(48000)),
    #   measured: energy 6.2e-12, hand-over material 1.0e-09, true peak 2.3e-07
    Case("whole-8-3w", 48000, 8, 200, 48000 + 7, WHOLE, LTW, 0, F32, (1, 1, 0, 0, 0, 4, 1), "3w", _e(48000)),
    #   measured: energy 1.2e-12, hand-over material 9.2e-10, true peak 2.4e-07
    Case("whole-8-4w", 48000, 8, 1100, 9600 + 9, WHOLE, LTW, 0, F32, (1, 1, 0, 0, 0, 4, 1), "4w", _e(48000)),
    # the few-streams form: eight waves per 0.2 s segment, LATE, run-in over the segment in front
    #   measured: energy 1.6e-11, hand-over material 7.1e-10, true peak 2.8e-07
    Case("few-2", 48000, 2, 40, 96000 + 11, AUTO, LTW | SERIES, 0, F32, (2, 10, 2, 2, 0, 4, 1), "8w", _e(48000)),
    #   measured: energy 1.2e-11, hand-over material 7.1e-10, true peak 2.4e-07
    Case("few-8", 48000, 8, 16, 96000 + 13, AUTO, LTW | SERIES, 0, F32, (2, 10, 2, 2, 0, 4, 1), "8w", _e(48000)),
    # ragged lengths: the split is forced off (one wave per segment); lengths end anywhere in a sub-block
    #   measured: energy 1.0e-11, hand-over material 1.3e-09, true peak 2.0e-07
    Case("ragged", 48000, 2, 96, 120000, AUTO, LTW | SERIES, 0, F32, (0, 13, 2, 0, 2, 4, 0), "3w", _e(48000), "ragged"),
    # channel counts: CT = 1 / 2 / 6 / 8 paths, matrix pipe at 1 / 4 / 16, plain FMA at 3 / 5
    #   measured: energy 8.7e-12, hand-over material 9.2e-10, true peak 2.3e-07
    Case("ch1", 48000, 1, 100, 96000 + 19, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 1.5e-11, hand-over material 1.3e-09, true peak 2.5e-07
    Case("ch3", 48000, 3, 64, 96000 + 21, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 3.8e-12, hand-over material 1.0e-09, true peak 2.6e-07
    Case("ch4", 48000, 4, 64, 96000 + 25, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 1.0e-11, hand-over material 7.8e-10, true peak 2.2e-07
    Case("ch5", 48000, 5, 64, 96000 + 27, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 4.5e-12, hand-over material 1.0e-09, true peak 2.0e-07
    Case("ch6", 48000, 6, 64, 96000 + 33, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 1.3e-11, hand-over material 9.9e-10, true peak 2.3e-07
    Case("ch8", 48000, 8, 64, 96000 + 35, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 1.6e-11, hand-over material 2.1e-09, true peak 2.3e-07
    Case("ch16", 48000, 16, 32, 96000 + 39, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    # true-peak factors: 2 at 96 kHz, none at 192 kHz, 2 forced at 48 kHz
    #   measured: energy 7.5e-11, hand-over material 8.9e-09, true peak 2.0e-07
    Case("tp2-96k", 96000, 2, 160, 192000 + 41, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 2, 1), "3w", _e(96000)),
    #   measured: energy 2.6e-10, hand-over material 1.3e-07, true peak 0.0e+00
    Case("tp0-192k", 192000, 2, 250, 211200 + 43, AUTO, LTW, 0, F32, (0, 6, 2, 0, 2, 0, 1), "3w", _e(192000)),
    #   measured: energy 5.6e-12, hand-over material 1.3e-09, true peak 2.1e-07
    Case("tp2-forced", 48000, 2, 100, 96000 + 45, AUTO, LTW, 2, F32, (0, 10, 2, 0, 2, 2, 1), "3w", _e(48000)),
    # the f16x3 split on the matrix cores
    #   measured: energy 1.5e-11, hand-over material 1.3e-09, true peak 3.6e-07
    Case("f16x3-2", 48000, 2, 100, 96000 + 47, AUTO, LTW, 0, F16X3, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    #   measured: energy 1.3e-11, hand-over material 9.9e-10, true peak 3.2e-07
    Case("f16x3-8", 48000, 8, 64, 96000 + 49, AUTO, LTW, 0, F16X3, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
]


def _lengths(case):
    if case.ragged is None:
        return np.full(case.ns, case.frames, np.int64)
    S = R.subblock_frames(case.rate)
    i = np.arange(case.ns)
    return case.frames - S * (i % 7) - (i * 613) % S         # every stream ends somewhere else in its last sub-block


def _boundaries(case, geo):
    """(segment boundary, sub-block boundary behind it) in frames: the first hand-over and the next sub-block's start"""
    S = R.subblock_frames(case.rate)
    seg = geo[2] * S if geo[1] > 1 else 3 * S
    return seg, seg + S


def _positions(case, geo, n, bench=False, end_only=False):
    """burst start frames of one stream of n frames: every frame within 64 of each boundary class, the rest of the sub-block behind
    the first segment boundary in steps of 7 (bench: every frame of it)"""
    S = R.subblock_frames(case.rate)
    seg, sub = _boundaries(case, geo)
    if end_only:
        return np.arange(max(n - SPAN - 63, 0), n - SPAN + 1)
    p = list(range(0, 64)) + list(range(n - SPAN - 63, n - SPAN + 1)) + list(range(seg - 64, seg + 64)) + list(range(sub - 64, sub + 64))
    p += list(range(seg - 64, seg + S)) if bench else list(range(seg + 64, seg + S - 64, 7))
    p = np.unique(np.clip(np.array(p), 0, n - SPAN))
    return p


def _waveform_bins(x, window_s):
    """R.waveform_numpy, vectorised for finite data"""
    w = int(window_s * 1000.0)
    n = len(x)
    spp = n / w
    i = np.arange(w)
    bs = np.floor(i * spp).astype(np.int64)
    be = np.minimum(np.ceil((i + 1) * spp).astype(np.int64), n)
    keep = bs < n
    bs, be = bs[keep], be[keep]
    lo = np.minimum.reduceat(x, bs)
    hi = np.maximum.reduceat(x, bs)
    nxt = np.append(bs[1:], n)                            # reduceat takes [bs_i, bs_i+1); a bin reaches to be_i
    tail = be > nxt
    lo[tail] = np.minimum(lo[tail], x[nxt[tail]])
    hi[tail] = np.maximum(hi[tail], x[nxt[tail]])
    last = bs[-1]
    lo[-1], hi[-1] = x[last:be[-1]].min(), x[last:be[-1]].max()
    return np.stack([lo, hi], 1).reshape(-1).astype(np.float32)


def _series_check(b, i, sub, case, worst):
    mom, st = b.loudness_series(i)
    rm, rs = R.loudness_series(sub, case.rate, case.ch)
    ext = b.loudness_extremes()[i]
    for got, want, first, vmax, at in ((mom, rm, 3, ext.max_momentary, ext.max_momentary_at),
                                       (st, rs, 29, ext.max_shortterm, ext.max_shortterm_at)):
        assert got.size == want.size, (case.name, i, got.size, want.size)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin]), (case.name, i)
        if fin.any():
            worst["series"] = max(worst["series"], float(np.abs(got[fin] - want[fin]).max()))
        full = want[first:]
        if full.size:
            j = int(np.argmax(full))
            worst["series"] = max(worst["series"], abs(vmax - full[j]))
            ru = np.sort(full)[-2] if full.size > 1 else -np.inf
            if full[j] - ru > 1e-5:
                assert at == first + j, (case.name, i, at, first + j)


def run_case(case, strict=True, runs=None, end_only=False):
    """Run one case; returns its measured worst values.  strict=False (diagnostics): no tuple / bound assertions."""
    rate, C, ns, F = case.rate, case.ch, case.ns, case.frames
    S = R.subblock_frames(rate)
    lengths = _lengths(case)
    wave_window = 1.0 if case.name == "fixup-wave3" else 0.0
    b = ssa.Batch(rate, C, ns, F, 4096, 1024, flags=case.flags, true_peak_factor=case.factor, waveform_window=wave_window)
    try:
        if case.ragged is not None:
            b.set_lengths(lengths)
        b.set_time_domain_mode(case.mode)
        b.set_true_peak_arith(case.arith)
        g = b.geometry
        geo = (g.td_split, g.td_segments, g.td_segment_subblocks, g.td_warm_subblocks, g.td_fixup_subblocks, g.td_true_peak_factor,
               g.waveform_fused)
        if strict:
            assert geo == case.geo, (case.name, geo, case.geo)
        factor = g.td_true_peak_factor
        bench = case.name == "bench"
        seg, sub = _boundaries(case, geo)
        tbounds = [k * seg for k in range(1, F // seg + 1)] if geo[1] > 1 else [k * S for k in range(3, F // S + 1, 3)]
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        bg = (rng.uniform(-1e-3, 1e-3, (F, C))).astype(np.float32)
        bound = R.tap_bound(factor) * float(np.abs(bg).max()) if factor else float(np.abs(bg).max())
        nt = min(N_TORTURE, ns // 4)
        torture = [_torture(rate, F, C, STEP_K[i % len(STEP_K)], tbounds, i) for i in range(nt)]
        plist = [_positions(case, geo, int(n), bench, end_only) for n in lengths]
        npos = max(p.size for p in plist)
        slots = (ns - nt) * C
        n_runs = runs or -(-npos // slots)
        burst = _burst()
        worst = {"tp": 0.0, "energy": 0.0, "energy_torture": 0.0, "series": 0.0, "runs": n_runs, "geo": geo, "tp_db_min": np.inf}
        x = np.empty((ns, F, C), np.float32)
        x[:] = bg[None]
        for i, t in enumerate(torture):
            x[i] = t
        si = np.repeat(np.arange(nt, ns), C)
        sc = np.tile(np.arange(C), ns - nt)
        ab = np.abs(bg).astype(np.float64)
        pre = np.maximum.accumulate(np.vstack([np.zeros((1, C)), ab]), axis=0)             # max |bg| over [0, t)
        suf = np.maximum.accumulate(np.vstack([ab, np.zeros((1, C))])[::-1], axis=0)[::-1]  # max |bg| over [t, F)
        sp_t = [np.abs(x[i, :lengths[i]]).max(axis=0) for i in range(nt)]
        tp_t = [np.array([R.true_peak(x[i, :lengths[i], c], factor) for c in range(C)]) for i in range(nt)]
        start = None
        for run in range(n_runs):
            if start is not None:                                   # the previous run's bursts out, this run's in
                for j in range(SPAN):
                    x[si, start + j, sc] = bg[start + j, sc]
            slot = run * slots + np.arange(slots)
            start = np.array([plist[i][(s * 7919) % plist[i].size if s >= plist[i].size else s] for i, s in zip(si, slot)])
            amp = 0.3 + 0.6 * ((slot * 0.6180339887) % 1.0)
            for j in range(SPAN):
                x[si, start + j, sc] += (amp * burst[j]).astype(np.float32)
            b.upload(0, x.reshape(-1))
            b.run(); b.sync()
            # peaks of the burst channels: exact around the burst, bounded elsewhere
            idx = start[:, None] + np.arange(SPAN)[None, :]
            sp_ev = np.abs(x[si[:, None], idx, sc[:, None]]).max(axis=1).astype(np.float64)
            if factor:
                pad = 40
                idx = start[:, None] - pad + np.arange(SPAN + 2 * pad)[None, :]
                win = np.where(idx < lengths[si][:, None], x[si[:, None], np.clip(idx, 0, F - 1), sc[:, None]], 0.0)
                win = np.where(idx >= 0, win, 0.0).astype(np.float64)     # (R.event_windows, without a copy of every channel)
                ev = R.event_true_peak(win, start, lengths[si], SPAN, factor)
            else:
                ev = sp_ev
            assert (ev > bound).all(), (case.name, float(ev.min()), bound)
            if case.ragged is None:                                 # sample peak: the burst, or the background around it
                sp = np.maximum(sp_ev, np.maximum(pre[start, sc], suf[start + SPAN, sc]))
            else:
                sp = np.concatenate([np.abs(x[i, :lengths[i]]).max(axis=0) for i in range(nt, ns)]).astype(np.float64)
            want = np.maximum(ev, sp)
            if factor:
                clear = start + SPAN + 48 // factor <= lengths[si]      # bursts whose ringing ends inside the stream: 2.6 dB over their samples
                worst["tp_db_min"] = min(worst["tp_db_min"], float((20 * np.log10(want / sp))[clear].min()))
                assert (want[clear] >= sp[clear] * 10 ** (1 / 20)).all(), case.name
            for i in range(ns):
                tp, spd = b.peaks(i)
                if i < nt:
                    ref, ref_sp = tp_t[i], sp_t[i].astype(np.float64)
                else:
                    ref, ref_sp = want[(i - nt) * C:(i - nt + 1) * C], sp[(i - nt) * C:(i - nt + 1) * C]
                assert np.array_equal(spd, ref_sp), (case.name, run, i, spd, ref_sp)
                rel = np.abs(tp - ref) / ref
                worst["tp"] = max(worst["tp"], float(rel.max()))
                if strict:
                    assert rel.max() <= TP_REL, (case.name, run, i, tp, ref, start[(i - nt) * C:(i - nt + 1) * C] if i >= nt else None)
            # energies (and series): the torture streams once (they do not change), a spread of the burst streams in the first
            # run, two of them in every other
            check = sorted(set(range(nt)) | set(range(nt, ns, max(1, (ns - nt) // 12))) | {ns - 1}) if run == 0 else [nt + run % (ns - nt), ns - 1]
            for i in check:
                n = int(lengths[i])
                ref = R.kweighted_subblocks(x[i, :n].reshape(-1), rate, C)
                got = b.subblocks(i)[:ref.shape[0]]
                rel = float((np.abs(got - ref) / ref).max())
                key = "energy_torture" if i < nt else "energy"
                worst[key] = max(worst[key], rel)
                if strict:
                    lim = (case.e_bound or RUN_IN_BOUND) if i >= nt else TORTURE_BOUND[(case.mode == RUN_IN, rate)]
                    assert rel <= lim, (case.name, run, i, key, rel, lim)
                if case.flags & SERIES:
                    _series_check(b, i, ref, case, worst)
            if case.flags & L.SS_BATCH_WAVEFORM and (run == 0 or run == n_runs - 1):
                win_s = wave_window or F / rate
                for i in check[::2]:
                    n = int(lengths[i])
                    want_w = _waveform_bins(x[i, :n].reshape(-1), win_s if case.ragged is None else n / rate)
                    got_w = b.waveform(i).reshape(-1)[:want_w.size]
                    assert np.array_equal(got_w.view(np.uint32), want_w.view(np.uint32)), (case.name, run, i)
        if strict:
            assert worst["series"] <= SERIES_LU, (case.name, worst)
        return worst
    finally:
        b.close()


# the run-in's truncation on the burst material (measured 4.2e-12), and every form on the hand-over's worst material (DC offset,
# 7 Hz, level steps: the near-double pole's cancellation makes the sequential f64 filter itself a rounding history of this size;
# the one-segment and whole-stream forms read the same) — keyed (run-in, rate), measured 48 kHz 2.1e-9, 44.1 kHz 7.1e-10,
# 96 kHz 8.9e-9, 192 kHz 1.3e-7, run-in 3.2e-9
RUN_IN_BOUND = 4e-11
TORTURE_BOUND = {(False, 44100): 5e-9, (False, 48000): 1e-8, (False, 96000): 5e-8, (False, 192000): 1e-6, (True, 48000): 3e-8}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_time_domain_form_against_f64(case):
    run_case(case)


# a short last tile in every form: frames mod (rate / 10) over 1 ... 40 and a few middle values, bursts at the stream's end
_REM = list(range(1, 41)) + [97, 480, 2399, 4799]
_REM_FORMS = [
    Case("rem-fixup", 48000, 2, 64, 96000, AUTO, LTW, 0, F32, (0, 10, 2, 0, 2, 4, 1), "3w", _e(48000)),
    Case("rem-few", 48000, 2, 32, 96000, AUTO, LTW, 0, F32, (2, 10, 2, 2, 0, 4, 1), "8w", _e(48000)),
    Case("rem-whole", 48000, 2, 64, 96000, WHOLE, LTW, 0, F32, (1, 1, 0, 0, 0, 4, 1), "3w", _e(48000)),
    Case("rem-run-in", 48000, 2, 64, 96000, RUN_IN, LTW, 0, F32, (0, 20, 1, 1, 0, 4, 1), "3w", None),
]


@pytest.mark.parametrize("rem", _REM)
def test_short_last_tile(rem):
    base = _REM_FORMS[rem % len(_REM_FORMS)]
    case = base._replace(name=base.name + "-%d" % rem, frames=base.frames + rem)
    run_case(case, runs=1, end_only=True)
