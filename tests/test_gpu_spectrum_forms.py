"""Every launch form of the spectrum kernels against the f64 rows of tests/_f64ref.py, at planted edges.

Each case of the table names a shape and the plan ssk::plan_spectrum must give it — (kernel name, fft_windows_per_block,
fft_blocks) — and asserts that tuple before anything else, so that a change of the plan fails here instead of quietly testing
another form.  A one-window caller (get_fft, a file tick) has no geometry getter: its case also runs a batch of one stream and
one window at hop 1024 with the same N and channel count, which gets the same plan, and asserts that batch's tuple.

Material.  Every (stream, row) carries one tone over quiet noise at its own level, both under a per-hop envelope.  The tones sit
on planted bins: the first and the last retained bin (the last 4-bin group, whose row is padded), the Nyquist bin at 40 kHz, the
publish-block boundaries of the N = 4096 kernels next to the band edges (k = 255, 256, 257: 4096 - k on either side of 3840).
The second row of a packed transform (side under mid; window w + 1 under window w in pairw) sits about +20, 0, -6, -20, -60, -90
and -120 dB from the first, or is exactly zero, cycled over the streams.  The envelope's steps are the block-exponent decisions
of ms1 and pairw: a hop 1.9x and 2.1x its neighbours (either side of the switch to the exact energy path), steps of 2x and 4x
up and down (E moves by one, which leaves the registers, and by two, which rewrites them), and silences.

Where: every window of the first and the last stream, the first and the last window of every run in the others, every window of
a ragged stream's last run.  Checks per row: row_error (the error as a fraction of the row's own peak, each stored value's two
ulps allowed) within the case's bound, floor_error (the same over the bins 40 dB and more under the peak: the transform's
rounding noise alone) within FLOOR, db_close at 0.01 dB as before, an all-zero row -150 + pink.  db_close takes `pink`: its 70 dB
are counted on the transform's levels, not on levels that carry the compensation — with a tone on the 20 Hz bin (pink -17 dB)
the plain form holds bins 96 dB under that tone near 20 kHz (pink +13 dB) to 0.01 dB, which no f32 transform meets, the oracle's
included (0.02 ... 0.045 dB there, 4e-8 of the peak).  Bounds: at most 4x the worst
value measured on the MI355X, noted at each case, and never above 1e-5 of the row's peak."""
import collections

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import db_close
import _f64ref as R

pytestmark = pytest.mark.gpu

CAP = 1e-5                       # no bound above 1e-5 of the row's peak (-100 dB)

MS1, MS, ANY, PAIRW = "k_fft4096_ms1", "k_fft4096_ms", "k_fft4096_ms_anyhop", "k_fft4096_pairw"
RUN, F16K, GEN = "k_fft16k_run", "k_fft16k", "k_fft_generic"

# name, rate, channels, streams, N, hop, windows per stream, plan (kernel, windows per block, blocks), bound (, ragged windows)
Case = collections.namedtuple("Case", "name rate ch ns n hop nw plan bound ragged")
Case.__new__.__defaults__ = (None,)

CASES = [
    # ms1: runs of 16 (many streams), runs of 2 from the 768-workgroup rule (few streams), 40 kHz (Nyquist), 40960 Hz (odd count)
    Case("ms1-many", 48000, 2, 260, 4096, 1024, 48, (MS1, 16, 780), 4e-6),     # measured 1.2e-6
    Case("ms1-few", 48000, 2, 3, 4096, 1024, 40, (MS1, 2, 60), 4e-6),     # measured 1.1e-6
    Case("ms1-40k", 40000, 2, 8, 4096, 1024, 40, (MS1, 2, 160), 4e-6),     # measured 1.1e-6
    Case("ms1-40960", 40960, 2, 64, 4096, 1024, 33, (MS1, 4, 576), 5e-6),     # measured 1.3e-6
    # ms<2>, ms<8>
    Case("ms-hop512", 48000, 2, 64, 4096, 512, 40, (MS, 4, 640), 5e-6),     # measured 1.3e-6
    Case("ms-hop2048", 48000, 2, 200, 4096, 2048, 34, (MS, 10, 800), 5e-6),     # measured 1.4e-6
    # ms_anyhop: overlap, none, gaps between windows
    Case("any-hop768", 48000, 2, 100, 4096, 768, 30, (ANY, 4, 800), 5e-6),     # measured 1.4e-6
    Case("any-hop4096", 48000, 2, 40, 4096, 4096, 20, (ANY, 2, 400), 5e-6),     # measured 1.3e-6
    Case("any-hop5120", 48000, 2, 40, 4096, 5120, 20, (ANY, 2, 400), 5e-6),     # measured 1.3e-6
    # pairw: mono, 3, 6, 8 channels; odd window counts (the last pair half empty); 63 blocks (the grid rounded up to 64)
    Case("pairw-mono", 48000, 1, 300, 4096, 1024, 33, (PAIRW, 18, 600), 4e-6),     # measured 1.1e-6
    Case("pairw-3ch-one", 48000, 3, 1, 4096, 1024, 41, (PAIRW, 2, 63), 4e-6),     # measured 1.1e-6
    Case("pairw-6ch", 48000, 6, 40, 4096, 1024, 45, (PAIRW, 4, 2880), 4e-6),     # measured 1.1e-6
    Case("pairw-8ch", 48000, 8, 64, 4096, 1024, 33, (PAIRW, 4, 4608), 4e-6),     # measured 1.1e-6
    # fft16k_run: NE_LAST 1 / 2 / 3 / 4 at 50 / 48 / 44.1 / 40 kHz, mid/side and per channel; exactly 8 windows; 12 blocks (grid 16)
    Case("run-ms-48k", 48000, 2, 3, 16384, 1024, 40, (RUN, 20, 12), 2.5e-6),     # measured 7.4e-7
    Case("run-ms-50k", 50000, 2, 2, 16384, 1024, 9, (RUN, 9, 4), 4e-6),     # measured 1.0e-6
    Case("run-ms-44k", 44100, 2, 2, 16384, 1024, 17, (RUN, 17, 4), 4e-6),     # measured 1.0e-6
    Case("run-ms-40k", 40000, 2, 2, 16384, 1024, 16, (RUN, 16, 4), 3e-6),     # measured 9.0e-7
    Case("run-ms-8win", 48000, 2, 2, 16384, 1024, 8, (RUN, 8, 4), 2.5e-6),     # measured 7.5e-7
    Case("run-6ch-50k", 50000, 6, 2, 16384, 1024, 20, (RUN, 20, 12), 3e-6),     # measured 9.5e-7
    Case("run-mono-44k", 44100, 1, 5, 16384, 1024, 33, (RUN, 17, 10), 2.5e-6),     # measured 7.4e-7
    Case("run-mono-40k", 40000, 1, 2, 16384, 1024, 12, (RUN, 12, 2), 3e-6),     # measured 8.5e-7
    Case("run-3ch-48k", 48000, 3, 2, 16384, 1024, 10, (RUN, 10, 6), 3e-6),     # measured 8.3e-7
    # fft16k: stereo at hop 2048, seven windows at hop 1024 (one under the run threshold), mono, 6 channels
    Case("16k-hop2048", 48000, 2, 2, 16384, 2048, 10, (F16K, 1, 40), 2.5e-6),     # measured 6.5e-7
    Case("16k-7win", 48000, 2, 2, 16384, 1024, 7, (F16K, 1, 28), 2.5e-6),     # measured 7.1e-7
    Case("16k-mono", 44100, 1, 3, 16384, 2048, 5, (F16K, 1, 15), 3e-6),     # measured 7.6e-7
    Case("16k-6ch", 40000, 6, 1, 16384, 1024, 7, (F16K, 1, 42), 3e-6),     # measured 8.8e-7
    # generic: N = 4096 stereo at hop 1000 (mode 1), 2048 mono, 8192 x 6, 32768 (LDS 128 KiB), N = 2 / 4 at 40 kHz (one / two bins,
    # the last of them Nyquist)
    Case("gen-4096-hop1000", 48000, 2, 2, 4096, 1000, 10, (GEN, 1, 40), 1e-5),     # measured 3.9e-6
    Case("gen-2048-mono", 48000, 1, 2, 2048, 1024, 10, (GEN, 1, 20), 1.2e-6),     # measured 3.0e-7
    Case("gen-8192-6ch", 48000, 6, 1, 8192, 1024, 5, (GEN, 1, 30), 3e-6),     # measured 7.9e-7
    Case("gen-32768", 48000, 2, 1, 32768, 1024, 4, (GEN, 1, 8), 8e-7),     # measured 2.0e-7
    Case("gen-n2-40k", 40000, 2, 2, 2, 1024, 16, (GEN, 1, 64), 6e-7),     # measured 1.7e-7
    Case("gen-n4-40k", 40000, 1, 2, 4, 1024, 16, (GEN, 1, 32), 5e-7),     # measured 1.3e-7
    # ragged: streams that end on a run boundary, one window into a run, with no window, ...
    Case("ragged-ms1", 48000, 2, 64, 4096, 1024, 48, (MS1, 4, 768), 4e-6, (48, 44, 45, 0, 47, 1, 4, 5)),     # measured 1.2e-6
    Case("ragged-pairw", 48000, 1, 64, 4096, 1024, 48, (PAIRW, 4, 768), 4e-6, (48, 44, 45, 0, 47, 1, 3, 5)),     # measured 1.0e-6
    Case("ragged-run", 48000, 2, 6, 16384, 1024, 40, (RUN, 20, 24), 4e-6, (40, 20, 21, 0, 1, 9)),     # measured 8.0e-7
]

# floor_error bounds (the bins 40 dB and more under a row's peak), 2x the measured worst (in brackets): the transform's own
# rounding noise, which the twiddle tables and the butterflies set and the dB conversion's per-bin rounding does not hide
FLOOR = {
    "ms1-many": 3.0e-7,  # [1.5e-7]
    "ms1-few": 1.7e-7,  # [8.4e-8]
    "ms1-40k": 2.2e-7,  # [1.1e-7]
    "ms1-40960": 4.5e-7,  # [2.2e-7]
    "ms-hop512": 2.4e-7,  # [1.2e-7]
    "ms-hop2048": 2.5e-7,  # [1.3e-7]
    "any-hop768": 4.3e-7,  # [2.1e-7]
    "any-hop4096": 2.4e-7,  # [1.2e-7]
    "any-hop5120": 2.0e-7,  # [1.0e-7]
    "pairw-mono": 3.3e-7,  # [1.6e-7]
    "pairw-3ch-one": 1.4e-7,  # [6.6e-8]
    "pairw-6ch": 3.9e-7,  # [1.9e-7]
    "pairw-8ch": 2.6e-7,  # [1.3e-7]
    "run-ms-48k": 2.0e-7,  # [9.9e-8]
    "run-ms-50k": 2.4e-7,  # [1.2e-7]
    "run-ms-44k": 1.8e-7,  # [8.9e-8]
    "run-ms-40k": 2.3e-7,  # [1.2e-7]
    "run-ms-8win": 2.2e-7,  # [1.1e-7]
    "run-6ch-50k": 2.4e-7,  # [1.2e-7]
    "run-mono-44k": 1.9e-7,  # [9.4e-8]
    "run-mono-40k": 1.7e-7,  # [8.6e-8]
    "run-3ch-48k": 1.7e-7,  # [8.4e-8]
    "16k-hop2048": 1.4e-7,  # [7.0e-8]
    "16k-7win": 1.3e-7,  # [6.1e-8]
    "16k-mono": 1.5e-7,  # [7.5e-8]
    "16k-6ch": 1.5e-7,  # [7.5e-8]
    "gen-4096-hop1000": 1.4e-7,  # [6.7e-8]
    "gen-2048-mono": 9.5e-8,  # [4.7e-8]
    "gen-8192-6ch": 2.4e-7,  # [1.2e-7]
    "gen-32768": 9.0e-8,  # [4.4e-8]
    "gen-n2-40k": 1.0e-8,  # [0]
    "gen-n4-40k": 1.0e-8,  # [0]
    "ragged-ms1": 2.8e-7,  # [1.4e-7]
    "ragged-pairw": 2.1e-7,  # [1.0e-7]
    "ragged-run": 2.3e-7,  # [1.1e-7]
}

# the forms the table must keep reaching: every kernel, both row modes of fft16k_run, and NE_LAST 1 ... 4
FORMS = {MS1, MS, ANY, PAIRW, RUN, F16K, GEN}

RATIOS_DB = (20.0, 0.0, -6.0, -20.0, -60.0, -90.0, -120.0, None)        # second row against the first; None: exactly zero
STEPS = (1.0, 1.9, 1.0, 2.1, 2.0, 4.0, 0.5, 0.25, 1.0, 1 / 1.9, 1.0, 1 / 2.1, 4.0, 0.0, 1.0, 2.0)   # envelope per hold of hops


def ne_last(rate):
    """slices of k_fft16k_run's last epilogue iteration at N = 16384 (launch_spectrum)"""
    ngroups = (R.retained_bins(rate, 16384)[1] + 3) >> 2
    n_iter = (4 * ngroups + 2047) >> 11
    return (4 * ngroups - 2048 * (n_iter - 1) + 511) >> 9


def first_end(n, hop):
    """window 0 ends at (N / hop + 1) hop (stream_shape)"""
    return (n // hop + 1) * hop


def frames_for(n, hop, nw):
    return first_end(n, hop) + (nw - 1) * hop if nw > 0 else first_end(n, hop) - 1


def plan_of(b):
    g = b.geometry
    return (L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT).decode(), g.fft_windows_per_block, g.fft_blocks)


def tone_bins(rate, n):
    """the planted bins of (rate, N): first and last retained bin, the N = 4096 publish-block edges, one inside"""
    first, count = R.retained_bins(rate, n)
    last = first + count - 1
    ks = [first, last, first + count // 3]
    if n == 4096:
        ks += [255, 256, 257]
    return [k for k in ks if first <= k <= last]


def _signal(rng, frames, n, hop, rate, k, level, noise_db, env):
    """level x (a tone on bin k of N + noise noise_db under it), times env per hop (hop h = frames [first_start + h hop, ...))"""
    t = np.arange(frames, dtype=np.float64)
    tone = np.cos(np.pi * t + 0.3) if 2 * k == n else np.sin(2 * np.pi * k * t / n + rng.uniform(0, 2 * np.pi))
    x = level * (tone + 10 ** (-noise_db / 20) * rng.uniform(-1, 1, frames))
    if env is not None:
        h = np.clip((t.astype(np.int64) - (first_end(n, hop) - n)) // hop, 0, None)
        x = x * env[np.minimum(h, env.size - 1)]
    return x


def _envelope(rng, hops, hold):
    """per-hop gains: STEPS each held `hold` hops from a random start (kept within 0 dB ... -60 dB, or silent)"""
    e = np.empty(hops)
    g, j0 = 1.0, int(rng.integers(0, len(STEPS)))
    for h in range(hops):
        if h % hold == 0:
            s = STEPS[(j0 + h // hold) % len(STEPS)]
            g = 1.0 if s == 0.0 and g == 0.0 else (0.0 if s == 0.0 else (g * s if g else 1.0))
            g = min(max(g, 1e-3), 1.0) if g else 0.0
        e[h] = g
    return e


def make_streams(case, lengths):
    """[stream] -> [frames][channels] f32"""
    rate, n, hop, Cc = case.rate, case.n, case.hop, case.ch
    F = frames_for(n, hop, case.nw)
    hops = case.nw + n // hop + 2
    bins = tone_bins(rate, n)
    out = []
    for i in range(case.ns):
        rng = np.random.default_rng(1000 * i + case.nw + Cc)
        ratio = RATIOS_DB[i % len(RATIOS_DB)]
        level = 0.5 * 10 ** (-(i % 5) * 9 / 20)                       # streams at their own levels, 0 ... -36 dB
        if Cc == 2:
            km, ks = bins[i % len(bins)], bins[(i + 1) % len(bins)]
            env = _envelope(rng, hops, 4 if i % 2 else 1)
            m = _signal(rng, F, n, hop, rate, km, level, 40 + 10 * (i % 4), None)
            if ratio is None:
                s = np.zeros(F)
            else:
                s = _signal(rng, F, n, hop, rate, ks, level * 10 ** (ratio / 20), 30 + 10 * (i % 5), env)
            x = np.stack([m + s, m - s], 1)
        else:
            x = np.empty((F, Cc))
            for c in range(Cc):
                j = i * Cc + c
                big = RATIOS_DB[j % len(RATIOS_DB)]
                env = _envelope(rng, hops, 1 + 3 * (j % 2))
                if big is None or big < -10:                         # a drop of that size between two windows (or silence)
                    a = int(rng.integers(2, max(3, hops - 8)))
                    env[a:a + 5] = 0.0 if big is None else 10 ** (big / 20)
                elif big > 0:
                    a = int(rng.integers(2, max(3, hops - 8)))
                    env[a:] *= 10 ** (big / 20) / 10
                x[:, c] = _signal(rng, F, n, hop, rate, bins[j % len(bins)], level * (0.9 ** c), 40 + 10 * (j % 4), env)
        x = x.astype(np.float32)
        x[int(lengths[i]):] = 0.0
        out.append(x)
    return out


def _rows(x, case, w):
    """the f64 rows of window w of one stream ([frames][channels] f32)"""
    p0 = first_end(case.n, case.hop) - case.n + w * case.hop
    seg = x[p0:p0 + case.n]
    if case.ch == 2:
        return [R.spectrum_row_f64(s, case.rate, case.n) for s in R.mid_side_f32(seg)]
    return [R.spectrum_row_f64(seg[:, c], case.rate, case.n) for c in range(case.ch)]


def _windows_to_check(case, i, nwi, wpb):
    if nwi == 0:
        return []
    if i in (0, case.ns - 1):
        return list(range(nwi))
    runs = set()
    for r0 in range(0, nwi, wpb):
        runs |= {r0, min(r0 + wpb, nwi) - 1}
    if case.ragged is not None:
        runs |= set(range((nwi - 1) // wpb * wpb, nwi))
    return sorted(runs)


def check_row(got, ref, pink, bound, what, worst, floor=None):
    zero = np.all(ref == -150.0 + pink)
    if zero:
        assert np.all(np.abs(got - (-150.0 + pink)) <= 1e-4), (what, "zero row")
        return
    e, f = R.row_error(got, ref, pink), R.floor_error(got, ref, pink)
    worst[0] = max(worst[0], e)
    if bound is not None:
        assert e <= bound, (what, e, bound)
        assert floor is None or f <= floor, (what, "floor", f, floor)
        assert db_close(got, ref, 0.01, pink=pink), what     # the 70 dB counted on the row's own levels, pink out


def _lengths(case):
    F = frames_for(case.n, case.hop, case.nw)
    if case.ragged is None:
        return np.full(case.ns, F, np.int64)
    nws = [case.ragged[i % len(case.ragged)] for i in range(case.ns)]
    extra = [(i * 37) % case.hop if v else 0 for i, v in enumerate(nws)]       # anywhere before the next window's end
    return np.array([frames_for(case.n, case.hop, v) + e for v, e in zip(nws, extra)], np.int64).clip(max=F)


def run_case(case, strict=True):
    """one case; returns (plan, worst row_error).  strict=False (diagnostics): no plan or bound assertions."""
    F = frames_for(case.n, case.hop, case.nw)
    lengths = _lengths(case)
    b = ssa.Batch(case.rate, case.ch, case.ns, F, case.n, case.hop, flags=L.SS_BATCH_FFT)
    try:
        assert b.layout.n_windows == case.nw, (case.name, b.layout.n_windows)
        if case.ragged is not None:
            b.set_lengths(lengths)
        plan = plan_of(b)
        if strict:
            assert plan == case.plan, (case.name, plan, case.plan)
        xs = make_streams(case, lengths)
        b.upload(0, np.concatenate([x.reshape(-1) for x in xs]))
        b.run(); b.sync()
        pink = R.pink_db(case.rate, case.n)
        worst = [0.0]
        bound = case.bound if strict else None
        wpb = plan[1]
        for i in range(case.ns):
            nwi = b.stream_shape(i).n_windows
            want = case.ragged[i % len(case.ragged)] if case.ragged is not None else case.nw
            assert nwi == want, (case.name, i, nwi, want)
            check = _windows_to_check(case, i, nwi, wpb)
            if not check:
                continue
            got = b.fft(i)
            for w in check:
                for c, ref in enumerate(_rows(xs[i], case, w)):
                    check_row(got[w, c].astype(np.float64), ref, pink, bound, (case.name, i, w, c), worst, FLOOR[case.name])
        return plan, worst[0]
    finally:
        b.close()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_spectrum_form_against_f64(case):
    run_case(case)


def test_the_table_reaches_every_form():
    """every kernel, both row modes of fft16k_run and NE_LAST 1 ... 4 in some case's asserted plan; every bound under CAP"""
    assert {c.plan[0] for c in CASES} | {p[0] for p in ONE_WINDOW_PLANS.values()} == FORMS
    runs = [c for c in CASES if c.plan[0] == RUN]
    assert {c.ch == 2 for c in runs} == {True, False}
    assert {ne_last(c.rate) for c in runs if c.ch == 2} == {1, 2, 3, 4}
    assert {ne_last(c.rate) for c in runs if c.ch != 2} >= {1, 3, 4}
    assert set(FLOOR) == {c.name for c in CASES}
    assert all(c.bound <= CAP for c in CASES) and all(v <= CAP for v in ONE_WINDOW_BOUNDS.values())
    assert any(c.plan[0] in (PAIRW, RUN) and c.plan[2] % 8 for c in CASES)          # a grid rounded up to a multiple of 8
    assert any(c.plan[0] == PAIRW and c.nw % 2 for c in CASES)                      # a half-empty last pair


# ---- one-window callers: the plan of a batch of one stream and one window at hop 1024, then the caller's row against f64

# (N, channels) -> plan
ONE_WINDOW_PLANS = {(4096, 1): (PAIRW, 2, 1), (16384, 1): (F16K, 1, 1), (2048, 1): (GEN, 1, 1), (32768, 1): (GEN, 1, 1),
                    (16384, 2): (F16K, 1, 2)}
# measured: get_fft 4096 7.7e-7, 16384 7.3e-7, 2048 2.3e-7, 32768 6.9e-7 (worst of 40 / 48 / 50 / 192 kHz); tick 2.5e-7
ONE_WINDOW_BOUNDS = {4096: 3e-6, 16384: 2.5e-6, 2048: 9e-7, 32768: 2.5e-6, "tick": 1e-6}
# floor_error, 2x the measured worst: get_fft 4096 4.2e-8, 16384 7.5e-8, 2048 3.3e-8, 32768 4.0e-8; tick 6.6e-8
ONE_WINDOW_FLOOR = {4096: 9e-8, 16384: 1.5e-7, 2048: 7e-8, 32768: 8e-8, "tick": 1.4e-7}


@pytest.mark.parametrize("key", list(ONE_WINDOW_PLANS), ids=["N%d-C%d" % k for k in ONE_WINDOW_PLANS])
def test_one_window_plan(key):
    n, ch = key
    b = ssa.Batch(48000, ch, 1, first_end(n, 1024), n, 1024, flags=L.SS_BATCH_FFT)
    try:
        assert b.layout.n_windows == 1
        assert plan_of(b) == ONE_WINDOW_PLANS[key]
    finally:
        b.close()


def get_fft_worst(n, rate, strict=True):
    """get_fft on windows with tones on the planted bins, quiet noise at several levels, one all-zero window"""
    pink = R.pink_db(rate, n)
    worst = [0.0]
    a = ssa.Analyzer(2, rate)
    try:
        rng = np.random.default_rng(n + rate)
        for j, k in enumerate(tone_bins(rate, n) + [None]):
            level = 0.7 * 10 ** (-j * 11 / 20)
            if k is None:
                x = np.zeros(n, np.float32)
            else:
                x = _signal(rng, n, n, 1024, rate, k, level, 30 + 12 * j, None).astype(np.float32)
            got = np.asarray(a.get_fft(x))[:, 1]
            ref = R.spectrum_row_f64(x, rate, n)
            check_row(got, ref, pink, ONE_WINDOW_BOUNDS[n] if strict else None, ("get_fft", n, rate, k), worst, ONE_WINDOW_FLOOR[n])
    finally:
        a.close()
    return worst[0]


@pytest.mark.parametrize("n", [4096, 16384, 2048, 32768])
@pytest.mark.parametrize("rate", [40000, 48000, 50000, 192000])
def test_get_fft_against_f64(n, rate):
    get_fft_worst(n, rate)


def tick_worst(strict=True):
    """ss_session_tick_file (k_fft16k, mid/side) at positions one frame past the first window, odd, and at the end of the file"""
    rate, frames = 48000, 16384 * 3 + 777
    rng = np.random.default_rng(3)
    bins = tone_bins(rate, 16384)
    m = _signal(rng, frames, 16384, 1024, rate, bins[0], 0.4, 50, None)
    s = _signal(rng, frames, 16384, 1024, rate, bins[1], 0.4e-3, 40, _envelope(rng, 60, 2))
    x = np.stack([m + s, m - s], 1).astype(np.float32)
    pink = R.pink_db(rate, 16384)
    worst = [0.0]
    sess = ssa.FileSession(x.reshape(-1), 2, rate)
    try:
        for pos_f in (16385, 20000 + 3, 33001, frames):
            res = sess.analyze_audio_file_samples(2 * pos_f)
            assert res.fft_ran and res.mid_status == 0 and res.side_status == 0, pos_f
            mid, side = R.mid_side_f32(x[pos_f - 16384:pos_f])
            for got, sig in ((sess.mid_fft[:, 1], mid), (sess.side_fft[:, 1], side)):
                check_row(np.asarray(got), R.spectrum_row_f64(sig, rate, 16384), pink, ONE_WINDOW_BOUNDS["tick"] if strict else None,
                          ("tick", pos_f), worst, ONE_WINDOW_FLOOR["tick"])
    finally:
        sess.close()
    return worst[0]


def test_tick_file_against_f64():
    tick_worst()
