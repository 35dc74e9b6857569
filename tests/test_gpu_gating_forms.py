"""Every launch form of the gating kernels (soundscope_amd/csrc/ss_loudness.hip) against the plain f64 gate of tests/_f64ref.py.

The forms share eval_hist, hist_index and gate_range; what differs is how blocks are dealt to threads, where the tables and the
histograms live, and how the window sums are requested.  Shapes are picked by the launchers' own rules (launch_finalize,
launch_loudness_series, region_gate_threads) at 8 kHz, where a sub-block is 800 frames and every case is small:

  form                                        reached by
  k_finalize<SMALL> (tables in LDS, eager)    small-1 / -3 / -5 / -6 / -8 / -64, small-2048, every plant (batch `plants`)
  k_finalize<false>, 256 threads              lean-65-1, lean-65-6, every plant as stream 64 of 65
  k_finalize<false>, 1024 threads             long-1, long-2 (a slot of 2050 sub-blocks)
  k_loudness_series small / large             the same cases: the maxima of every stream
  k_region_gate 256 / 1024, k_group_eval      the region lists of every case; long-*: one list with a region over 2048 sub-blocks
  k_hist_eval                                 corpus_gate_read of every case and plant
  k_finalize_stream, k_ring_energy + tick     test_streaming_forms_handle[2], [5]
  k_meter_bank_gate, k_meter_bank_readings    test_streaming_forms_bank[*-bank], [*-ragged]

Batch forms and plants: the reference of a stream is gate_blocks over the stream's OWN downloaded sub-block sums, so the gate is
isolated from the filter and no slack at bin edges is needed: block counts and histograms are compared exactly, evaluations
within 1e-11 LU (derived in test_f64_reference.py: the order of at most 1000 positive additions, a tenfold margin for log10).
The series maxima are loudness values, 10 log10 of an energy the reference forms with the same operations: they are held to the
same 1e-11 (two implementations of log10 may differ in the last bit).  Streaming forms: the window readings against a
sequential f64 K-weighting at 1e-6 LU (the bar of test_gpu_independent.py); histograms against the f64 sub-blocks exactly, after
asserting that no reference value lies within 1e-5 LU of a bin edge (the rule of test_gpu_loudness_regions.py; the seeds were
picked on the CPU for it).  Measured worst deviations: 7.1e-15 LU against the 1e-11 bar, 3.2e-14 LU against the 1e-6 bar of
the window readings."""
import collections
import functools

import numpy as np
import pytest
from scipy import signal

import soundscope_amd as ssa
from soundscope_amd import _lib as L
import _f64ref as R
import _gating_plants as P

pytestmark = pytest.mark.gpu

RATE, S = P.RATE, P.S
METER = L.SS_BATCH_LUFS | L.SS_BATCH_LOUDNESS_SERIES
TOL_LU = 1e-11
READING_LU = 1e-6
CLEAR_LU = 1e-5
NONE = 0xFFFFFFFF
LENS = (0, 1, 3, 4, 29, 30, 31, 39, 40, 41)                # ragged lengths in sub-blocks: around every count at which a block appears
REGION_N = (0, 3, 4, 30, 39, 40)


def close(got, want, tol=TOL_LU):
    """infinities and the 0 of an empty range exactly, everything else within tol"""
    if np.isinf(want) or want == 0.0:
        return got == want
    return abs(got - want) <= tol


def lufs_max(e):
    """the largest loudness among energies (NaN never wins); -inf where there is none"""
    v = P.lufs(e)
    v = v[~np.isnan(v)]
    return float(v.max()) if v.size else -np.inf


def shortterm_every_subblock(sub, channels):
    """short-term energies ending with EVERY sub-block j >= 29 (the series has one after each): the ten phases of gate_blocks"""
    n = sub.shape[0]
    out = np.full(max(n - 29, 0), np.nan)
    for first in range(min(10, max(n - 29, 0))):
        out[first::10] = R.gate_blocks(sub, RATE, channels, first, n - first)[1]
    return out


Ref = collections.namedtuple("Ref", "blocks st hb hs integrated lra")


def reference(sub, channels, first=0, n=None):
    blocks, st = R.gate_blocks(sub, RATE, channels, first, n)
    hb, hs = R.gate_histograms(blocks, st)
    return Ref(blocks, st, hb, hs, R.integrated_from_hist(hb), R.lra_from_hist(hs))


def check_result(tag, res, ref):
    """a stream's, region's or group's result record against the reference evaluation"""
    assert (res.n_gating_blocks, res.n_st_blocks) == (ref.blocks.size, ref.st.size), (tag, res.n_gating_blocks, res.n_st_blocks)
    assert close(res.integrated_lufs, ref.integrated), (tag, "integrated", res.integrated_lufs, ref.integrated)
    assert close(res.loudness_range, ref.lra), (tag, "range", res.loudness_range, ref.lra)


def check_hists(tag, got, hb, hs):
    assert np.array_equal(got[0], hb), (tag, "block bins", np.flatnonzero(got[0] != hb)[:8])
    assert np.array_equal(got[1], hs), (tag, "short-term bins", np.flatnonzero(got[1] != hs)[:8])


def check_extremes(tag, ext, sub, ref, channels):
    st_all = shortterm_every_subblock(sub, channels)
    for got, at, e, first in ((ext.max_momentary, ext.max_momentary_at, ref.blocks, 3), (ext.max_shortterm, ext.max_shortterm_at, st_all, 29)):
        want = lufs_max(e)
        assert close(got, want), (tag, first, got, want)
        if not e.size:
            assert at == NONE, (tag, at)
        elif np.isfinite(want):
            v = P.lufs(e)
            assert abs(v[at - first] - want) <= TOL_LU, (tag, "the maximum's place", at)


def check_regions(tag, b, regions, subs, channels):
    """queue `regions` (stream, a, n), each in a group of its own and all of them once more in one shared group; every region's
    result and group against the reference of its range, the shared group against the sum"""
    k = len(regions)
    rows = [(s, a, n, g) for g, (s, a, n) in enumerate(regions)] + [(s, a, n, k) for s, a, n in regions]
    b.loudness_regions(rows, n_groups=k + 1)
    res, grp = b.region_results(), b.group_results()
    hb_all, hs_all = np.zeros(1000, np.uint64), np.zeros(1000, np.uint64)
    nb_all = ns_all = 0
    for g, (s, a, n) in enumerate(regions):
        ref = reference(subs[s], channels, a, n)
        check_hists((tag, "region", s, a, n), b.group_histograms(g), ref.hb, ref.hs)
        check_result((tag, "region", s, a, n), res[g], ref)
        check_result((tag, "region in the shared group", s, a, n), res[k + g], ref)
        check_result((tag, "group of", s, a, n), grp[g], ref)
        hb_all += ref.hb; hs_all += ref.hs
        nb_all += ref.blocks.size; ns_all += ref.st.size
    check_hists((tag, "shared group"), b.group_histograms(k), hb_all, hs_all)
    assert (grp[k].n_gating_blocks, grp[k].n_st_blocks) == (nb_all, ns_all), tag
    assert close(grp[k].integrated_lufs, R.integrated_from_hist(hb_all)), (tag, grp[k].integrated_lufs)
    assert close(grp[k].loudness_range, R.lra_from_hist(hs_all)), (tag, grp[k].loudness_range)
    return hb_all, hs_all


# ---------------------------------------------------------------- 1. batch forms
Case = collections.namedtuple("Case", "name ch ns slot_sub lens")
CASES = [
    # k_finalize<SMALL>: at most 64 streams of at most 2048 sub-blocks; one case per channel count — 1; 3: the eager form's unpaired
    # last channel; 5: weights 1, 1, 1, 1.41, 1.41; 6: a loud channel 3 of weight 0; 8: loud channels 6 and 7 of weight 0
    Case("small-1", 1, 10, 42, LENS),
    Case("small-3", 3, 10, 42, LENS),
    Case("small-5", 5, 10, 42, LENS),
    Case("small-6", 6, 10, 42, LENS),
    Case("small-8", 8, 10, 42, LENS),
    Case("small-64", 3, 64, 42, LENS),                    # the last stream count of the form
    Case("small-2048", 1, 2, 2048, (2048, 40)),           # ... and its last slot length: a thread walks eight blocks
    # k_finalize<false> on 256 threads: the 65th stream
    Case("lean-65-1", 1, 65, 42, LENS),
    Case("lean-65-6", 6, 65, 42, LENS),
    # k_finalize<false> on 1024 threads: a slot over 2048 sub-blocks, equal lengths and ragged
    Case("long-1", 1, 1, 2050, None),
    Case("long-2", 1, 2, 2050, (2050, 41)),
]


def material(seed, frames, slot_frames, channels):
    """one slot of a batch: `frames` frames that rise from far under the absolute gate (-90 dBFS) to about -15 LUFS — blocks under the
    absolute gate, blocks the relative gate drops and a wide spread of bins, whatever the length — every channel its own tone and
    noise; channel 3 of six and more and channels 6, 7 are twenty times louder (weight 0: nothing of them may count); the slot's
    tail behind the stream is loud and not part of it"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.9, 0.9, (slot_frames, channels)).astype(np.float32)
    if frames:
        t = np.arange(frames) / RATE
        env = np.exp(np.linspace(np.log(3e-5), np.log(0.12), frames))
        for c in range(channels):
            f = np.exp(rng.uniform(np.log(200.0), np.log(2500.0)))
            g = 20.0 if (c == 3 and channels >= 6) or c >= 6 else 1.0 + 0.3 * c
            x[:frames, c] = (g * env * (np.sin(2 * np.pi * f * t + c) + 0.2 * rng.standard_normal(frames))).astype(np.float32)
    return x


def case_lengths(case):
    """frames of every stream: its sub-blocks plus a few odd frames that complete none"""
    if case.lens is None:
        return None
    return [case.lens[s % len(case.lens)] * S + (5 + 11 * s) % 37 for s in range(case.ns)]


def case_regions(lens_sub):
    """whole streams, and ranges (s, a, n) with a > 0 for every n of REGION_N that fits"""
    regions = []
    for s, n in enumerate(lens_sub):
        regions.append((s, 0, n))
        for k in REGION_N:
            if k < n:
                regions.append((s, min(n - k, 1 + s % 3), k))
    return regions


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_batch_form_against_the_f64_gate(case):
    C, ns = case.ch, case.ns
    slot = case.slot_sub * S + 37
    frames = case_lengths(case)
    b = ssa.Batch(RATE, C, ns, slot, 4096, 1024, flags=METER)
    try:
        assert b.layout.n_subblocks == case.slot_sub
        if frames is not None:
            b.set_lengths(frames)
        x = np.stack([material(1000 * len(case.name) + s, slot if frames is None else frames[s], slot, C) for s in range(ns)])
        b.upload(0, x.reshape(-1))
        b.run()
        b.corpus_gate_enqueue()
        res, ext = b.results(), b.loudness_extremes()
        lens_sub = [int(b.stream_shape(s).n_subblocks) for s in range(ns)]
        assert lens_sub == ([case.slot_sub] * ns if frames is None else [f // S for f in frames])
        subs, refs = [], []
        for s in range(ns):
            sub = b.subblocks(s)[:lens_sub[s]]
            ref = reference(sub, C)
            subs.append(sub); refs.append(ref)
            check_result((case.name, s), res[s], ref)
            check_extremes((case.name, s), ext[s], sub, ref, C)
        hb_all = sum((r.hb for r in refs), np.zeros(1000, np.uint64))
        hs_all = sum((r.hs for r in refs), np.zeros(1000, np.uint64))
        check_hists((case.name, "corpus"), b.histograms(), hb_all, hs_all)
        ci, cl = b.corpus_gate_read()
        assert close(ci, R.integrated_from_hist(hb_all)) and close(cl, R.lra_from_hist(hs_all)), (case.name, ci, cl)
        # the material does what it is for: blocks under the absolute gate, blocks the relative gate drops, many bins
        longest = refs[int(np.argmax(lens_sub))]
        assert 0 < longest.hb.sum() < longest.blocks.size and np.count_nonzero(longest.hb) >= 15, case.name
        first_bin = int(np.flatnonzero(longest.hb)[0])
        assert R.gate_start_bin(0.1 * R.hist_moments(longest.hb)[1])[1] > first_bin, case.name
        assert longest.lra > 0.0
        # regions: on 256 threads; in the long cases a second list with a region over 2048 sub-blocks, on 1024
        n0 = lens_sub[0]
        regions = case_regions(lens_sub) if n0 < 2048 else \
            [(0, 0, 40), (0, 7, 30), (0, 1000, 39), (0, n0 - 40, 40), (0, 3, 2045), (0, 0, 2048), (ns - 1, 1, 4), (ns - 1, 2, 3), (ns - 1, lens_sub[-1], 0)]
        assert max(n for _, _, n in regions) <= 2048
        check_regions(case.name, b, regions, subs, C)
        if n0 > 2048:
            check_regions(case.name + " long list", b, regions + [(0, 1, 2049), (0, 0, 2050)], subs, C)
    finally:
        b.close()


# ---------------------------------------------------------------- 2. planted gate edges
@functools.lru_cache(maxsize=None)
def plant_signal(name):
    p = P.PLANTS[P.PLANT_IDS.index(name)]
    x = P.signal_of(p)
    ref = P.reference(x)
    p.check(ref)                                            # the plant's condition, from the reference alone
    assert P.edge_clearance(ref) >= CLEAR_LU, (name, P.edge_clearance(ref))
    return x, ref


PLANT_SLOT = max(sum(n for n, _ in p.segments) for p in P.PLANTS) * S + 37


def plant_slot(x, seed):
    """the plant in a slot: a loud tail behind it"""
    slot = np.random.default_rng(seed).uniform(-0.9, 0.9, PLANT_SLOT).astype(np.float32)
    slot[:x.size] = x
    return slot


def check_plant(tag, plant, x, cpu_ref, sub, res, ext):
    """the device's result of a planted stream: its own sub-blocks meet the plant's condition too and fall into the bins of the
    f64 filter's (the edge clearance is asserted), and the result record and the maxima are the reference's"""
    ref = P.reference_of_subblocks(sub)
    plant.check(ref)
    assert np.array_equal(ref.hb, cpu_ref.hb) and np.array_equal(ref.hs, cpu_ref.hs), tag
    check_result(tag, res, ref)
    check_extremes(tag, ext, sub, ref, 1)
    return ref


@pytest.fixture(scope="module")
def small_plants():
    """every plant as a stream of one batch in the SMALL form, with the regions queued: whole streams and each plant's tail"""
    n = len(P.PLANTS)
    xs = [plant_signal(p.name)[0] for p in P.PLANTS]
    b = ssa.Batch(RATE, 1, n, PLANT_SLOT, 4096, 1024, flags=METER)
    b.set_lengths([x.size for x in xs])
    b.upload(0, np.concatenate([plant_slot(x, 50 + i) for i, x in enumerate(xs)]))
    b.run()
    b.corpus_gate_enqueue()
    yield b
    b.close()


@pytest.fixture(scope="module")
def lean_plants():
    """65 streams, 64 of them digital silence: the plant goes into stream 64"""
    b = ssa.Batch(RATE, 1, 65, PLANT_SLOT, 4096, 1024, flags=METER)
    b.upload(0, np.zeros(65 * PLANT_SLOT, np.float32))
    yield b
    b.close()


@pytest.mark.parametrize("name", P.PLANT_IDS)
def test_planted_edge_small_form_and_region(small_plants, name):
    b = small_plants
    i = P.PLANT_IDS.index(name)
    plant = P.PLANTS[i]
    x, cpu_ref = plant_signal(name)
    n = int(b.stream_shape(i).n_subblocks)
    assert n == cpu_ref.n_sub
    sub = b.subblocks(i)[:n]
    ref = check_plant((name, "small"), plant, x, cpu_ref, sub, b.results()[i], b.loudness_extremes()[i])
    # the whole plant as a region, and the plant without its first second (another short-term phase is another set of blocks)
    b.loudness_regions([(i, 0, n, 0), (i, 10, n - 10, 1)], n_groups=2)
    res, grp = b.region_results(), b.group_results()
    check_hists((name, "region"), b.group_histograms(0), ref.hb, ref.hs)
    check_result((name, "region"), res[0], ref)
    check_result((name, "group"), grp[0], ref)
    tail = reference(sub, 1, 10, n - 10)
    check_hists((name, "tail region"), b.group_histograms(1), tail.hb, tail.hs)
    check_result((name, "tail region"), res[1], tail)
    check_result((name, "tail group"), grp[1], tail)


def test_planted_edges_corpus(small_plants):
    """the pooled histograms of all plants, and their gate (k_hist_eval)"""
    b = small_plants
    refs = [plant_signal(p.name)[1] for p in P.PLANTS]
    hb = sum((r.hb for r in refs), np.zeros(1000, np.uint64))
    hs = sum((r.hs for r in refs), np.zeros(1000, np.uint64))
    check_hists("plants", b.histograms(), hb, hs)
    ci, cl = b.corpus_gate_read()
    assert close(ci, R.integrated_from_hist(hb)) and close(cl, R.lra_from_hist(hs)), (ci, cl)
    assert hb[0] > 0 and hb[999] > 0 and np.isfinite(ci)
    # ... and without the +50 LUFS plant, whose blocks gate every other plant away: one group of the others (k_group_eval)
    rest = [i for i, p in enumerate(P.PLANTS) if p.name != "top-bin"]
    b.loudness_regions([(i, 0, refs[i].n_sub, 0) for i in rest], n_groups=1)
    hb = sum((refs[i].hb for i in rest), np.zeros(1000, np.uint64))
    hs = sum((refs[i].hs for i in rest), np.zeros(1000, np.uint64))
    check_hists("plants but the loudest", b.group_histograms(0), hb, hs)
    g = b.group_results()[0]
    want_i, want_l = R.integrated_from_hist(hb), R.lra_from_hist(hs)
    assert close(g.integrated_lufs, want_i) and close(g.loudness_range, want_l), (g.integrated_lufs, want_i, g.loudness_range, want_l)
    assert np.isfinite(want_i) and want_l > 1.0 and R.lra_entries_from_hist(hs)[0] > int(np.flatnonzero(hs)[0])


@pytest.mark.parametrize("name", P.PLANT_IDS)
def test_planted_edge_lean_form(lean_plants, name):
    b = lean_plants
    plant = P.PLANTS[P.PLANT_IDS.index(name)]
    x, cpu_ref = plant_signal(name)
    b.set_lengths([x.size] * 65)
    b.upload(64, plant_slot(x, 77))
    b.run()
    b.corpus_gate_enqueue()
    n = int(b.stream_shape(64).n_subblocks)
    sub = b.subblocks(64)[:n]
    res = b.results()
    ref = check_plant((name, "lean"), plant, x, cpu_ref, sub, res[64], b.loudness_extremes()[64])
    for s in (0, 31, 63):                                   # the silent streams count their blocks and bin none
        assert (res[s].n_gating_blocks, res[s].n_st_blocks, res[s].integrated_lufs, res[s].loudness_range) == \
               (ref.blocks.size, ref.st.size, -np.inf, 0.0), (name, s)
    check_hists((name, "corpus"), b.histograms(), ref.hb, ref.hs)          # the corpus is the plant alone
    ci, cl = b.corpus_gate_read()
    assert close(ci, ref.integrated) and close(cl, ref.lra), (name, ci, cl)


# ---------------------------------------------------------------- 3. streaming forms
SECONDS = 13                                                # 130 sub-blocks: the ring of 96 slots wraps
CALLS = (1, 799, 800, 801, 2400, 27000, 12345)             # frames per call; 27000: over 32 sub-blocks in one call
SEEDS = {2: 3, 5: 6}                                        # picked on the CPU: no reference value within 1e-5 LU of a bin edge


@functools.lru_cache(maxsize=None)
def live_material(channels):
    """three streams of 13 s whose level rises over 45 dB, the f64-filtered signal of each, and the gate's reference from the f64
    sub-blocks"""
    frames = SECONDS * RATE
    bq, aq = R.kweight_coeffs(RATE)
    out = []
    for s in range(3):
        rng = np.random.default_rng(100 * SEEDS[channels] + 10 * channels + s)
        t = np.arange(frames) / RATE
        env = np.exp(np.linspace(np.log(2e-3 * (1 + s)), np.log(0.35), frames))
        x = np.empty((frames, channels), np.float32)
        for c in range(channels):
            f = np.exp(rng.uniform(np.log(150.0), np.log(3000.0)))
            x[:, c] = (env * (np.sin(2 * np.pi * f * t + c) + 0.3 * rng.standard_normal(frames)) / (1 + 0.5 * c)).astype(np.float32)
        y = signal.lfilter(bq, aq, x.astype(np.float64), axis=0)
        ref = reference(R.kweighted_subblocks(x.reshape(-1), RATE, channels), channels)
        clear = P.edge_clearance(ref)
        assert clear >= CLEAR_LU, (channels, s, clear)
        assert np.count_nonzero(ref.hb) >= 20 and ref.hs.sum() == 11 and ref.lra > 0.0
        out.append((x, y, ref))
    return out


def call_sizes(total, offset):
    """CALLS in a cycle from entry `offset` on until `total` frames are fed"""
    sizes, fed, i = [], 0, offset
    while fed < total:
        n = min(CALLS[i % len(CALLS)], total - fed)
        sizes.append(n); fed += n; i += 1
    return sizes


def check_readings(tag, y, w, fed, momentary, shortterm):
    for frames, got in ((4 * S, momentary), (30 * S, shortterm)):
        want = R.window_reading(y, w, fed, frames)
        assert close(got, want, READING_LU), (tag, fed, fed % S, frames, got, want)


@pytest.mark.parametrize("channels", [2, 5])
def test_streaming_forms_handle(channels):
    """k_finalize_stream, and both window readings after every call: partial windows before 0.4 s and 3 s, calls that end on a
    sub-block boundary and inside one, across the ring's wrap"""
    x, y, ref = live_material(channels)[0]
    w = R.channel_weights(channels)
    a = ssa.Analyzer(channels, RATE)
    try:
        fed, on_boundary = 0, 0
        for n in call_sizes(x.shape[0], 0):
            a.add_samples(x[fed:fed + n].reshape(-1))
            fed += n
            on_boundary += fed % S == 0
            check_readings(("handle", channels), y, w, fed, a.get_momentary_lufs(), a.get_shortterm_lufs())
        assert fed == SECONDS * RATE and 0 < on_boundary < len(call_sizes(x.shape[0], 0))
        assert close(a.get_integrated_lufs(), ref.integrated), (a.get_integrated_lufs(), ref.integrated)
        assert close(a.get_loudness_range(), ref.lra), (a.get_loudness_range(), ref.lra)
    finally:
        a.close()


@pytest.mark.parametrize("ragged", [False, True], ids=["bank", "ragged"])
@pytest.mark.parametrize("channels", [2, 5])
def test_streaming_forms_bank(channels, ragged):
    """k_meter_bank_gate and k_meter_bank_readings: three streams advanced together, or each on its own phase (add_ragged: the
    call sizes start elsewhere in the cycle, and a stream that is done gets nothing)"""
    mat = live_material(channels)
    w = R.channel_weights(channels)
    frames = SECONDS * RATE
    plans = [call_sizes(frames, 2 * s if ragged else 0) for s in range(3)]
    bank = ssa.MeterBank(3, channels, RATE)
    fed = [0, 0, 0]
    phases = set()
    for k in range(max(len(p) for p in plans)):
        sizes = [p[k] if k < len(p) else 0 for p in plans]
        blocks = [mat[s][0][fed[s]:fed[s] + sizes[s]].reshape(-1) if sizes[s] else None for s in range(3)]
        if ragged:
            bank.add_ragged(blocks)
        else:
            bank.add(np.stack(blocks))
        fed = [f + n for f, n in zip(fed, sizes)]
        rd = bank.read()
        for s in range(3):
            assert int(rd["frames"][s]) == fed[s]
            check_readings(("bank", channels, ragged, s), mat[s][1], w, fed[s], float(rd["momentary"][s]), float(rd["shortterm"][s]))
        phases.add(tuple(f % S for f in fed))
    assert fed == [frames] * 3
    assert any(len(set(p)) == 3 for p in phases) == ragged          # the streams' phases really differ in the ragged pass
    rd = bank.read()
    for s in range(3):
        ref = mat[s][2]
        hb, hs = bank.histograms(s)
        check_hists(("bank", channels, ragged, s), (hb, hs), ref.hb, ref.hs)
        assert close(float(rd["integrated"][s]), R.integrated_from_hist(hb)), (s, rd["integrated"][s])
        assert close(float(rd["loudness_range"][s]), R.lra_from_hist(hs)), (s, rd["loudness_range"][s])
