"""Batch pair series and pair regions (ss_batch_pair_series, ss_batch_pair_regions): per (stream, 100 ms entry, channel pair) the
f64 sums of x_a^2, x_b^2 and x_a x_b, and their reduction over time ranges and groups.

The reference is numpy, in this file.  Where the samples are multiples of 2^-8 in [-1, 1] every product is a multiple of 2^-16 and
an entry's sums stay far under 2^53 units, so f64 addition is exact in any order and the records must be EQUAL byte for byte (the
sums start from +0).  On random f32 material the sums are held to the worst-case bound of recursive f64 summation in any order
against math.fsum of the exact products: |got - ref| <= g * sum|x_a x_b|, g = (N - 1) u / (1 - (N - 1) u), u = 2^-53, N the entry's
counted frames.  The regions are reduced from the DOWNLOADED series with the header's rule as a few lines of Python floats (one
rounded f64 operation each) and every field must be equal."""
import ctypes
import math

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import (GROUP_PAIR_DTYPE, PAIR_ENTRY_DTYPE, REGION_PAIR_DTYPE, pair_balance_db, pair_correlation,
                                  pair_mono_loss_db)

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NO_GROUP = L.SS_REGION_NO_GROUP
DEFAULT = [(0, 1)]


def make_batch(rate, channels, streams, frames, flags=L.SS_BATCH_TRUE_PEAK):
    return ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=flags)


def s100(rate):
    return (rate + 5) // 10


def exact_noise(rng, frames, channels):
    """multiples of 2^-8 in [-1, 1]"""
    return (rng.integers(-256, 257, (frames, channels)) / 256.0).astype(np.float32)


def upload(b, streams, fill=0.0):
    slot, C = int(b.cfg.frames_per_stream), int(b.cfg.channels)
    pcm = np.full((len(streams), slot, C), fill, np.float32)
    for s, x in enumerate(streams):
        pcm[s, :len(x)] = x
    b.upload(0, pcm)


# ------------------------------------------------------------------------------------------------------------ reference
def reference(x, S, pairs, exact):
    """one stream x [frames][channels] f32 -> (records [entries][pairs], sum|x_a x_b| bounds [entries][pairs][3])"""
    x = np.asarray(x, np.float32)
    F = x.shape[0]
    E = (F + S - 1) // S
    out, bound = np.zeros((E, len(pairs)), PAIR_ENTRY_DTYPE), np.zeros((E, len(pairs), 3))
    add = (lambda v: float(np.sum(np.concatenate(([0.0], v))))) if exact else math.fsum
    for j in range(E):
        e = x[j * S:min((j + 1) * S, F)]
        for k, (pa, pb) in enumerate(pairs):
            ok = np.isfinite(e[:, pa]) & np.isfinite(e[:, pb])
            a, b = e[ok, pa].astype(np.float64), e[ok, pb].astype(np.float64)
            out[j, k] = (add(a * a), add(b * b), add(a * b), int(ok.sum()), int((~ok).sum()))
            bound[j, k] = (math.fsum(a * a), math.fsum(b * b), math.fsum(np.abs(a * b)))
    return out, bound


def gamma(n):
    u = 2.0 ** -53
    return (n - 1) * u / (1 - (n - 1) * u) if n > 1 else 0.0


def check_series(b, streams, pairs, tag, exact=True):
    """queue the series for `pairs` (None: the default) and hold every stream's download against reference()"""
    S = s100(int(b.cfg.sample_rate))
    b.pair_series(pairs)
    got_all = []
    for s, x in enumerate(streams):
        got = b.pair_entries(s)
        ref, bound = reference(x, S, DEFAULT if pairs is None else pairs, exact)
        assert got.shape == ref.shape, (tag, s, got.shape, ref.shape)
        if exact:
            assert got.tobytes() == ref.tobytes(), (tag, s, got[got != ref][:4], ref[got != ref][:4])
        else:
            assert np.array_equal(got["frames"], ref["frames"]) and np.array_equal(got["skipped"], ref["skipped"]), (tag, s)
            for i, f in enumerate(("s_aa", "s_bb", "s_ab")):
                err, lim = np.abs(got[f] - ref[f]), np.vectorize(gamma)(ref["frames"]) * bound[:, :, i]
                assert (err <= lim).all(), (tag, s, f, float((err - lim).max()))
        got_all.append(got)
    return got_all


# ------------------------------------------------------------------------------------------------------------ 1. exact sums
@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("channels", [2, 3, 6])
def test_exact_sums_at_every_entry_edge(channels, rate):
    S = s100(rate)
    lengths = [0, 1, S - 1, S, S + 1, 2 * S + 71]
    slot = 2 * S + 71                                        # odd: every other stream starts off a 16-byte boundary
    lists = [None, [(1, 0)], [(0, 0)]] + ([[(0, 1), (4, 5)]] if channels == 6 else [[(2, 0), (1, 1), (0, 2)]] if channels == 3 else [[(0, 1), (1, 0)]])
    rng = np.random.default_rng(rate + channels)
    for turn in (0, 1):                                      # ... and every length meets both alignments
        order = lengths[turn:] + lengths[:turn]
        streams = [exact_noise(rng, n, channels) for n in order]
        b = make_batch(rate, channels, len(order), slot)
        upload(b, streams, fill=0.5)                         # (behind a stream's own length: not silence)
        b.set_lengths(order)
        for pairs in lists:
            got = check_series(b, streams, pairs, (rate, channels, turn, pairs))
            tile, cap, n_pairs = b.pair_series_plan()
            assert cap == 3 and n_pairs == len(pairs or DEFAULT) and tile > 0
            assert got[order.index(0)].shape == (0, n_pairs)                 # F_s == 0: no entries
            assert int(got[order.index(S + 1)][1, 0]["frames"]) == 1
        b.close()


def test_mono_off_a_16_byte_boundary():
    rate, S = 44100, 4410                                    # entry j starts at float 4410 j: every other one off the boundary
    lengths = [2 * S + 71, S + 1, 3]
    rng = np.random.default_rng(1)
    streams = [exact_noise(rng, n, 1) for n in lengths]
    b = make_batch(rate, 1, 3, 2 * S + 71)
    upload(b, streams, fill=0.5)
    b.set_lengths(lengths)
    got = check_series(b, streams, [(0, 0)], "mono")
    assert all(np.array_equal(g["s_aa"], g["s_ab"]) and np.array_equal(g["s_bb"], g["s_ab"]) for g in got)
    assert L.lib().ss_batch_pair_series(b._h, None, 0) == L.SS_ERR_INVALID_ARG          # the default pair needs two channels
    b.close()


# ------------------------------------------------------------------------------------------------------------ 2. planted relations
@pytest.mark.parametrize("pairs", [None, [(0, 1), (0, 0)]])
def test_planted_relations_stay_in_their_entries(pairs):
    rate, S = 48000, 4800
    F = 7 * S
    rng = np.random.default_rng(2)
    x = exact_noise(rng, F, 2)
    x[1 * S:2 * S, 1] = x[1 * S:2 * S, 0]                    # b = a
    x[3 * S:4 * S, 1] = -x[3 * S:4 * S, 0]                   # b = -a
    x[5 * S:6 * S, 1] = 0.0                                  # b = 0
    b = make_batch(rate, 2, 2, F)                            # (not ragged: the slot's length for every stream)
    upload(b, [x, x[::-1].copy()])
    got = check_series(b, [x, x[::-1].copy()], pairs, "planted")[0][:, 0]     # (equal to the reference: nothing leaks into a neighbour)
    assert got[1]["s_ab"] == got[1]["s_aa"] == got[1]["s_bb"] > 0
    assert got[3]["s_ab"] == -got[3]["s_aa"] and got[3]["s_aa"] == got[3]["s_bb"] > 0
    assert got[5]["s_ab"] == 0 and got[5]["s_bb"] == 0 and got[5]["s_aa"] > 0
    for j in (0, 2, 4, 6):
        assert abs(got[j]["s_ab"]) < 0.2 * got[j]["s_aa"]
    c, loss = pair_correlation(got), pair_mono_loss_db(got)
    assert c[1] == 1.0 and c[3] == -1.0 and np.isnan(c[5]) and loss[1] == 0.0 and loss[3] == -np.inf
    assert pair_balance_db(got)[1] == 0.0 and pair_balance_db(got)[5] == -np.inf
    b.close()


# ------------------------------------------------------------------------------------------------------------ 3. random f32 material
@pytest.mark.parametrize("pairs", [None, [(1, 0), (0, 0)]])
def test_random_material_within_the_summation_bound(pairs):
    rate, S = 48000, 4800
    F = 2 * S + 71
    rng = np.random.default_rng(5)
    streams = [rng.uniform(-1, 1, (F, 2)).astype(np.float32), (0.3 + 0.1 * rng.standard_normal((F, 2))).astype(np.float32),
               np.full((F, 2), 0.25, np.float32)]
    b = make_batch(rate, 2, 3, F)
    upload(b, streams)
    got = check_series(b, streams, pairs, "random", exact=False)
    assert (got[2]["s_ab"] == 0.0625 * got[2]["frames"]).all()
    b.close()


# ------------------------------------------------------------------------------------------------------------ 4. ragged lengths, isolation
@pytest.mark.parametrize("channels", [2, 3])
def test_ragged_lengths_and_isolation(channels):
    rate, S = 48000, 4800
    slot = 2 * S + 71
    lengths = [S + 7, slot, 333]
    pairs = None if channels == 2 else [(0, 2), (1, 1)]
    rng = np.random.default_rng(40 + channels)
    streams = [exact_noise(rng, n, channels) for n in lengths]
    b = make_batch(rate, channels, 3, slot)
    upload(b, streams)
    b.set_lengths(lengths)
    clean = [g.tobytes() for g in check_series(b, streams, pairs, "ragged, clean")]
    poison = np.tile(np.array([np.nan, 1e30], np.float32), 3 * slot * channels // 2 + 1)[:3 * slot * channels].reshape(3, slot, channels)
    for s, n in enumerate(lengths):                          # stream s as it was; NaN and 1e30 behind it and in the whole slots next to it
        pcm = poison.copy()
        pcm[s, :n] = streams[s]
        b.upload(0, pcm)
        b.pair_series(pairs)
        assert b.pair_entries(s).tobytes() == clean[s], (channels, s)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 5. non-finite samples
@pytest.mark.parametrize("channels", [2, 6])
def test_nonfinite_samples_are_skipped(channels):
    rate, S = 48000, 4800
    F = 3 * S + 71
    pairs = None if channels == 2 else [(0, 1), (4, 5), (1, 0)]
    rng = np.random.default_rng(50 + channels)
    x = exact_noise(rng, F, channels)
    b = make_batch(rate, channels, 2, F)
    upload(b, [x, x])
    clean = check_series(b, [x, x], pairs, "before")[0]
    y = x.copy()
    y[[0, S + 1, 2 * S - 1], 0] = np.nan                     # channel a: an entry's first frame, mid-entry, an entry's last frame
    y[[S - 1, S, 2 * S + 2000], 1] = [np.inf, -np.inf, np.inf]       # channel b
    y[[S + 2, 3 * S, F - 1], 0] = np.nan                     # both in one frame: counted once
    y[[S + 2, 3 * S, F - 1], 1] = np.inf
    upload(b, [y, x])
    got, other = check_series(b, [y, x], pairs, "planted")   # (the reference's sums run over the remaining frames)
    assert got[:, 0]["skipped"].tolist() == [2, 4, 1, 2] and got[:, 0]["frames"].tolist() == [S - 2, S - 4, S - 1, 69]
    assert other.tobytes() == clean.tobytes()                # the stream next to it
    if channels == 6:
        assert got[:, 1].tobytes() == clean[:, 1].tobytes()  # a pair that does not use the channels
        assert np.array_equal(got[:, 2]["skipped"], got[:, 0]["skipped"]) and np.array_equal(got[:, 2]["s_aa"], got[:, 0]["s_bb"])
    b.close()


# ------------------------------------------------------------------------------------------------------------ 6. regions
def below(aa, bb, ab, t):
    """the header's rule: every product one rounded f64 multiplication"""
    p, q, tt = aa * bb, ab, t * t
    return (q < 0 or q * q < tt * p) if t >= 0 else (q < 0 and q * q > tt * p)


def reduce_regions(series, rows, n_groups, t, floor, min_run):
    """(region records [n][pairs], group records [n_groups][pairs]) from the downloaded series, in the stated order"""
    P = series[0].shape[1]
    reg, grp = np.zeros((len(rows), P), REGION_PAIR_DTYPE), np.zeros((n_groups, P), GROUP_PAIR_DTYPE)
    for i, (s, first, n, g) in enumerate(rows):
        for k in range(P):
            aa = bb = ab = 0.0
            frames = skipped = n_active = n_below = runs = best = run = 0
            first_below = best_at = NONE
            for j in range(first, first + n):
                e = series[s][j, k]
                eaa, ebb, eab = float(e["s_aa"]), float(e["s_bb"]), float(e["s_ab"])
                aa, bb, ab = aa + eaa, bb + ebb, ab + eab
                frames, skipped = frames + int(e["frames"]), skipped + int(e["skipped"])
                active = eaa + ebb > floor * float(e["frames"])
                n_active += active
                if active and below(eaa, ebb, eab, t):
                    n_below += 1
                    first_below = j if first_below == NONE else first_below
                    run += 1
                    if run > best:
                        best, best_at = run, j + 1 - run
                    runs += run == min_run
                else:
                    run = 0
            reg[i, k] = (aa, bb, ab, frames, skipped, n_active, n_below, first_below, best, best_at, runs)
    for g in range(n_groups):
        for k in range(P):
            acc = [0.0, 0.0, 0.0, 0, 0, 0, 0, 0]
            for i, row in enumerate(rows):
                if row[3] == g:
                    r = reg[i, k]
                    for m, f in enumerate(("s_aa", "s_bb", "s_ab")):
                        acc[m] = acc[m] + float(r[f])
                    for m, f in enumerate(("frames", "skipped", "n_active", "n_below", "below_runs")):
                        acc[3 + m] += int(r[f])
            grp[g, k] = tuple(acc)
    return reg, grp


def region_corpus(rng, S, lengths):
    """streams whose entries run through every kind: unrelated (0, 9), out of phase, in phase, mixtures a + noise of correlation about
    -0.77, -0.37, 0.37 and 0.77 (k / sqrt(k^2 + 0.25): either side of -0.5, 0 and 0.5), quiet, silent"""
    streams = []
    for n in lengths:
        x = rng.uniform(-0.5, 0.5, (n, 2)).astype(np.float32)
        E = (n + S - 1) // S
        kinds = rng.integers(0, 10, E)
        kinds[:8] = [1, 1, 6, 1, 1, 1, 7, 1][:E]             # a run of out-of-phase entries with a quiet and a silent one inside
        for j, kind in enumerate(kinds):
            e = x[j * S:(j + 1) * S]
            a = e[:, 0].copy()
            if kind == 1:
                e[:, 1] = -a
            elif kind == 2:
                e[:, 1] = a
            elif kind in (3, 4, 5, 8):
                e[:, 1] = np.float32({3: -0.6, 4: -0.2, 5: 0.2, 8: 0.6}[kind]) * a + np.float32(0.5) * e[:, 1]
            elif kind == 6:
                e[:, 0], e[:, 1] = a * np.float32(1e-3), -a * np.float32(1e-3)       # under the power floor, and out of phase
            elif kind == 7:
                e[:] = 0.0
        streams.append(x)
    return streams


@pytest.mark.parametrize("pairs", [None, [(1, 0), (0, 0), (0, 1)]])
def test_regions_and_groups_equal_the_reduced_series(pairs):
    rate, S = 48000, 4800
    lengths = [23 * S + 100, 9 * S, 3 * S + 1]
    E = [24, 9, 4]
    rng = np.random.default_rng(6)
    streams = region_corpus(rng, S, lengths)
    b = make_batch(rate, 2, 3, max(lengths))
    upload(b, streams)
    b.set_lengths(lengths)
    b.pair_series(pairs)
    series = [b.pair_entries(s) for s in range(3)]
    assert [len(x) for x in series] == E
    rows = [(s, 0, E[s], 0) for s in range(3)]                               # whole streams, several streams in one group
    rows += [(0, j, 1, NO_GROUP) for j in range(0, 24, 5)] + [(2, 3, 1, 1), (0, 23, 1, 1)]      # one entry; the tail entry alone
    rows += [(0, 20, 4, 1), (2, 1, 3, 1)]                                    # ends with the tail entry
    rows += [(1, 4, 0, 1), (0, 24, 0, 0), (2, 0, 0, NO_GROUP)]               # empty
    rows += [(0, 0, 10, 3), (0, 5, 10, 3), (0, 0, 10, 3), (1, 2, 6, 3), (1, 2, 6, 0)]        # overlapping and repeated
    n_groups = 4                                                             # group 2 has no regions
    floor = 1e-4
    seen = set()
    for t in (-0.5, 0.0, 0.5):
        for min_run in (1, 3):
            b.pair_regions(rows, n_groups, threshold=t, power_floor=floor, min_run=min_run)
            got_r, got_g = b.region_pairs(), b.group_pairs()
            ref_r, ref_g = reduce_regions(series, rows, n_groups, t, floor, min_run)
            assert got_r.tobytes() == ref_r.tobytes(), (t, min_run, got_r[got_r != ref_r][:3], ref_r[got_r != ref_r][:3])
            assert got_g.tobytes() == ref_g.tobytes(), (t, min_run, got_g, ref_g)
            assert not got_g[2].tobytes().strip(b"\0")
            seen.add((t, min_run, int(got_r[0, 0]["below_runs"]), int(got_r[0, 0]["longest_below"]), int(got_r[0, 0]["n_below"])))
    whole = b.region_pairs()[0, -1]                          # stream 0, pair (0, 1): entries 0 .. 7 are out, out, quiet, out x 3, silent, out
    assert int(whole["n_active"]) < E[0] and int(whole["first_below"]) == 0 and int(whole["longest_below"]) >= 3
    b.pair_regions(rows[:1], 1, threshold=0.0, power_floor=0.0, min_run=1)   # without a floor the quiet entry joins the run
    assert int(b.region_pairs()[0, -1]["longest_below"]) >= 6
    assert len({x[2:] for x in seen}) > 2                    # the thresholds and minima tell the entries apart
    b.close()


# ------------------------------------------------------------------------------------------------------------ 7. determinism, side effects
def test_determinism_and_replacing():
    rate, S = 48000, 4800
    F = 4 * S + 71
    rng = np.random.default_rng(7)
    streams = [rng.uniform(-1, 1, (F, 2)).astype(np.float32) for _ in range(3)]
    rows = [(0, 0, 5, 0), (1, 1, 3, 0), (2, 0, 5, NO_GROUP)]

    def downloads(b):
        return [b.pair_entries(s).tobytes() for s in range(3)] + [b.region_pairs().tobytes(), b.group_pairs().tobytes()]

    b = make_batch(rate, 2, 3, F)
    upload(b, streams)
    b.pair_series()
    b.pair_regions(rows, 1, threshold=0.5)
    first = downloads(b)
    b.pair_series()
    b.pair_regions(rows, 1, threshold=0.5)
    assert downloads(b) == first                             # byte for byte
    b.pair_series([(1, 0), (1, 1)])                          # another pair list replaces the series ...
    assert b.pair_series_plan()[2] == 2 and b.pair_entries(0).shape == (5, 2)
    assert b.region_pairs().tobytes() == first[3]            # ... and the regions stay what was reduced from the one before
    b.pair_regions(rows, 1, threshold=0.5)
    assert b.region_pairs().shape == (3, 2) and b.group_pairs().shape == (1, 2)
    b.pair_series()
    b.pair_regions(rows, 1, threshold=0.5)
    assert downloads(b) == first
    b.close()


def test_a_pair_series_moves_nothing_else():
    b = make_batch(48000, 2, 2, 48000, flags=L.SS_BATCH_ALL)
    b.synthesize(11)
    b.run()
    before = (b.checksums().tobytes(), bytes(b.results()), b.download_input(0).tobytes(), b.download_input(1).tobytes())
    x = [b.download_input(s).reshape(-1, 2) for s in range(2)]
    check_series(b, x, None, "behind a pass", exact=False)
    b.pair_regions([(0, 0, 10, 0), (1, 0, 10, 0)], 1)
    assert int(b.group_pairs()[0, 0]["frames"]) == 96000
    assert (b.checksums().tobytes(), bytes(b.results()), b.download_input(0).tobytes(), b.download_input(1).tobytes()) == before
    b.close()
    b = make_batch(48000, 2, 2, 48000, flags=L.SS_BATCH_ALL)            # a batch that never ran a pass
    b.synthesize(11)
    check_series(b, x, None, "no pass", exact=False)
    b.close()


# ------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_previous_results():
    rate, S = 48000, 4800
    F = 2 * S + 71
    rng = np.random.default_rng(8)
    lib = L.lib()
    b = make_batch(rate, 2, 2, F)
    upload(b, [exact_noise(rng, F, 2), exact_noise(rng, F, 2)])
    ent, reg, grp = np.zeros((3, 2), PAIR_ENTRY_DTYPE), np.zeros((2, 2), REGION_PAIR_DTYPE), np.zeros((1, 2), GROUP_PAIR_DTYPE)
    p_ent, p_reg, p_grp = (a.ctypes.data_as(ctypes.POINTER(t)) for a, t in ((ent, L.PairEntry), (reg, L.RegionPair), (grp, L.GroupPair)))
    n = ctypes.c_uint32(777)
    rows = np.array([(0, 0, 3, 0), (1, 1, 2, 0)], np.uint32)
    p_rows = rows.ctypes.data_as(ctypes.POINTER(L.LoudnessRegion))
    cfg = L.PairRegionConfig(0.0, 0.0, 1, 0)
    # before the first call of each kind
    assert lib.ss_batch_download_pair_series(b._h, 0, p_ent, 3, ctypes.byref(n)) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_pair_regions(b._h, p_rows, 2, 1, ctypes.byref(cfg)) == L.SS_ERR_INVALID_MODE
    b.pair_series([(0, 1), (1, 1)])
    assert lib.ss_batch_download_region_pairs(b._h, p_reg, 4) == L.SS_ERR_INVALID_MODE
    assert lib.ss_batch_download_group_pairs(b._h, p_grp, 2) == L.SS_ERR_INVALID_MODE
    b.pair_regions(rows, 1, threshold=0.25, power_floor=1e-3, min_run=2)

    def downloads():
        return [b.pair_entries(0).tobytes(), b.pair_entries(1).tobytes(), b.region_pairs().tobytes(), b.group_pairs().tobytes(), b.pair_series_plan()]

    good = downloads()
    # the series' refusals
    P = L.ChannelPair
    for pairs, count in (((P(0, 2),), 1), ((P(2, 0),), 1), ((P(0, 1), P(0, NONE)), 2), ((P(0, 1),) * 17, 17), (None, 1)):
        arr = (P * len(pairs))(*pairs) if pairs else None
        assert lib.ss_batch_pair_series(b._h, arr, count) == L.SS_ERR_INVALID_ARG, (pairs, count)
        assert downloads() == good
    assert lib.ss_batch_pair_series(b._h, (P * 16)(*[P(i & 1, 1) for i in range(16)]), 16) == L.SS_OK        # sixteen are allowed
    assert b.pair_entries(0).shape == (3, 16)
    b.pair_series([(0, 1), (1, 1)])
    assert downloads() == good
    # the regions' refusals
    nan = float("nan")
    for fields in ((nan, 0.0, 1, 0), (1.0, 0.0, 1, 0), (-1.0, 0.0, 1, 0), (1.5, 0.0, 1, 0), (0.0, nan, 1, 0), (0.0, -1e-9, 1, 0), (0.0, 0.0, 0, 0),
                   (0.0, 0.0, 1, 1)):
        bad = L.PairRegionConfig(*fields)
        assert lib.ss_batch_pair_regions(b._h, p_rows, 2, 1, ctypes.byref(bad)) == L.SS_ERR_INVALID_ARG, fields
        assert downloads() == good, fields
    assert lib.ss_batch_pair_regions(b._h, p_rows, 2, 1, None) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_pair_regions(b._h, None, 2, 1, ctypes.byref(cfg)) == L.SS_ERR_INVALID_ARG
    for row in ((2, 0, 1, 0), (0, 0, 4, 0), (0, 3, 1, 0), (0, NONE, 2, 0), (0, 0, 1, 1), (0, 0, 1, 5)):     # the peak regions' list errors
        one = np.array([rows[0], row], np.uint32)
        assert lib.ss_batch_pair_regions(b._h, one.ctypes.data_as(ctypes.POINTER(L.LoudnessRegion)), 2, 1, ctypes.byref(cfg)) == L.SS_ERR_INVALID_ARG, row
        assert downloads() == good, row
    # the downloads' own refusals write nothing
    assert lib.ss_batch_download_pair_series(b._h, 2, p_ent, 3, ctypes.byref(n)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_pair_series(b._h, 0, p_ent, 2, ctypes.byref(n)) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_region_pairs(b._h, p_reg, 3) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_group_pairs(b._h, p_grp, 1) == L.SS_ERR_CAPACITY
    assert n.value == 777 and not ent.tobytes().strip(b"\0") and not reg.tobytes().strip(b"\0") and not grp.tobytes().strip(b"\0")
    assert downloads() == good
    b.close()
