"""The pair watch of a meter bank (ss_meter_bank_pair_watch*): the batch pair series' entries of everything a stream was given, kept
live — the ring of the newest complete entries, their window sum, the running totals and the runs of entries below a correlation
threshold.

The reference of an entry is numpy, in this file (model_entry): the samples widened to f64, the three products (exact), per lane
i mod 256 a sequential sum in ascending frames from +0, the xor butterfly at distances 32 .. 1 inside each 64 lanes, the four waves
added in wave order; a frame with a non-finite sample adds +0 and is counted.  Every comparison is BIT EQUALITY on random f32
material unless it says otherwise: against that model, against the batch series' general form on the same frames, against
ss_batch_pair_regions on the concatenation, and between every way of cutting the material into calls.  The window, the totals and
the run fields are reduced from the entries with the header's rule as a few lines of Python floats (one rounded f64 operation each)."""
import ctypes

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import PAIR_ENTRY_DTYPE, pair_correlation
from soundscope_amd.ingest import pcm_decode
from soundscope_amd.meter_bank import PAIR_WATCH_DTYPE, MeterBank
from test_gpu_pair_series import below, exact_noise, gamma, make_batch, reference, region_corpus, s100, upload

pytestmark = pytest.mark.gpu

NONE64 = 0xFFFFFFFFFFFFFFFF
NONE32 = 0xFFFFFFFF
DEFAULT = [(0, 1)]
SIXTEEN = [(0, 1), (1, 0), (2, 3), (4, 5), (5, 5), (0, 0), (3, 2), (0, 1), (5, 0), (0, 5), (2, 2), (1, 4), (4, 1), (3, 3), (0, 1), (2, 5)]
COUNTS = ("entries", "n_active", "n_below", "first_below", "longest_below", "longest_below_at", "below_runs", "trailing_below",
          "open_frames", "window_count", "reserved")


# ------------------------------------------------------------------------------------------------------------ the model
def model_entry(e, pa, pb):
    """one complete entry e [S][channels] f32 -> (s_aa, s_bb, s_ab, frames, skipped) in the kernel's order of additions"""
    ok = np.isfinite(e[:, pa]) & np.isfinite(e[:, pb])
    a = np.where(ok, e[:, pa], np.float32(0)).astype(np.float64)
    b = np.where(ok, e[:, pb], np.float32(0)).astype(np.float64)
    rows, lane_of = -(-len(e) // 256), np.arange(64)
    sums = []
    for prod in (a * a, b * b, a * b):                       # exact: 24 x 24 bits
        q = np.zeros(rows * 256)
        q[:len(prod)] = prod                                 # (a lane without a frame in the last row adds +0: nothing)
        lane = np.zeros(256)
        for r in q.reshape(rows, 256):                       # lane i mod 256, ascending frames, from +0
            lane = lane + r
        v = lane.reshape(4, 64)
        for d in (32, 16, 8, 4, 2, 1):                       # the butterfly: every lane of a wave ends with the same tree
            v = v + v[:, lane_of ^ d]
        sums.append(float(((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]))       # the waves in wave order
    return (*sums, int(ok.sum()), int((~ok).sum()))


def model_entries(x, S, pairs):
    """the complete entries of one stream x [frames][channels]: [E][pairs] of PAIR_ENTRY_DTYPE"""
    E = len(x) // S
    out = np.zeros((E, len(pairs)), PAIR_ENTRY_DTYPE)
    for j in range(E):
        for k, (pa, pb) in enumerate(pairs):
            out[j, k] = model_entry(x[j * S:(j + 1) * S], pa, pb)
    return out


def reduce_watch(entries, R, t, floor, min_run, open_frames=0):
    """the record of one (stream, pair) from ALL its complete entries [E] in order, as the header states it"""
    rec = np.zeros((), PAIR_WATCH_DTYPE)
    E = len(entries)
    for name, part in (("window", entries[E - min(R, E):]), ("total", entries)):
        aa = bb = ab = 0.0
        frames = skipped = 0
        for e in part:
            aa, bb, ab = aa + float(e["s_aa"]), bb + float(e["s_bb"]), ab + float(e["s_ab"])
            frames, skipped = frames + int(e["frames"]), skipped + int(e["skipped"])
        rec[name] = (aa, bb, ab, frames, skipped)
    n_active = n_below = runs = best = run = 0
    first_below = best_at = NONE64
    for j, e in enumerate(entries):
        eaa, ebb, eab = float(e["s_aa"]), float(e["s_bb"]), float(e["s_ab"])
        active = eaa + ebb > floor * float(e["frames"])
        n_active += active
        if active and below(eaa, ebb, eab, t):
            n_below += 1
            first_below = j if first_below == NONE64 else first_below
            run += 1
            if run > best:
                best, best_at = run, j + 1 - run
            runs += run == min_run
        else:
            run = 0
    for name, v in zip(COUNTS, (E, n_active, n_below, first_below, best, best_at, runs, run, open_frames, min(R, E), 0)):
        rec[name] = v
    return rec


def empty_record():
    return reduce_watch(np.zeros(0, PAIR_ENTRY_DTYPE), 1, 0.0, 0.0, 1)


# ------------------------------------------------------------------------------------------------------------ feeding
def watched(n, channels, rate, pairs=None, R=30, **cfg):
    bank = MeterBank(n, channels, rate)
    bank.enable_pair_watch(pairs, window_s=R / 10.0, **cfg)
    assert bank.pair_watch_plan() == (256, R, len(pairs or DEFAULT))
    return bank


def feed(bank, xs, calls):
    """calls: an int (add: that many frames to every stream) or a list (add_ragged: stream s's own count) per call"""
    fed = [0] * len(xs)
    for call in calls:
        counts = [call] * len(xs) if isinstance(call, int) else list(call)
        blocks = [x[f:f + c] for x, f, c in zip(xs, fed, counts)]
        if isinstance(call, int):
            bank.add(np.stack(blocks))
        else:
            bank.add_ragged([b if len(b) else None for b in blocks])
        fed = [f + c for f, c in zip(fed, counts)]
    return fed


def state(bank):
    """everything a caller can read: the records' bytes and every stream's (first_entry, ring bytes)"""
    rings = [bank.pair_watch_entries(s) for s in range(bank.n_streams)]
    return bank.pair_watch().tobytes(), [(first, ring.tobytes()) for first, ring in rings]


def general_list(channels, pairs):
    """a batch pair list that holds `pairs` in front and takes the general form (the stereo form: two channels, one pair a != b)"""
    pairs = list(pairs)
    return pairs + [(0, 0)] if channels == 2 and len(pairs) == 1 and pairs[0][0] != pairs[0][1] else pairs


# ------------------------------------------------------------------------------------------------------------ 1. entries
@pytest.mark.parametrize("rate", [48000, 44100])
@pytest.mark.parametrize("channels", [2, 3, 6])
def test_entries_against_the_model_and_the_batch(channels, rate):
    S, n = s100(rate), 5
    F = 2 * S + 71
    rng = np.random.default_rng(rate + channels)
    xs = [rng.uniform(-1, 1, (F, channels)).astype(np.float32) for _ in range(n)]
    lists = [None, [(1, 0)], [(0, 1), (1, 0), (0, 0)]] + ([SIXTEEN] if channels == 6 else [])
    batch = make_batch(rate, channels, n, F)
    upload(batch, xs)
    seen = {}
    for pairs in lists:
        plist = pairs or DEFAULT
        bank = watched(n, channels, rate, pairs)
        assert feed(bank, xs, [F]) == [F] * n
        rec = bank.pair_watch()
        assert rec.shape == (n, len(plist))
        batch.pair_series(general_list(channels, plist))
        assert not batch.pair_series_plan()[0] % 1024 and batch.pair_series_plan()[2] == len(general_list(channels, plist))
        for s in range(n):
            first, ring = bank.pair_watch_entries(s)
            want = model_entries(xs[s], S, plist)
            assert first == 0 and ring.shape == want.shape == (2, len(plist))
            assert ring.tobytes() == want.tobytes(), (pairs, s, ring, want)
            general = batch.pair_entries(s)[:2, :len(plist)]                 # (only complete entries are compared)
            assert ring.tobytes() == np.ascontiguousarray(general).tobytes(), (pairs, s)
            for k, pair in enumerate(plist):                                # a pair's record does not depend on the other pairs listed
                got = rec[s, k].tobytes()
                assert seen.setdefault((s, pair), got) == got, (pairs, s, pair)
                assert rec[s, k].tobytes() == reduce_watch(want[:, k], 30, 0.0, 0.0, 1, open_frames=71).tobytes(), (pairs, s, pair)
        del bank
    batch.close()


def test_against_the_stereo_form():
    """the batch's stereo form (16-byte loads, two frames a lane) adds in another order: equal where f64 addition is exact, and
    within the summation bound of tests/test_gpu_pair_series.py on random material"""
    rate, S, n = 48000, 4800, 3
    F = 2 * S + 71
    rng = np.random.default_rng(12)
    for exact in (True, False):
        xs = [exact_noise(rng, F, 2) if exact else rng.uniform(-1, 1, (F, 2)).astype(np.float32) for _ in range(n)]
        bank = watched(n, 2, rate)
        feed(bank, xs, [F])
        batch = make_batch(rate, 2, n, F)
        upload(batch, xs)
        batch.pair_series()                                  # the default pair on a stereo batch: the stereo form
        assert batch.pair_series_plan()[0] == 2048
        for s in range(n):
            ring, stereo = bank.pair_watch_entries(s)[1], batch.pair_entries(s)[:2]
            if exact:
                assert ring.tobytes() == np.ascontiguousarray(stereo).tobytes(), s
                continue
            ref, bound = reference(xs[s], S, DEFAULT, False)
            assert np.array_equal(ring["frames"], stereo["frames"]) and np.array_equal(ring["skipped"], stereo["skipped"])
            for i, f in enumerate(("s_aa", "s_bb", "s_ab")):
                lim = np.vectorize(gamma)(ref["frames"][:2]) * bound[:2, :, i]
                print(f, "bank - stereo", np.abs(ring[f] - stereo[f]).max(), "bank - fsum", np.abs(ring[f] - ref[f][:2]).max(), "bound", lim.min())
                assert (np.abs(ring[f] - stereo[f]) <= lim).all() and (np.abs(ring[f] - ref[f][:2]) <= lim).all(), (s, f)
        batch.close()


# ------------------------------------------------------------------------------------------------------------ 2. cuts
@pytest.mark.parametrize("rate", [48000, 44100])
def test_cuts_change_no_bit(rate):
    S, n, channels, pairs, R = s100(rate), 3, 3, [(0, 1), (2, 0)], 3
    F = 3 * S + 100
    rng = np.random.default_rng(rate + 2)
    xs = [rng.uniform(-1, 1, (F, channels)).astype(np.float32) for _ in range(n)]
    xs[1][[5, S + 300, 2 * S - 1], 1] = [np.nan, np.inf, -np.inf]              # skipped frames cross the cuts too

    def run(calls, bank=None):
        bank = bank or watched(n, channels, rate, pairs, R, threshold=0.5)
        assert feed(bank, xs, calls) == [F] * n
        return state(bank)

    def cut(*at):
        edges = [0, *at, F]
        return [b - a for a, b in zip(edges, edges[1:])]

    whole = run([F])
    for s in range(n):                                       # the one call against the model
        want = model_entries(xs[s], S, pairs)
        assert whole[1][s] == (0, want.tobytes()), s
    feeds = {"blocks of S / 10": cut(*range(S // 10, F, S // 10))}
    for at in (255, 256, 257):
        feeds["cut %d frames into an entry" % at] = cut(S + at)
    for at in (S - 1, S, S + 1):
        feeds["cut at %d" % at] = cut(at)
    feeds["cuts at both ends of entry 1"] = cut(S, 2 * S)   # each call completes an entry exactly and leaves nothing open
    feeds["one frame at a time around 2 S"] = cut(*range(2 * S - 300, 2 * S + 301))
    # ragged: random counts with zeros; stream 0 takes 2 S + 10 frames — two entries completed — in one call from inside an entry
    ragged = []
    for s in range(n):
        counts = [100, 2 * S + 10] if s == 0 else []
        while sum(counts) < F:
            counts.append(min(F - sum(counts), int(rng.choice([0, 1, 255, 256, 257, S // 10, S - 1, int(rng.integers(1, 2 * S))]))))
        ragged.append(counts)
    calls = max(len(c) for c in ragged)
    feeds["ragged"] = [[c[i] if i < len(c) else 0 for c in ragged] for i in range(calls)]
    assert any(0 in call for call in feeds["ragged"])
    for name, calls in feeds.items():
        assert run(calls) == whole, name
    assert run(feeds["ragged"]) == whole                     # two banks fed the same calls


# ------------------------------------------------------------------------------------------------------------ 3. non-finite samples
def test_nonfinite_samples_are_skipped_in_their_stream():
    rate, S, n = 44100, 4410, 3
    F = 3 * S + 5
    rng = np.random.default_rng(3)
    xs = [rng.uniform(-1, 1, (F, 2)).astype(np.float32) for _ in range(n)]
    bank = watched(n, 2, rate)
    feed(bank, xs, [F])
    clean = state(bank)
    ys = [x.copy() for x in xs]
    ys[1][[S + 0, S + 255], 0] = [np.nan, np.inf]            # entry 1 of stream 1: frames 0, 255, 256 and S - 1
    ys[1][[S + 256, 2 * S - 1], 1] = [-np.inf, np.nan]
    ys[1][S + 256, 0] = np.nan                               # both samples of one frame: counted once
    ys[0][[2 * S, 2 * S + 255], 1] = [np.inf, np.nan]        # the neighbouring stream, entry 2
    for calls in ([F], [1000] * (F // 1000) + [F % 1000]):   # in one call, and with the skipped counts carried across calls
        bank.enable_pair_watch()
        feed(bank, ys, calls)
        rec, got = bank.pair_watch(), state(bank)
        for s in range(n):
            want = model_entries(ys[s], S, DEFAULT)
            first, ring = bank.pair_watch_entries(s)
            assert first == 0 and ring.tobytes() == want.tobytes(), (calls[0], s)
            assert rec[s, 0].tobytes() == reduce_watch(want[:, 0], 30, 0.0, 0.0, 1, open_frames=5).tobytes(), (calls[0], s)
        ring1, ring0 = bank.pair_watch_entries(1)[1][:, 0], bank.pair_watch_entries(0)[1][:, 0]
        assert ring1["skipped"].tolist() == [0, 4, 0] and ring1["frames"].tolist() == [S, S - 4, S]
        assert ring0["skipped"].tolist() == [0, 0, 2] and int(rec[1, 0]["total"]["skipped"]) == 4 == int(rec[1, 0]["window"]["skipped"])
        assert np.isfinite([rec[s, 0]["total"][f] for s in range(n) for f in ("s_aa", "s_bb", "s_ab")]).all()
        assert got[1][2] == clean[1][2] and rec[2].tobytes() == np.frombuffer(clean[0], PAIR_WATCH_DTYPE).reshape(n, 1)[2].tobytes()


# ------------------------------------------------------------------------------------------------------------ 4. window and ring
RATE, S48 = 48000, 4800
_corpus = {}


def corpus():
    """two stereo streams of 35 entries that run through every kind of entry (test_gpu_pair_series.region_corpus), and the model's
    entries of them for the pairs (0, 1), (1, 0): computed once, shared, never changed"""
    if not _corpus:
        xs = region_corpus(np.random.default_rng(4), S48, [35 * S48 + 17, 35 * S48 + 17])
        _corpus["xs"] = xs
        _corpus["entries"] = [model_entries(x, S48, [(0, 1), (1, 0)]) for x in xs]
    return _corpus["xs"], _corpus["entries"]


@pytest.mark.parametrize("R", [1, 3, 30])
def test_window_ring_totals_and_runs(R):
    xs, entries = corpus()
    pairs, floor, n = [(0, 1), (1, 0)], 1e-4, 2
    stops = sorted({0, 1, R - 1, R, R + 5})
    bank = MeterBank(n, 2, RATE)
    seen = set()
    for t in (-0.5, 0.0, 0.5):
        for min_run in (1, 3):
            bank.enable_pair_watch(pairs, window_s=R / 10.0, threshold=t, power_floor=floor, min_run=min_run)
            fed = 0
            for E in stops:
                upto = E * S48 + (S48 - 1 if E == 0 else 17)                 # E == 0: one frame short of the first entry
                bank.add(np.stack([x[fed:upto] for x in xs]))
                fed = upto
                rec = bank.pair_watch()
                for s in range(n):
                    first, ring = bank.pair_watch_entries(s)
                    assert first == E - min(R, E) and ring.shape == (min(R, E), 2), (R, E, s)
                    assert ring.tobytes() == entries[s][first:E].tobytes(), (R, E, s)       # across the wrap: the newest, in order
                    for k in range(2):
                        want = reduce_watch(entries[s][:E, k], R, t, floor, min_run, open_frames=fed - E * S48)
                        assert rec[s, k].tobytes() == want.tobytes(), (R, E, s, k, t, min_run, rec[s, k], want)
                        aa = bb = ab = 0.0                   # the window is the sequential sum of the ring as downloaded
                        for e in ring[:, k]:
                            aa, bb, ab = aa + float(e["s_aa"]), bb + float(e["s_bb"]), ab + float(e["s_ab"])
                        w = rec[s, k]["window"]
                        assert (float(w["s_aa"]), float(w["s_bb"]), float(w["s_ab"])) == (aa, bb, ab)
                        assert int(w["frames"]) == int(ring[:, k]["frames"].sum()) and int(rec[s, k]["window_count"]) == len(ring)
                    seen.add((t, min_run, E, int(rec[s, 0]["n_below"]), int(rec[s, 0]["below_runs"]), int(rec[s, 0]["trailing_below"])))
    # the corpus starts out, out, quiet, out, out, out, silent, out: runs with inactive entries inside, told apart by the minima
    full = reduce_watch(entries[0][:R + 5, 0], R, 0.0, floor, 3)
    if R + 5 >= 8:
        assert int(full["first_below"]) == 0 and int(full["longest_below"]) >= 3 and int(full["n_active"]) < R + 5 and int(full["below_runs"]) >= 1
    assert len({x[3:] for x in seen}) > 3
    assert pair_correlation(bank.pair_watch()["total"]).shape == (n, 2)


# ------------------------------------------------------------------------------------------------------------ 5. against the batch regions
@pytest.mark.parametrize("R", [3, 30])
def test_against_batch_pair_regions(R):
    xs, _ = corpus()
    pairs, n, E = [(0, 1), (1, 0)], 2, 35
    batch = make_batch(RATE, 2, n, len(xs[0]))
    upload(batch, xs)
    batch.pair_series(pairs)                                 # two pairs: the general form
    bank = MeterBank(n, 2, RATE)
    for t, floor, min_run in ((0.0, 0.0, 1), (0.5, 1e-4, 3), (-0.5, 1e-4, 1)):
        bank.enable_pair_watch(pairs, window_s=R / 10.0, threshold=t, power_floor=floor, min_run=min_run)
        feed(bank, xs, [7 * S48 + 1234, len(xs[0]) - 7 * S48 - 1234])
        rec = bank.pair_watch()
        wc = min(R, E)
        batch.pair_regions([(s, 0, E, L.SS_REGION_NO_GROUP) for s in range(n)] + [(s, E - wc, wc, L.SS_REGION_NO_GROUP) for s in range(n)],
                           1, threshold=t, power_floor=floor, min_run=min_run)
        reg = batch.region_pairs()
        for s in range(n):
            for k in range(2):
                whole, window, r = reg[s, k], reg[n + s, k], rec[s, k]
                assert int(r["entries"]) == E and int(r["window_count"]) == wc
                for f in ("s_aa", "s_bb", "s_ab", "frames", "skipped"):
                    assert r["total"][f].tobytes() == whole[f].astype(r["total"][f].dtype).tobytes(), (t, s, k, f)
                    assert r["window"][f].tobytes() == window[f].astype(r["window"][f].dtype).tobytes(), (t, s, k, f)
                for f in ("n_active", "n_below", "longest_below", "below_runs"):
                    assert int(r[f]) == int(whole[f]), (t, s, k, f)
                for f in ("first_below", "longest_below_at"):
                    assert int(r[f]) == (NONE64 if int(whole[f]) == NONE32 else int(whole[f])), (t, s, k, f)
    batch.close()


# ------------------------------------------------------------------------------------------------------------ 6. input forms
def test_input_forms():
    """add_device from a base one float off an 8-byte boundary at an odd stride (a stereo frame is not 8-byte aligned in every other
    stream), and the 16-bit PCM forms: the records and rings of the f32 host feed of the decoded values"""
    rate, S, n, channels = 48000, 4800, 3, 2
    F = 2 * S + 71
    rng = np.random.default_rng(6)
    raw16 = [rng.integers(-32768, 32768, (F, channels)).astype(np.int16).view(np.uint8).reshape(-1) for _ in range(n)]
    xs = [pcm_decode(r.tobytes(), L.SS_PCM_S16).reshape(-1, channels) for r in raw16]             # ss_pcm_decode's values
    uniform, ragged = [S + 7, F - S - 7], [[S + 7, 0, F], [F - S - 7, F, 0]]
    src = ssa.Batch(rate, channels, n + 1, F, flags=L.SS_BATCH_LUFS)         # a device buffer of (n + 1) F frames
    floats = (n + 1) * F * channels
    bank = MeterBank(n, channels, rate)

    def run(form):
        bank.enable_pair_watch()
        fed = [0] * n
        for call in (ragged if "ragged" in form else uniform):
            counts = call if "ragged" in form else [call] * n
            blocks = [xs[s][fed[s]:fed[s] + f] for s, f in enumerate(counts)]
            raws = [raw16[s][fed[s] * channels * 2:(fed[s] + f) * channels * 2] for s, f in enumerate(counts)]
            if form == "add":
                bank.add(np.stack(blocks))
            elif form == "add_pcm":
                bank.add_pcm(np.concatenate(raws), L.SS_PCM_S16)
            elif form == "add_ragged":
                bank.add_ragged([b if len(b) else None for b in blocks])
            elif form == "add_ragged_pcm":
                bank.add_ragged_pcm([r if len(r) else None for r in raws], L.SS_PCM_S16)
            else:                                            # the device forms: stream s at base + s * stride floats
                base, stride = (1, F * channels + 1) if form.endswith("odd") else (0, F * channels)
                flat = np.zeros(floats, np.float32)
                for s, b in enumerate(blocks):
                    flat[base + s * stride:base + s * stride + b.size] = b.reshape(-1)
                src.upload(0, flat)
                src.sync()
                ptr = src.input_device_ptr() + 4 * base
                if "ragged" in form:
                    bank.add_ragged_device(ptr, counts, stride)
                else:
                    bank.add_device(ptr, counts[0], stride)
                bank.pair_watch()                            # (waits: the buffer may be overwritten now)
            fed = [a + f for a, f in zip(fed, counts)]
        assert fed == [F] * n
        return state(bank)

    want = run("add")
    for s in range(n):
        assert want[1][s] == (0, model_entries(xs[s], S, DEFAULT).tobytes()), s
    for form in ("add_pcm", "add_device", "add_device odd", "add_ragged", "add_ragged_pcm", "add_ragged_device", "add_ragged_device odd"):
        assert run(form) == want, form
    src.close()


# ------------------------------------------------------------------------------------------------------------ 7. stays out of the way
def test_the_pair_watch_moves_nothing_else():
    rate, S, n = 48000, 4800, 3
    F = 4 * S + 100
    rng = np.random.default_rng(7)
    xs = [(0.3 * rng.standard_normal((F, 2))).astype(np.float32) for _ in range(n)]
    xs[1][2000:9000] = 0.0
    calls = [480] * 8 + [[100, 0, 2 * S], [S, S, 0]]
    calls += [[F - sum(c if isinstance(c, int) else c[s] for c in calls) for s in range(n)]]

    def everything(pair_watch):
        bank = MeterBank(n, 2, rate)
        bank.enable_spectrum()
        bank.enable_signal_watch()
        if pair_watch:
            bank.enable_pair_watch(threshold=0.5)
        assert feed(bank, xs, calls) == [F] * n
        st, ch = bank.signal_watch()
        rows, status = bank.spectrum()
        out = [bank.read().tobytes(), st.tobytes(), ch.tobytes(), rows.tobytes(), status.tobytes()]
        for s in range(n):
            out += [a.tobytes() for a in bank.peaks(s)] + [a.tobytes() for a in bank.histograms(s)]
        return bank, out

    plain, off = everything(False)
    bank, on = everything(True)
    assert on == off
    del plain
    rec = bank.pair_watch()
    assert rec["entries"].tolist() == [[4]] * n and rec["open_frames"].tolist() == [[100]] * n
    # ss_meter_bank_reset leaves it alone
    before = state(bank)
    bank.reset()
    assert int(bank.read()[0]["frames"]) == 0 and state(bank) == before
    bank.reset([1])
    assert state(bank) == before
    # a stream given nothing keeps its bytes
    bank.add_ragged([xs[0][:S + 3], None, xs[2][:5]])
    after = bank.pair_watch()
    assert after[1].tobytes() == rec[1].tobytes() and bank.pair_watch_entries(1)[1].tobytes() == before[1][1][1]
    assert (int(after[0, 0]["entries"]), int(after[0, 0]["open_frames"]), int(after[2, 0]["open_frames"])) == (5, 103, 105)
    # the selective reset empties only the listed streams
    kept = state(bank)
    bank.reset_pair_watch([2, 0])
    got = bank.pair_watch()
    assert got[0].tobytes() == got[2].tobytes() == empty_record().tobytes() and got[1].tobytes() == rec[1].tobytes()
    assert bank.pair_watch_entries(0)[1].shape == (0, 1) and bank.pair_watch_entries(0)[0] == 0 and state(bank)[1][1] == kept[1][1]
    bank.add(np.stack([x[:S + 1] for x in xs]))              # a reset stream starts from +0 lane sums and entry 0
    assert bank.pair_watch_entries(0)[1].tobytes() == model_entries(xs[0][:S], S, DEFAULT).tobytes()
    assert int(bank.pair_watch()[0, 0]["open_frames"]) == 1 and int(bank.pair_watch()[1, 0]["entries"]) == 5
    bank.reset_pair_watch()
    assert bank.pair_watch().tobytes() == np.stack([empty_record()] * n).tobytes()
    # enabling again starts empty; off and on again as well
    bank.add(np.stack([x[:S + 1] for x in xs]))
    bank.enable_pair_watch(threshold=0.5)
    assert bank.pair_watch().tobytes() == np.stack([empty_record()] * n).tobytes()
    bank.disable_pair_watch()
    bank.disable_pair_watch()
    with pytest.raises(Exception):
        bank.pair_watch_plan()
    bank.add(np.stack([x[:100] for x in xs]))
    bank.enable_pair_watch([(1, 1), (0, 1)], window_s=0.2)
    assert bank.pair_watch_plan() == (256, 2, 2) and bank.pair_watch().tobytes() == np.stack([empty_record()] * 2 * n).tobytes()


def test_refusals_leave_the_previous_watch():
    rate, S, n = 48000, 4800, 2
    lib = L.lib()
    rng = np.random.default_rng(8)
    xs = [rng.uniform(-1, 1, (2 * S + 9, 2)).astype(np.float32) for _ in range(n)]
    bank = MeterBank(n, 2, rate)
    rec = np.zeros((n, 2), PAIR_WATCH_DTYPE)
    ent = np.zeros((5, 2), PAIR_ENTRY_DTYPE)
    p_rec, p_ent = rec.ctypes.data_as(ctypes.POINTER(L.PairWatch)), ent.ctypes.data_as(ctypes.POINTER(L.PairEntry))
    a, b, c = ctypes.c_uint32(7), ctypes.c_uint32(8), ctypes.c_uint32(9)
    first, count = ctypes.c_uint64(777), ctypes.c_uint32(778)
    # before enable
    assert lib.ss_meter_bank_pair_watch_plan(bank._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_pair_watch_reset(bank._h, None, 0) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_pair_watch(bank._h, p_rec, rec.size) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_pair_watch_entries(bank._h, 0, p_ent, 5, ctypes.byref(first), ctypes.byref(count)) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_pair_watch_enable(bank._h, None, 0, None) == L.SS_OK               # off while off
    bank.enable_pair_watch([(0, 1), (1, 1)], window_s=0.5, threshold=0.25, power_floor=1e-3, min_run=2)
    feed(bank, xs, [2 * S + 9])
    good = (state(bank), bank.pair_watch_plan())
    P, cfg, nan = L.ChannelPair, L.PairWatchConfig(0.0, 0.0, 1, 30), float("nan")
    for pairs, cnt in (((P(0, 2),), 1), ((P(2, 0),), 1), ((P(0, 1), P(0, NONE32)), 2), ((P(0, 1),) * 17, 17), (None, 1)):
        arr = (P * len(pairs))(*pairs) if pairs else None
        assert lib.ss_meter_bank_pair_watch_enable(bank._h, arr, cnt, ctypes.byref(cfg)) == L.SS_ERR_INVALID_ARG, (pairs, cnt)
        assert (state(bank), bank.pair_watch_plan()) == good
    for fields in ((nan, 0.0, 1, 30), (1.0, 0.0, 1, 30), (-1.0, 0.0, 1, 30), (1.5, 0.0, 1, 30), (0.0, nan, 1, 30), (0.0, -1e-9, 1, 30),
                   (0.0, 0.0, 0, 30), (0.0, 0.0, 1, 0), (0.0, 0.0, 1, 601)):
        bad = L.PairWatchConfig(*fields)
        assert lib.ss_meter_bank_pair_watch_enable(bank._h, None, 0, ctypes.byref(bad)) == L.SS_ERR_INVALID_ARG, fields
        assert (state(bank), bank.pair_watch_plan()) == good, fields
    mono = MeterBank(1, 1, rate)                             # the default pair on a mono bank
    assert lib.ss_meter_bank_pair_watch_enable(mono._h, None, 0, ctypes.byref(cfg)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_pair_watch_plan(mono._h, None, None, None) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_pair_watch_enable(mono._h, (P * 1)(P(0, 0)), 1, ctypes.byref(cfg)) == L.SS_OK
    # a bad stream index, with nothing reset; caps too small, with nothing written
    bad_list = np.array([1, n], np.uint32)
    assert lib.ss_meter_bank_pair_watch_reset(bank._h, bad_list.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 2) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_pair_watch_entries(bank._h, n, p_ent, 5, ctypes.byref(first), ctypes.byref(count)) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_pair_watch(bank._h, p_rec, rec.size - 1) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_pair_watch_entries(bank._h, 0, p_ent, 1, ctypes.byref(first), ctypes.byref(count)) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_pair_watch(bank._h, None, rec.size) == L.SS_ERR_INVALID_ARG
    assert (first.value, count.value) == (777, 778) and not rec.tobytes().strip(b"\0") and not ent.tobytes().strip(b"\0")
    assert (state(bank), bank.pair_watch_plan()) == good
    assert lib.ss_meter_bank_pair_watch_enable(bank._h, (P * 16)(*[P(i & 1, 1) for i in range(16)]), 16, ctypes.byref(L.PairWatchConfig(0.0, 0.0, 1, 600))) == L.SS_OK
    assert bank.pair_watch_plan() == (256, 600, 16) and bank.pair_watch().shape == (n, 16)      # sixteen pairs and 60 s are allowed
