"""Tracked meter-bank spectra on the MI355X (ss_meter_bank_spectrum_track*): per row an exponentially averaged and a peak-hold
curve, advanced on each stream's own clock.

The yardstick at every tick is what `MeterBank.spectrum()` — the existing, tested call — returns at that tick: its rows and
statuses feed `Model`, the header's rule written out in numpy, f64 where the header says f64.  What is compared:

  hold_db, updates   bit for bit.  hold_db is (float)((double)peak - decay * ((double)over / rate)), IEEE operations in a fixed
                     order without a fused multiply-add, so the host gets the same bits; which bins capture is decided by f32 / f64
                     comparisons of exact values, so the state (peak, age) is exact as well.
  avg_db             within 1e-4 dB at every bin: the bound tests/test_gpu_spectrum_stats.py derives for one exp2f power (f32
                     exponent argument 6e-6 dB, exp2f at 1-2 ulp 1e-6 dB, the f32 result 8e-6 dB: under 2e-5 dB, a factor of five
                     left for the device's exp2f).  It carries over: the average is a convex combination of such powers with
                     positive weights, so its relative error is at most the largest of theirs; alpha's few f64 ulps do not count.

Every test prints its worst avg_db deviation (pytest -rA)."""
import ctypes as C

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.meter_bank import MeterBank

from oracle.render import spectrum_columns_f32

pytestmark = pytest.mark.gpu

TOL_DB = 1e-4
K = np.float32(0.33219280948873623)                       # log2(10) / 10, the f32 constant k_spectrum_stats uses
U32_MAX = 0xFFFFFFFF


class Model:
    """The header's rule for every (stream, row), fed the rows and statuses spectrum() returns and each stream's own fed."""

    def __init__(self, n, rows, n_bins, rate, tau, hold_s, decay):
        self.rate, self.tau, self.decay = float(rate), float(tau), float(decay)
        self.hold_frames = None if np.isinf(hold_s) else int(hold_s * rate + 0.5)
        self.P = np.zeros((n, rows, n_bins), np.float64)
        self.peak = np.zeros((n, rows, n_bins), np.float32)
        self.age = np.zeros((n, rows, n_bins), np.uint64)            # (u32 values: saturated by hand)
        self.last = np.zeros((n, rows), np.uint64)
        self.updates = np.zeros((n, rows), np.uint32)
        self.captured = self.fell = 0                                 # bins that took a new peak / whose peak is falling

    def _hold_db(self, peak, age):
        over = np.zeros(age.shape, np.float64) if self.hold_frames is None else \
            np.maximum(age.astype(np.int64) - self.hold_frames, 0).astype(np.float64)
        return (peak.astype(np.float64) - self.decay * (over / self.rate)).astype(np.float32)

    def track(self, rows, status, fed):
        n, R, _ = rows.shape
        for s in range(n):
            for r in range(R):
                if status[s, r] != 0:
                    continue                                          # refused: not touched, last stays
                v = rows[s, r]
                p = np.exp2(v * K).astype(np.float64)                 # f32 product, f32 exp2, widened
                assert (v * K).dtype == np.float32
                if self.updates[s, r] == 0:
                    self.P[s, r], self.peak[s, r], self.age[s, r] = p, v, 0
                else:
                    delta = int(fed[s]) - int(self.last[s, r])
                    assert delta >= 0
                    if delta == 0:
                        continue
                    alpha = 1.0 if self.tau == 0.0 else -np.expm1(-float(delta) / (self.rate * self.tau))
                    self.P[s, r] = self.P[s, r] + alpha * (p - self.P[s, r])
                    age = np.minimum(self.age[s, r] + np.uint64(min(delta, U32_MAX)), np.uint64(U32_MAX))
                    d = self._hold_db(self.peak[s, r], age)
                    cap = v >= d
                    self.fell += int((~cap & (d < self.peak[s, r])).sum())
                    self.captured += int(cap.sum())
                    self.peak[s, r] = np.where(cap, v, self.peak[s, r])
                    self.age[s, r] = np.where(cap, np.uint64(0), age)
                self.last[s, r] = fed[s]
                self.updates[s, r] += 1

    def curves(self):
        """(avg_db f64 before the cast to f32, hold_db f32); rows without state NaN"""
        with np.errstate(divide="ignore"):
            avg = 10.0 * np.log10(self.P)
        hold = self._hold_db(self.peak, self.age)
        none = self.updates == 0
        avg[none] = np.nan
        hold[none] = np.nan
        return avg, hold


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_values(a, b):
    """bit-equal where both are numbers, NaN at the same places"""
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


WORST = {"avg": 0.0}


def check(bank, model, tag):
    """tracked() against the model: hold_db and updates exact, avg_db within TOL_DB; returns the device's three arrays"""
    avg, hold, upd = bank.tracked_spectrum()
    want_avg, want_hold = model.curves()
    assert np.array_equal(upd, model.updates), (tag, upd, model.updates)
    assert same_values(hold, want_hold), (tag, np.argwhere(~((hold == want_hold) | (np.isnan(hold) & np.isnan(want_hold))))[:5])
    assert np.array_equal(np.isnan(avg), np.isnan(want_avg)), tag
    ok = ~np.isnan(want_avg)
    dev = np.abs(avg[ok].astype(np.float64) - want_avg[ok]).max() if ok.any() else 0.0
    WORST["avg"] = max(WORST["avg"], dev)
    print(tag, "worst avg_db deviation", dev)
    assert dev <= TOL_DB, (tag, dev)
    return avg, hold, upd


def moving(seed, frames, channels, rate, start=0):
    """[frames, channels] f32 whose spectrum moves: a sweep of about four octaves per second (phase continuous over `start`),
    a steady low tone, and a noise burst in every third stretch of 1500 frames"""
    rng = np.random.default_rng(seed * 1000003 + start)
    t = (start + np.arange(frames)) / rate
    f0 = 200.0 * (1 + seed % 5)
    phase = 2 * np.pi * f0 * (np.exp2(4.0 * (t % 1.0)) - 1.0) / (4.0 * np.log(2.0))
    x = 0.3 * np.sin(phase) + 0.1 * np.sin(2 * np.pi * 110.0 * t)
    burst = (((start + np.arange(frames)) // 1500) % 3 == (seed % 3)).astype(np.float64)
    out = np.empty((frames, channels), np.float32)
    for c in range(channels):
        out[:, c] = (x * (1.0 - 0.2 * c) + burst * 0.2 * rng.standard_normal(frames)).astype(np.float32)
    return out


def new_bank(n, channels, rate, tau, hold_s, decay):
    bank = MeterBank(n, channels, rate)
    bank.enable_spectrum()
    bank.enable_spectrum_tracking(tau, hold_s, decay)
    r, nb, _ = bank.spectrum_layout()
    return bank, Model(n, r, nb, rate, tau, hold_s, decay)


def run_uniform(bank, model, ticks, tag, every=None):
    """uniform adds of ticks[i] frames, an update and a comparison behind each; every(i, rows, status): extra checks"""
    n, fed = bank.n_streams, 0
    for i, f in enumerate(ticks):
        bank.add(np.stack([moving(s, f, bank.channels, bank.rate, fed) for s in range(n)]))
        fed += f
        bank.track_spectrum()
        rows, st = bank.spectrum()
        model.track(rows, st, [fed] * n)
        out = check(bank, model, (tag, i, f))
        if every:
            every(i, rows, st, out)


# ---- 1. model parity ---------------------------------------------------------------------------------------------------------------
TICKS = [375 * k for k in (1, 2, 1, 4, 3, 8, 1, 5, 2, 16, 1, 44)]     # the last one replaces the whole window


def test_model_parity_exact_falls():
    """48 kHz, hold of 1500 frames, 16 dB/s: every fall is a multiple of 1/8 dB."""
    rate = 48000
    bank, model = new_bank(3, 2, rate, 0.125, 375 * 4 / 48000, 16.0)
    assert model.hold_frames == 1500
    run_uniform(bank, model, TICKS, "parity48")
    assert model.captured > 1000 and model.fell > 1000                # both branches of the peak hold were taken
    over = np.maximum(model.age.astype(np.int64) - model.hold_frames, 0).astype(np.float64)
    falls = model.decay * (over / model.rate) * 8.0                   # (in f64, ahead of the subtraction and the cast to f32)
    assert falls.max() >= 8.0 and np.array_equal(falls, np.round(falls))


def test_model_parity_odd_bins_awkward_parameters():
    """44.1 kHz: 7423 bins, rows not 16-byte aligned; parameters whose products round."""
    rate = 44100
    bank, model = new_bank(3, 2, rate, 0.3, 0.05, 7.3)
    assert bank.spectrum_layout()[1] % 4 != 0 and model.hold_frames == 2205
    run_uniform(bank, model, [441, 1000, 1, 4410, 3333, 2205, 2206, 7, 16384, 999], "parity44")
    assert model.captured > 1000 and model.fell > 1000


# ---- 2. identities -----------------------------------------------------------------------------------------------------------------
def test_identity_tau_zero_and_no_hold():
    """tau == 0: the average is the newest row; hold_s == 0 with an immense fall rate: the peak hold is the newest accepted row."""
    bank, model = new_bank(2, 2, 48000, 0.0, 0.0, 1e9)

    def newest(i, rows, st, out):
        avg, hold, _ = out
        assert (st == 0).all()
        assert np.abs(avg.astype(np.float64) - rows.astype(np.float64)).max() <= TOL_DB
        assert same_bits(hold, rows)
    run_uniform(bank, model, [480, 4800, 375, 20000], "identity0", newest)


def test_identity_hold_for_ever():
    """hold_s == +inf: the running maximum of the accepted rows."""
    bank, model = new_bank(2, 2, 48000, 0.125, np.inf, 16.0)
    best = []

    def running(i, rows, st, out):
        assert (st == 0).all()
        best[:] = [rows.copy() if not best else np.fmax(best[0], rows)]
        assert same_bits(out[1], best[0])
    run_uniform(bank, model, [480, 4800, 375, 20000, 960], "identityinf", running)
    assert model.fell == 0


# ---- 3. own clocks -----------------------------------------------------------------------------------------------------------------
def test_ragged_streams_run_on_their_own_clocks():
    rate, n = 48000, 4
    bank, model = new_bank(n, 2, rate, 0.125, 375 * 4 / 48000, 16.0)
    sched = [[375, 750, 375, 1125], [1500, 1, 375, 0], [100, 3000, 0, 375], [375, 0, 0, 20000], [7, 375, 0, 750],
             [375, 375, 1875, 375], [0, 0, 0, 0], [750, 375, 375, 1],          # stream 2 starves on ticks 2, 3, 4; nobody moves on 6
             [3000, 4500, 2250, 1500], [2250, 0, 3000, 6000]]                  # steps beyond the hold: peaks fall at different ages
    fed = [0] * n
    for i, frames in enumerate(sched):
        before = bank.tracked_spectrum()
        bank.add_ragged([moving(s, f, 2, rate, fed[s]) if f else None for s, f in enumerate(frames)])
        fed = [a + b for a, b in zip(fed, frames)]
        bank.track_spectrum()
        rows, st = bank.spectrum()
        model.track(rows, st, fed)
        out = check(bank, model, ("ragged", i))
        for s, f in enumerate(frames):
            if f == 0:                                                # given nothing: the three outputs stay byte for byte
                assert all(same_bits(a[s], b[s]) for a, b in zip(out, before)), (i, s)
    assert list(model.updates[:, 0]) == [sum(1 for frames in sched if frames[s]) for s in range(n)] == [9, 7, 6, 8]
    assert model.captured > 1000 and model.fell > 1000


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refused_rows_freeze_and_decay_over_the_gap():
    """Three channels: a NaN in channel 1 of stream 0 refuses that row while it is inside the window; the row is frozen, rows 0 and
    2 go on, and the first update after the NaN has left decays over the whole gap."""
    rate, n, blk = 48000, 2, 4500
    bank, model = new_bank(n, 3, rate, 0.125, 375 * 4 / 48000, 16.0)
    twin, twin_model = new_bank(n, 3, rate, 0.125, 375 * 4 / 48000, 16.0)      # the same feed without the NaN
    fed, seen, frozen = 0, [], None
    for i in range(8):
        data = np.stack([moving(s, blk, 3, rate, fed) for s in range(n)])
        clean = data.copy()
        if i == 2:
            data[0, 100, 1] = np.nan
        bank.add(data)
        twin.add(clean)
        fed += blk
        bank.track_spectrum()
        twin.track_spectrum()
        rows, st = bank.spectrum()
        trows, tst = twin.spectrum()
        if i == 5:                                                    # the NaN has left: row (0, 1) decays over the whole gap
            assert st[0, 1] == 0 and fed - int(model.last[0, 1]) == 4 * blk
        model.track(rows, st, [fed] * n)
        twin_model.track(trows, tst, [fed] * n)
        out = check(bank, model, ("refusal", i))
        tout = check(twin, twin_model, ("refusal twin", i))
        seen.append(int(st[0, 1]))
        assert st[0, 0] == st[0, 2] == 0 and (st[1] == 0).all()
        for r in (0, 2):                                              # the rows beside the refused one: as if nothing had happened
            assert all(same_bits(a[0, r], b[0, r]) for a, b in zip(out, tout)), (i, r)
        assert all(same_bits(a[1], b[1]) for a, b in zip(out, tout)), i
        if st[0, 1]:
            state = [a[0, 1].tobytes() for a in out]
            assert frozen is None or state == frozen, i
            frozen = state
    # NaN at frame 9100: inside the window for the ticks that end at 13500 .. 22500 (9100 + 16384 = 25484 > 22500)
    assert seen == [0, 0, L.SS_ERR_NAN, L.SS_ERR_NAN, L.SS_ERR_NAN, 0, 0, 0]
    assert list(model.updates[0]) == [8, 5, 8]


def test_infinity_in_left_refuses_mid_and_side():
    rate, blk = 48000, 4500
    bank, model = new_bank(2, 2, rate, 0.125, 375 * 4 / 48000, 16.0)
    fed, frozen = 0, None
    for i in range(3):
        data = np.stack([moving(s, blk, 2, rate, fed) for s in range(2)])
        if i == 1:
            data[1, 7, 0] = np.inf
        bank.add(data)
        fed += blk
        bank.track_spectrum()
        rows, st = bank.spectrum()
        model.track(rows, st, [fed] * 2)
        out = check(bank, model, ("inf", i))
        if i >= 1:
            assert list(st[1]) == [L.SS_ERR_INFINITY, L.SS_ERR_INFINITY] and (st[0] == 0).all()
            state = [a[1].tobytes() for a in out]
            assert frozen is None or state == frozen
            frozen = state
    assert list(model.updates[:, 0]) == [3, 1]


# ---- 5. columns --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def columns_bank():
    """three stereo streams after four ticks, stream 2 emptied: (bank, avg, hold, updates, pink, chart_x, integrated)"""
    rate, n = 48000, 3
    bank, model = new_bank(n, 2, rate, 0.125, 375 * 4 / 48000, 16.0)
    run_uniform(bank, model, [24000, 375, 3000, 750], "columns")
    bank.reset_spectrum_tracking([2])
    avg, hold, upd = bank.tracked_spectrum()
    assert list(upd[:, 0]) == [4, 4, 0]
    integ = bank.read()["integrated"]
    assert np.isfinite(integ).all()
    return bank, avg, hold, upd, bank.spectrum_pink(), bank.spectrum_layout()[2], integ


@pytest.mark.parametrize("cols", [1, 160, 512])
def test_columns(columns_bank, cols):
    bank, avg, hold, upd, pink, chart_x, integ = columns_bank
    for gain in (17.5, "reference"):
        cavg, chold, cupd = bank.tracked_spectrum_columns(cols, gain)
        assert np.array_equal(cupd, upd)
        assert np.isnan(cavg[2]).all() and np.isnan(chold[2]).all()   # updates == 0
        for s in range(2):
            g = np.float32(-13.0) - np.float32(integ[s]) if gain == "reference" else np.float32(gain)
            for r in range(2):
                for got, curve in ((cavg, avg), (chold, hold)):
                    x = (curve[s, r].astype(np.float64) + pink).astype(np.float32)
                    want = spectrum_columns_f32(x, chart_x, g, cols)
                    assert same_values(got[s, r], want), (cols, gain, s, r)
                    assert np.array_equal(np.isnan(got[s, r]), np.isnan(want))
        if cols == 512:
            assert np.isnan(cavg[0, 0]).any() and not np.isnan(cavg[0, 0]).all()      # columns without a bin exist


# ---- 6. lifecycle ------------------------------------------------------------------------------------------------------------------
def _raw_calls():
    lib = L.lib()
    f = np.empty(8, np.float32)
    u = np.empty(8, np.uint32)
    fp, up = f.ctypes.data_as(C.POINTER(C.c_float)), u.ctypes.data_as(C.POINTER(C.c_uint32))
    return lib, fp, up


def test_status_codes():
    rate, n = 48000, 3
    bank = MeterBank(n, 2, rate)
    lib, fp, up = _raw_calls()
    good = L.SpectrumBallistics(0.125, 0.5, 16.0)
    # no history yet
    assert lib.ss_meter_bank_spectrum_track_enable(bank._h, C.byref(good)) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_spectrum_track_enable(bank._h, None) == L.SS_OK
    bank.enable_spectrum()
    # before enabling
    assert lib.ss_meter_bank_spectrum_track(bank._h) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_spectrum_track_reset(bank._h, None, 0) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_spectrum_tracked(bank._h, fp, fp, 8, up, 8) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 2, 0, 0.0, fp, fp, 8, up, 8) == L.SS_ERR_INVALID_MODE
    # bad parameters
    inf, nan = float("inf"), float("nan")
    for bad in ((-1.0, 0.5, 16.0), (nan, 0.5, 16.0), (inf, 0.5, 16.0), (0.1, -0.5, 16.0), (0.1, nan, 16.0), (0.1, 0.5, -1.0),
                (0.1, 0.5, nan), (0.1, 0.5, inf)):
        assert lib.ss_meter_bank_spectrum_track_enable(bank._h, C.byref(L.SpectrumBallistics(*bad))) == L.SS_ERR_INVALID_ARG, bad
    assert lib.ss_meter_bank_spectrum_track(bank._h) == L.SS_ERR_INVALID_MODE       # (none of them enabled anything)
    assert lib.ss_meter_bank_spectrum_track_enable(bank._h, C.byref(L.SpectrumBallistics(0.0, inf, 0.0))) == L.SS_OK
    assert lib.ss_meter_bank_spectrum_track_enable(bank._h, C.byref(good)) == L.SS_OK
    r, nb, _ = bank.spectrum_layout()
    rows = n * r
    big = np.empty(rows * nb, np.float32)
    bp = big.ctypes.data_as(C.POINTER(C.c_float))
    # capacities
    assert lib.ss_meter_bank_spectrum_tracked(bank._h, bp, bp, rows * nb - 1, up, rows) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_spectrum_tracked(bank._h, bp, None, rows * nb, up, rows - 1) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_spectrum_tracked(bank._h, None, bp, rows * nb, up, rows) == L.SS_OK
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 2, 0, 0.0, bp, bp, rows * 2 - 1, up, rows) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 2, 0, 0.0, bp, bp, rows * 2, up, rows - 1) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 2, 0, 0.0, bp, bp, rows * 2, up, rows) == L.SS_OK
    # bad arguments
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 0, 0, 0.0, bp, bp, rows * nb, up, rows) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 513, 0, 0.0, bp, bp, rows * nb, up, rows) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_tracked_columns(bank._h, 2, 5, 0.0, bp, bp, rows * nb, up, rows) == L.SS_ERR_INVALID_ARG
    idx = np.array([0, n], np.uint32)
    assert lib.ss_meter_bank_spectrum_track_reset(bank._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), 2) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_track_reset(bank._h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), 1) == L.SS_OK
    # turning the spectrum off, or on again, turns tracking off
    bank.enable_spectrum()
    assert lib.ss_meter_bank_spectrum_track(bank._h) == L.SS_ERR_INVALID_MODE
    bank.enable_spectrum_tracking(0.125, 0.5, 16.0)
    bank.enable_spectrum(False)
    assert lib.ss_meter_bank_spectrum_track(bank._h) == L.SS_ERR_INVALID_MODE
    with pytest.raises(ssa.AnalyzerError) as e:
        bank.tracked_spectrum()
    assert e.value.code == L.SS_ERR_INVALID_MODE


def test_resets_and_a_twin_without_tracking():
    """track_reset empties the listed streams only; the meters' reset leaves the curves byte for byte; enabling again starts from
    empty state; and a bank that tracks returns the same spectrum(), spectrum_columns() and read() bytes as one that does not."""
    rate, n = 48000, 3
    bank, model = new_bank(n, 2, rate, 0.125, 375 * 4 / 48000, 16.0)
    twin = MeterBank(n, 2, rate)
    twin.enable_spectrum()
    fed = 0
    for i, f in enumerate([4800, 375, 20000, 750]):
        data = np.stack([moving(s, f, 2, rate, fed) for s in range(n)])
        bank.add(data)
        twin.add(data)
        fed += f
        bank.track_spectrum()
        rows, st = bank.spectrum()
        trows, tst = twin.spectrum()
        assert same_bits(rows, trows) and same_bits(st, tst)
        a, b = bank.spectrum_columns(160, "reference"), twin.spectrum_columns(160, "reference")
        assert same_values(a[0], b[0]) and same_bits(a[1], b[1])
        if i == 1:
            bank.tracked_spectrum_columns(160, "reference")            # a read-out in between changes nothing either
        assert bank.read().tobytes() == twin.read().tobytes()
        model.track(rows, st, [fed] * n)
        check(bank, model, ("twin", i))
    before = bank.tracked_spectrum()
    bank.reset([1])
    bank.reset()
    after = bank.tracked_spectrum()
    assert all(same_bits(a, b) for a, b in zip(before, after))
    bank.reset_spectrum_tracking([1])
    avg, hold, upd = bank.tracked_spectrum()
    assert list(upd[:, 0]) == [4, 0, 4] and np.isnan(avg[1]).all() and np.isnan(hold[1]).all()
    for s in (0, 2):
        assert same_bits(avg[s], before[0][s]) and same_bits(hold[s], before[1][s])
    # stream 1 is seeded again by the next update although nothing arrived; the others, given nothing, stay
    model.updates[1] = 0
    bank.track_spectrum()
    rows, st = bank.spectrum()
    model.track(rows, st, [fed] * n)
    avg, hold, upd = check(bank, model, "reseed")
    assert list(upd[:, 0]) == [4, 1, 4] and same_bits(hold[1], rows[1])
    assert same_bits(avg[0], before[0][0]) and same_bits(hold[2], before[1][2])
    bank.reset_spectrum_tracking()
    assert (bank.tracked_spectrum()[2] == 0).all()
    bank.track_spectrum()
    bank.enable_spectrum_tracking(0.5, 0.0, 1.0)                       # enabling again: empty state
    avg, hold, upd = bank.tracked_spectrum()
    assert (upd == 0).all() and np.isnan(avg).all() and np.isnan(hold).all()
    bank.disable_spectrum_tracking()
    with pytest.raises(ssa.AnalyzerError) as e:
        bank.track_spectrum()
    assert e.value.code == L.SS_ERR_INVALID_MODE
    rows, st = bank.spectrum()                                         # the spectrum itself goes on
    assert same_bits(rows, twin.spectrum()[0])


# ---- 7. indexing beyond a few rows -------------------------------------------------------------------------------------------------
def test_sixty_four_mono_streams():
    bank, model = new_bank(64, 1, 48000, 0.125, 375 * 4 / 48000, 16.0)
    run_uniform(bank, model, [3000, 375, 3750], "mono64")
    assert (model.updates == 3).all()
    avg, hold, _ = bank.tracked_spectrum()
    assert len({hold[s].tobytes() for s in range(64)}) >= 5            # (the material has five different sweeps)
