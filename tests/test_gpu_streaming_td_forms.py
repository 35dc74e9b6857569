"""Every STREAMING form of the time-domain kernel (RING = true: the handle's add_samples, the meter banks' adds, the session ticks)
against the f64 prefix reference of tests/_td_plants.py, at planted call and tile edges.

Each case names the plan tuples it must reach — (form, waves, tile_frames, chunk_frames, true_peak_factor) of its one-wave calls
and of its shared calls, from ss_td_streaming_plan, which asks the functions the launch asks — and asserts them before anything
else: a change of td_chunk_frames, td_split_chunk_frames or the form switch fails there instead of quietly testing another form.
The schedules take every boundary from that plan (tests/_td_plants.py: call boundaries of either form, calls of 1 ... 25 frames,
tile boundaries of the absolute grid inside a one-wave and inside a shared call, sub-block boundaries, a ninth tile, a first tile
of one frame, a call that ends one frame behind a tile boundary, a piece boundary inside a call of more than 32 sub-blocks, a
reset), and tests/test_td_streaming_plants.py shows on the CPU that a lost, zeroed or late history frame, a zeroed filter state
or a swapped channel at any of these classes reads at least 100 bars away.

Checks behind EVERY call: each channel's true peak within 1e-6 (relative) of the f64 prefix value — the batch forms' bar, the
per-tile arithmetic is the same —, its sample peak bit for bit, the momentary and short-term readings within 1e-6 LU on burst
streams (test_gpu_independent.py's bar) and within 4.343 x TORTURE_BOUND[(False, rate)] LU on the hand-over torture material (the
batch file's relative-energy bound in LU).  Measured worst values stand beside the cases.

What a single handle stream of about 40 sub-blocks cannot hold: the whole sweep of d at the classes that cost a long call each (a
ninth tile: two to six anchors; a piece boundary: one) — there the most telling offsets come first (_td_plants.d_order), and the
uniform bank, one offset per stream, sweeps every d at every class.  In the file and capture ticks every tick's new burst, 10 % over
the last, stands in the 1024 frames its slice has that the one before had not, so it moves the running maximum: on two ticks of
three around a tile boundary of the fed stream's absolute grid inside the slice (the tick launch's seventh or eighth tile, a
hand-over between two of its waves), otherwise around the slice's end (a call boundary).  What stands there stands again, whole,
further in the next slice, so a history lost at a slice's end shows only where the cut burst reads higher than the whole one; and a
slice's first tiles hold only bursts that earlier ticks brought, at or under the running maximum: a history lost there moves the
readings alone, which the handle and bank cases cover for the same shared form.

The four-wave fallback (eight LDS slices do not fit): the plan reports it at 56 and 63 channels (48 kHz: tiles of 50 frames, four
waves), and nowhere under 56 channels at 8 ... 384 kHz; the 56-channel handle case runs it."""
import collections
import functools

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
import _f64ref as R
import _td_plants as P
from test_gpu_time_domain_forms import TORTURE_BOUND

pytestmark = pytest.mark.gpu

TP_REL = 1e-6
READING_LU = 1e-6
ARITH = {"f32": L.SS_TP_ARITH_F32, "f16x3": L.SS_TP_ARITH_F16X3, None: None}


def reading_bar(rate, torture):
    return 4.343 * TORTURE_BOUND[(False, rate)] if torture else READING_LU


class Worst:
    """the measured worst values of one test, printed at its end (pytest -s / -rP shows them)"""

    def __init__(self, name):
        self.name, self.tp, self.lu, self.calls = name, 0.0, 0.0, 0

    def peaks(self, tag, tp, sp, ref, k):
        want_tp, want_sp = ref.true_peak(k), ref.sample_peak(k)
        assert np.array_equal(sp, want_sp), (self.name, tag, sp, want_sp)
        rel = np.abs(tp - want_tp) / want_tp
        self.tp = max(self.tp, float(rel.max()))
        assert rel.max() <= TP_REL, (self.name, tag, tp, want_tp)

    def readings(self, tag, momentary, shortterm, ref, k, bar, st_only=False):
        for got, want in ((shortterm, ref.shortterm(k)),) if st_only else ((momentary, ref.momentary(k)), (shortterm, ref.shortterm(k))):
            if np.isfinite(want):
                self.lu = max(self.lu, abs(got - want))
                assert abs(got - want) <= bar, (self.name, tag, got, want)
            else:
                assert got == want, (self.name, tag, got, want)

    def report(self):
        print("\n[measured] %s: true peak %.1e, readings %.1e LU, %d calls" % (self.name, self.tp, self.lu, self.calls))


# ---------------------------------------------------------------- 1. the handle
HCase = collections.namedtuple("HCase", "name one shared")
# name (tests/_td_plants.py HANDLE_SHAPES), the plan of a one-wave call, the plan of a shared call
HANDLE = [
    #   measured: true peak 1.1e-07, readings 1.6e-12 LU (187 calls)
    HCase("48k-2-f32", (0, 1, 960, 30, 4), (1, 8, 1200, 40, 4)),
    #   measured: true peak 2.2e-07, readings 1.6e-12 LU (187 calls)
    HCase("48k-2-f16x3", (0, 1, 960, 30, 4), (1, 8, 1200, 40, 4)),
    #   measured: true peak 1.3e-07, readings 8.6e-10 LU (187 calls)
    HCase("48k-2-torture", (0, 1, 960, 30, 4), (1, 8, 1200, 40, 4)),
    #   measured: true peak 8.9e-08, readings 7.7e-13 LU (162 calls)
    HCase("44k-2", (0, 1, 1470, 49, 4), (1, 8, 1470, 49, 4)),          # S = 4410: three tiles of 1470, the batch's chunk length
    #   measured: true peak 1.8e-07, readings 2.3e-11 LU (251 calls)
    HCase("96k-2", (0, 1, 960, 30, 2), (1, 8, 1200, 40, 2)),
    #   measured: true peak 0.0e+00, readings 9.5e-11 LU (161 calls)
    HCase("192k-2", (0, 1, 960, 30, 0), (1, 8, 1280, 40, 0)),
    #   measured: true peak 1.3e-07, readings 2.8e-12 LU (148 calls)
    HCase("48k-1", (0, 1, 1600, 25, 4), (1, 8, 2400, 40, 4)),
    #   measured: true peak 1.5e-07, readings 1.8e-12 LU (169 calls)
    HCase("48k-3", (0, 1, 600, 30, 4), (1, 8, 800, 40, 4)),
    #   measured: true peak 1.1e-07, readings 1.5e-12 LU (137 calls)
    HCase("48k-5", (0, 1, 600, 50, 4), (1, 8, 480, 40, 4)),
    #   measured: true peak 1.4e-07, readings 2.0e-12 LU (129 calls)
    HCase("48k-6", (0, 1, 300, 30, 4), (1, 8, 400, 40, 4)),
    #   measured: true peak 2.0e-07, readings 1.0e-12 LU (121 calls)
    HCase("48k-8", (0, 1, 240, 30, 4), (1, 8, 320, 40, 4)),
    #   measured: true peak 2.1e-07, readings 1.0e-12 LU (121 calls)
    HCase("48k-16", (0, 1, 160, 40, 4), (1, 8, 160, 40, 4)),
    #   measured: true peak 2.2e-07, readings 1.1e-12 LU (121 calls)
    # (a one-wave tile of 50 frames is shorter than the sweep of d with its ringing, 55 frames: no anchor fits INSIDE a one-wave call,
    #  the tile-one-wave class is not required of this case; its one-wave tile boundaries are all call boundaries, which are anchored)
    HCase("48k-56-four-waves", (0, 1, 50, 50, 4), (1, 4, 50, 50, 4)),
]
assert [c.name for c in HANDLE] == [s[0] for s in P.HANDLE_SHAPES]


def assert_plan(name, channels, rate, one, shared):
    got = tuple(tuple(p) for p in P.forms(channels, rate))
    assert got == (one, shared), (name, got, (one, shared))


@pytest.mark.parametrize("case", HANDLE, ids=[c.name for c in HANDLE])
def test_handle_form_against_f64(case):
    _, rate, ch, arith, torture = P.HANDLE_SHAPES[[c.name for c in HANDLE].index(case.name)]
    assert_plan(case.name, ch, rate, case.one, case.shared)
    segs = P.handle_stream(ch, rate, torture)
    reached = {a.cls for seg, _, _ in segs for a in seg.anchors}
    assert reached >= set(P.CLASSES) - ({P.TILE_ONE} if case.one[2] < 100 else set()), reached
    forms = collections.Counter(P.plan(ch, rate, n).form for seg, _, _ in segs for n in seg.sizes)
    assert forms[P.ONE_WAVE] > 50 and forms[P.SHARED] > 10, forms
    bar = reading_bar(rate, torture is not None)
    w = Worst(case.name)
    a = ssa.Analyzer(ch, rate)
    try:
        if ARITH[arith] is not None:
            a.set_true_peak_arith(ARITH[arith])
        for si, (seg, x, ref) in enumerate(segs):
            if si:
                a.reset()
            fed = 0
            for k, n in enumerate(seg.sizes):
                a.add_samples(x[fed:fed + n].reshape(-1))
                fed += n
                tp = np.array([a.get_true_peak_channel(c) for c in range(ch)])
                sp = np.array([a.get_sample_peak_channel(c) for c in range(ch)])
                w.peaks((si, k, n, fed), tp, sp, ref, k)
                w.readings((si, k, n, fed), a.get_momentary_lufs(), a.get_shortterm_lufs(), ref, k, bar)
                w.calls += 1
                if si and k == 0 and torture is None:       # behind the reset the first call is noise alone: the DEVICE reads the noise's
                    bound = P.NOISE * (R.tap_bound(ref.factor) if ref.factor else 1.0) * (1 + TP_REL)      # own true peak, nothing older
                    assert 0.0 < tp.max() <= bound and sp.max() <= P.NOISE, (case.name, tp, sp, bound)
    finally:
        a.close()
        w.report()


# ---------------------------------------------------------------- 2. banks
@functools.lru_cache(maxsize=None)
def bank_streams(channels, rate, n, n_torture=0):
    """[stream] -> ((segment, x, SegRef), ...): the light schedule; stream s takes offset d_order[s + 7 c + anchor] around every
    anchor, so a pass of uniform calls sweeps every d over the streams; the first n_torture streams carry the torture material"""
    segs = P.handle_segments(channels, rate, light=True)
    factor = P.forms(channels, rate)[0].factor
    out = []
    for s in range(n):
        one = []
        for i, seg in enumerate(segs):
            if s < n_torture:
                x = P.torture_segment(seg, rate, channels, P.STEP_K[(3 * s + 1) % len(P.STEP_K)], 50 + s)
            else:
                x = P.plant(seg, channels, factor, 7000 + 10 * s + i, turn=lambda a, c, s=s: s + 7 * c + a)[0]
            one.append((seg, x, P.SegRef(x, rate, factor, seg.sizes)))
        out.append(tuple(one))
    return out


def check_bank(w, bank, refs, k, tag, torture_streams, rate, fed):
    rd = bank.read()
    for s, ref in enumerate(refs):
        assert int(rd["frames"][s]) == fed[s], (tag, s)
        if fed[s] == 0:
            continue
        tp, sp = bank.peaks(s)
        w.peaks((tag, s), tp, sp, ref, k[s])
        w.readings((tag, s), float(rd["momentary"][s]), float(rd["shortterm"][s]), ref, k[s], reading_bar(rate, s < torture_streams))
    w.calls += 1


# measured: true peak 2.3e-07, readings 8.0e-10 LU (69 calls)
def test_bank_uniform_sweeps_every_offset():
    """48 kHz stereo, 32 streams, uniform calls: 29 burst streams (every d at every anchor) and 3 torture streams; the same calls
    through add_device, from a buffer whose stream stride is the whole material, agree byte for byte"""
    rate, ch, n, nt = 48000, 2, 32, 3
    assert_plan("bank-uniform", ch, rate, (0, 1, 960, 30, 4), (1, 8, 1200, 40, 4))
    assert n - nt >= len(P.d_order(4))
    streams = bank_streams(ch, rate, n, nt)
    w = Worst("bank 48k x 2 x 32")
    bank, dev = ssa.MeterBank(n, ch, rate), ssa.MeterBank(n, ch, rate)
    total = sum(sum(seg.sizes) for seg, _, _ in streams[0])
    xs = np.stack([np.concatenate([x for _, x, _ in st]) for st in streams])          # [n][total][ch]
    src = ssa.Batch(rate, ch, n, total, flags=L.SS_BATCH_LUFS)
    try:
        src.upload(0, xs.reshape(-1))
        base, pos = src.input_device_ptr(), 0
        for si in range(len(streams[0])):
            seg = streams[0][si][0]
            if si:
                bank.reset(); dev.reset()
            fed = 0
            for k, f in enumerate(seg.sizes):
                bank.add(np.stack([st[si][1][fed:fed + f] for st in streams]))
                dev.add_device(base + 4 * pos * ch, f, total * ch)
                fed += f; pos += f
                check_bank(w, bank, [st[si][2] for st in streams], [k] * n, (si, k, f), nt, rate, [fed] * n)
                assert dev.read().tobytes() == bank.read().tobytes(), (si, k)
            for s in range(n):
                assert all(np.array_equal(u, v) for u, v in zip(dev.peaks(s), bank.peaks(s))), s
    finally:
        src.close()
        w.report()


# measured: true peak 3.3e-07, readings 1.4e-11 LU (69 calls)
def test_bank_96k_six_channels():
    rate, ch, n = 96000, 6, 4
    assert_plan("bank-96k-6", ch, rate, (0, 1, 300, 30, 2), (1, 8, 400, 40, 2))
    streams = bank_streams(ch, rate, n)
    w = Worst("bank 96k x 6 x 4")
    bank = ssa.MeterBank(n, ch, rate)
    for si in range(len(streams[0])):
        seg = streams[0][si][0]
        if si:
            bank.reset()
        fed = 0
        for k, f in enumerate(seg.sizes):
            bank.add(np.stack([st[si][1][fed:fed + f] for st in streams]))
            fed += f
            check_bank(w, bank, [st[si][2] for st in streams], [k] * n, (si, k, f), 0, rate, [fed] * n)
    w.report()


# measured: 3 channels true peak 1.0e-07, readings 2.7e-12 LU; 5 channels true peak 1.3e-07, readings 2.3e-12 LU (40 calls each)
@pytest.mark.parametrize("ch,one,shared", [(3, (0, 1, 600, 30, 4), (1, 8, 800, 40, 4)), (5, (0, 1, 600, 50, 4), (1, 8, 480, 40, 4))],
                         ids=["3ch", "5ch"])
def test_bank_ragged(ch, one, shared):
    """add_ragged: every stream its own frames per call — none, fewer than the history, either side of the form switch in ONE piece
    (both forms launched for it), several tiles; odd channel counts, so packed starts are 16-byte aligned only by padding"""
    rate, n = 48000, 8
    assert_plan("bank-ragged", ch, rate, one, shared)
    segs = [P.ragged_segment(ch, rate, s) for s in range(n)]
    factor = one[4]
    mats = [P.plant(seg, ch, factor, 8000 + s) for s, seg in enumerate(segs)]
    refs = [P.SegRef(x, rate, factor, seg.sizes) for seg, (x, _) in zip(segs, mats)]
    T1 = one[2]
    both = zero = 0
    w = Worst("ragged bank 48k x %d x 8" % ch)
    bank = ssa.MeterBank(n, ch, rate)
    fed = [0] * n
    for k in range(len(segs[0].sizes)):
        sizes = [seg.sizes[k] for seg in segs]
        both += any(0 < f <= T1 for f in sizes) and any(f > T1 for f in sizes)
        zero += 0 in sizes
        bank.add_ragged([mats[s][0][fed[s]:fed[s] + sizes[s]] if sizes[s] else None for s in range(n)])
        fed = [a + b for a, b in zip(fed, sizes)]
        check_bank(w, bank, refs, [k] * n, (k, tuple(sizes)), 0, rate, fed)
    assert both > 10 and zero > 10, (both, zero)
    w.report()


# measured: true peak 7.0e-08, readings 1.3e-12 LU (51 calls)
def test_bank_selective_reset():
    """a reset of two streams in the middle of the schedule: they read fresh values (the f64 reference of what followed), their
    neighbours stay bit-identical to a bank that was never reset"""
    rate, ch, n = 48000, 2, 6
    assert_plan("bank-reset", ch, rate, (0, 1, 960, 30, 4), (1, 8, 1200, 40, 4))
    streams = bank_streams(ch, rate, 32, 3)[3:3 + n]
    seg = streams[0][0][0]
    cut = len(seg.sizes) // 2
    at = int(sum(seg.sizes[:cut]))
    hit = [1, 4]
    fresh = {s: P.SegRef(streams[s][0][1][at:], rate, 4, seg.sizes[cut:]) for s in hit}
    w = Worst("bank selective reset")
    a, b = ssa.MeterBank(n, ch, rate), ssa.MeterBank(n, ch, rate)
    fed = 0
    for k, f in enumerate(seg.sizes):
        if k == cut:
            a.reset(hit)
        blk = np.stack([st[0][1][fed:fed + f] for st in streams])
        a.add(blk); b.add(blk)
        fed += f
        ra, rb = a.read(), b.read()
        for s in range(n):
            if s in hit and k >= cut:
                tp, sp = a.peaks(s)
                assert int(ra["frames"][s]) == fed - at
                w.peaks(("reset", k, s), tp, sp, fresh[s], k - cut)
                w.readings(("reset", k, s), float(ra["momentary"][s]), float(ra["shortterm"][s]), fresh[s], k - cut, READING_LU)
            else:
                assert ra[s].tobytes() == rb[s].tobytes(), (k, s)
                assert all(np.array_equal(u, v) for u, v in zip(a.peaks(s), b.peaks(s))), (k, s)
        w.calls += 1
    w.report()


# ---------------------------------------------------------------- 3. sessions
HOP, SLICE, tick_file = P.HOP, P.SLICE, P.tick_file


# measured (60 ticks each): 48 kHz true peak 9.5e-08, short-term 1.6e-12 LU; 44.1 kHz true peak 1.4e-07, short-term 4.4e-13 LU; 96 kHz true peak 1.3e-07, short-term 8.5e-12 LU; 192 kHz true peak 0.0e+00, short-term 1.4e-10 LU
@pytest.mark.parametrize("rate,shared", [(48000, (1, 8, 1200, 40, 4)), (44100, (1, 8, 1470, 49, 4)), (96000, (1, 8, 1200, 40, 2)),
                                         (192000, (1, 8, 1280, 40, 0))], ids=["48k", "44k", "96k", "192k"])
def test_session_file_ticks(rate, shared):
    """file ticks at hop 1024: k_tick (asserted through ss_session_last_tick_forms) on the 8192-frame slices, the reference f64
    over their concatenation; a restart in the middle"""
    assert tuple(P.plan(2, rate, SLICE)) == shared
    n_ticks, restart_at = P.TICK_CASE
    x, pos, anchors = tick_file(rate, n_ticks, 11, restart_at)
    classes = collections.Counter(a.cls for a in anchors)
    assert min(classes[P.TICK_TILE], classes[P.TICK_END]) >= len(P.d_order(shared[4])) // 2, classes
    factor = shared[4]
    parts = [(0, restart_at), (restart_at, n_ticks)]
    refs = [P.SegRef(np.vstack([x[p - SLICE:p] for p in pos[a:b]]), rate, factor, [SLICE] * (b - a)) for a, b in parts]
    w = Worst("file ticks %d" % rate)
    sess = ssa.FileSession(x.reshape(-1), 2, rate)
    try:
        for (a, b), ref in zip(parts, refs):
            if a:
                sess.restart()
            for k in range(a, b):
                res = sess.analyze_audio_file_samples(2 * pos[k])
                assert sess.last_tick_forms() == (True, True), (rate, k, sess.last_tick_forms())
                assert res.fed == 1 and res.add_status == 0 and res.shortterm_status == 0 and res.fft_ran == 1
                an = sess.analyzer
                tp = np.array([an.get_true_peak_channel(c) for c in range(2)])
                sp = np.array([an.get_sample_peak_channel(c) for c in range(2)])
                w.peaks((rate, k), tp, sp, ref, k - a)
                w.readings((rate, k), None, res.shortterm, ref, k - a, READING_LU, st_only=True)
                w.calls += 1
    finally:
        sess.close()
        w.report()


# measured: true peak 8.1e-08, short-term 1.8e-12 LU (40 ticks)
def test_session_capture_resident():
    """capture_push + tick_capture_resident: 1024 new frames per tick, the loudness call on the ring's newest 8192; every tick's
    short-term reading and peaks against the f64 reference over the concatenated slices"""
    rate, n_ticks = 48000, 40
    x, pos, anchors = tick_file(rate, n_ticks, 12)
    assert {a.cls for a in anchors} == {P.TICK_TILE, P.TICK_END}
    ring = np.zeros((15 * rate, 2), np.float32)
    slices, got = [], []
    w = Worst("capture ticks")
    sess = ssa.CaptureSession(2, rate)
    try:
        at = pos[0] - SLICE
        sess.push(x[at:pos[0] - HOP].reshape(-1))
        ring = np.vstack([ring, x[at:pos[0] - HOP]])[-15 * rate:]
        for k in range(n_ticks):
            new = x[pos[k] - HOP:pos[k]]
            sess.push(new.reshape(-1))
            ring = np.vstack([ring, new])[-15 * rate:]
            res = sess.analyze_resident()
            assert sess.last_tick_forms() == (True, True), (k, sess.last_tick_forms())
            slices.append(ring[-SLICE:].copy())
            an = sess.analyzer
            got.append((np.array([an.get_true_peak_channel(c) for c in range(2)]), np.array([an.get_sample_peak_channel(c) for c in range(2)]),
                        res.shortterm))
        ref = P.SegRef(np.vstack(slices), rate, 4, [SLICE] * n_ticks)
        assert np.array_equal(np.vstack(slices), np.vstack([x[p - SLICE:p] for p in pos]))      # (the slices are the file ticks' slices)
        for k, (tp, sp, st) in enumerate(got):
            w.peaks(("capture", k), tp, sp, ref, k)
            w.readings(("capture", k), None, st, ref, k, READING_LU, st_only=True)
            w.calls += 1
    finally:
        sess.close()
        w.report()
