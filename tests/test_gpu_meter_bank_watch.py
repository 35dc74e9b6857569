"""Meter banks' signal watch (ss_meter_bank_signal_watch*): after any sequence of adds, stream s's records are what the batch signal
scan defines for the concatenation of every frame stream s was given since its watch reset.

The model is numpy: reference() of tests/test_gpu_signal_scan.py on the concatenation, and three lines for frames, trailing_clip
and last_clip_frame.  Every integer must be EQUAL, however the material was cut into calls.  The two f64 sums are held to the
worst-case bound of recursive f64 summation in any order against math.fsum: |got - ref| <= gamma(N) * sum|x| (gamma(N) * sum x^2),
the bound the batch test derives; two feeds of the same calls must agree byte for byte.  Streams are 2 T + 71 frames, T from the
plan call."""
import ctypes

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.analyzer import AnalyzerError
from soundscope_amd.batch import STREAM_SCAN_DTYPE
from soundscope_amd.ingest import pcm_decode
from soundscope_amd.meter_bank import CHANNEL_WATCH_DTYPE, STREAM_WATCH_DTYPE, MeterBank
from test_gpu_signal_scan import INT_FIELDS, U64, gamma, loud, planted_intervals, reference

pytestmark = pytest.mark.gpu

RATE = 48000
CH_INT_FIELDS = INT_FIELDS + ("trailing_clip", "last_clip_frame")
EDGES = dict(silence_threshold=0.0, clip_level=1.0, silence_min_frames=3, clip_min_samples=3)


# ------------------------------------------------------------------------------------------------------------ model
def model(x, silence_threshold=0.0, clip_level=1.0, silence_min_frames=None, clip_min_samples=3):
    """one stream's concatenated input [frames][channels] -> (stream record, channel records [C], (sum|x|, sum x^2, N) [C])"""
    x = np.asarray(x, np.float32)
    smin = (RATE + 5) // 10 if silence_min_frames is None else silence_min_frames
    st, ch, _, _, bounds = reference(x, silence_threshold, clip_level, smin, clip_min_samples)
    wst, wch = np.zeros((), STREAM_WATCH_DTYPE), np.zeros(x.shape[1], CHANNEL_WATCH_DTYPE)
    for n in st.dtype.names:
        wst[n] = st[n]
    for n in ch.dtype.names:
        wch[n] = ch[n]
    wst["frames"] = len(x)
    with np.errstate(invalid="ignore"):
        clipped = np.abs(x) >= np.float32(clip_level)
    for c in range(x.shape[1]):
        at = np.flatnonzero(clipped[:, c])
        wch[c]["last_clip_frame"] = int(at[-1]) if at.size else U64
        wch[c]["trailing_clip"] = len(x) - 1 - int(np.flatnonzero(~clipped[:, c])[-1]) if not clipped[:, c].all() else len(x)
    return wst, wch, bounds


def hold(got, s, x, cfg, tag):
    """stream s of a read `got` = (streams, channels) against the model of its concatenated input x"""
    got_st, got_ch = got
    st, ch, bounds = model(x, **cfg)
    assert got_st[s] == st, (tag, s, got_st[s], st)
    for f in CH_INT_FIELDS:
        assert np.array_equal(got_ch[s][f], ch[f]), (tag, s, f, got_ch[s][f], ch[f])
    for c, (sum_abs, sum_sq, n) in enumerate(bounds):
        assert abs(got_ch[s][c]["sum"] - ch[c]["sum"]) <= gamma(n) * sum_abs, (tag, s, c, "sum", got_ch[s][c]["sum"], ch[c]["sum"])
        assert abs(got_ch[s][c]["sum_sq"] - ch[c]["sum_sq"]) <= gamma(n) * sum_sq, (tag, s, c, "sum_sq")


def watched(n, channels, **cfg):
    bank = MeterBank(n, channels, RATE)
    bank.enable_signal_watch(**cfg)
    return bank


def tile_of(bank):
    t = bank.signal_watch_plan()
    assert t % 64 == 0 and 0 < t * bank.channels <= 8192
    return t


def planes(channels, T, seed):
    """test_planted_runs_at_every_edge's two planes: per stream of planted_intervals() a silence plane and a clip plane"""
    F, plan = planted_intervals(T, 3)
    rng = np.random.default_rng(seed)
    silent, clipped = [], []
    for s, intervals in enumerate(plan):
        x, y = loud(rng, F, channels), loud(rng, F, channels)
        for (lo, hi) in intervals:
            x[lo:hi] = 0.0
            y[lo:hi, (s + lo) % channels] = rng.choice([-1.0, 1.0, 1.5], hi - lo)
        if s < 5:
            x[100] = 0.0
            x[100, s % channels] = 0.25                      # every channel but one is silent: not a silent frame
        silent.append(x)
        clipped.append(y)
    return F, plan, silent, clipped


def mixed(channels, T, seed):
    """both kinds of planted run in every stream: stream s has the silence of plan[s] and, on top, the clips of plan[(s + 3) % 8]"""
    F, plan, silent, _ = planes(channels, T, seed)
    rng = np.random.default_rng(seed + 1)
    out = []
    for s, x in enumerate(silent):
        x = x.copy()
        for (lo, hi) in plan[(s + 3) % len(plan)]:
            x[lo:hi, (s + lo) % channels] = rng.choice([-1.0, 1.0, 1.5], hi - lo)
        out.append(x)
    return F, plan, out


# ------------------------------------------------------------------------------------------------------------ 1. planted runs, one call
@pytest.mark.parametrize("channels", [1, 2, 3, 6])
def test_planted_runs_at_every_edge_one_call(channels):
    bank = watched(8, channels, **EDGES)
    T = tile_of(bank)
    F, plan, silent, clipped = planes(channels, T, channels * 7)
    assert len(plan) == 8
    empty = bank.signal_watch()
    assert (empty[0]["frames"] == 0).all() and (empty[0]["longest_silence_at"] == U64).all() and (empty[1]["last_clip_frame"] == U64).all()
    for tag, plane in (("silence", silent), ("clips", clipped)):
        bank.enable_signal_watch(**EDGES)                    # (enabling again starts empty)
        bank.add(np.stack(plane))
        got = bank.signal_watch()
        for s, x in enumerate(plane):
            hold(got, s, x, EDGES, (tag, channels))
        if tag == "silence":
            assert int(got[0][7]["leading_silence"]) == int(got[0][7]["trailing_silence"]) == F and int(got[0][0]["trailing_silence"]) == 7
    bank.enable_signal_watch()                               # the default minimum follows the rate
    bank.add(np.stack(silent))
    got = bank.signal_watch()
    for s, x in enumerate(silent):
        hold(got, s, x, {}, ("silence, 100 ms", channels))


# ------------------------------------------------------------------------------------------------------------ 2. every cut
def feed_and_hold(bank, streams, calls, cfg, tag, only=None):
    """calls: per call one frame count per stream (ragged) or one int (uniform); a read after every call, held against the model of
    every stream's prefix"""
    fed = [0] * len(streams)
    for k, call in enumerate(calls):
        if isinstance(call, int):
            bank.add(np.stack([x[fed[s]:fed[s] + call] for s, x in enumerate(streams)]))
            call = [call] * len(streams)
        else:
            bank.add_ragged([x[fed[s]:fed[s] + f] if f else None for s, (x, f) in enumerate(zip(streams, call))])
        fed = [a + f for a, f in zip(fed, call)]
        got = bank.signal_watch()
        for s, x in enumerate(streams):
            if only is None or s in only:
                hold(got, s, x[:fed[s]], cfg, (tag, k, call[s]))
    return fed


@pytest.mark.parametrize("scheme", ["10 ms blocks", "one cut", "one frame at a time", "ragged"])
def test_every_cut(scheme):
    channels = 2
    bank = watched(8, channels, **EDGES)
    T = tile_of(bank)
    F, plan, streams = mixed(channels, T, 22)
    if scheme == "10 ms blocks":
        fed = feed_and_hold(bank, streams, [480] * (F // 480) + [F % 480], EDGES, scheme)
        assert fed == [F] * 8
    elif scheme == "one cut":
        lo, hi = plan[1][0]                                  # a planted run of stream 1 (and, as clips, of stream 6)
        assert hi - lo >= 3 and (lo, hi) in plan[(6 + 3) % 8]
        for cut in (lo, lo + 2, hi, T - 1, T, T + 1, T + 64):
            bank.enable_signal_watch(**EDGES)
            feed_and_hold(bank, streams, [cut, F - cut], EDGES, (scheme, cut))
    elif scheme == "one frame at a time":
        head = T + 64 - 65                                   # 130 one-frame calls across the word seam at T + 64, four streams held
        feed_and_hold(bank, streams, [head], EDGES, scheme, only=())
        fed = [head] * 8
        for k in range(130):
            bank.add(np.stack([x[fed[s]:fed[s] + 1] for s, x in enumerate(streams)]))
            fed = [a + 1 for a in fed]
            got = bank.signal_watch()
            for s in (0, 1, 4, 6):
                hold(got, s, streams[s][:fed[s]], EDGES, (scheme, k))
    else:
        rng = np.random.default_rng(2)
        sizes = [0, 0, 1, 63, 64, 65, 480, 1000, T - 1, T, T + 1]
        left, calls = [F] * 8, []
        while any(left):
            call = [min(int(rng.choice(sizes)), n) for n in left]
            calls.append(call)
            left = [n - f for n, f in zip(left, call)]
        assert any(0 in c and any(c) for c in calls) and len(calls) < 40
        fed = feed_and_hold(bank, streams, calls, EDGES, scheme)
        assert fed == [F] * 8


# ------------------------------------------------------------------------------------------------------------ 3. forms
def test_forms():
    """the seven add forms, and add_device from a base one float off a 16-byte boundary at an odd stride: the same records"""
    n, channels = 4, 2
    cfg = dict(silence_threshold=0.0, clip_level=0.5, silence_min_frames=3, clip_min_samples=3)
    bank = watched(n, channels, **cfg)
    T = tile_of(bank)
    F, plan, planted = mixed(channels, T, 33)
    q16 = [np.round(x * 13000).astype(np.int16) for x in planted[:n]]      # loud() stays below 0.4 * 13000 / 32768 = 0.16
    for q in q16:
        q[np.abs(q) >= 13000] = 20000                        # the planted clips (1, 1.5) decode to 0.61 >= 0.5
    raw16 = [q.view(np.uint8).reshape(-1) for q in q16]
    raw24 = [np.stack([np.zeros(q.size, np.uint8), q.reshape(-1).astype(np.int32) & 0xFF, (q.reshape(-1).astype(np.int32) >> 8) & 0xFF],
                      axis=-1).astype(np.uint8).reshape(-1) for q in q16]
    xs = [pcm_decode(r.tobytes(), L.SS_PCM_S16).reshape(-1, channels) for r in raw16]             # ss_pcm_decode's values
    assert all(np.array_equal(pcm_decode(r.tobytes(), L.SS_PCM_S24).reshape(-1, channels), x) for r, x in zip(raw24, xs))
    assert max(float(np.abs(x).max()) for x in xs) > 0.5
    uniform, ragged = [T + 7, F - T - 7], [[T + 7, 0, 5, F], [F - T - 7, F, F - 5, 0]]
    src = ssa.Batch(RATE, channels, n + 1, F, flags=L.SS_BATCH_LUFS)        # a device buffer of (n + 1) F frames
    floats = (n + 1) * F * channels

    def bytes_of(raw, sb, lo, hi):
        return raw[lo * channels * sb:hi * channels * sb]

    def run(form):
        bank.enable_signal_watch(**cfg)
        fed = [0] * n
        for call in (ragged if "ragged" in form else uniform):
            counts = call if "ragged" in form else [call] * n
            blocks = [xs[s][fed[s]:fed[s] + f] for s, f in enumerate(counts)]
            if form == "add":
                bank.add(np.stack(blocks))
            elif form in ("add_pcm s16", "add_pcm s24"):
                raw, sb, fmt = (raw16, 2, L.SS_PCM_S16) if form.endswith("s16") else (raw24, 3, L.SS_PCM_S24)
                bank.add_pcm(np.concatenate([bytes_of(raw[s], sb, fed[s], fed[s] + f) for s, f in enumerate(counts)]), fmt)
            elif form == "add_ragged":
                bank.add_ragged([b if len(b) else None for b in blocks])
            elif form in ("add_ragged_pcm s16", "add_ragged_pcm s24"):
                raw, sb, fmt = (raw16, 2, L.SS_PCM_S16) if form.endswith("s16") else (raw24, 3, L.SS_PCM_S24)
                bank.add_ragged_pcm([bytes_of(raw[s], sb, fed[s], fed[s] + f) if f else None for s, f in enumerate(counts)], fmt)
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
                bank.signal_watch()                          # (waits: the buffer may be overwritten now)
            fed = [a + f for a, f in zip(fed, counts)]
        assert fed == [F] * n
        got = bank.signal_watch()
        for s in range(n):
            hold(got, s, xs[s], cfg, form)
        return got

    same_cut = {"uniform": ["add", "add_pcm s16", "add_pcm s24", "add_device", "add_device odd"],
                "ragged": ["add_ragged", "add_ragged_pcm s16", "add_ragged_pcm s24", "add_ragged_device", "add_ragged_device odd"]}
    first = None
    for cut, forms in same_cut.items():
        want = run(forms[0])
        first = first or want
        assert want[0].tobytes() == first[0].tobytes()       # the stream records are integers: equal however the feed was cut
        for f in CH_INT_FIELDS:
            assert np.array_equal(want[1][f], first[1][f]), (cut, f)
        for form in forms[1:]:
            got = run(form)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), form       # the same calls: byte for byte
    src.close()


# ------------------------------------------------------------------------------------------------------------ 4. untouched streams, isolation
@pytest.mark.parametrize("threshold", [0.0, float("inf")])
def test_untouched_streams_and_isolation(threshold):
    channels, n = 2, 4
    cfg = dict(silence_threshold=threshold, clip_level=1.0, silence_min_frames=1, clip_min_samples=1)
    bank, clean = watched(n, channels, **cfg), watched(n, channels, **cfg)
    T = tile_of(bank)
    F = 2 * T + 71
    rng = np.random.default_rng(4)
    streams = []
    for s, bad in enumerate((np.nan, np.inf, -np.inf, None)):
        x = loud(rng, F, channels)
        x[:T // 2] = 0.0
        x[T - 10:T + 10] = -0.0                              # (-0.0 is digital silence)
        x[F - 20:] = 0.0
        x[0:5, 1] = x[T - 10:T + 10, 1] = x[F - 20:, 1] = 1.0
        if bad is not None:
            x[0, 1] = x[T, 1] = x[F - 1, 1] = bad
        streams.append(x)
    ok = [np.where(np.isfinite(x), x, np.float32(1.0)) for x in streams]      # the same material without the non-finite samples
    calls = [[T + 3, 0, 100, T], [0, T + 3, F - 100, 0], [F - T - 3, F - T - 3, 0, F - T]]
    fed = [0] * n
    for k, call in enumerate(calls):
        before = bank.signal_watch()
        bank.add_ragged([x[fed[s]:fed[s] + f] if f else None for s, (x, f) in enumerate(zip(streams, call))])
        clean.add_ragged([x[fed[s]:fed[s] + f] if f else None for s, (x, f) in enumerate(zip(ok, call))])
        fed = [a + f for a, f in zip(fed, call)]
        got = bank.signal_watch()
        for s, f in enumerate(call):
            if not f:                                        # a stream given nothing: byte for byte
                assert got[0][s].tobytes() == before[0][s].tobytes() and got[1][s].tobytes() == before[1][s].tobytes(), (k, s)
            hold(got, s, streams[s][:fed[s]], cfg, ("nonfinite", threshold, k))
    bank.add_ragged([None] * n)                              # an all-zero call
    got, want = bank.signal_watch(), clean.signal_watch()
    # stream 3 never saw a non-finite sample: it equals the same stream of a bank that saw none at all, byte for byte
    assert got[0][3].tobytes() == want[0][3].tobytes() and got[1][3].tobytes() == want[1][3].tobytes()
    ch = got[1]
    assert (ch[:3, 1]["nonfinite"] == 3).all() and (ch[:3, 1]["first_nonfinite"] == 0).all() and (ch[:, 0]["nonfinite"] == 0).all()
    assert int(ch[3, 1]["nonfinite"]) == 0 and int(ch[3, 1]["first_nonfinite"]) == U64
    # a NaN is neither silent nor clipped; an infinity is clipped and, at +inf only, silent
    assert int(ch[0, 1]["trailing_clip"]) == 0 and int(ch[1, 1]["trailing_clip"]) == 20 and int(ch[0, 1]["last_clip_frame"]) == F - 2
    if threshold == 0.0:
        assert int(got[0][0]["leading_silence"]) == 0 and int(got[0][1]["trailing_silence"]) == 0
    else:
        assert int(got[0][0]["silent_frames"]) == F - 3 and int(got[0][1]["silent_frames"]) == int(got[0][2]["silent_frames"]) == F


# ------------------------------------------------------------------------------------------------------------ 5. nothing else moves
def test_the_watch_moves_nothing_else():
    n, channels = 4, 2
    rng = np.random.default_rng(5)
    plain, both = MeterBank(n, channels, RATE), MeterBank(n, channels, RATE)
    for bank in (plain, both):
        bank.enable_spectrum()
    both.enable_signal_watch(silence_threshold=0.01, clip_level=0.5)
    for call in ([480] * 4, [4800, 0, 17, 9601], [16384] * 4, [0, 333, 4799, 1]):
        blocks = [rng.uniform(-1, 1, (f, channels)).astype(np.float32) for f in call]
        for bank in (plain, both):
            if len(set(call)) == 1:
                bank.add(np.stack(blocks))
            else:
                bank.add_ragged([b if len(b) else None for b in blocks])
        assert plain.read().tobytes() == both.read().tobytes()
        for s in range(n):
            assert all(np.array_equal(u, v) for u, v in zip(plain.peaks(s), both.peaks(s)))
            assert all(np.array_equal(u, v) for u, v in zip(plain.histograms(s), both.histograms(s)))
        assert all(u.tobytes() == v.tobytes() for u, v in zip(plain.spectrum(), both.spectrum()))
    assert [int(v) for v in both.signal_watch()[0]["frames"]] == [480 + 4800 + 16384, 480 + 16384 + 333, 480 + 17 + 16384 + 4799, 480 + 9601 + 16384 + 1]


# ------------------------------------------------------------------------------------------------------------ 6. equals the batch
def test_equals_the_batch_scan():
    channels = 3
    cfg = dict(silence_threshold=1e-3, clip_level=0.9, silence_min_frames=2, clip_min_samples=2)
    bank = watched(4, channels, **cfg)
    T = tile_of(bank)
    F = 2 * T + 71
    rng = np.random.default_rng(6)
    streams = []
    for _ in range(4):
        x = rng.uniform(-1.2, 1.2, (F, channels)).astype(np.float32)
        x[rng.random((F, channels)) < 0.5] = 0.0
        streams.append(x)
    feed_and_hold(bank, streams, [[480, 0, 7, T], [T, T + 1, F - 7, 0], [F - T - 480, F - T - 1, 0, F - T]], cfg, "batch")
    wst, wch = bank.signal_watch()
    b = ssa.Batch(RATE, channels, 4, F, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
    assert b.signal_scan_plan()[0] == T
    b.upload(0, np.stack(streams))
    b.signal_scan(max_events=0, **cfg)
    st, ch = b.stream_scans(), b.channel_scans()
    b.close()
    for f in STREAM_SCAN_DTYPE.names:
        assert np.array_equal(wst[f], st[f]), f
    for f in INT_FIELDS:
        assert np.array_equal(wch[f], ch[f]), f
    for s, x in enumerate(streams):
        for c, (sum_abs, sum_sq, n) in enumerate(model(x, **cfg)[2]):
            assert abs(wch[s][c]["sum"] - ch[s][c]["sum"]) <= 2 * gamma(n) * sum_abs          # (the sum of both bounds)
            assert abs(wch[s][c]["sum_sq"] - ch[s][c]["sum_sq"]) <= 2 * gamma(n) * sum_sq


# ------------------------------------------------------------------------------------------------------------ 7. 64 channels
def test_sixty_four_channels():
    """65 sequences: the owning lanes span two waves"""
    channels = 64
    cfg = dict(silence_threshold=0.0, clip_level=1.0, silence_min_frames=2, clip_min_samples=2)
    bank = watched(4, channels, **cfg)
    T = tile_of(bank)
    F = 2 * T + 71
    rng = np.random.default_rng(64)
    streams = []
    for s in range(4):
        x = loud(rng, F, channels)
        for c in (0, 31, 63):
            for lo in (5 + c, T - 2, T + 61 + s, F - 3):     # short runs: inside a word, across the tile seam, across a word seam, to the end
                x[lo:lo + 4, c] = -1.0
        x[T - 1:T + 3] = 0.0                                 # (silence takes the clips of that stretch away again)
        x[F - 2:, :63] = 0.0                                 # every channel but the last: not silent
        streams.append(x)
    feed_and_hold(bank, streams, [[F, T, 1, 0], [0, F - T, F - 1, F]], cfg, "64 channels")
    st, ch = bank.signal_watch()
    assert int(st[0]["clip_runs"]) == int(ch[0]["clip_runs"].sum()) > 6 and int(st[0]["trailing_silence"]) == 0
    assert int(ch[0, 63]["trailing_clip"]) == 3 and int(ch[0, 31]["trailing_clip"]) == 0


# ------------------------------------------------------------------------------------------------------------ 8. a long call
def test_a_long_call():
    """one stream, 40 tiles and 71 frames in one call: the workgroup walks them in order"""
    channels = 2
    bank = watched(1, channels, **EDGES)
    T = tile_of(bank)
    F = 40 * T + 71
    rng = np.random.default_rng(8)
    x = loud(rng, F, channels)
    for k, seam in enumerate((T, 20 * T, 39 * T)):           # runs across tiles 0/1, 19/20, 38/39
        x[seam - 5 - k:seam + 6 + k] = 0.0
        x[seam + 100 - 2:seam + 100 + 3, k % channels] = 1.0
        x[seam - T + 10:seam - T + 12, 1] = -1.0             # (too short to count)
    x[3 * T - 1:5 * T + 1] = 0.0                             # two whole tiles and a frame on either side
    bank.add(x[None])
    got = bank.signal_watch()
    hold(got, 0, x, EDGES, "long")
    assert int(got[0][0]["longest_silence"]) == 2 * T + 2 and int(got[0][0]["longest_silence_at"]) == 3 * T - 1 and int(got[0][0]["frames"]) == F


# ------------------------------------------------------------------------------------------------------------ 9. state management
def records(bank):
    st, ch = bank.signal_watch()
    return st.tobytes(), ch.tobytes()


def test_state_management():
    n, channels = 4, 2
    cfg = dict(silence_threshold=0.0, clip_level=1.0, silence_min_frames=2, clip_min_samples=1)
    bank, twin = watched(n, channels, **cfg), watched(n, channels, **cfg)
    T = tile_of(bank)
    F = 2 * T + 71
    rng = np.random.default_rng(9)
    streams = []
    for _ in range(n):
        x = rng.uniform(-1.2, 1.2, (F, channels)).astype(np.float32)
        x[rng.random((F, channels)) < 0.5] = 0.0
        streams.append(x)
    calls = [[T + 1, 480, 0, F], [F - T - 1, F - 480, F, 0]]
    for b in (bank, twin):
        feed_and_hold(b, streams, calls[:1], cfg, "first call")
    assert records(bank) == records(twin)                    # identical calls: byte for byte, sums included
    # selective reset: the others byte-equal, the reset streams hold what followed
    before = bank.signal_watch()
    bank.reset_signal_watch([1, 3])
    after = bank.signal_watch()
    for s in (0, 2):
        assert after[0][s].tobytes() == before[0][s].tobytes() and after[1][s].tobytes() == before[1][s].tobytes()
    for s in (1, 3):
        hold(after, s, streams[s][:0], cfg, "reset")
    bank.reset()                                             # the meters' reset leaves the watch alone
    assert records(bank) == (after[0].tobytes(), after[1].tobytes()) and (bank.read()["frames"] == 0).all()
    bank.add_ragged([x[c:c + f] if f else None for x, c, f in zip(streams, calls[0], calls[1])])
    twin.add_ragged([x[c:c + f] if f else None for x, c, f in zip(streams, calls[0], calls[1])])
    got = bank.signal_watch()
    for s in (0, 2):
        hold(got, s, streams[s], cfg, "went on")
    hold(got, 1, streams[1][480:], cfg, "after its reset")
    hold(got, 3, streams[3][:0], cfg, "after its reset, given nothing")
    assert records(twin) != records(bank)
    for s in (0, 2):
        assert got[0][s].tobytes() == twin.signal_watch()[0][s].tobytes() and got[1][s].tobytes() == twin.signal_watch()[1][s].tobytes()
    # every refusal leaves the previous records
    good = records(bank)
    lib, h = L.lib(), bank._h
    nan, inf = float("nan"), float("inf")
    assert int(bank.signal_watch()[0][0]["frames"]) == F
    for fields in [(nan, 1.0, 1, 1, 0, 0), (-1e-9, 1.0, 1, 1, 0, 0), (0.0, nan, 1, 1, 0, 0), (0.0, 0.0, 1, 1, 0, 0), (0.0, -1.0, 1, 1, 0, 0),
                   (0.0, 1.0, 0, 1, 0, 0), (0.0, 1.0, 1, 0, 0, 0), (0.0, 1.0, 1, 1, 1, 0), (0.0, 1.0, 1, 1, 65536, 0), (0.0, 1.0, 1, 1, 0, 1)]:
        assert lib.ss_meter_bank_signal_watch_enable(h, ctypes.byref(L.SignalScanConfig(*fields))) == L.SS_ERR_INVALID_ARG, fields
        assert records(bank) == good, fields
    bad = np.array([0, n], np.uint32)
    assert lib.ss_meter_bank_signal_watch_reset(h, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 2) == L.SS_ERR_INVALID_ARG
    st, ch = np.zeros(n, STREAM_WATCH_DTYPE), np.zeros((n, channels), CHANNEL_WATCH_DTYPE)
    p_st, p_ch = st.ctypes.data_as(ctypes.POINTER(L.StreamWatch)), ch.ctypes.data_as(ctypes.POINTER(L.ChannelWatch))
    assert lib.ss_meter_bank_signal_watch(h, p_st, n - 1, p_ch, n * channels) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_signal_watch(h, p_st, n, p_ch, n * channels - 1) == L.SS_ERR_CAPACITY
    assert not st.tobytes().strip(b"\0") and not ch.tobytes().strip(b"\0")           # nothing written
    assert lib.ss_meter_bank_signal_watch(h, p_st, n, None, 0) == L.SS_OK and st.tobytes() == good[0]
    assert lib.ss_meter_bank_signal_watch(h, None, 0, p_ch, n * channels) == L.SS_OK and ch.tobytes() == good[1]
    assert records(bank) == good
    # both infinities are allowed, and enabling again starts empty
    assert lib.ss_meter_bank_signal_watch_enable(h, ctypes.byref(L.SignalScanConfig(inf, inf, 1, 1, 0, 0))) == L.SS_OK
    got = bank.signal_watch()
    for s in range(n):
        hold(got, s, streams[s][:0], cfg, "enabled again")
    # off: plan, reset and read are refused; the adds go on
    bank.disable_signal_watch()
    t = ctypes.c_uint32(0)
    assert lib.ss_meter_bank_signal_watch_plan(h, ctypes.byref(t)) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_signal_watch_reset(h, None, 0) == L.SS_ERR_INVALID_MODE
    assert lib.ss_meter_bank_signal_watch(h, p_st, n, p_ch, n * channels) == L.SS_ERR_INVALID_MODE
    with pytest.raises(AnalyzerError):
        bank.signal_watch()
    bank.add(np.stack([x[:480] for x in streams]))
    assert [int(v) for v in bank.read()["frames"]] == [f + 480 for f in calls[1]]         # (what followed the meters' reset)
    bank.disable_signal_watch()                              # (off twice is fine)
