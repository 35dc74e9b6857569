"""Planted material for the time-domain forms (a helper module, not a test file): the burst and the hand-over torture material
the batch forms are walked with (test_gpu_time_domain_forms.py), and — for the STREAMING forms (test_gpu_streaming_td_forms.py,
test_td_streaming_plants.py) — call schedules whose boundaries come from ss_td_streaming_plan, the bursts planted around them, the
f64 prefix reference of a stream, and four deliberately wrong f64 models that show the plants can fail.

A stream is a list of segments, a reset between them.  A segment is a list of call sizes and a list of `Anchor`s: a boundary of
one class at frame b (counted from the reset), and the call behind which it is read.  Around every anchor each channel c carries
one burst that starts at b - d, d taken from `d_order` at index (the anchor's turn within its class * channels + c): all of -2 ... SPAN + 48 / factor + 2 where
a class has enough anchors (the burst, then its ringing, then nothing straddle b frame by frame), the most telling offsets first
where it has not (a piece boundary happens once per call of 32 sub-blocks).  Amplitudes rise by GROW >= 2 % per anchor, so the
running maximum moves at every burst; channel c has its own factor, so a swapped channel or packed half reads wrong.
`tick_file` is the session ticks' material: every tick's new, highest burst straddles a tile boundary of the fed stream's grid or
the end of the 8192-frame slice the tick feeds.
"""
import collections
import functools

import numpy as np
from scipy import signal

import _f64ref as R

SPAN = 12
STEP_K = (0, 1, 2, 7, 15, 64, 481, 1999, 4799, 4801)      # frames between a level step and the boundary behind it
NOISE = 1e-3
AMP0 = 0.02
ONE_WAVE, SHARED = 0, 1

# boundary classes
CALL, CALL_SHARED, SHORT, TILE_ONE, TILE_SHARED, SUBBLOCK, NINTH, FIRST_1, END_1, PIECE, RESET = (
    "call", "call-shared", "short-calls", "tile-one-wave", "tile-shared", "sub-block", "ninth-tile", "first-tile-1", "end-1-behind",
    "piece", "reset")
CLASSES = (CALL, CALL_SHARED, SHORT, TILE_ONE, TILE_SHARED, SUBBLOCK, NINTH, FIRST_1, END_1, PIECE, RESET)

Plan = collections.namedtuple("Plan", "form waves tile chunk factor")
Anchor = collections.namedtuple("Anchor", "cls b read")             # read: index of the call behind which the boundary is read
Segment = collections.namedtuple("Segment", "sizes anchors")


def burst():
    t = np.arange(SPAN)
    return np.sin(np.pi / 2 * t + np.pi / 4) * np.hanning(SPAN + 2)[1:-1]


def torture(rate, n, ch, k, bounds, seed):
    """DC offset + 7 Hz + noise, its level stepping k frames in front of each boundary"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    g = np.ones(n)
    for j, b in enumerate(bounds):
        if b - k > 0:
            g[b - k:] = 0.25 if j % 2 == 0 else 1.0
    x = np.empty((n, ch))
    for c in range(ch):
        x[:, c] = g * ((0.45 - 0.1 * c) + 0.2 * np.sin(2 * np.pi * 7 * t + c) + 0.01 * rng.standard_normal(n))
    return x.astype(np.float32)


# ---------------------------------------------------------------- the plan
def plan(channels, rate, frames, factor=0):
    """(form, waves, tile_frames, chunk_frames, true_peak_factor) of one streaming call of `frames` frames (host only)"""
    import soundscope_amd as ssa
    p = ssa.streaming_plan(channels, rate, frames, factor)
    assert p.subblock_frames == R.subblock_frames(rate) and p.piece_frames == 32 * p.subblock_frames, (p.subblock_frames, p.piece_frames)
    return Plan(p.form, p.waves, p.tile_frames, p.chunk_frames, p.true_peak_factor)


def forms(channels, rate, factor=0):
    """(one-wave plan, shared plan): the longest one-wave call is one tile of the one-wave form, one frame more is shared"""
    one = plan(channels, rate, 1, factor)
    assert one.form == ONE_WAVE and one.waves == 1 and plan(channels, rate, one.tile, factor) == one, one
    shared = plan(channels, rate, one.tile + 1, factor)
    assert shared.form == SHARED and plan(channels, rate, 32 * R.subblock_frames(rate) + 999, factor) == shared, shared
    return one, shared


def history(factor):
    """frames of interpolator history an output reads in front of its own frame"""
    return 48 // factor if factor else 0


def d_order(factor):
    """every offset d in -2 ... SPAN + 48 / factor + 2, the most telling first: with the boundary 5 ... 8 frames into the burst, a
    history that is zeroed or one frame late moves the true peak by 7 % and more at either factor (with the whole burst in front
    of the boundary a late history only delays it, and behind the boundary nothing is lost)"""
    ds = list(range(-2, SPAN + history(factor) + 3))
    return sorted(ds, key=lambda d: (abs(d - 7), d))


def _grid_next(f, tile, S):
    """the first tile boundary of the absolute grid behind frame f: multiples of `tile` inside every sub-block of S frames"""
    base = f - f % S
    g = base + ((f - base) // tile + 1) * tile
    return min(g, base + S)


def _grid_in(a, b, tile, S):
    """tile boundaries g of the absolute grid with a < g < b"""
    out, g = [], _grid_next(a, tile, S)
    while g < b:
        out.append(g)
        g = _grid_next(g, tile, S)
    return out


def handle_segments(channels, rate, factor=0, light=False):
    """The call-size schedule of a handle case: two segments with a reset between them, reaching every boundary class.
    Counts per class: as many anchors as the sweep of d needs (ceil(ND / channels)), capped so that no segment is longer than
    about 40 sub-blocks.  light: a bank's schedule, one or two anchors per class — the sweep of d goes over its streams."""
    one, shared = forms(channels, rate, factor)
    S = R.subblock_frames(rate)
    T1, T8, H = one.tile, shared.tile, history(one.factor)
    nd = len(d_order(one.factor))
    gap = nd + SPAN + H + 2                                 # anchors at least this far apart carry bursts that do not overlap
    K = 2 if light else max(-(-nd // channels), 4)

    # ---- segment A
    sizes, anchors, fed = [], [], 0

    def clear(b):
        return not anchors or b - anchors[-1].b >= gap or anchors[-1].cls == RESET

    def call(n, cls=None, at=None, soft=False):
        """one call of n frames; cls: with an anchor at frame `at` (the call's start) — soft: unless the last anchor is too near"""
        nonlocal fed
        assert n > 0
        b = fed if at is None else at
        if cls is not None and (clear(b) or not soft):
            assert fed <= b < fed + n and clear(b), (cls, b, anchors[-1:])
            anchors.append(Anchor(cls, b, len(sizes)))
        sizes.append(n)
        fed += n

    # calls of 1 ... 25 frames and back: shorter than the history; anchors on call boundaries `gap` apart, read behind the ringing
    first = len(sizes)
    for n in (list(range(1, 26, 2)) + list(range(24, 0, -3))) if light else (list(range(1, 26)) + list(range(25, 0, -1))):
        call(n)
    ends = np.cumsum(sizes[first:])
    last = -gap
    for i, b in enumerate(ends[:-1]):
        if b - last >= gap and b + SPAN + H + 2 <= ends[-1] and b >= gap:
            read = first + int(np.searchsorted(ends, b + H + 2))
            anchors.append(Anchor(SHORT, int(b), read))
            last = b
    call(gap)                                               # clear of the block above
    # one-wave calls: anchors in turn on the call boundary and on the grid boundary inside the call
    n1 = T1 - 37 if T1 - 37 >= 2 * gap else T1 - 1              # (the grid boundary wanders through the calls)
    assert plan(channels, rate, n1, factor).form == ONE_WAVE and plan(channels, rate, 2 * T8 + 7, factor).form == SHARED

    def inner(n, tile):
        return [g for g in _grid_in(fed, fed + n, tile, S) if clear(g) and fed + n - g >= min(gap, n // 3)]

    for i in range(min(2 * K, 8 * S // n1)):
        call(gap)                                           # (a spacer: the bursts in front of the next anchor stand in no call that is read)
        inside = inner(n1, T1)
        if i % 2 and inside:
            call(n1, SUBBLOCK if inside[0] % S == 0 else TILE_ONE, inside[0])
        else:
            call(n1, CALL, soft=True)
    # shared calls of two tiles and a bit
    n8 = 2 * T8 + 7
    for i in range(min(2 * K, 10 * S // n8)):
        call(gap)
        inside = inner(n8, T8)
        if i % 2 and inside:
            g = inside[i // 2 % len(inside)]
            call(n8, SUBBLOCK if g % S == 0 else TILE_SHARED, g)
        else:
            call(n8, CALL_SHARED, soft=True)
    # a sub-block boundary inside a one-wave call and inside a shared call, whatever the loops above met
    for n, back in ((n1, n1 // 2), (n8, T8 + 3)):
        target = (fed + gap + back) // S * S + S              # the next sub-block boundary with room for a filler in front
        call(target - back - fed)
        call(n, SUBBLOCK, target)
    # a first tile of 1 frame, seven whole tiles, a ninth tile (wave 0's second) of 1 frame: the call ends 1 frame behind a boundary
    # (the ninth-tile anchors: a ninth tile that holds the whole ringing, read behind its own call)
    assert S % T8 == 0, (S, T8)                                # (td_split_chunk_frames' own condition for these shapes)
    inst = 7 * T8 + 2
    for i in range(3 if light else max(3, min(6, 14 * S // (inst + T8)))):
        call(_grid_next(fed + gap, T8, S) - 1 - fed)            # filler up to 1 frame in front of a boundary
        tiles = _grid_in(fed, fed + inst, T8, S)
        assert len(tiles) == 8 and tiles[0] == fed + 1 and tiles[-1] == fed + inst - 1, (fed, tiles)
        which = (FIRST_1, NINTH, END_1)[i % 3]
        call(inst + (H + 5 if which == NINTH else 0), which, tiles[0] if which == FIRST_1 else tiles[-1])
        if which == END_1:                                      # read behind the NEXT call: the ringing crosses the call's end
            anchors[-1] = anchors[-1]._replace(read=len(sizes))
            call(H + 4)                                         # (a call of its own: no later burst stands in it)
    call(gap)
    call(T1 - 1, CALL)
    seg_a = Segment(tuple(sizes), tuple(anchors))

    # ---- segment B, behind the reset: noise only, a few planted calls, one call of more than 32 sub-blocks, a last short one
    sizes, anchors, fed = [], [], 0
    call(T1 // 2, RESET, 0)                                 # (no burst is planted on a RESET anchor: the call is noise alone)
    call(gap)
    for i in range(6):
        call(gap)
        call(T1 - 1 if i % 2 else n8, CALL if i % 2 else CALL_SHARED, soft=True)
    call(gap + 5)
    call(32 * S + max(T8 + 11, 2 * gap), PIECE, fed + 32 * S)
    call(gap)                                               # (the next anchor's bursts stay out of the long call)
    call(T1 - 3, CALL)
    return seg_a, Segment(tuple(sizes), tuple(anchors))


# ---------------------------------------------------------------- the material
def growth(n_anchors):
    """amplitude ratio from one anchor to the next: at least 2 %, more where the segment is short"""
    return float(np.clip((0.9 / AMP0) ** (1.0 / max(n_anchors, 1)), 1.02, 1.06))


def channel_gain(c, channels):
    return 1.0 - 0.45 * c / max(channels, 2)


def plant(seg, channels, factor, seed, turn=None):
    """f32 [frames][channels] of one segment: quiet noise and one burst per (anchor, channel); returns (x, starts[anchor][channel]).
    turn(anchor index, channel): the index into d_order (default: the anchor's turn within its class * channels + channel)"""
    n = int(sum(seg.sizes))
    rng = np.random.default_rng(seed)
    x = rng.uniform(-NOISE, NOISE, (n, channels))
    g = growth(len(seg.anchors))
    bst = burst()
    starts = np.full((len(seg.anchors), channels), -1, np.int64)
    seen = collections.Counter()
    for i, a in enumerate(seg.anchors):
        if a.cls == RESET:
            continue
        for c in range(channels):
            order = d_order(factor)
            d = order[(seen[a.cls] * channels + c if turn is None else turn(i, c)) % len(order)]
            s = int(np.clip(a.b - d, 0, n - SPAN))
            x[s:s + SPAN, c] += AMP0 * g ** i * channel_gain(c, channels) * bst
            starts[i, c] = s
        seen[a.cls] += 1
    return x.astype(np.float32), starts


def torture_segment(seg, rate, channels, k, seed):
    """the hand-over torture material over a segment's schedule: a level step k frames in front of every anchor"""
    return torture(rate, int(sum(seg.sizes)), channels, k, sorted({a.b for a in seg.anchors if a.b > 0}), seed)


# ---------------------------------------------------------------- the f64 reference of one segment
class SegRef:
    """Causal prefix readings of one segment (everything since a reset) behind each of its calls, f64, computed once.
    True peak after `fed` frames: max over the interpolated outputs [0, factor * fed) and the samples [0, fed)."""

    def __init__(self, x, rate, factor, sizes):
        self.x = np.asarray(x)
        self.rate, self.factor = rate, factor
        self.n, self.channels = self.x.shape
        self.ends = np.cumsum(np.asarray(sizes, np.int64))
        assert self.ends[-1] == self.n
        x64 = self.x.astype(np.float64)
        self.sp_ends = np.maximum.accumulate(np.abs(x64), axis=0)[self.ends - 1]
        self.tp_ends = self.sp_ends.copy()
        if factor:
            taps = R.interpolator_taps(factor)
            for c in range(self.channels):                  # (one channel at a time: the interpolated signal is not kept)
                u = np.maximum.accumulate(np.abs(signal.upfirdn(taps, x64[:, c], up=factor)[:factor * self.n]))
                self.tp_ends[:, c] = np.maximum(u[factor * self.ends - 1], self.sp_ends[:, c])
        bq, aq = R.kweight_coeffs(rate)
        self.y = signal.lfilter(bq, aq, x64, axis=0)
        self.w = R.channel_weights(self.channels)
        self.S = R.subblock_frames(rate)

    def sample_peak(self, k):
        """behind call k"""
        return self.sp_ends[k]

    def true_peak(self, k):
        return self.tp_ends[k]

    def momentary(self, k):
        return R.window_reading(self.y, self.w, int(self.ends[k]), 4 * self.S)

    def shortterm(self, k):
        return R.window_reading(self.y, self.w, int(self.ends[k]), 30 * self.S)

    def _up_max(self, lo, hi, w=None, w_at=0):
        """max |interpolated output| of the frames [lo, hi) per channel; w: other input frames, w[0] standing at frame w_at"""
        f, H = self.factor, history(self.factor)
        out = np.zeros(self.channels)
        if not f or hi <= lo:
            return out
        if w is None:
            w_at = max(lo - H - 1, 0)
            w = self.x[w_at:hi].astype(np.float64)
        taps = R.interpolator_taps(f)
        for c in range(self.channels):
            out[c] = np.abs(signal.upfirdn(taps, w[:hi - w_at, c], up=f))[f * (lo - w_at):f * (hi - w_at)].max()
        return out

    def _prefix(self, fed):
        """max |interpolated output| of the frames [0, fed), any fed"""
        k = int(np.searchsorted(self.ends, fed, side="right")) - 1
        base = self.tp_ends[k] if k >= 0 else np.zeros(self.channels)       # (holds the samples' maximum too: harmless below)
        at = int(self.ends[k]) if k >= 0 else 0
        return np.maximum(base, self._up_max(at, fed))

    # ---- deliberately wrong models, each wrong at ONE boundary b and read behind call k
    def wrong_history(self, b, k, mode):
        """true peak where the outputs of frame b and later read a history that was zeroed ('zero') or is one frame late ('shift')"""
        H, fed = history(self.factor), int(self.ends[k])
        lo, hi = max(b - H - 2, 0), min(fed, b + H + 2)
        w = self.x[lo:hi].astype(np.float64)
        if mode == "zero":
            w[:b - lo] = 0.0
        else:
            w[1:b - lo] = w[:b - lo - 1].copy()
            w[0] = 0.0
        got = np.maximum(self._up_max(b, hi, w, lo), self._up_max(hi, fed))
        if b > 0:
            got = np.maximum(got, self._prefix(b))
        return np.maximum(got, self.sp_ends[k])

    def wrong_filter_state(self, b, k, subblocks=4):
        """momentary (subblocks = 30: short-term) reading where the filter state was zeroed at frame b"""
        fed = int(self.ends[k])
        bq, aq = R.kweight_coeffs(self.rate)
        y = np.vstack([self.y[:b], signal.lfilter(bq, aq, self.x[b:fed].astype(np.float64), axis=0)])
        return R.window_reading(y, self.w, fed, subblocks * self.S)

    def wrong_swapped(self, k):
        """true peaks with channels 0 and 1 swapped (mono: none to swap)"""
        tp = self.tp_ends[k].copy()
        tp[[0, 1]] = tp[[1, 0]]
        return tp


def ragged_segment(channels, rate, stream, n_calls=40):
    """one stream of a ragged bank: its own call sizes — none, a few frames, either side of the form switch, several tiles — from a
    menu turned by the stream's number, anchors on the call boundaries"""
    one, shared = forms(channels, rate)
    T1, T8 = one.tile, shared.tile
    nd = len(d_order(one.factor))
    gap = nd + SPAN + history(one.factor) + 2
    menu = (0, T1, T1 + 1, 1, 2 * T8 + 7, 17, T1 - 1, 0, T8 + 333, 25, 3 * T8 - 5, T1 // 2 + 1)
    sizes, anchors, fed = [], [], 0
    for k in range(n_calls):
        n = menu[(k + 5 * stream) % len(menu)]
        if n and fed >= gap and (not anchors or fed - anchors[-1].b >= gap) and n >= history(one.factor) + 2 and k + 1 < n_calls:
            anchors.append(Anchor(CALL_SHARED if n > T1 else CALL, fed, k))
        sizes.append(n)
        fed += n
    return Segment(tuple(sizes), tuple(anchors))


# ---------------------------------------------------------------- session ticks
TICK_AMP0, TICK_GROW = 0.003, 1.10         # (10 % per burst: the newest burst carries a sixth of a slice's energy, so a lost state shows)
HOP, SLICE, WINDOW = 1024, 8192, 16384          # frames: the tick hop, the loudness slice (16384 samples of stereo), the spectrum window
TICK_TILE, TICK_END = "tick-tile", "tick-slice-end"
TICK_CASE = (60, 34)                        # ticks of the file cases, and the tick in front of which the session restarts
TickAnchor = collections.namedtuple("TickAnchor", "cls tick b")     # b: frame of the FED stream, counted from the last restart


def tick_file(rate, n_ticks, seed, restart_at=None):
    """A stereo file, its tick positions and the anchors of its plants.  A tick at position p feeds the slice [p - 8192, p) of the
    file; the fed stream is the concatenation of the slices since the last restart (before tick `restart_at`), and the tiles of the
    tick launch lie on ITS absolute grid.  Every tick brings one new burst per channel, 10 % over the last, inside the 1024 frames
    the slice has that the one before had not — so it is the burst that moves the running maximum of that tick.  Where a tile
    boundary g of the fed stream's grid falls into those frames with room for the burst in front and its ringing behind, two
    ticks of three plant at g - d (TICK_TILE: the hand-over between two waves of the tick launch, its seventh or eighth tile);
    the others at the slice's end e (TICK_END: the call boundary).  d: each class's own turn through d_order, channel by channel."""
    one, shared = forms(2, rate)
    factor, H, T8, S = one.factor, history(one.factor), plan(2, rate, SLICE).tile, R.subblock_frames(rate)
    assert plan(2, rate, SLICE).form == SHARED
    order = d_order(factor)
    reach = max(order) + 2                                   # a burst starts at most this far in front of its boundary
    pos = [WINDOW + 17 + HOP * k for k in range(n_ticks)]
    n = pos[-1] + 64
    rng = np.random.default_rng(seed)
    x = rng.uniform(-NOISE, NOISE, (n, 2))
    taken = np.zeros(n, bool)
    bst = burst()
    anchors, turn, eligible = [], collections.Counter(), 0
    for k, p in enumerate(pos):
        kk = k - (restart_at if restart_at is not None and k >= restart_at else 0)       # ticks since the restart
        new0 = SLICE * kk + SLICE - HOP                      # the slice's newest frames, in the fed stream: [new0, new0 + HOP)
        inside = [g for g in _grid_in(new0 + reach, new0 + HOP - SPAN - H - 4, T8, S)]
        cls, b = TICK_END, SLICE * (kk + 1)
        if inside:
            eligible += 1
            if eligible % 3:
                cls, b = TICK_TILE, inside[0]
        starts = [p - SLICE + (b - SLICE * kk) - order[(turn[cls] * 2 + c) % len(order)] for c in range(2)]       # file frames
        if any(taken[q - 1:q + SPAN + 1].any() for q in starts):
            continue                                         # (the burst of the tick in front reaches here: this tick brings none)
        for c, q in enumerate(starts):
            x[q:q + SPAN, c] += TICK_AMP0 * TICK_GROW ** k * channel_gain(c, 2) * bst
            taken[q:q + SPAN] = True
        anchors.append(TickAnchor(cls, k, b))
        turn[cls] += 1
    return x.astype(np.float32), pos, anchors


# name, rate, channels, true-peak arithmetic (None: the default), torture step k (None: bursts)
HANDLE_SHAPES = [
    ("48k-2-f32", 48000, 2, "f32", None), ("48k-2-f16x3", 48000, 2, "f16x3", None), ("48k-2-torture", 48000, 2, "f32", 7),
    ("44k-2", 44100, 2, None, None), ("96k-2", 96000, 2, None, None), ("192k-2", 192000, 2, None, None),
    ("48k-1", 48000, 1, None, None), ("48k-3", 48000, 3, None, None), ("48k-5", 48000, 5, None, None), ("48k-6", 48000, 6, None, None),
    ("48k-8", 48000, 8, None, None), ("48k-16", 48000, 16, None, None), ("48k-56-four-waves", 48000, 56, None, None),
]


@functools.lru_cache(maxsize=2)
def handle_starts(channels, rate):
    """[segment] -> starts[anchor][channel] of handle_stream's bursts (-1: none)"""
    tpf = forms(channels, rate)[0].factor
    return tuple(plant(seg, channels, tpf, 1000 * channels + rate % 997 + i)[1] for i, seg in enumerate(handle_segments(channels, rate)))


@functools.lru_cache(maxsize=2)
def handle_stream(channels, rate, torture_k=None):
    """((segment, x, SegRef), ...) of a handle case, computed once"""
    out = []
    tpf = forms(channels, rate)[0].factor
    for i, seg in enumerate(handle_segments(channels, rate)):
        seed = 1000 * channels + rate % 997 + i
        x = plant(seg, channels, tpf, seed)[0] if torture_k is None else torture_segment(seg, rate, channels, torture_k, seed)
        out.append((seg, x, SegRef(x, rate, tpf, seg.sizes)))
    return tuple(out)
