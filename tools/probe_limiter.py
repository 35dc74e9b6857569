#!/usr/bin/env python3
"""ss_batch_limit on the device, in three parts (`--part timing|long|residual`, one process each; run each under its own `timeout
-k 10 <seconds>` and chain them with `&&`, so that the first failure ends the run):

timing    the bench shape (1024 x 10 s x 48 kHz stereo), ms per call of the limiter's two launches beside the yardstick, on the same
          batch in the same run: ss_batch_peak_series plus ss_batch_apply_gain with one point per stream, which together read the
          corpus twice and write it once as the limiter does.  Three cases: nothing over the ceiling (the constant form in every
          tile, no scratch traffic), events in 1 % of the tiles, every tile limited.  A call is timed with the host clock around REPS
          calls queued back to back and one synchronise; the figure is the median of WINDOWS such windows, with the fastest and the
          slowest beside it.  The limiter changes the corpus, so a window of the two limiting cases starts from the synthetic corpus
          again (1 %: with events planted by a gain spike of 64 frames) and lowers the ceiling by 3 % from call to call: what the call
          before pinned at its ceiling is over the next one's.
long      one stream of 600 s: the same, nothing over the ceiling and every tile limited.
residual  the true peak left behind the call, in dB over the ceiling, for an fs/4 burst, a clipped 1 kHz burst and a full-scale noise
          burst at +8 dB of gain, ceiling -1 dBTP, hold 10 ms, look-ahead 1.5 ms and 0, true-peak detector — beside the same figure
          of the numpy limiter (f64 polyphase levels, limit_curve, f64 products) on the same input.
only      queues nothing but REPS + 3 calls with nothing over the ceiling and one peak series (for `rocprofv3 --kernel-trace --stats
          -- python tools/probe_limiter.py --part only`: the kernels' own device times)."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import GAIN_POINT_DTYPE, LIMIT_ITEM_DTYPE, limit_curve

REPS, WINDOWS = 20, 9
RATE = 48000
LOOKAHEAD_S, HOLD_S = 0.0015, 0.010

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["timing", "long", "residual", "only"], required=True)
ap.add_argument("--streams", type=int, default=1024)
args = ap.parse_args()


def timed(b, enqueue, prepare=None):
    """median, fastest, slowest ms per call over WINDOWS windows of REPS queued calls; enqueue(k) queues call k of a window"""
    ms = []
    for w in range(WINDOWS + 1):                                # (the first window warms up)
        if prepare:
            prepare()
        b.sync()
        t0 = time.perf_counter()
        for k in range(REPS):
            enqueue(k)
        b.sync()
        if w:
            ms.append((time.perf_counter() - t0) * 1e3 / REPS)
    return statistics.median(ms), min(ms), max(ms)


def line(name, t):
    print(f"    {name:<58s}{t[0]:8.4f} ms per call ({t[1]:.4f} .. {t[2]:.4f})", flush=True)
    return t[0]


def items_of(n, gain=1.0):
    it = np.zeros(n, LIMIT_ITEM_DTYPE)
    it["stream"], it["gain"] = np.arange(n), gain
    return it


def time_batch(streams, frames, with_events):
    b = ssa.Batch(RATE, 2, streams, frames, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
    seed = 0x5EED0000
    synth = lambda: b.synthesize(seed, 0)
    synth()
    one = np.zeros(streams, GAIN_POINT_DTYPE)
    one["stream"], one["gain"] = np.arange(streams), 1.0
    b.apply_gain(one)
    top = float(b.gain_stats()["sample_peak"].max())
    tile, group, scratch = b.limit_plan(streams, lookahead_s=LOOKAHEAD_S, hold_s=HOLD_S)
    tiles = streams * ((frames + tile - 1) // tile)
    print(f"{streams} x {frames} frames x 2 channels, tiles of {tile} frames ({tiles} of them), groups of {group} streams, {scratch / 2**20:.1f} MiB "
          f"of scratch; look-ahead {LOOKAHEAD_S * 1e3} ms, hold {HOLD_S * 1e3} ms, true-peak detector; largest sample {top:.4f}; {WINDOWS} windows "
          f"of {REPS} calls each: median (fastest .. slowest)", flush=True)
    items = items_of(streams)
    limit = lambda ceiling: b.limit(items, ceiling, lookahead_s=LOOKAHEAD_S, hold_s=HOLD_S)
    y0 = line("peak_series (yardstick, reads once)", timed(b, lambda k: b.peak_series()))
    y1 = line("apply_gain, one point per stream (yardstick, reads + writes)", timed(b, lambda k: b.apply_gain(one)))
    t_none = line("limit, nothing over the ceiling", timed(b, lambda k: limit(4.0 * top)))
    assert int(b.limit_stats()[0]["n_limited"].sum()) == 0
    print(f"        over the yardsticks' sum: {t_none / (y0 + y1):.3f}", flush=True)
    if with_events:
        # a spike of x 40 over 64 frames in 1 % of the tiles, spread over the streams: at most one per tile
        rng = np.random.default_rng(1)
        per_stream = (frames + tile - 1) // tile
        chosen = np.sort(rng.choice(tiles, max(1, tiles // 100), replace=False))
        rows = []
        for t in chosen:
            s, f = int(t // per_stream), int(t % per_stream) * tile + int(rng.integers(100, max(101, min(tile, frames - (t % per_stream) * tile) - 100)))
            rows += [(s, f - 1, 1.0), (s, f, 40.0), (s, f + 63, 40.0), (s, f + 64, 1.0)]
        spikes = np.zeros(len(rows), GAIN_POINT_DTYPE)
        for i, (s, f, g) in enumerate(rows):
            spikes[i] = (f, s, g)

        def plant():
            synth()
            b.apply_gain(spikes)
        t_some = line("limit, events in 1 % of the tiles", timed(b, lambda k: limit(2.0 * top * 0.97 ** k), plant))
        n = b.limit_stats()[0]["n_limited"]
        print(f"        the last call lowered {int(n.sum())} frames in {int((n > 0).sum())} streams; over the yardsticks' sum: {t_some / (y0 + y1):.3f}", flush=True)
    t_all = line("limit, every tile limited", timed(b, lambda k: limit(0.5 * top * 0.97 ** k), synth))
    n = b.limit_stats()[0]["n_limited"]
    print(f"        the last call lowered {int(n.sum())} of {streams * frames} frames; over the yardsticks' sum: {t_all / (y0 + y1):.3f}", flush=True)
    line("peak_series (again)", timed(b, lambda k: b.peak_series()))
    line("apply_gain, one point per stream (again)", timed(b, lambda k: b.apply_gain(one)))
    b.close()


# ---- residual true peak ----------------------------------------------------------------------------------------------------------
def taps_of(factor):
    t, n = np.zeros(36, np.float32), C.c_uint32()
    assert L.lib().ss_inspect_true_peak(factor, t.ctypes.data_as(C.POINTER(C.c_float)), 36, C.byref(n)) == L.SS_OK
    return t[:(factor - 1) * n.value].reshape(factor - 1, n.value).astype(np.float64)      # [branch][delay]


def frame_levels(x, taps):
    """[frames][channels] f64: max over the branches of every frame, x [frames][channels] (finite)"""
    x = np.asarray(x, np.float64)
    v = np.abs(x)
    for branch in taps:
        y = np.zeros_like(x)
        for d in range(len(branch) - 1, -1, -1):
            sh = np.zeros_like(x)
            sh[d:] = x[:x.shape[0] - d] if d else x
            y = y + branch[d] * sh
        v = np.maximum(v, np.abs(y))
    return v


def residual():
    F, ceiling = RATE // 2, float(np.float32(10.0 ** (-1.0 / 20.0)))
    n = np.arange(F)
    rng = np.random.default_rng(3)
    inside = (n >= F // 2 - 2400) & (n < F // 2 + 2400)
    signals = {"fs/4 sine burst at 45 degrees": np.sin(2 * np.pi * n / 4 + np.pi / 4),
               "1 kHz burst x 4, clipped at +-1": np.clip(4.0 * np.sin(2 * np.pi * 1000.0 * n / RATE), -1.0, 1.0),
               "full-scale noise burst, +8 dB": rng.uniform(-1.0, 1.0, F)}
    gains = [1.0, 1.0, float(np.float32(10.0 ** (8.0 / 20.0)))]
    x = np.stack([np.stack([(1e-3 * rng.uniform(-1, 1, F) + np.where(inside, s, 0.0)).astype(np.float32)] * 2, axis=1) for s in signals.values()])
    taps = taps_of(4)
    print(f"residual true peak behind the call, dB over the ceiling of {20 * np.log10(ceiling):.2f} dBTP; hold {HOLD_S * 1e3} ms, true-peak detector, "
          f"{RATE} Hz stereo; device (peak series behind the call) | numpy limiter on the same input", flush=True)
    worst = 0.0
    for lookahead_s in (LOOKAHEAD_S, 0.0):
        Lk, H = round(lookahead_s * RATE), round(HOLD_S * RATE)
        b = ssa.Batch(RATE, 2, len(signals), F, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
        b.upload(0, x)
        b.limit([(s, g) for s, g in enumerate(gains)], ceiling, lookahead_s=lookahead_s, hold_s=HOLD_S)
        b.peak_series()
        for s, name in enumerate(signals):
            got = float(b.peak_series_of(s)["true_peak"].max())
            level = frame_levels(x[s], taps).max(axis=1)
            c = limit_curve(level.astype(np.float32), gains[s], ceiling, Lk, H, 11)[2]
            ref = float(frame_levels(x[s].astype(np.float64) * (gains[s] * c)[:, None], taps).max())
            worst = max(worst, abs(got - ref) / ref)
            print(f"    look-ahead {lookahead_s * 1e3:3.1f} ms  {name:<34s}{20 * np.log10(got / ceiling):+8.4f} dB | {20 * np.log10(ref / ceiling):+8.4f} dB   "
                  f"(lowest gain {c.min():.4f})", flush=True)
        b.close()
    print(f"    device against numpy: worst |got - ref| / ref {worst:.2e}", flush=True)
    assert worst <= 1e-4, worst


if args.part == "only":              # nothing but REPS + 3 calls with nothing over the ceiling, for a kernel trace
    b = ssa.Batch(RATE, 2, args.streams, RATE * 10, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
    b.synthesize(0x5EED0000, 0)
    for _ in range(REPS + 3):
        b.limit(items_of(args.streams), 4.0, lookahead_s=LOOKAHEAD_S, hold_s=HOLD_S)
    b.peak_series()
    b.sync()
    b.close()
elif args.part == "timing":
    time_batch(args.streams, RATE * 10, True)
elif args.part == "long":
    time_batch(1, RATE * 600, False)
else:
    residual()
