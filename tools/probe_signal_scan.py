#!/usr/bin/env python3
"""ss_batch_signal_scan at the bench shape (1024 x 10 s x 48 kHz stereo) on clean material, on the same corpus with events planted
in 1 % of its frames, and on one 600 s stream: ms per call, beside ss_batch_peak_series on the same batch and beside the time the
corpus takes at the 6.3 TB/s the card reads HBM at best.  A call is timed with the host clock around REPS calls queued back to back
and one synchronise (the batch's stream is its own and does not wait for the null stream, so there is no event to record from
outside; the call is three launches of which the first takes most of a millisecond, which the queue hides); the figure is the
median of WINDOWS such windows, with the fastest and the slowest beside it.  `--only clean|planted|long` queues nothing but the
scan of that shape (for `rocprofv3 --kernel-trace --stats -- python tools/probe_signal_scan.py --only clean`: each kernel's own
device time)."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L

REPS, WINDOWS = 20, 9
HBM_TBS = 6.3           # achievable HBM read bandwidth of the card, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["clean", "planted", "long"], default=None)
args = ap.parse_args()


def timed(b, enqueue, windows=WINDOWS):
    for _ in range(3):
        enqueue()
    b.sync()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(REPS):
            enqueue()
        b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / REPS)
    return statistics.median(ms), min(ms), max(ms)


def plant(b, streams, frames, rng):
    """1 % of every stream's frames: 24 runs of 100 silent frames and 24 runs of 100 clipped samples, at random places"""
    for s in range(streams):
        x = b.download_input(s).reshape(frames, -1)
        at = rng.choice(frames // 100 - 1, 48, replace=False) * 100 + int(rng.integers(0, 100))
        for i, a in enumerate(at):
            if i < 24:
                x[a:a + 100] = 0.0
            else:
                x[a:a + 100, i % x.shape[1]] = 1.0 if i % 4 < 2 else -1.0
        b.upload(s, x)


SCAN = dict(silence_threshold=0.0, clip_level=1.0, silence_min_frames=48, clip_min_samples=3, max_events=256)
SHAPES = {"clean": ("bench shape, clean", 1024, 10, False), "planted": ("bench shape, events in 1 % of the frames", 1024, 10, True),
          "long": ("one 600 s stream", 1, 600, False)}
for key, (name, streams, seconds, planted) in SHAPES.items():
    if args.only and args.only != key:
        continue
    rate, channels = 48000, 2
    frames = rate * seconds
    b = ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
    b.synthesize(0x5EED0000, 0)
    if planted:
        plant(b, streams, frames, np.random.default_rng(1))
    b.sync()
    tile, cap = b.signal_scan_plan()
    read = 4.0 * streams * frames * channels
    floor = read / (HBM_TBS * 1e12) * 1e3
    scan = lambda: b.signal_scan(**SCAN)
    if args.only:
        for _ in range(REPS + 3):
            scan()
        b.sync()
        b.close()
        continue
    print(f"{name}: {streams} x {cap} tiles of {tile} frames x {channels} channels; {read / 1e9:.3f} GB read, "
          f"{(80.0 * channels + 48.0) * streams * cap / 1e6:.2f} MB of tile records; at {HBM_TBS} TB/s the corpus takes {floor:.4f} ms", flush=True)
    ms, lo, hi = timed(b, scan)
    print(f"    signal_scan, lists of 256                {ms:8.4f} ms per call ({lo:.4f} .. {hi:.4f})   {read / ms / 1e9:6.3f} TB/s   "
          f"{ms / floor:5.2f} x the floor", flush=True)
    ms0, lo, hi = timed(b, lambda: b.signal_scan(**dict(SCAN, max_events=0)))
    print(f"    signal_scan, max_events = 0 (two launches) {ms0:6.4f} ms per call ({lo:.4f} .. {hi:.4f})", flush=True)
    pk, lo, hi = timed(b, b.peak_series)
    print(f"    peak_series                              {pk:8.4f} ms per call ({lo:.4f} .. {hi:.4f})   the scan takes {ms / pk:.2f} x its time", flush=True)
    b.signal_scan(**SCAN)
    st, ch = b.stream_scans(), b.channel_scans()
    print(f"    streams with silence runs: {int((st['silence_runs'] > 0).sum())}, with clip runs: {int((st['clip_runs'] > 0).sum())}; "
          f"runs listed: {int(np.minimum(st['silence_runs'], 256).sum() + np.minimum(st['clip_runs'], 256).sum())}; stream 0: "
          f"{int(st[0]['silent_frames'])} silent frames, DC {[float(v) for v in ch[0]['sum'] / frames]}, "
          f"RMS {[float(v) for v in np.sqrt(ch[0]['sum_sq'] / frames)]}", flush=True)
    b.close()
