#!/usr/bin/env python3
"""ss_batch_apply_gain and ss_batch_download_pcm at the bench shape (1024 x 10 s x 48 kHz stereo): ms per call of the sweep with one
point per stream (the constant form: 16-byte loads, packed f32 multiplies, 16-byte stores), with a two-point ramp over every whole
stream (the f64 form in every tile) and with a quarter of the streams touched — beside ss_batch_pair_series on the same batch in the
same run, which reads the corpus once where the sweep reads and writes it once each: the figure to read is the sweep's time over
TWICE the pair series'.  Then ss_batch_download_pcm (24-bit, 64 streams in one call) beside ss_batch_download_input for the same
streams.  A call is timed with the host clock around REPS calls queued back to back and one synchronise; the figure is the median of
WINDOWS such windows, with the fastest and the slowest beside it; the yardstick is timed before and after, so a drift of the box
shows.  The constant gain is 1 and the ramps fall from 1 to 0.9999, so the corpus stays what it was to within a few per cent over
the run.  `--only constant|ramp` queues nothing but that sweep (for `rocprofv3 --kernel-trace --stats -- python
tools/probe_apply_gain.py --only constant`: the kernel's own device time).  One process: the first failure ends it with a non-zero
status; run it under `timeout -k 10 600`."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import GAIN_POINT_DTYPE

REPS, WINDOWS = 20, 9
HBM_TBS = 6.3           # achievable HBM bandwidth of the card, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["constant", "ramp"], default=None)
ap.add_argument("--streams", type=int, default=1024)
args = ap.parse_args()


def timed(b, enqueue, reps=REPS):
    for _ in range(3):
        enqueue()
    b.sync()
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(reps):
            enqueue()
        b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(ms), min(ms), max(ms)


def points(streams, rows):
    """rows [(frame, gain)] for every stream of `streams`"""
    p = np.zeros(len(streams) * len(rows), GAIN_POINT_DTYPE)
    p["stream"] = np.repeat(np.asarray(streams, np.uint32), len(rows))
    p["frame"] = np.tile(np.asarray([f for f, _ in rows], np.uint64), len(streams))
    p["gain"] = np.tile(np.asarray([g for _, g in rows], np.float32), len(streams))
    return p


rate, channels, streams, seconds = 48000, 2, args.streams, 10
frames = rate * seconds
b = ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=L.SS_BATCH_ALL)
b.synthesize(0x5EED0000, 0)
b.sync()
constant = points(range(streams), [(0, 1.0)])
ramp = points(range(streams), [(0, 1.0), (frames - 1, 0.9999)])
quarter = points(range(0, streams, 4), [(0, 1.0)])
if args.only:
    p = constant if args.only == "constant" else ramp
    for _ in range(REPS + 3):
        b.apply_gain(p)
    b.sync()
    b.close()
    sys.exit(0)
corpus = 4.0 * streams * frames * channels
floor = 2.0 * corpus / (HBM_TBS * 1e12) * 1e3
print(f"bench shape: {streams} x {frames} frames x {channels} channels, {b.apply_gain_plan()} frames per workgroup; the corpus is "
      f"{corpus / 1e9:.3f} GB: read and written once at {HBM_TBS} TB/s it takes {floor:.4f} ms; {WINDOWS} windows of {REPS} calls each: "
      f"median (fastest .. slowest)", flush=True)


def line(name, t, moved):
    ms, lo, hi = t
    print(f"    {name:<46s}{ms:8.4f} ms per call ({lo:.4f} .. {hi:.4f})   {moved / ms / 1e9:6.3f} TB/s moved", flush=True)
    return ms


pair0 = line("pair_series, default pair (yardstick)", timed(b, b.pair_series), corpus)
t_const = line("apply_gain, one point per stream", timed(b, lambda: b.apply_gain(constant)), 2 * corpus)
t_ramp = line("apply_gain, a ramp over every whole stream", timed(b, lambda: b.apply_gain(ramp)), 2 * corpus)
t_quarter = line("apply_gain, a quarter of the streams", timed(b, lambda: b.apply_gain(quarter)), corpus / 2)
t_again = line("apply_gain, one point per stream (again)", timed(b, lambda: b.apply_gain(constant)), 2 * corpus)
pair1 = line("pair_series, default pair (again)", timed(b, b.pair_series), corpus)
print(f"    over twice the pair series' time: constant {t_const / (2 * max(pair0, pair1)):.2f} .. {t_again / (2 * min(pair0, pair1)):.2f}, "
      f"ramp {t_ramp / (2 * max(pair0, pair1)):.2f} .. {t_ramp / (2 * min(pair0, pair1)):.2f}; a quarter of the streams takes "
      f"{t_quarter / min(t_const, t_again):.2f} of all of them", flush=True)
stats = b.gain_stats()
print(f"    records: {int(stats['touched'].sum())} touched, largest sample peak {float(stats['sample_peak'].max()):.4f}, "
      f"{int(stats['n_over'].sum())} samples at or over 1.0, {int(stats['n_nonfinite'].sum())} non-finite", flush=True)

n_out = min(64, streams)
t_pcm = timed(b, lambda: b.download_pcm(0, n_out, L.SS_PCM_S24), reps=1)
t_in = timed(b, lambda: [b.download_input(s) for s in range(n_out)], reps=1)
print(f"    download_pcm, 24-bit, {n_out} streams in one call   {t_pcm[0]:8.3f} ms ({t_pcm[1]:.3f} .. {t_pcm[2]:.3f}), "
      f"{3.0 * n_out * frames * channels / 1e6:.1f} MB out;   download_input, the same streams one by one {t_in[0]:8.3f} ms "
      f"({t_in[1]:.3f} .. {t_in[2]:.3f}), {4.0 * n_out * frames * channels / 1e6:.1f} MB out", flush=True)
b.close()
