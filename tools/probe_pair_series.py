#!/usr/bin/env python3
"""ss_batch_pair_series and ss_batch_pair_regions at the bench shape (1024 x 10 s x 48 kHz stereo): ms per call of the series for
the default pair (the 16-byte-load form) and for the list (1, 0), (0, 0) (the general form), and of the regions for 1024
whole-stream regions in one group and 10 240 one-second regions — beside ss_batch_signal_scan and ss_batch_peak_series on the same
batch in the same run, ss_batch_traffic_floor (the spectrum kernel's loads and stores alone: it reads every frame four times and
writes the spectra, so it is a floor for that pattern, not for one read of the corpus) and the time the corpus takes at the
6.3 TB/s the card reads HBM at best.  A call is timed with the host clock around REPS calls queued back to back and one
synchronise; the figure is the median of WINDOWS such windows, with the fastest and the slowest beside it.  The yardsticks are
timed before and after the series, so a drift of the box shows.  `--only series` queues nothing but the default-pair series (for
`rocprofv3 --kernel-trace --stats -- python tools/probe_pair_series.py --only series`: the kernel's own device time).  One process:
the first failure ends it with a non-zero status; run it under `timeout -k 10 600`."""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import pair_balance_db, pair_correlation, pair_mono_loss_db

REPS, WINDOWS = 20, 9
HBM_TBS = 6.3           # achievable HBM read bandwidth of the card, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["series"], default=None)
ap.add_argument("--streams", type=int, default=1024)
args = ap.parse_args()


def timed(b, enqueue):
    for _ in range(3):
        enqueue()
    b.sync()
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            enqueue()
        b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / REPS)
    return statistics.median(ms), min(ms), max(ms)


rate, channels, streams, seconds = 48000, 2, args.streams, 10
frames = rate * seconds
b = ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=L.SS_BATCH_ALL)
b.synthesize(0x5EED0000, 0)
b.sync()
if args.only:
    for _ in range(REPS + 3):
        b.pair_series()
    b.sync()
    b.close()
    sys.exit(0)
read = 4.0 * streams * frames * channels
floor = read / (HBM_TBS * 1e12) * 1e3
tile, cap, _ = b.pair_series_plan()
print(f"bench shape: {streams} x {cap} entries x {channels} channels, {tile} frames in flight per workgroup; {read / 1e9:.3f} GB read, "
      f"{32.0 * streams * cap / 1e6:.2f} MB written per pair; at {HBM_TBS} TB/s the corpus takes {floor:.4f} ms; "
      f"{WINDOWS} windows of {REPS} calls each: median (fastest .. slowest)", flush=True)


def line(name, t, more=""):
    ms, lo, hi = t
    print(f"    {name:<44s}{ms:8.4f} ms per call ({lo:.4f} .. {hi:.4f})   {read / ms / 1e9:6.3f} TB/s   {ms / floor:5.2f} x the floor{more}", flush=True)
    return ms


SCAN = dict(silence_threshold=0.0, clip_level=1.0, silence_min_frames=48, clip_min_samples=3, max_events=0)
scan0 = line("signal_scan, max_events = 0 (yardstick)", timed(b, lambda: b.signal_scan(**SCAN)))
peak0 = line("peak_series (yardstick)", timed(b, b.peak_series))
pair = line("pair_series, default pair", timed(b, b.pair_series))
pair2 = line("pair_series, (1, 0) + (0, 0): general form", timed(b, lambda: b.pair_series([(1, 0), (0, 0)])))
pair_again = line("pair_series, default pair (again)", timed(b, b.pair_series))
scan1 = line("signal_scan, max_events = 0 (again)", timed(b, lambda: b.signal_scan(**SCAN)))
peak1 = line("peak_series (again)", timed(b, b.peak_series))
print(f"    the default-pair series takes {pair / min(scan0, scan1):.2f} .. {pair_again / max(scan0, scan1):.2f} x the scan's time and "
      f"{pair / min(peak0, peak1):.2f} .. {pair_again / max(peak0, peak1):.2f} x the peak series'", flush=True)

b.pair_series()
whole = [(s, 0, cap, 0) for s in range(streams)]
seconds_rows = [(s, 10 * k, 10, s % 16) for s in range(streams) for k in range(seconds)]
for name, rows, groups in (("whole-stream regions, one group", whole, 1), ("one-second regions, 16 groups", seconds_rows, 16)):
    rows = np.asarray(rows, np.uint32)
    ms, lo, hi = timed(b, lambda: b.pair_regions(rows, groups, threshold=0.0, power_floor=1e-8, min_run=3))
    r, g = b.region_pairs(), b.group_pairs()
    print(f"    {name:<34s}{len(rows):6d} regions  {ms:8.4f} ms per call ({lo:.4f} .. {hi:.4f})   region 0: correlation "
          f"{float(pair_correlation(r[0, 0])):+.4f}, balance {float(pair_balance_db(r[0, 0])):+.3f} dB, mono loss "
          f"{float(pair_mono_loss_db(r[0, 0])):+.3f} dB, {int(r[0, 0]['n_below'])} of {int(r[0, 0]['n_active'])} active entries below 0; "
          f"group 0: correlation {float(pair_correlation(g[0, 0])):+.4f} over {int(g[0, 0]['frames'])} frames", flush=True)

tf = b.traffic_floor(20)
print(f"    ss_batch_traffic_floor (the spectrum kernel's loads and stores alone, 20 launches): {tf:.4f} ms per launch", flush=True)
b.close()
