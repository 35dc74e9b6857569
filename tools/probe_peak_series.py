#!/usr/bin/env python3
"""ss_batch_peak_series and ss_batch_peak_regions at the bench shape (1024 x 10 s x 48 kHz stereo), on one 600 s stream and at
64 x 10 s x 96 kHz x 8 channels with the factor forced to 4: ms per call (host clock around REPS calls queued back to back and one
synchronise: the batch's stream is its own, so there is no event to record from outside; the launch is one kernel of a millisecond
or more, which the queue hides), the corpus bytes read and the record bytes written over that time, and beside it the k_time_domain
time of a pass of the same batch made with SS_BATCH_TRUE_PEAK alone (event-timed inside passes) — until now the only way to a true
peak.  `--only series` queues nothing but the series (for `rocprofv3 --kernel-trace --stats -- python tools/probe_peak_series.py
--only series`: the kernel's own device time)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L

REPS = 20

ap = argparse.ArgumentParser()
ap.add_argument("--only", choices=["series"], default=None)
args = ap.parse_args()


def timed(b, enqueue):
    for _ in range(3):
        enqueue()
    b.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        enqueue()
    b.sync()
    return (time.perf_counter() - t0) * 1e3 / REPS


def time_domain_ms(b):
    """the TIME_DOMAIN slot of a pass (k_time_domain and its hand-over launches), ms per pass"""
    b.run(); b.sync()
    b.timing_enable(True)
    for _ in range(10):
        b.run()
    b.sync()
    ms, n = b.timing_read(L.SS_KERNEL_TIME_DOMAIN)
    b.timing_enable(False)
    return ms / max(n, 1)


SHAPES = (("bench shape", 48000, 2, 1024, 10, 0), ("one 600 s stream", 48000, 2, 1, 600, 0),
          ("64 x 10 s x 96 kHz x 8 ch, factor 4", 96000, 8, 64, 10, 4))
for name, rate, channels, streams, seconds, forced in SHAPES[:1] if args.only else SHAPES:
    frames = rate * seconds
    b = ssa.Batch(rate, channels, streams, frames, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK, true_peak_factor=forced)
    b.synthesize(0x5EED0000, 0)
    b.sync()
    tile, cap = b.peak_series_plan()
    read, written = 4.0 * streams * frames * channels, 16.0 * streams * cap * channels
    ms = timed(b, b.peak_series)
    print(f"{name}: {streams} x {cap} entries x {channels} channels, tiles of {tile} frames; {read / 1e9:.3f} GB read, "
          f"{written / 1e6:.2f} MB written", flush=True)
    print(f"    peak_series                          {ms:8.4f} ms per call   {(read + written) / ms / 1e9:6.3f} TB/s", flush=True)
    if args.only:
        b.close()
        continue
    print(f"    k_time_domain, TRUE_PEAK-only pass   {time_domain_ms(b):8.4f} ms per pass", flush=True)
    again = timed(b, b.peak_series)
    print(f"    peak_series (again)                  {again:8.4f} ms per call   {(read + written) / again / 1e9:6.3f} TB/s", flush=True)
    lists = [("whole-stream regions, one group", [(s, 0, cap, 0) for s in range(streams)], 1),
             ("one-second regions, 16 groups", [(s, a, 10, s % 16) for s in range(streams) for a in range(0, cap - 9, 10)], 16)]
    for what, regions, n_groups in lists:
        rows = np.array(regions, np.uint32)
        rms = timed(b, lambda: b.peak_regions(rows, n_groups, 0.5))
        res, grp = b.region_peaks(), b.group_peaks()
        print(f"    {what:34s} {len(rows):6d} regions  {rms:8.4f} ms per call   region 0: {res[0].true_peak:.4f} at frame "
              f"{res[0].true_peak_frame} ch {res[0].true_peak_channel}, {res[0].n_over} over; group 0: {grp[0].true_peak:.4f} in region "
              f"{grp[0].true_peak_region}", flush=True)
    tp, _ = b.peaks(0)
    mine = b.peak_series_of(0)["true_peak"].max(axis=0)
    print(f"    stream 0: series maximum {[float(v) for v in mine[:2]]}, the pass's true peak {[float(v) for v in tp[:2]]}", flush=True)
    b.close()
