#!/usr/bin/env python3
"""ss_batch_spectrum_regions at the bench shape (1024 x 10 s x 48 kHz stereo, N = 4096, hop 1024) and at one 600 s file: ms per call
(its launches, the list's upload included) and the rows its regions cover / time, each case alternated with ss_batch_spectrum_stats
on the same batch in the same process — the reduction of the same rows over whole streams."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L

REPS = 20
NO_GROUP = L.SS_REGION_NO_GROUP


def timed(b, enqueue):
    for _ in range(3):
        enqueue()
    b.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        enqueue()
    b.sync()
    return (time.perf_counter() - t0) * 1e3 / REPS


def rows_of(regions):
    return np.ascontiguousarray(np.array(regions, dtype=np.uint32).reshape(-1, 4))


def run_case(b, what, regions, n_groups):
    lay = b.layout
    regions = rows_of(regions)
    covered = sum(hi - lo for lo, hi in (b.region_windows(r) for r in regions)) * lay.fft_channels * lay.fft_bin_stride * 4.0
    stats = timed(b, b.spectrum_stats)
    ms = timed(b, lambda: b.spectrum_regions(regions, n_groups))
    chunks, chunk_windows = b.spectrum_regions_plan
    print(f"    {what:46s} {ms:8.4f} ms per call   {covered / 1e6:8.1f} MB covered  {covered / ms / 1e9:6.3f} TB/s   "
          f"plan {chunks} x {chunk_windows}   (spectrum_stats beside it: {stats:.4f} ms, {float(lay.fft_bytes) / stats / 1e9:.3f} TB/s)", flush=True)
    mean, mx, cnt = b.region_spectra(len(regions) - 1, 1)
    line = f"        last region: counted {[int(c) for c in cnt[0]]}, mid mean {np.nanmin(mean[0, 0]):.2f} .. {np.nanmax(mean[0, 0]):.2f} dB"
    if n_groups:
        gmean, gmx, gcnt = b.group_spectra(0, 1)
        line += f"; group 0: counted {[int(c) for c in gcnt[0]]}, peak-hold up to {np.nanmax(gmx[0, 0]):.2f} dB"
    print(line, flush=True)


b = ssa.Batch(48000, 2, 1024, 48000 * 10, 4096, 1024, flags=L.SS_BATCH_FFT)
b.synthesize(0x5EED0000, 0)
b.run(); b.sync()
lay = b.layout
print(f"bench shape: 1024 x {lay.n_windows} windows x {lay.fft_channels} rows of {lay.fft_bin_stride} floats = {float(lay.fft_bytes) / 1e6:.1f} MB", flush=True)
run_case(b, "1024 whole-stream regions, one group", [(s, 0, 100, 0) for s in range(1024)], 1)
run_case(b, "1024 whole-stream regions, no group", [(s, 0, 100, NO_GROUP) for s in range(1024)], 0)
run_case(b, "10240 one-second regions, 16 groups", [(s, 10 * j, 10, (10 * s + j) % 16) for s in range(1024) for j in range(10)], 16)
run_case(b, "8192 three-second regions sliding by 1 s", [(s, 10 * j, 30, NO_GROUP) for s in range(1024) for j in range(8)], 0)
b.close()

b = ssa.Batch(48000, 2, 1, 48000 * 600, 4096, 1024, flags=L.SS_BATCH_FFT)
b.synthesize(0x5EED0000, 0)
b.run(); b.sync()
lay = b.layout
print(f"one 600 s file: 1 x {lay.n_windows} windows x {lay.fft_channels} rows of {lay.fft_bin_stride} floats = {float(lay.fft_bytes) / 1e6:.1f} MB", flush=True)
run_case(b, "200 regions of 3 s, one group", [(0, 30 * j, 30, 0) for j in range(200)], 1)
run_case(b, "2 regions of 300 s (chunked plan), one group", [(0, 0, 3000, 0), (0, 3000, 3000, 0)], 1)
b.close()
