#!/usr/bin/env python3
"""ss_batch_spectrum_stats at the bench shape (1024 x 10 s x 48 kHz stereo, N = 4096, hop 1024) and at one 600 s file: ms per
launch and rows read / time, beside ss_batch_render_spectrum(160 columns) on the same batch — the launch that also reads every
row exactly once.  (render_spectrum waits for its small table upload inside every call: its figure includes that.)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa
from soundscope_amd import _lib as L

REPS = 20


def timed(b, enqueue):
    for _ in range(3):
        enqueue()
    b.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        enqueue()
    b.sync()
    return (time.perf_counter() - t0) * 1e3 / REPS


for name, streams, seconds in (("bench shape", 1024, 10), ("one 600 s file", 1, 600)):
    b = ssa.Batch(48000, 2, streams, 48000 * seconds, 4096, 1024, flags=L.SS_BATCH_FFT)
    b.synthesize(0x5EED0000, 0)
    b.run(); b.sync()
    lay = b.layout
    chunks, chunk_windows = b.spectrum_stats_plan
    row_bytes = float(lay.fft_bytes)
    stats = timed(b, b.spectrum_stats)
    render = timed(b, lambda: b.render_spectrum(160, 0.0))
    again = timed(b, b.spectrum_stats)
    print(f"{name}: {streams} x {lay.n_windows} windows x {lay.fft_channels} rows of {lay.fft_bin_stride} floats = {row_bytes / 1e6:.1f} MB; "
          f"plan {chunks} chunk(s) of {chunk_windows} windows", flush=True)
    for what, ms in (("spectrum_stats", stats), ("render_spectrum(160)", render), ("spectrum_stats (again)", again)):
        print(f"    {what:24s} {ms:8.4f} ms per launch   {row_bytes / ms / 1e9:6.3f} TB/s of rows read", flush=True)
    print(f"    spectrum_stats / render_spectrum = {min(stats, again) / render:.2f}", flush=True)
    mean, mx, cnt = b.spectrum_stats_of(streams - 1)
    print(f"    last stream: counted {[int(c) for c in cnt]}, mid mean {mean[0].min():.2f} .. {mean[0].max():.2f} dB, peak-hold up to {mx[0].max():.2f} dB", flush=True)
    b.close()
