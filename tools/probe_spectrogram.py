#!/usr/bin/env python3
"""ss_batch_spectrogram at the bench shape (1024 x 10 s x 48 kHz stereo, N = 4096, hop 1024), 200 x 160 cells per row over the whole
batch, and at one 600 s file with 1 and 200 time columns: ms per call and rows read / time, beside ss_batch_spectrum_stats and
ss_batch_render_spectrum(160) on the same batch in the same process — the launches that also read every row exactly once.  The bench
shape is also timed with fewer time columns and with 1 and 512 frequency columns: what the cells themselves cost.  Every
figure is the median of REPS timed repetitions behind a warm-up; a repetition queues INNER calls and waits for them.
(render_spectrum waits for its small table upload inside every call: its figure includes that.)"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L

REPS, INNER, WARM = 9, 25, 3


def timed(b, enqueue):
    for _ in range(WARM):
        enqueue()
    b.sync()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(INNER):
            enqueue()
        b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / INNER)
    return statistics.median(ms), min(ms), max(ms)


for name, streams, seconds, views in (("bench shape", 1024, 10, ((1, 160), (20, 160), (200, 1), (200, 512), (200, 160))),
                                       ("one 600 s file", 1, 600, ((1, 160), (200, 160)))):
    b = ssa.Batch(48000, 2, streams, 48000 * seconds, 4096, 1024, flags=L.SS_BATCH_FFT)
    b.synthesize(0x5EED0000, 0)
    b.run(); b.sync()
    lay = b.layout
    row_bytes = float(lay.fft_bytes)
    print(f"{name}: {streams} x {lay.n_windows} windows x {lay.fft_channels} rows of {lay.fft_bin_stride} floats = {row_bytes / 1e6:.1f} MB; "
          f"stats plan {b.spectrum_stats_plan[0]} chunk(s) of {b.spectrum_stats_plan[1]} windows", flush=True)
    lines = [("spectrum_stats", timed(b, b.spectrum_stats)), ("render_spectrum(160)", timed(b, lambda: b.render_spectrum(160, 0.0)))]
    for t_cols, f_cols in views:
        runs, run_windows = b.spectrogram_plan(t_cols, f_cols, gain_db=0.0)
        lines.append((f"spectrogram({t_cols} x {f_cols}), {runs} run(s) of {run_windows}", timed(b, lambda: b.spectrogram(t_cols, f_cols, gain_db=0.0))))
    lines.append(("spectrum_stats (again)", timed(b, b.spectrum_stats)))
    for what, (med, lo, hi) in lines:
        print(f"    {what:44s} {med:8.4f} ms median ({lo:.4f} .. {hi:.4f})   {row_bytes / med / 1e9:6.3f} TB/s of rows read", flush=True)
    stats = min(lines[0][1][0], lines[-1][1][0])
    for what, (med, _, _) in lines[2:-1]:
        print(f"    {what.split(',')[0]} / spectrum_stats = {med / stats:.2f}", flush=True)
    got = b.spectrogram_of(streams - 1)
    print(f"    last stream, last view: {got.shape} cells, {int(np.isnan(got).sum())} NaN, mid {np.nanmin(got[0]):.2f} .. {np.nanmax(got[0]):.2f} dB, "
          f"download of the batch's pictures {b.spectrograms().nbytes / 1e6:.2f} MB", flush=True)
    b.close()
