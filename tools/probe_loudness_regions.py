#!/usr/bin/env python3
"""ss_batch_loudness_regions at the bench shape (1024 x 10 s x 48 kHz stereo) — every stream one region, ten regions per stream, a
3 s window sliding by 1 s — and on one 600 s stream cut into 200 regions: ms per call (host clock around REPS calls queued back to
back and one synchronise; a call is the list's copy, two fills, k_region_gate and k_group_eval), beside the same batch's gating
launch (k_finalize, event-timed inside passes) and the gating launch with the loudness series behind it (k_finalize +
k_loudness_series) on a batch made with the series."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L

REPS = 50


def timed(b, enqueue):
    for _ in range(3):
        enqueue()
    b.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        enqueue()
    b.sync()
    return (time.perf_counter() - t0) * 1e3 / REPS


def gating_ms(b):
    """the FINALIZE slot of a pass (k_finalize, and k_loudness_series where the batch has the series), ms per pass"""
    b.timing_enable(True)
    for _ in range(10):
        b.run()
    b.sync()
    ms, n = b.timing_read(L.SS_KERNEL_FINALIZE)
    b.timing_enable(False)
    return ms / max(n, 1)


def cases(streams, n_sub):
    if streams == 1:
        step = n_sub // 200
        return [("200 regions of the stream", [(0, i * step, step, i % 8) for i in range(200)], 8),
                ("the whole stream", [(0, 0, n_sub, 0)], 1)]
    return [("whole-stream regions, one album", [(s, 0, n_sub, 0) for s in range(streams)], 1),
            ("ten regions per stream", [(s, i * (n_sub // 10), n_sub // 10, s % 16) for s in range(streams) for i in range(10)], 16),
            ("3 s window sliding by 1 s", [(s, a, 30, s % 16) for s in range(streams) for a in range(0, n_sub - 29, 10)], 16)]


for name, streams, seconds in (("bench shape", 1024, 10), ("one 600 s stream", 1, 600)):
    per_flags = {}
    for flags in (L.SS_BATCH_LUFS, L.SS_BATCH_LUFS | L.SS_BATCH_LOUDNESS_SERIES):
        b = ssa.Batch(48000, 2, streams, 48000 * seconds, 4096, 1024, flags=flags)
        b.synthesize(0x5EED0000, 0)
        b.run(); b.sync()
        per_flags[flags] = gating_ms(b)
        if flags != L.SS_BATCH_LUFS:
            b.close()
            continue
        n_sub = b.layout.n_subblocks
        print(f"{name}: {streams} x {n_sub} sub-blocks", flush=True)
        for what, regions, n_groups in cases(streams, n_sub):
            rows = np.array(regions, np.uint32)
            ms = timed(b, lambda: b.loudness_regions(rows, n_groups))
            blocks = int(np.maximum(rows[:, 2].astype(np.int64) - 3, 0).sum())
            res, grp = b.region_results(), b.group_results()
            print(f"    {what:34s} {len(rows):6d} regions {n_groups:3d} groups {blocks:8d} gating blocks  {ms:8.4f} ms per call   "
                  f"region 0: {res[0].integrated_lufs:.3f} LUFS, group 0: {grp[0].integrated_lufs:.3f} LUFS", flush=True)
        b.close()
    print(f"    k_finalize (event-timed, per pass)                 {per_flags[L.SS_BATCH_LUFS]:8.4f} ms", flush=True)
    print(f"    k_finalize + k_loudness_series (per pass)          {per_flags[L.SS_BATCH_LUFS | L.SS_BATCH_LOUDNESS_SERIES]:8.4f} ms", flush=True)
