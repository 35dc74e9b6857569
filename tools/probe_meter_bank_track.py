#!/usr/bin/env python3
"""Tracked meter-bank spectra: wall time of one live tick of a bank of N stereo 48 kHz meters fed 480 frames — `add`, then
`track_spectrum()` and `tracked_spectrum_columns(160, "reference")` (the averaged and the peak-hold curve of every row), then
`read()` — against the same tick with the instantaneous `spectrum_columns(160, "reference")`, on the same bank in the same run,
the two alternating in stretches of ten ticks.  Medians over --iters ticks of each behind --warmup.  Also printed: the bytes one
update moves (rows read, state read and written) and the state's device memory.

    python tools/probe_meter_bank_track.py [--n 1,16,256,1024] [--iters 60] [--warmup 20] [--only tracked] [--json out.jsonl]

For the kernel times run one kind alone (--only tracked) under rocprofv3 --kernel-trace --stats: the update is
k_bank_spectrum_track, the read-outs k_bank_spectrum_tracked_columns and (--rows: tracked_spectrum() once per ten ticks)
k_bank_spectrum_tracked_rows."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa  # noqa: E402

RATE, CH, BLOCK, COLS = 48000, 2, 480, 160
TAU_S, HOLD_S, DECAY = 0.125, 1.0, 16.0
STRETCH = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,256,1024")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="", help="tracked | instant")
    ap.add_argument("--rows", action="store_true", help="also read the full tracked rows once per ten ticks (outside the clock)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    out = []
    for n in [int(v) for v in a.n.split(",")]:
        x = (0.2 * rng.standard_normal((4, n, BLOCK * CH))).astype(np.float32)
        bank = ssa.MeterBank(n, CH, RATE)
        bank.enable_spectrum()
        bank.enable_spectrum_tracking(TAU_S, HOLD_S, DECAY)
        rows_per_stream, n_bins, _ = bank.spectrum_layout()

        def tracked(i):
            bank.add(x[i % 4])
            bank.track_spectrum()
            bank.tracked_spectrum_columns(COLS, "reference")
            bank.read()

        def instant(i):
            bank.add(x[i % 4])
            bank.spectrum_columns(COLS, "reference")
            bank.read()

        kinds = [k for k in (("tracked", tracked), ("instant", instant)) if not a.only or k[0] == a.only]
        times = {name: [] for name, _ in kinds}
        i = 0
        while min(len(t) for t in times.values()) < a.iters + a.warmup:
            for name, fn in kinds:
                for _ in range(STRETCH):
                    t0 = time.perf_counter()
                    fn(i)
                    times[name].append(time.perf_counter() - t0)
                    i += 1
            if a.rows:
                bank.tracked_spectrum()
        stride = (n_bins + 3) & ~3
        row = {"n": n, "rows": n * rows_per_stream, "n_bins": n_bins,
               "update_bytes": n * rows_per_stream * (n_bins * 4 + stride * 32),
               "state_bytes": n * rows_per_stream * stride * 16, "row_buffer_bytes": n * rows_per_stream * n_bins * 4}
        for name, t in times.items():
            t = np.asarray(t[a.warmup:a.warmup + a.iters])
            row[name + "_tick_us"] = round(float(np.median(t) * 1e6), 1)
            row[name + "_tick_p90_us"] = round(float(np.percentile(t, 90) * 1e6), 1)
        if "tracked_tick_us" in row:
            row["tracked_of_10ms"] = round(row["tracked_tick_us"] / 1e4, 4)
        out.append(row)
        print(json.dumps(row), flush=True)
        del bank
    if a.json:
        with open(a.json, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
