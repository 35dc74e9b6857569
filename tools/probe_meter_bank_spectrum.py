#!/usr/bin/env python3
"""Meter-bank spectra against handles: wall time of one live tick of the reference's microphone view for N stereo 48 kHz inputs.
  (a) bank: add one block + spectrum_columns(160, reference) + read
  (b) bank: add one block + spectrum (full rows) + read
  (c) N handles, each fed the same window on the host: ss_get_fft of mid and of side (2N calls), for N <= --handles-max
Medians over --iters ticks behind --warmup.

    python tools/probe_meter_bank_spectrum.py [--n 1,16,256,1024] [--frames 480] [--handles-max 256] [--json out.jsonl]

For the kernel times (k_meter_bank_spectrum, k_bank_history_append) run it alone under rocprofv3 --kernel-trace --stats with
--bank-only."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa  # noqa: E402

RATE, CH, N = 48000, 2, 16384


def median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e6), float(np.percentile(t, 90) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1,16,256,1024")
    ap.add_argument("--frames", default="480")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--handles-max", type=int, default=256)
    ap.add_argument("--bank-only", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rows = []
    rng = np.random.default_rng(1)
    for n in [int(v) for v in a.n.split(",")]:
        bank = ssa.MeterBank(n, CH, RATE)
        bank.enable_spectrum()
        for f in [int(v) for v in a.frames.split(",")]:
            x = (0.2 * rng.standard_normal((n, f * CH))).astype(np.float32)
            for _ in range(N // f + 1):
                bank.add(x)                               # a full window first
            cols_us, cols_p90 = median_us(lambda: (bank.add(x), bank.spectrum_columns(160, "reference"), bank.read()),
                                          a.iters, a.warmup)
            rows_us, rows_p90 = median_us(lambda: (bank.add(x), bank.spectrum(), bank.read()), a.iters, a.warmup)
            row = {"n": n, "frames": f, "columns_us": round(cols_us, 1), "columns_p90_us": round(cols_p90, 1),
                   "rows_us": round(rows_us, 1), "rows_p90_us": round(rows_p90, 1), "realtime_us": round(f / RATE * 1e6, 1)}
            if not a.bank_only and n <= a.handles_max:
                handles = [ssa.Analyzer(CH, RATE) for _ in range(n)]
                win = (0.2 * rng.standard_normal((n, N * CH))).astype(np.float32)
                ms = [ssa.get_mid_and_side_samples(win[s]) for s in range(n)]

                def tick():
                    for s, h in enumerate(handles):
                        h.get_fft(ms[s][0])
                        h.get_fft(ms[s][1])
                it = max(5, a.iters // max(1, n // 16))
                h_us, h_p90 = median_us(tick, it, max(2, a.warmup // max(1, n // 16)))
                row.update({"handles_us": round(h_us, 1), "handles_p90_us": round(h_p90, 1),
                            "speedup_columns": round(h_us / cols_us, 1), "speedup_rows": round(h_us / rows_us, 1)})
                del handles
            rows.append(row)
            print(json.dumps(row), flush=True)
        del bank
    if a.json:
        with open(a.json, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
