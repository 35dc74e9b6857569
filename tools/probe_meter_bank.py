#!/usr/bin/env python3
"""Meter banks against handles: wall time of one live tick — every stream fed one block, then every stream's readings — for a
bank of N stereo 48 kHz meters (ss_meter_bank_add + ss_meter_bank_read) beside N handles doing the same work (ss_add_samples +
the four getters: momentary, short-term, integrated, range, per handle).  Medians over --iters ticks behind --warmup.

    python tools/probe_meter_bank.py [--n 1,16,256,1024] [--frames 480,4800] [--handles-max 256] [--json out.jsonl]

For the per-kernel split run it alone under rocprofv3 --kernel-trace --stats (--bank-only keeps the handles out of the trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa  # noqa: E402

RATE, CH = 48000, 2


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
    ap.add_argument("--frames", default="480,4800")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--handles-max", type=int, default=256, help="largest N also measured as N handles (each holds a HIP stream)")
    ap.add_argument("--bank-only", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rows = []
    rng = np.random.default_rng(1)
    for n in [int(v) for v in a.n.split(",")]:
        bank = ssa.MeterBank(n, CH, RATE)
        handles = []
        if not a.bank_only and n <= a.handles_max:
            for _ in range(n):
                h = ssa.Analyzer()
                h.create_loudness_meter(CH, RATE)
                handles.append(h)
        for f in [int(v) for v in a.frames.split(",")]:
            x = (0.2 * rng.standard_normal((n, f * CH))).astype(np.float32)
            bank_us, bank_p90 = median_us(lambda: (bank.add(x), bank.read()), a.iters, a.warmup)
            row = {"n": n, "frames": f, "bank_us": round(bank_us, 1), "bank_p90_us": round(bank_p90, 1),
                   "realtime_us": round(f / RATE * 1e6, 1)}
            if handles:
                def tick():
                    for s, h in enumerate(handles):
                        h.add_samples(x[s])
                        h.get_momentary_lufs(); h.get_shortterm_lufs(); h.get_integrated_lufs(); h.get_loudness_range()
                it = max(5, a.iters // max(1, n // 16))
                h_us, h_p90 = median_us(tick, it, max(2, a.warmup // max(1, n // 16)))
                row.update({"handles_us": round(h_us, 1), "handles_p90_us": round(h_p90, 1), "speedup": round(h_us / bank_us, 1)})
            rows.append(row)
            print(json.dumps(row), flush=True)
        del handles, bank
    if a.json:
        with open(a.json, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
