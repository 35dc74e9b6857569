#!/usr/bin/env python3
"""Ragged meter-bank ticks: wall time of one live tick — every stream fed its block, then every stream's readings — for a bank of
N stereo 48 kHz meters under three feeds: the uniform `add` of 480 frames, `add_ragged` of 480 frames for all, and `add_ragged`
of 432 ... 528 frames per stream with one stream in twenty idle (a fresh draw every tick).  --spectrum adds the largest bank's
jittered tick with the spectrum history on and `spectrum_columns(160, "reference")` behind the read.  Medians over --iters ticks
behind --warmup; the ragged calls are made as a C caller makes them (pointer and length arrays prepared outside the clock).

    python tools/probe_meter_bank_ragged.py [--n 16,256,1024] [--iters 60] [--warmup 15] [--spectrum] [--only jitter] [--json out.jsonl]

For the per-kernel split run one feed alone (--only) under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa  # noqa: E402
from soundscope_amd import _lib as L  # noqa: E402

RATE, CH, BLOCK, LO, HI = 48000, 2, 480, 432, 528


def median_us(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    t = []
    for i in range(iters):
        t0 = time.perf_counter()
        fn(warmup + i)
        t.append(time.perf_counter() - t0)
    return round(float(np.median(t) * 1e6), 1), round(float(np.percentile(t, 90) * 1e6), 1)


def ragged_args(x, lens):
    """(pointer array, frames array) of one tick: stream s's first lens[s] frames of x[s]"""
    n = len(lens)
    ptrs, frames = (C.c_void_p * n)(), (C.c_uint64 * n)()
    for s in range(n):
        frames[s] = int(lens[s])
        ptrs[s] = x[s].ctypes.data if lens[s] else None
    return ptrs, frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="16,256,1024")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--spectrum", action="store_true")
    ap.add_argument("--only", default="", help="uniform | ragged480 | jitter | jitter_spectrum")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    lib = L.lib()
    rows = []
    rng = np.random.default_rng(1)
    sizes = [int(v) for v in a.n.split(",")]
    ticks = a.iters + a.warmup
    for n in sizes:
        x = (0.2 * rng.standard_normal((n, HI * CH))).astype(np.float32)
        even = [ragged_args(x, np.full(n, BLOCK))] * ticks
        lens = rng.integers(LO, HI + 1, (ticks, n))
        lens[rng.random((ticks, n)) < 0.05] = 0
        jitter = [ragged_args(x, lens[t]) for t in range(ticks)]
        xu = np.ascontiguousarray(x[:, :BLOCK * CH])
        feeds = [("uniform", None), ("ragged480", even), ("jitter", jitter)]
        if a.spectrum and n == max(sizes):
            feeds.append(("jitter_spectrum", jitter))
        for name, args in feeds:
            if a.only and name != a.only:
                continue
            bank = ssa.MeterBank(n, CH, RATE)
            if name == "jitter_spectrum":
                bank.enable_spectrum()

            def tick(i):
                if args is None:
                    bank.add(xu)
                else:
                    rc = lib.ss_meter_bank_add_ragged(bank._h, args[i][0], args[i][1])
                    assert rc == 0, rc
                bank.read()
                if name == "jitter_spectrum":
                    bank.spectrum_columns(160, "reference")
            us, p90 = median_us(tick, a.iters, a.warmup)
            row = {"n": n, "feed": name, "tick_us": us, "tick_p90_us": p90, "of_10ms": round(us / 1e4, 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del bank
    if a.json:
        with open(a.json, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
