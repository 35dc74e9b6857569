#!/usr/bin/env python3
"""Meter banks' signal watch: what the watch adds to a live tick, and what its serial walk costs on a long call.  Every figure is
wall time against the same bank with the watch off, in the same run, the two alternating in stretches (the watch is switched
outside the clock).  Medians over --iters ticks of each behind --warmup.

  ticks      a bank of --n stereo 48 kHz meters fed 480 frames (10 ms): `add` + `read()`, and with the watch on `add` + `read()` +
             `signal_watch()`; once on clean noise, once with silent and clipped runs planted in 1 % of the frames
  long call  one stereo stream given --seconds of input in ONE `add` call, watch off and on: one workgroup walks the whole call
             tile by tile, so the difference is the serial walk ("not built: tile-parallel form for long calls")

    python tools/probe_meter_bank_watch.py [--n 1024] [--iters 60] [--warmup 20] [--seconds 600] [--reps 3] [--json out.jsonl]

For the kernel times run under rocprofv3 --kernel-trace --stats: the watch is k_bank_signal_watch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa  # noqa: E402

RATE, CH, BLOCK = 48000, 2, 480
STRETCH = 10


def planted(rng, x):
    """silent and clipped runs of five frames in about 1 % of the frames of blocks x [k][n][BLOCK * CH]"""
    y = x.reshape(x.shape[0], x.shape[1], BLOCK, CH).copy()
    starts = rng.random(y.shape[:3]) < 0.002
    for d in range(5):
        hit = np.roll(starts, d, axis=2)
        y[..., 0][hit & (np.arange(BLOCK) % 2 == 0)[None, None, :]] = 1.0
        y[hit & (np.arange(BLOCK) % 2 == 1)[None, None, :]] = 0.0
    return y.reshape(x.shape)


def ticks(bank, x, iters, warmup):
    def plain(i):
        bank.add(x[i % len(x)])
        bank.read()

    def watch(i):
        bank.add(x[i % len(x)])
        bank.read()
        bank.signal_watch()

    times = {"plain": [], "watch": []}
    i = 0
    need = (iters + warmup) * STRETCH // (STRETCH - 1) + STRETCH         # (a stretch's first tick is dropped below)
    while min(len(t) for t in times.values()) < need:
        for name, fn in (("plain", plain), ("watch", watch)):
            if name == "watch":
                bank.enable_signal_watch()
            else:
                bank.disable_signal_watch()
            bank.read()                                      # (the switch has left the stream)
            for _ in range(STRETCH):
                t0 = time.perf_counter()
                fn(i)
                times[name].append(time.perf_counter() - t0)
                i += 1
    row = {}
    for name, t in times.items():
        # the first tick of a stretch pays for the switch's cold buffers: every stretch's first is dropped
        t = np.asarray([v for k, v in enumerate(t) if k % STRETCH][warmup:warmup + iters])
        row[name + "_tick_us"] = round(float(np.median(t) * 1e6), 1)
        row[name + "_tick_p90_us"] = round(float(np.percentile(t, 90) * 1e6), 1)
    row["watch_adds_us"] = round(row["watch_tick_us"] - row["plain_tick_us"], 1)
    row["watch_over_plain"] = round(row["watch_tick_us"] / row["plain_tick_us"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    out = []
    x = (0.2 * rng.standard_normal((4, a.n, BLOCK * CH))).astype(np.float32)
    bank = ssa.MeterBank(a.n, CH, RATE)
    for kind, blocks in (("clean", x), ("events in 1 % of the frames", planted(rng, x))):
        row = {"probe": "ticks", "input": kind, "n": a.n, "block_frames": BLOCK}
        row.update(ticks(bank, blocks, a.iters, a.warmup))
        bank.enable_signal_watch()
        bank.add(blocks[0])
        st, ch = bank.signal_watch()
        row["silent_frames_per_block"] = round(float(st["silent_frames"].mean()), 2)
        row["clipped_samples_per_block"] = round(float(ch["clipped_samples"].sum(axis=1).mean()), 2)
        out.append(row)
        print(json.dumps(row), flush=True)
    del bank
    frames = a.seconds * RATE
    long_x = np.tile((0.2 * rng.standard_normal((RATE, CH))).astype(np.float32), (a.seconds, 1))[None]
    one = ssa.MeterBank(1, CH, RATE)
    one.enable_signal_watch()
    tile = one.signal_watch_plan()
    times = {"plain": [], "watch": []}
    for _ in range(a.reps + 1):                              # (the first repetition of each grows the staging buffers: dropped)
        for name in ("plain", "watch"):
            if name == "watch":
                one.enable_signal_watch()
            else:
                one.disable_signal_watch()
            one.read()
            t0 = time.perf_counter()
            one.add(long_x)
            one.read()
            times[name].append(time.perf_counter() - t0)
    row = {"probe": "long call", "n": 1, "frames": frames, "seconds_of_input": a.seconds, "tile_frames": tile,
           "tiles": (frames + tile - 1) // tile}
    for name, t in times.items():
        row[name + "_call_ms"] = round(float(np.median(t[1:]) * 1e3), 2)
    row["watch_adds_ms"] = round(row["watch_call_ms"] - row["plain_call_ms"], 2)
    row["watch_us_per_tile"] = round(row["watch_adds_ms"] * 1e3 / row["tiles"], 3)
    st, _ = one.signal_watch()
    assert int(st[0]["frames"]) == frames
    out.append(row)
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
