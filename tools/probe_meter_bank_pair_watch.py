#!/usr/bin/env python3
"""Meter banks' pair watch: what the watch adds to a live tick — beside what the signal watch adds, measured the same way in the
same run as the yardstick — and what its serial walk costs on a long call.  Every figure is wall time against the same bank with
the watch off, in the same run, the two alternating in stretches of ten ticks (the watch is switched outside the clock).

  ticks      a bank of --n stereo 48 kHz meters fed 480 frames (10 ms): `add` + `read()`, and with a watch on `add` + `read()` +
             `pair_watch()` (or `signal_watch()`).  Ten ticks are one entry: one tick of a stretch completes an entry in every
             stream and sums the window, so the mean is printed beside the median.
  long call  one stereo stream given --seconds of input in ONE `add` call, pair watch off and on: one workgroup walks the whole call
             entry by entry, so the difference is the serial walk ("not built: tile-parallel form for long calls")

    python tools/probe_meter_bank_pair_watch.py [--n 1024] [--iters 60] [--warmup 20] [--seconds 600] [--reps 3] [--bench] [--out FILE]

Without --step this is the driver: it touches no GPU itself and starts every step as a fresh process under a time limit of its own
(--limit seconds each); the first step that fails, faults or runs out of time ends the run, and nothing is started behind it.
--bench runs `bench.py --gpus 1` as a last step, to hold the batch step time against the parent's.  The steps' JSON lines go to
stdout and, with --out, into that file (profiles/meter_bank_pair_watch_probe.txt).
For the kernel times run a step under rocprofv3 --kernel-trace --stats: the watch is k_bank_pair_watch."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE, CH, BLOCK = 48000, 2, 480
STRETCH = 10
STEPS = ("ticks", "long")


def ticks(bank, x, iters, warmup, watch):
    """watch: 'pair' or 'signal' — (switch on, switch off, the read) of the watch that alternates with the plain tick"""
    on, off, read = {"pair": (bank.enable_pair_watch, bank.disable_pair_watch, bank.pair_watch),
                     "signal": (bank.enable_signal_watch, bank.disable_signal_watch, bank.signal_watch)}[watch]

    def plain(i):
        bank.add(x[i % len(x)])
        bank.read()

    def watched(i):
        bank.add(x[i % len(x)])
        bank.read()
        read()

    times = {"plain": [], "watch": []}
    i = 0
    need = (iters + warmup) * STRETCH // (STRETCH - 1) + STRETCH         # (a stretch's first tick is dropped below)
    while min(len(t) for t in times.values()) < need:
        for name, fn in (("plain", plain), ("watch", watched)):
            (on if name == "watch" else off)()
            bank.read()                                      # (the switch has left the stream)
            for _ in range(STRETCH):
                t0 = time.perf_counter()
                fn(i)
                times[name].append(time.perf_counter() - t0)
                i += 1
    off()
    row = {}
    for name, t in times.items():
        # the first tick of a stretch pays for the switch's cold buffers: every stretch's first is dropped
        t = np.asarray([v for k, v in enumerate(t) if k % STRETCH][warmup:warmup + iters])
        row[name + "_tick_us"] = round(float(np.median(t) * 1e6), 1)
        row[name + "_tick_p90_us"] = round(float(np.percentile(t, 90) * 1e6), 1)
        row[name + "_tick_mean_us"] = round(float(np.mean(t) * 1e6), 1)
    row["watch_adds_us"] = round(row["watch_tick_us"] - row["plain_tick_us"], 1)
    row["watch_adds_mean_us"] = round(row["watch_tick_mean_us"] - row["plain_tick_mean_us"], 1)
    row["watch_over_plain"] = round(row["watch_tick_us"] / row["plain_tick_us"], 3)
    return row


def step_ticks(a):
    import soundscope_amd as ssa
    rng = np.random.default_rng(1)
    x = (0.2 * rng.standard_normal((4, a.n, BLOCK * CH))).astype(np.float32)
    bank = ssa.MeterBank(a.n, CH, RATE)
    rows = []
    for watch in ("pair", "signal", "pair"):                 # the pair watch on either side of its yardstick
        row = {"probe": "ticks", "watch": watch, "n": a.n, "block_frames": BLOCK}
        row.update(ticks(bank, x, a.iters, a.warmup, watch))
        rows.append(row)
        print(json.dumps(row), flush=True)
    bank.enable_pair_watch()
    for i in range(2 * STRETCH):
        bank.add(x[i % len(x)])
    rec = bank.pair_watch()
    assert (rec["entries"] == 2).all() and (rec["open_frames"] == 0).all() and (rec["window"]["frames"] == 2 * STRETCH * BLOCK).all()
    pair = min(r["watch_adds_us"] for r in rows if r["watch"] == "pair")
    signal = [r["watch_adds_us"] for r in rows if r["watch"] == "signal"][0]
    print(json.dumps({"probe": "ticks, summary", "pair_watch_adds_us": pair, "signal_watch_adds_us": signal,
                      "pair_over_signal": round(pair / signal, 2) if signal > 0 else None}), flush=True)


def step_long(a):
    import soundscope_amd as ssa
    rng = np.random.default_rng(2)
    frames = a.seconds * RATE
    long_x = np.tile((0.2 * rng.standard_normal((RATE, CH))).astype(np.float32), (a.seconds, 1))[None]
    one = ssa.MeterBank(1, CH, RATE)
    times = {"plain": [], "watch": []}
    for _ in range(a.reps + 1):                              # (the first repetition of each grows the staging buffers: dropped)
        for name in ("plain", "watch"):
            if name == "watch":
                one.enable_pair_watch()
            else:
                one.disable_pair_watch()
            one.read()
            t0 = time.perf_counter()
            one.add(long_x)
            one.read()
            times[name].append(time.perf_counter() - t0)
    entries = frames // ((RATE + 5) // 10)
    row = {"probe": "long call", "n": 1, "frames": frames, "seconds_of_input": a.seconds, "entries": entries}
    for name, t in times.items():
        row[name + "_call_ms"] = round(float(np.median(t[1:]) * 1e3), 2)
    row["watch_adds_ms"] = round(row["watch_call_ms"] - row["plain_call_ms"], 2)
    row["watch_us_per_entry"] = round(row["watch_adds_ms"] * 1e3 / entries, 3)
    rec = one.pair_watch()
    assert int(rec[0, 0]["entries"]) == entries and int(rec[0, 0]["total"]["frames"]) == frames
    print(json.dumps(row), flush=True)


def drive(a):
    """every step a fresh process under its own time limit; a failure ends the run"""
    lines = []
    passed = ["--n", str(a.n), "--iters", str(a.iters), "--warmup", str(a.warmup), "--seconds", str(a.seconds), "--reps", str(a.reps)]
    steps = [(name, [sys.executable, os.path.abspath(__file__), "--step", name] + passed) for name in STEPS]
    if a.bench:
        steps.append(("bench", [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]))
    for name, cmd in steps:
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"step {name}: no result within {a.limit} s; nothing more is started")
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"step {name}: exit status {r.returncode}; nothing more is started")
        if name == "bench":                                  # the result line: the step time and the rate alone
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            lines.append(json.dumps({"probe": "bench.py --gpus 1", "value": res.get("value"), "unit": res.get("unit"),
                                     "ms_per_step": res.get("ms_per_step")}))
        else:
            lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--step", choices=STEPS, default=None)
    a = ap.parse_args()
    if a.step == "ticks":
        step_ticks(a)
    elif a.step == "long":
        step_long(a)
    else:
        drive(a)


if __name__ == "__main__":
    main()
