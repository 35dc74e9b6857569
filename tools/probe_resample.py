#!/usr/bin/env python3
"""ss_batch_resample at the bench shape (1024 x 10 s stereo): ms per call of one conversion (--case IN:OUT, default 44100:48000),
beside ss_batch_pair_series (the time to read the corpus once) and ss_batch_peak_series (36 FMAs per input sample against the T per
output here) on the SAME source batch in the same run, each timed before and after the conversion so that a drift of the box shows.
A call is timed with the host clock around REPS calls queued one behind the other and one synchronise; the figure is the median of
WINDOWS such windows with the fastest and the slowest beside it.  Printed: ms per call, output samples/s, FMAs/s against the f32 FMA
rate of profiles/r01_ubench_valu_rates.txt, the ratios to the two yardsticks — per call and, for the peak series, per FMA — and an
order-independent checksum of the result.  `--check` first converts one short ragged batch and compares every output with
ss_resample_host in bits.  With a -DSS_TUNING build of the library (SOUNDSCOPE_HIP_LIB=...) SS_RESAMPLE_FORM=1|2|3 picks the
register-taps, LDS-taps or direct kernel where it can run the plan: one process per form, equal checksums = equal bytes.
`--only` queues nothing but the conversion (for `rocprofv3 --kernel-trace --stats -- python tools/probe_resample.py --only`).
One conversion is one process, fail-fast: the first failure ends it with a non-zero status; the lines go to standard output and,
with `--out FILE`, behind what that file holds.  `--all [--tuning-lib LIB]` is the driver that writes profiles/resample_probe.txt
(or --out): it starts every case of that profile as a fresh child process under a time limit of its own (STEP_LIMIT seconds) — the
release library's two conversions, then, given a -DSS_TUNING build (make -C soundscope_amd/csrc OBJDIR=build_tuning OUT=<LIB>
EXTRA=-DSS_TUNING), the same form by form and 128 streams through the direct form — and stops at the first child that fails or runs
out of time."""
import argparse, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.batch import resample_host, resample_length, resample_plan

REPS, WINDOWS = 20, 9
# f32 fma x8 independent at 4 waves per SIMD: 1.29 ns per wave-instruction per SIMD (profiles/r01_ubench_valu_rates.txt); 1024 SIMDs
VALU_FMAS = 1024 * 64 / 1.29e-9

ap = argparse.ArgumentParser()
ap.add_argument("--case", default="44100:48000")
ap.add_argument("--streams", type=int, default=1024)
ap.add_argument("--seconds", type=int, default=10)
ap.add_argument("--channels", type=int, default=2)
ap.add_argument("--check", action="store_true")
ap.add_argument("--only", action="store_true")
ap.add_argument("--out", default=None, help="append the lines to this file too (profiles/resample_probe.txt)")
ap.add_argument("--all", action="store_true", help="the driver: every case of the profile, a child process and a time limit each")
ap.add_argument("--tuning-lib", default=None, help="with --all: a -DSS_TUNING build of the library, for the form-by-form cases")
args = ap.parse_args()
in_rate, out_rate = (int(v) for v in args.case.split(":"))
plan = resample_plan(in_rate, out_rate)
form = os.environ.get("SS_RESAMPLE_FORM", "auto")


def say(text):
    if args.out:
        say_to(args.out, text)
    else:
        print(text, flush=True)


STEP_LIMIT = 300
HEADER = """tools/probe_resample.py --all on one MI355X: every case below is its own process under its own time limit, one after the other; the
release library first, then a -DSS_TUNING build of the same sources with SS_RESAMPLE_FORM picking the kernel (1 register taps, 2 LDS
taps, 3 direct).  1024 x 10 s stereo (the bench shape) unless a line says otherwise; a call: the median of nine host-clock windows of
20 calls queued one behind the other and one synchronise, with the fastest and the slowest window.  ss_batch_pair_series (the corpus
read once) and ss_batch_peak_series (36 FMAs per input sample) run on the SAME source batch before and after the conversion.  The f32
FMA rate is profiles/r01_ubench_valu_rates.txt's "f32 fma x8 indep" at 4 waves per SIMD: 1.29 ns per wave-instruction per SIMD, 1024
SIMDs, 50.8 T FMAs/s.  Equal checksums are equal bytes, and every `check` line compared seven ragged streams with ss_resample_host
in bits first.
"""


def drive():
    out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_probe.txt")
    with open(out, "w") as f:
        f.write(HEADER)
    steps = [("== release library", None, None, [])]
    steps += [(None, None, None, ["--check", "--case", c]) for c in ("44100:48000", "48000:44100")]
    if args.tuning_lib:
        steps.append(("== SS_TUNING build, form by form (SS_RESAMPLE_FORM: 1 register taps, 2 LDS taps, 3 direct)", None, None, []))
        steps += [(None, args.tuning_lib, f, ["--check", "--case", c]) for c in ("44100:48000", "48000:44100") for f in ("1", "2")]
        steps.append(("== 128 streams: the direct form beside the register form", None, None, []))
        steps += [(None, args.tuning_lib, f, ["--check", "--case", "44100:48000", "--streams", "128"]) for f in ("1", "3")]
    for title, lib, form, argv in steps:
        if title:
            say_to(out, "\n" + title)
            continue
        env = dict(os.environ)
        if lib:
            env.update(SOUNDSCOPE_HIP_LIB=os.path.abspath(lib), SS_RESAMPLE_FORM=form)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out] + argv, env=env, timeout=STEP_LIMIT).returncode
        except subprocess.TimeoutExpired:
            sys.exit("a case ran past its %d s: nothing more is started" % STEP_LIMIT)
        if rc:
            sys.exit("a case ended with status %d: nothing more is started" % rc)


def say_to(path, text):
    print(text, flush=True)
    with open(path, "a") as f:
        f.write(text + "\n")


if args.all:
    drive()
    sys.exit(0)


def timed(sync, enqueue):
    for _ in range(3):
        enqueue()
    sync()
    ms = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            enqueue()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3 / REPS)
    return statistics.median(ms), min(ms), max(ms)


def word_sum(batch, frames_out):
    """an order-independent checksum of every stream's outputs: the sum of their bit patterns, modulo 2^64"""
    total = 0
    for s in range(0, int(batch.cfg.n_streams), max(1, int(batch.cfg.n_streams) // 16)):
        total += int(batch.download_input(s)[:frames_out * int(batch.cfg.channels)].view(np.uint32).astype(np.uint64).sum())
    return total & 0xFFFFFFFFFFFFFFFF


if args.check:
    rng = np.random.default_rng(1)
    probe = ssa.Batch(in_rate, args.channels, 1, 1, flags=L.SS_BATCH_TRUE_PEAK)
    tile_out, tile_in = probe.resample_tiles(plan)
    probe.close()
    lengths = [0, 1, int(plan.taps) // 2, tile_in - 1, tile_in, tile_in + 1, 2 * tile_in + 71]
    fps = max(lengths) | 1
    x = (0.3 * rng.standard_normal((len(lengths), fps, args.channels))).astype(np.float32)
    src = ssa.Batch(in_rate, args.channels, len(lengths), fps, flags=L.SS_BATCH_TRUE_PEAK)
    src.upload(0, x)
    src.set_lengths(lengths)
    dst = src.resample(out_rate)
    for s, F in enumerate(lengths):
        got = dst.download_input(s).reshape(-1, args.channels)[:resample_length(plan, F)]
        ref = resample_host(plan, x[s, :F], args.channels)
        if got.tobytes() != ref.tobytes():
            sys.exit(f"form {form}: stream {s} of {F} frames differs from ss_resample_host")
    say(f"check: {in_rate} -> {out_rate}, {args.channels} channels, form {form}, tiles of {tile_out} outputs from {tile_in} inputs: "
          f"{len(lengths)} ragged streams equal ss_resample_host in bits")
    src.close()
    dst.close()

frames = in_rate * args.seconds
src = ssa.Batch(in_rate, args.channels, args.streams, frames, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
src.synthesize(0x5EED0000, 0)
src.sync()
frames_out = resample_length(plan, frames)
dst = ssa.Batch(out_rate, args.channels, args.streams, frames_out, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)
convert = lambda: src.resample_into(dst, plan)
if args.only:
    for _ in range(REPS + 3):
        convert()
    dst.sync()
    sys.exit(0)
tile_out, tile_in = src.resample_tiles(plan)
samples_out = args.streams * frames_out * args.channels
samples_in = args.streams * frames * args.channels
say(f"{in_rate} -> {out_rate}: L / M = {plan.up} / {plan.down}, T = {plan.taps}; {args.streams} x {frames} frames x {args.channels} "
      f"channels in, {frames_out} frames out; form {form}, tiles of {tile_out} outputs from {tile_in} inputs; {WINDOWS} windows of "
      f"{REPS} calls each: median (fastest .. slowest)")


def line(name, t):
    say(f"    {name:<44s}{t[0]:8.4f} ms per call ({t[1]:.4f} .. {t[2]:.4f})")
    return t[0]


pair0 = line("pair_series, default pair (yardstick)", timed(src.sync, src.pair_series))
peak0 = line("peak_series (yardstick)", timed(src.sync, src.peak_series))
t = line("resample_into", timed(dst.sync, convert))
peak1 = line("peak_series (again)", timed(src.sync, src.peak_series))
pair1 = line("pair_series, default pair (again)", timed(src.sync, src.pair_series))
fmas = samples_out * int(plan.taps)
peak, pair = 0.5 * (peak0 + peak1), 0.5 * (pair0 + pair1)
per_fma = (t / fmas) / (peak / (36.0 * samples_in))
say(f"    {samples_out / t / 1e6:.1f} G output samples/s; {fmas / t / 1e9:.2f} T FMAs/s = {fmas / t * 1e3 / VALU_FMAS:.3f} of the f32 FMA rate "
      f"({VALU_FMAS / 1e12:.1f} T/s); {t / pair:.2f} x the pair series, {t / peak:.2f} x the peak series per call, {per_fma:.2f} x per FMA "
      f"(36 per input sample there, {plan.taps} per output here)")
say(f"    checksum of every {max(1, args.streams // 16)}th stream's outputs: {word_sum(dst, frames_out):016x}")
src.close()
dst.close()
