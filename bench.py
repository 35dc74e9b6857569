#!/usr/bin/env python3
"""bench.py — throughput of the soundscope analyzer hot path on MI355X.  No PyTorch anywhere.

One step = one pass of the whole hot path (mid/side 4096-pt Hann FFT spectrum at hop 1024,
K-weighted gated loudness + LRA, 4x true peak at the reference's f32 width, min-max decimation) over a batch of synthetic
48 kHz stereo f32 streams already resident in HBM, followed by the corpus gate (one RCCL
all-reduce of the 2x1000-bin u64 histograms when N > 1, issued by the C-ABI library itself).

  N = 1 : BASELINE config 3 — 1024 streams x 10 s on the GPU.
  N > 1 : BASELINE config 4 — 8192 streams IN TOTAL sharded over the ranks (strong scaling);
          `--scaling weak` keeps `--streams` per GPU instead.

Launch:  python bench.py --gpus 1 --steps K --warmup W            (plain run)
         python bench.py --gpus 1 --steps K --warmup W --full     (plain run + every other leg)
         python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...
         (torchrun is only the process launcher: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT)
Prints ONE JSON line on rank 0.

A plain run does what the headline needs and no more: set-up, W warm-up steps, the K timed steps (with the per-kernel HIP
events that ride inside them), --dump-outputs, the line.  `--full` adds, around the very same timed steps, everything else
the line can carry: the spectrum kernel's traffic floor, the host copy of the corpus gate, the sustained run, the f16x3
true-peak leg and both modes' errors against an f64 convolution, an overlap mode's separate per-kernel pass, the
PCIe-inclusive rates, the CPU baseline with its parity check (--no-cpu skips it) and the other configurations
(--no-extra skips them).  The entries of the line that only `--full` measures are null, or absent, in a plain run.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

# the host driver only supports dmabuf IPC: RCCL across processes needs this (inherited on the GPU boxes; set if missing)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
# one node: RCCL's bootstrap needs nothing but loopback (the container's other interfaces / hostname may not be usable);
# the data path between the GPUs is xGMI peer-to-peer either way.  An exported value wins.
if int(os.environ.get("WORLD_SIZE", "1")) > 1:
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0         # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP32_VECTOR_PEAK_TFLOPS = 157.3
LDS_PEAK_GBS = 256 * 128 * 2.4   # 256 CUs x 128 B/clk x 2.4 GHz
CONFIG4_TOTAL_STREAMS = 8192


def cgroup_cpu_quota():
    """CPUs the container may actually use (cgroup v2 cpu.max or v1 cfs quota / period), or None if unlimited / unknown:
    sched_getaffinity lists every host core even where the container runs under a quota of a few CPUs' worth of time."""
    try:
        txt = open("/sys/fs/cgroup/cpu.max").read().split()
        if txt and txt[0] != "max":
            return float(txt[0]) / float(txt[1])
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0 and per > 0:
            return q / per
    except Exception:
        pass
    return None


def cpu_baseline(batch, rate, fft_n, hop, budget_s=15.0, all_cores_budget_s=8.0):
    """The CPU leg: times the CPU restatement (oracle, kind 'port') on a bounded sample of the same streams and —
    with the oracle's outputs for the first sampled stream in hand — checks the GPU results of the timed run
    against them (so a driver-run number is never unaccompanied by a parity check)."""
    from oracle import pyoracle as po
    native = True
    try:
        po.build(native=True)
        po.lib(native=True)
    except Exception:
        native = False
    if native:      # keep whichever build is faster on this host (AVX-512 codegen can lose)
        x0 = batch.download_input(0)
        tt = []
        for nat in (False, True):
            t0 = time.perf_counter()
            po.analyze_stream(rate, x0, fft_n, hop, native=nat)
            tt.append(time.perf_counter() - t0)
        native = tt[1] < tt[0]
    n_streams = int(batch.cfg.n_streams)
    done, samples, t_used = 0, 0, 0.0
    check = None
    while done < n_streams and t_used < budget_s:
        x = batch.download_input(done)
        t0 = time.perf_counter()
        ref = po.analyze_stream(rate, x, fft_n, hop, want_fft=True, want_wave=True, native=False if done == 0 else native)
        if done != 0:
            t_used += time.perf_counter() - t0
            samples += x.size
        else:       # stream 0: the parity check (strict-FP build of the oracle), not part of the timing
            check = self_check(batch, 0, ref)
        done += 1
    out = {"value": samples / t_used, "unit": "samples/s", "cores": 1, "kind": "port",
           "sample": f"{done - 1} of the batch's streams ({samples} samples), single thread, "
                     f"gcc -O3{' -march=native' if native else ''}, full analyze_stream pass "
                     "(waveform + mid/side + 2 FFTs/window incl. the crate's stats sorts + meter with true peak)"}
    # the same pass on every host core: POSIX threads INSIDE the oracle library, streams dealt round-robin,
    # eight whole stream passes per core, the clock started and stopped in C — no Python, no pool start-up in the timed
    # region.  Informational: the reference itself is single-threaded (main.rs:67).
    try:
        affinity = len(os.sched_getaffinity(0))
        quota = cgroup_cpu_quota()
        cores = affinity if quota is None else max(1, min(affinity, int(math.ceil(quota))))     # threads beyond the quota only time-slice
        distinct = min(n_streams, 64, 2 * cores)
        xs = np.stack([batch.download_input(i) for i in range(distinct)])
        # calibration (also pages the library in): one stream pass per thread.  If that takes much longer than one pass takes
        # alone, the threads are not running side by side (a CPU quota this process cannot read, SMT siblings): continue
        # with as many threads as the measured parallelism supports.
        t1 = samples / t_used and (xs.shape[1] / (samples / t_used))                       # seconds of one pass on one thread
        dcal = po.analyze_streams_all_cores(rate, xs[:min(distinct, cores)], cores, fft_n, hop, cores, 1, native=native)
        par = cores * t1 / dcal if dcal > 0 else cores
        if par < 0.6 * cores:
            cores = max(1, int(round(par)))
        n_mt, reps = 2 * cores, 4
        dt = po.analyze_streams_all_cores(rate, xs, n_mt, fft_n, hop, cores, reps, native=native)
        out["all_cores"] = {"value": n_mt * reps * xs.shape[1] / dt, "cores": cores, "affinity_cores": affinity, "cgroup_cpu_quota": quota, "measured_parallelism": round(par, 1),
                            "stream_passes": n_mt * reps, "seconds": dt,
                            "how": "pthread workers inside oracle/libss_oracle (so_analyze_streams_mt), timed in C; one thread per CPU "
                                   "the container may use (cgroup quota), not per core the host lists"}
    except Exception as e:            # never let the informational leg break the bench line
        out["all_cores"] = {"error": str(e)}
    return out, check


def gpu_sclk_mhz(dev=0):
    """Current shader clock of GPU `dev` as rocm-smi reports it ("sclk clock level: 1: (2034Mhz)"), or None where it cannot be
    read.  (sysfs lists every card of the host, visible or not: rocm-smi numbers the visible ones.)  About 0.3 s per call."""
    try:
        import re
        import subprocess
        txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        for line in txt.splitlines():
            m = re.search(r"GPU\[(\d+)\]\s*:\s*sclk clock level:\s*\S+\s*\((\d+)\s*[Mm][Hh]z\)", line)
            if m and int(m.group(1)) == dev:
                return int(m.group(2))
    except Exception:
        pass
    return None


def interpolator_taps_f64(factor):
    """ebur128's 49-tap Hann-windowed sinc (kept as f32 by the crate), as f64 — restated from the published design, SURVEY A5."""
    j = np.arange(49, dtype=np.float64)
    m = j - 24.0
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(np.abs(m) > 1e-6, np.sin(m * np.pi / factor) / (m * np.pi / factor), 1.0)
    c *= 0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0))
    return c.astype(np.float32).astype(np.float64)


def self_check(batch, stream, ref):
    """GPU results of the run just timed vs the oracle's for one stream, at the north_star tolerances."""
    got = batch.fft(stream)
    r = batch.results()[stream]
    # per window row, relative to the row's own loudest bin (an f32 transform's error is scale-invariant): 0.01 dB down to
    # 70 dB under it, 1e-4 of its amplitude below that
    rf = ref["fft"].astype(np.float64)
    peak = rf.max(axis=2, keepdims=True)
    strong = rf >= peak - 70.0
    d = np.abs(got - rf)
    fft_err = float(d[strong].max()) if strong.any() else 0.0
    lin = np.abs(10.0 ** ((got - peak) / 20.0) - 10.0 ** ((rf - peak) / 20.0))
    weak_err = float(lin[~strong].max()) if (~strong).any() else 0.0
    # SURVEY section 7's wording of the same bar, kept beside it (the key of rounds 1-2): 0.01 dB wherever the oracle's bin is
    # >= -90 dBFS, 1e-4 of the row's largest amplitude below
    loud = rf >= -90.0
    abs_err = float(d[loud].max()) if loud.any() else 0.0
    abs_weak = float(lin[~loud].max()) if (~loud).any() else 0.0
    lufs_err = abs(r.integrated_lufs - ref["integrated"]) if math.isfinite(ref["integrated"]) else (0.0 if r.integrated_lufs == ref["integrated"] else float("inf"))
    lra_err = abs(r.loudness_range - ref["lra"])
    tp_rel = max(abs(r.true_peak[c] - ref["true_peak"][c]) / max(ref["true_peak"][c], 1e-30) for c in range(2))
    wave_ok = bool(np.array_equal(batch.waveform(stream).reshape(-1), ref["wave"][:, 1].astype(np.float32)))
    survey_ok = abs_err <= 0.01 and abs_weak <= 1e-4
    ok = fft_err <= 0.01 and weak_err <= 1e-4 and survey_ok and lufs_err <= 0.01 and lra_err <= 0.01 and tp_rel <= 1e-4 and wave_ok
    return {"stream": stream, "windows": int(got.shape[0]), "fft_max_err_db_within_70dB_of_row_peak": fft_err,
            "fft_max_err_rel_to_row_peak_below": weak_err, "fft_max_err_db_above_-90dB": abs_err,
            "fft_max_err_rel_to_row_peak_below_-90dB": abs_weak, "survey_metric_ok": bool(survey_ok), "integrated_err_lu": lufs_err, "lra_err_lu": lra_err,
            "true_peak_rel_err": tp_rel, "decimation_bit_exact": wave_ok, "ok": bool(ok)}


DUMP_MAX_BYTES = 64 * 10**6
DUMP_STREAMS = 64
# bytes per kind; a kind that would exceed its share keeps a seeded sample of its rows (windows, decimation bins, sub-blocks, streams)
DUMP_BUDGET = {"spectrum": 32 * 10**6, "waveform": 12 * 10**6, "subblocks": 8 * 10**6, "results": 4 * 10**6}


def dump_outputs(b, first, corpus, path):
    """--dump-outputs: what the last timed step left in the batch, as a caller of the path receives it, written as float32 /
    float64 .npy files under `path` (this rank's shard).  The sample is drawn with a fixed seed from the shapes alone, so the
    same arguments select the same rows in every run and every build.  Files (the *_index / streams arrays hold positions):
      streams            [S]                 global ids of the sampled streams (at most 64)
      spectrum           [S, w, 2, bins] f32 dB rows of the sampled windows (Batch.fft), spectrum_windows [w]
      waveform           [S, p, 2] f32       (min, max) of the sampled decimation bins (Batch.waveform), waveform_bins [p]
      subblocks          [S, q, channels] f64 K-weighted 100 ms sub-block energies (Batch.subblocks), subblocks_index [q]
      results            [r, 8] f64          per stream: integrated LUFS, LRA, true peak L/R, sample peak L/R, gating blocks,
                                             short-term blocks (Batch.results), results_streams [r] global ids
      histograms         [2, 1000] f64       the corpus histograms (block, short-term) the gate read
      corpus_gate        [2] f64             corpus integrated LUFS and LRA"""
    rng = np.random.default_rng(0x5EED)
    lay, count = b.layout, int(b.cfg.n_streams)

    def pick(n, k):                                    # sorted seeded sample of k of range(n), or all of it
        return np.arange(n) if k >= n else np.sort(rng.choice(n, k, replace=False))

    def rows(kind, row_bytes):                         # rows that fit the kind's budget, each with its f64 index entry
        return max(1, DUMP_BUDGET[kind] // (row_bytes + 8))

    streams = pick(count, DUMP_STREAMS)
    S = streams.size
    win = pick(lay.n_windows, rows("spectrum", S * lay.fft_channels * lay.n_bins * 4))
    wbin = pick(lay.n_wave_points // 2, rows("waveform", S * 2 * 4))
    sub = pick(lay.n_subblocks, rows("subblocks", S * int(b.cfg.channels) * 8))
    rstreams = pick(count, rows("results", 8 * 8))
    res = b.results()
    out = {
        "streams": (first + streams).astype(np.float64),
        "spectrum": np.stack([b.fft(int(s))[win] for s in streams]).astype(np.float32),
        "spectrum_windows": win.astype(np.float64),
        "waveform": np.stack([b.waveform(int(s))[wbin] for s in streams]).astype(np.float32),
        "waveform_bins": wbin.astype(np.float64),
        "subblocks": np.stack([b.subblocks(int(s))[sub] for s in streams]).astype(np.float64),
        "subblocks_index": sub.astype(np.float64),
        "results": np.array([[res[s].integrated_lufs, res[s].loudness_range, res[s].true_peak[0], res[s].true_peak[1],
                              res[s].sample_peak[0], res[s].sample_peak[1], res[s].n_gating_blocks, res[s].n_st_blocks]
                             for s in rstreams], np.float64).reshape(-1, 8),
        "results_streams": (first + rstreams).astype(np.float64),
        "histograms": np.stack(b.histograms()).astype(np.float64),
        "corpus_gate": np.array(corpus, np.float64),
    }
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES} byte cap")
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return len(out), total


def reference_tick_workload(ssa, L, rate=48000, secs=12, cpu_ticks=60):
    """The reference's OWN workload, one file and one tick at a time, beside the CPU oracle driven the same way:
      tick  = analyze_audio_file_samples (tui.rs:1482-1552): get_fft(mid) + get_fft(side) on the last 16384 frames, add_samples of the
              last 16384 interleaved samples, get_shortterm_lufs — every 1024 frames (2048 interleaved samples, audio_player.rs:65);
      open  = receive_audio_file (tui.rs:1207-1241): whole-file get_waveform + calculate_integrated_lufs (+ the upload to HBM here)."""
    from oracle import app_driver
    out = {"workload": f"reference tick: 1 stream x {secs} s, {rate} Hz stereo, N = 16384 mid + side, 16384-sample LUFS refeed, every 1024 frames "
                       "(ss_session_tick_file, wall clock of the C call incl. its read-backs) and receive_audio_file (ss_session_open_file)"}
    frames = rate * secs
    b = ssa.Batch(rate, 2, 1, frames, 4096, 1024, flags=L.SS_BATCH_LUFS)
    b.synthesize(0x5EED0000, 0)
    x = b.download_input(0)
    b.close()
    t0 = time.perf_counter(); sess = ssa.FileSession(x, 2, rate); open_ms = (time.perf_counter() - t0) * 1e3
    warm = []                                                # tables and buffers warm: three more opens of the same file
    for _ in range(3):
        t0 = time.perf_counter(); sess2 = ssa.FileSession(x, 2, rate); warm.append((time.perf_counter() - t0) * 1e3)
        sess2.close()
    open2_ms = float(np.median(warm))
    positions = list(range(16384 * 2 + 2048, x.size + 1, 2048))
    ticks = []
    check_at = {19 + cpu_ticks // 2: None, 19 + cpu_ticks: None}       # ticks whose results are compared with the CPU driver's
    for k, pos in enumerate(positions):
        t0 = time.perf_counter()
        sess.analyze_audio_file_samples(pos)
        t1 = time.perf_counter()
        if k >= 20:
            ticks.append((t1 - t0) * 1e6)
        if k in check_at:
            check_at[k] = (sess.mid_fft.copy(), sess.side_fft.copy(), float(sess.lufs[299]))
        # (the reference's ticks are 21.3 ms apart; each leaves work behind its results — the gating of the new sub-blocks, the
        # readings the render loop will ask for — that a call issued the very next microsecond would queue behind)
        time.sleep(0.0003)
    # ... and 60 ticks at the reference's own cadence (1024 frames = 21.3 ms between ticks at 48 kHz: clocks and caches go idle)
    slow = []
    for pos in positions[len(positions) // 2:len(positions) // 2 + 60]:
        t0 = time.perf_counter()
        sess.analyze_audio_file_samples(pos)
        slow.append((time.perf_counter() - t0) * 1e6)
        time.sleep(1024.0 / rate)
    sess.close()
    t0 = time.perf_counter(); app = app_driver.FileApp(x, 2, rate); cpu_open_ms = (time.perf_counter() - t0) * 1e3
    cpu = []
    worst_db, worst_lu, compared = 0.0, 0.0, 0
    for k, pos in enumerate(positions[:20 + cpu_ticks]):
        t0 = time.perf_counter()
        app.analyze_audio_file_samples(pos)
        cpu.append((time.perf_counter() - t0) * 1e6)
        if check_at.get(k) is not None:
            gm, gs, gst = check_at[k]
            for got, want in ((gm, app.mid_fft), (gs, app.side_fft)):
                if got.shape == want.shape and want.shape[0] > 1:
                    near = want[:, 1] >= want[:, 1].max() - 70.0                 # (the bar's range: within 70 dB of the row's peak)
                    worst_db = max(worst_db, float(np.max(np.abs(got[near, 1] - want[near, 1]))))
                else:
                    worst_db = float("inf")
            worst_lu = max(worst_lu, abs(gst - float(app.lufs[299])))
            compared += 1
    out["tick_check_vs_cpu_driver"] = {"ticks_compared": compared, "spectrum_max_err_db": worst_db, "shortterm_err_lu": worst_lu,
                                       "ok": bool(compared > 0 and worst_db <= 0.01 and worst_lu <= 0.01)}
    out["gpu_tick_us"] = {"median": float(np.median(ticks)), "p99": float(np.percentile(ticks, 99)), "ticks": len(ticks),
                          "pause_between_ticks_ms": 0.3,
                          "at_reference_cadence": {"median": float(np.median(slow)), "p90": float(np.percentile(slow, 90)), "ticks": len(slow),
                                                   "pause_between_ticks_ms": round(1024.0 / rate * 1e3, 1)}}
    out["cpu_oracle_tick_us"] = {"median": float(np.median(cpu[20:])), "ticks": len(cpu) - 20, "cores": 1,
                                 "what": "oracle/app_driver.FileApp (the C restatement behind the same driver rules), 1 thread"}
    out["file_open_ms"] = {"gpu_first": open_ms, "gpu_warm": open2_ms, "gpu_warm_each": [round(v, 2) for v in warm], "cpu_oracle": cpu_open_ms,
                           "seconds": secs}
    out["budget"] = "8 ms TUI loop + 21.3 ms between ticks at 48 kHz (SURVEY section 6)"
    # the microphone mode: analyze_microphone_input (tui.rs:1427-1480) on the 30 * rate-sample capture ring — as a snapshot per tick
    # (the reference's to_vec()), and with the ring kept on the device (the capture callback pushes 1024 frames per tick)
    try:
        ring = np.concatenate([x, x, x])[:30 * rate].copy()
        cap = ssa.CaptureSession(2, rate)
        t_snap, t_res = [], []
        for k in range(50):
            t0 = time.perf_counter(); cap.analyze_microphone_input(ring); t1 = time.perf_counter()
            if k >= 10: t_snap.append((t1 - t0) * 1e6)
            time.sleep(0.0003)
        for k in range(110):
            cap.push(x[2048 * k:2048 * (k + 1)])
            t0 = time.perf_counter(); cap.analyze_resident(); t1 = time.perf_counter()
            if k >= 10: t_res.append((t1 - t0) * 1e6)
            time.sleep(0.0003)
        capp = app_driver.CaptureApp(2, rate)
        t_cpu = []
        for k in range(6):
            t0 = time.perf_counter(); capp.analyze_microphone_input(ring); t_cpu.append((time.perf_counter() - t0) * 1e6)
        out["capture_tick_us"] = {"snapshot_per_tick": float(np.median(t_snap)), "ring_resident_on_device": float(np.median(t_res)),
                                  "cpu_oracle": float(np.median(t_cpu[1:])), "snapshot_bytes": int(ring.nbytes)}
        cap.close()
    except Exception as ex:
        out["capture_tick_us"] = {"error": repr(ex)}
    # the long file: receive_audio_file only (600 s = 57.6 M samples)
    try:
        long_s = 600
        bl = ssa.Batch(rate, 2, 1, rate * long_s, 4096, 1024, flags=L.SS_BATCH_LUFS)
        bl.synthesize(0x5EED0001, 0)
        xl = bl.download_input(0)
        bl.close()
        t0 = time.perf_counter(); sl = ssa.FileSession(xl, 2, rate); long_ms = (time.perf_counter() - t0) * 1e3
        sl.close()
        t0 = time.perf_counter(); app_driver.FileApp(xl, 2, rate); long_cpu_ms = (time.perf_counter() - t0) * 1e3
        out["file_open_ms_600s"] = {"gpu": long_ms, "cpu_oracle": long_cpu_ms, "h2d_bytes": int(xl.nbytes)}
    except Exception as ex:
        out["file_open_ms_600s"] = {"error": repr(ex)}
    return out


def time_config(ssa, L, rate, channels, streams, frames, fft_n, hop, tp_factor, steps, warmup=1, flags=None, tp_arith=None, cols=0):
    """Per-kernel HIP-event times of one extra BASELINE configuration (informational lines under config.extra)."""
    b = ssa.Batch(rate, channels, streams, frames, fft_n, hop, flags=L.SS_BATCH_ALL if flags is None else flags, true_peak_factor=tp_factor,
                  spectrum_columns=cols)
    b.synthesize(0x5EED0000, 0)
    if tp_arith is not None:
        b.set_true_peak_arith(tp_arith)
    for _ in range(warmup):
        b.run(); b.sync()
    # wall clock of a pass as a caller sees it (run + sync, no event recording), then the same passes with per-kernel events
    nwall = max(steps, 20 if streams * frames <= 48000 * 60 else steps)
    t0 = time.perf_counter()
    for _ in range(nwall):
        b.run(); b.sync()
    wall_ms = (time.perf_counter() - t0) / nwall * 1e3
    b.timing_enable(True)
    for _ in range(steps):
        b.run(); b.sync()
    kern = {}
    for k in range(L.SS_KERNEL_COUNT):
        ms, n = b.timing_read(k)
        kern[L.lib().ss_batch_kernel_name(b._h, k).decode()] = round(ms / max(n, 1), 4)
    lay, geo = b.layout, b.geometry
    fft_ms = b.timing_read(L.SS_KERNEL_FFT)[0] / steps
    td_ms = b.timing_read(L.SS_KERNEL_TIME_DOMAIN)[0] / steps
    gpu_ms = sum(kern.values())
    samples = streams * frames * channels
    in_bytes = samples * 4
    out_bytes = streams * lay.n_windows * lay.fft_channels * (cols if cols else lay.n_bins) * 4
    res = {"ms_per_pass_wall": round(wall_ms, 4), "kernel_ms": kern, "gpu_ms": round(gpu_ms, 4),
           "samples_per_s": samples / (gpu_ms * 1e-3) if gpu_ms > 0 else None,
           "windows_per_stream": lay.n_windows, "fft_channels": lay.fft_channels, "bins": lay.n_bins,
           "geometry": {"fft_windows_per_block": geo.fft_windows_per_block, "fft_blocks": geo.fft_blocks,
                        "td_segments": geo.td_segments, "true_peak_factor": geo.td_true_peak_factor}}
    if fft_ms > 0:
        alg = in_bytes + out_bytes
        flops = 5.0 * fft_n * math.log2(fft_n) * streams * lay.n_windows * (1 if (channels == 2 and fft_n == 4096) else lay.fft_channels)
        res["spectrum_kernel"] = {"algorithmic_bytes": alg, "hbm_frac": alg / (fft_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                  "algorithmic_flops": flops, "fp32_frac": flops / (fft_ms * 1e-3) / 1e12 / FP32_VECTOR_PEAK_TFLOPS}
        if fft_n == 16384 and hop == 1024:
            # what k_fft16k_run executes per real window: two complex 4096-point transforms (the real 16384-point transform as a
            # decimation in time by four, two halves packed), the Hann weights, and per retained bin the four-term recombination
            # and the dB conversion (~30 flops) — about half of the nominal 5 N log2 N
            executed = (2 * 5.0 * 4096 * 12 + 3.0 * fft_n + 30.0 * lay.n_bins) * streams * lay.n_windows * lay.fft_channels
            res["spectrum_kernel"]["executed_flops"] = executed
            res["spectrum_kernel"]["fp32_frac_executed"] = executed / (fft_ms * 1e-3) / 1e12 / FP32_VECTOR_PEAK_TFLOPS
            # k_fft16k_run moves, per window and channel, 2 halves x (3 exchanges written + read) of 4096 complex f32
            # plus the 4 KB dB staging row: the design's LDS traffic against 128 B/clk/CU
            lds = streams * lay.n_windows * lay.fft_channels * (2 * 3 * 2 * 4096 * 8 + 2 * 4 * lay.n_bins)
            res["spectrum_kernel"]["lds_bytes_by_design"] = lds
            res["spectrum_kernel"]["lds_frac"] = lds / (fft_ms * 1e-3) / 1e9 / LDS_PEAK_GBS
    if td_ms > 0:
        res["time_domain_kernel"] = {"algorithmic_bytes": in_bytes, "hbm_frac": in_bytes / (td_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    b.close()
    return res


def arg_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed passes (default: a timed region of about 1 s)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--streams", type=int, default=1024, help="streams per GPU (config 3; weak scaling)")
    ap.add_argument("--scaling", choices=["auto", "weak", "strong"], default="auto",
                    help="auto: config 3 on one GPU, config 4 (8192 streams in total, strong scaling) on several")
    ap.add_argument("--total-streams", type=int, default=0, help="strong scaling with this many streams in total")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--fft-n", type=int, default=4096)
    ap.add_argument("--hop", type=int, default=1024)
    ap.add_argument("--sequential", action="store_true", help="(the default) spectrum kernel, then the time-domain chain, on one stream")
    ap.add_argument("--overlap", type=int, default=0, choices=[0, 1, 2],
                    help="ss_batch_set_overlap mode: 0 (default) sequential; 1 = spectrum kernel beside the whole time-domain chain; "
                         "2 = beside its tail only.  Measured step times are equal within 1 %% (DESIGN section 4), so the simplest one is timed")
    ap.add_argument("--allow-host-fallback", action="store_true",
                    help="N > 1: if the RCCL communicator cannot be created, stage the 16 kB exchange through host memory instead of failing "
                         "(the JSON says which transport ran).  Without this flag a failed RCCL setup ends the run non-zero.")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline, measure and check everything else the line can carry (traffic floor, host copy of the "
                         "corpus gate, sustained run, f16x3 true-peak leg, PCIe-inclusive rates, CPU baseline and parity check, the "
                         "other configurations); off by default: a plain run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline leg (and its parity check)")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the config 2 / config 5 lines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (a fixed seeded sample, at most 64 MB) as "
                         "DIR/<name>.npy, float32 / float64 (rank 0's shard); see dump_outputs")
    return ap


def main():
    ap = arg_parser()
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # stdout carries exactly ONE line (the JSON): native libraries print to file descriptor 1 on their own (RCCL's
    # version banner at communicator creation), so everything but the final line is sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import soundscope_amd as ssa
    from soundscope_amd import _lib as L
    from soundscope_amd.distributed import Comm, corpus_gate, shard_streams

    lib = L.lib()
    if lib.ss_device_count() <= 0:
        raise SystemExit("bench.py needs a GPU (soundscope_amd has no CPU path)")
    # SS_BENCH_SHARED_GPU=1 + SS_BENCH_TRANSPORT=host-tcp: launch-path check on a 1-GPU box (all ranks on device 0,
    # the 16 kB exchange staged through host memory); the judged runs use one GPU per rank and RCCL
    transport = os.environ.get("SS_BENCH_TRANSPORT", "rccl")
    dev = 0 if os.environ.get("SS_BENCH_SHARED_GPU") == "1" else local_rank
    if lib.ss_set_device(dev):
        raise SystemExit("ss_set_device failed: " + lib.ss_last_device_error().decode())
    comm = None
    if world > 1:
        os.environ["SS_COMM_DEVICE"] = str(dev)   # the communicator's GPU = this rank's GPU (LOCAL_RANK, or 0 in the shared-GPU launch check)
        # The ranks must agree on the transport BEFORE using it.  With --allow-host-fallback every rank first joins a host-TCP
        # control communicator, tries RCCL (the library makes ncclCommInitRank all-or-nothing across ranks and bounds it with
        # a watchdog), and the ranks then sum their verdicts over the control channel: RCCL is used only if every rank has
        # it.  Without the flag a rank that cannot create the RCCL communicator ends the run non-zero.
        ctrl = None
        if args.allow_host_fallback and transport == "rccl":
            os.environ["SS_COMM_FILE"] = f"/tmp/ss_comm_ctrl_{os.getppid()}_{os.environ.get('MASTER_PORT', '0')}.rdzv"
            ctrl = Comm.from_env("host-tcp")
            os.environ.pop("SS_COMM_FILE")
        err = None
        try:
            comm = Comm.from_env(transport)       # RCCL: ncclCommInitRank inside the library
            comm.barrier()                        # proves the communicator before anything is timed
        except Exception as e:                    # noqa: BLE001
            err, comm = e, None
        if ctrl is not None:
            n_bad = int(ctrl.allreduce_sum_u64(np.array([0 if err is None else 1], np.uint64))[0])
            if n_bad:
                print(f"[bench] rank {rank}: {transport} unavailable on {n_bad} rank(s) ({err}); all ranks use host-tcp", file=sys.stderr, flush=True)
                if comm is not None:
                    comm.close()
                comm = ctrl
            else:
                ctrl.close()
        elif err is not None:
            print(f"[bench] rank {rank}: {transport} communicator failed: {err} (--allow-host-fallback would stage the exchange "
                  "through host memory)", file=sys.stderr, flush=True)
            sys.exit(3)
        if comm.size != world:
            raise SystemExit(f"communicator reports {comm.size} ranks, expected {world}")
        print(f"[bench] rank {rank}/{world}: collective = {comm.transport}, {comm.size} ranks", file=sys.stderr, flush=True)

    frames = int(round(args.seconds * args.rate))
    strong = args.scaling == "strong" or args.total_streams > 0 or (args.scaling == "auto" and world > 1)
    total_streams = (args.total_streams or CONFIG4_TOTAL_STREAMS) if strong else args.streams * world
    first, count = shard_streams(total_streams, rank, world)
    b = ssa.Batch(args.rate, 2, count, frames, args.fft_n, args.hop, flags=L.SS_BATCH_ALL)
    b.synthesize(0x5EED0000, first)
    lay = b.layout
    ov_mode = 0 if args.sequential else args.overlap
    b.set_overlap(ov_mode)
    hist = [None]
    # the memory system's floor for the spectrum kernel's access pattern on THIS box: its loads and stores alone, same
    # grid / occupancy / addresses, no arithmetic (overwrites the spectra, so it runs before anything is computed)
    io_floor_ms = None
    if args.full and rank == 0:
        try:
            io_floor_ms = b.traffic_floor(5)
        except Exception:
            io_floor_ms = None

    def step():
        # one pass + the corpus gate, all queued on the device: [ncclAllReduce of the 2 x 1000 u64 histograms in place on
        # the batch's stream when N > 1] + gate / LRA of the summed histograms.  No host synchronisation per step.
        b.run()
        b.corpus_gate_enqueue(comm)

    def fence():
        lib.ss_device_synchronize()
        if comm is not None:
            comm.barrier()
        lib.ss_device_synchronize()

    # Per-kernel HIP events INSIDE the timed region (sequential mode: ss_batch_timing_enable records an event pair around every
    # kernel on the batch's own stream into a ring of 32 passes' event sets — no host synchronisation between passes, the ring
    # is read behind the fence; a K beyond the ring collects every 32 passes).  roofline.achieved is the spectrum kernel's
    # average duration over exactly these K steps.  (Overlap modes: a per-kernel time would not describe either of two kernels
    # sharing the chip — there the kernels are timed in a separate sequential pass further down.)
    timed_in_region = ov_mode == 0
    for _ in range(args.warmup):
        step()
    fence()
    region0 = None
    if timed_in_region:
        b.timing_enable(True)
        region0 = [b.timing_read(k) for k in range(L.SS_KERNEL_COUNT)]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    region = None
    if timed_in_region:
        region = [tuple(a - b0 for a, b0 in zip(b.timing_read(k), region0[k])) for k in range(L.SS_KERNEL_COUNT)]
        b.timing_enable(False)
    if comm is not None:
        dt = float(comm.allreduce_max_f64(np.array([dt]))[0])
    b.sync()

    samples_per_step = total_streams * frames * 2
    value = samples_per_step * args.steps / dt
    corpus_i, corpus_lra = b.corpus_gate_read()                 # what the last step left on the device
    if args.full:
        hist[0] = np.concatenate(b.histograms())                # (all-reduced in place when N > 1)
        host_i, host_lra = corpus_gate(hist[0])                 # the same gate on the host copy of the histograms
        if abs(corpus_i - host_i) > 1e-9 or abs(corpus_lra - host_lra) > 1e-9:
            raise SystemExit(f"device corpus gate {corpus_i, corpus_lra} != host {host_i, host_lra}")
    if args.dump_outputs and rank == 0:
        # before anything else runs on the batch: --full's sustained and f16x3 passes below overwrite its results
        n_files, n_bytes = dump_outputs(b, first, (corpus_i, corpus_lra), args.dump_outputs)
        print(f"[bench] wrote {n_files} arrays ({n_bytes / 1e6:.1f} MB) to {args.dump_outputs}", file=sys.stderr, flush=True)

    # The reference's true-peak arithmetic is an f32 FIR (ebur128's interpolator: f32 taps, f32 accumulation; analyzer.rs:139-141,
    # 159-164).  The timed step above runs it at that width (SS_TP_ARITH_F32, the library's default: an f32 fma chain per output —
    # v_pk_fma_f32 on the packed VALU for 2 / 6 / 8 channels since round 6, v_mfma_f32_16x16x4_f32 for other counts).  The SAME step is timed again with the opt-in f16x3 split on the matrix cores
    # (ss_batch_set_true_peak_arith), and both modes' peaks of the timed batch are measured against an f64 polyphase
    # convolution of the same streams (numpy, independent of the oracle).  (--full; the mode the step ran in is read either way.)
    if b.true_peak_arith != L.SS_TP_ARITH_F32:
        raise SystemExit("the timed step did not run at the reference's f32 true-peak width")
    tp_arith = None
    sustained = None
    if args.full and comm is None:
        # a sustained run of the same step (>= 1 s): clocks and thermals of the driver's short headline are otherwise invisible
        n_sus = max(200, int(math.ceil(1.2 / (dt / args.steps))))
        sclk0 = gpu_sclk_mhz(dev)
        import threading
        clk = [None]
        th = threading.Thread(target=lambda: (time.sleep(0.35), clk.__setitem__(0, gpu_sclk_mhz(dev))))   # read while the steps run
        t1 = time.perf_counter()
        th.start()
        for _ in range(n_sus):
            step()
        fence()
        dts = time.perf_counter() - t1
        th.join()
        mid_clk = clk[0]
        b.sync()
        sustained = {"steps": n_sus, "seconds": dts, "ms_per_step": dts / n_sus * 1e3, "value": samples_per_step * n_sus / dts,
                     "sclk_mhz_idle_before": sclk0, "sclk_mhz_under_load": mid_clk,
                     "what": "the timed step again, back to back for >= 1 s right behind the headline's steps (same batch, same mode)"}

        def tp_error(nstreams=4):
            worst = 0.0
            taps = interpolator_taps_f64(4)
            for i in range(min(nstreams, count)):
                x = b.download_input(i)
                tp, _ = b.peaks(i)
                for c in range(2):
                    ch = x[c::2].astype(np.float64)
                    want = max(max(np.abs(np.convolve(ch, taps[ph::4])[:ch.size]).max() for ph in range(4)), np.abs(ch).max())
                    worst = max(worst, abs(tp[c] - want) / want)
            return worst
        err_f32 = tp_error()
        b.set_true_peak_arith(L.SS_TP_ARITH_F16X3)
        for _ in range(args.warmup):
            step()
        fence()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step()
        fence()
        dt16 = time.perf_counter() - t1
        b.sync()
        err_f16x3 = tp_error()
        b.set_true_peak_arith(L.SS_TP_ARITH_F32)
        b.run(); b.sync()
        tp_arith = {"timed_default": "SS_TP_ARITH_F32 (f32 fma chain per output on the packed VALU, v_pk_fma_f32: the reference's width)",
                    "value_f16x3_split": samples_per_step * args.steps / dt16, "ms_per_step_f16x3_split": dt16 / args.steps * 1e3,
                    "max_rel_err_vs_f64_polyphase": {"f32 (timed default, reference width)": err_f32, "f16x3_split (opt-in)": err_f16x3},
                    "streams_checked": min(4, count), "bar": 1e-4,
                    "what": "the same timed step with SS_TP_ARITH_F16X3 (opt-in, not the headline); errors of the 4x true peak of the "
                            "timed batch against an f64 polyphase convolution with the crate's f32 taps (numpy)"}

    # per-kernel times of an overlap mode: a separate SEQUENTIAL pass (with two kernels sharing the chip a per-kernel HIP-event time
    # would not describe either of them); HIP events on the batch's own stream.  A run of its own: --full
    if args.full and region is None:
        b.timing_enable(True)
        region0 = [b.timing_read(k) for k in range(L.SS_KERNEL_COUNT)]
        for _ in range(max(3, min(args.steps, 10))):
            b.run(); b.sync()
        region = [tuple(a - b0 for a, b0 in zip(b.timing_read(k), region0[k])) for k in range(L.SS_KERNEL_COUNT)]
        b.timing_enable(False)
    if comm is not None:
        comm.barrier()

    if rank == 0:
        # dominant kernel: the spectrum kernel.  Algorithmic bytes per launch:
        # every input f32 once + every retained bin once = 4 B/sample + 4*W*2*nbins per stream.
        kernels_timed = region is not None       # (a plain run in an overlap mode has no per-kernel times: their pass is --full's)
        if not kernels_timed:
            region = [(0.0, 0)] * L.SS_KERNEL_COUNT
        fft_ms, fft_n_launch = region[L.SS_KERNEL_FFT]
        alg_bytes = count * (frames * 2 * 4 + lay.n_windows * lay.fft_channels * lay.n_bins * 4)
        achieved = alg_bytes / (fft_ms / max(fft_n_launch, 1) * 1e-3) / 1e9 if fft_ms > 0 else None
        kernels = {}
        for k in range(L.SS_KERNEL_COUNT):
            ms, n = region[k]
            kernels[lib.ss_batch_kernel_name(b._h, k).decode()] = round(ms / max(n, 1), 4) if kernels_timed else None
        seq_ms = sum(kernels.values()) if kernels_timed else None
        traffic, traffic_src = None, None
        tpath = os.path.join(ROOT, "profiles", "fft_hbm_traffic.json")
        if os.path.exists(tpath):        # PMC counters cannot be read inside this run: committed rocprofv3 passes, labelled as such
            try:
                traffic = json.load(open(tpath)).get("hbm_bytes_per_launch")
                traffic_src = "profiles/fft_hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, not this run)"
            except Exception:
                traffic = None
        td_ms, td_n = region[L.SS_KERNEL_TIME_DOMAIN]
        td = {"kernel": lib.ss_batch_kernel_name(b._h, L.SS_KERNEL_TIME_DOMAIN).decode(),
              "algorithmic_bytes_per_launch": count * frames * 2 * 4}
        if td_ms > 0:
            td["achieved_GBps"] = td["algorithmic_bytes_per_launch"] / (td_ms / max(td_n, 1) * 1e-3) / 1e9
            td["hbm_frac"] = td["achieved_GBps"] / HBM_PEAK_GBS
        geo = b.geometry
        step_alg = alg_bytes + count * (lay.n_wave_points * 4 + 8 * 110)
        out = {
            "metric": "audio samples/s analyzed (48 kHz stereo)", "value": value, "unit": "samples/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "f32 + f64", "data": "synthetic", "full": bool(args.full),
            "value_f16x3_split": tp_arith["value_f16x3_split"] if tp_arith else None,
            "true_peak_arithmetic": tp_arith,
            "config": {"workload": (f"{total_streams} streams in total (BASELINE config 4) sharded over {world} GPU(s)" if strong
                                    else f"{args.streams} streams/GPU (BASELINE config 3)") +
                                   f" x {args.seconds:g} s, {args.rate} Hz stereo f32: mid/side {args.fft_n}-pt Hann FFT "
                                   f"hop {args.hop} + K-weighted gated LUFS/LRA + 4x true peak + min-max decimation "
                                   "+ corpus gate (1 all-reduce of 2x1000 u64)",
                       "n1_workload": "N = 1: value = BASELINE config 3 (1024 streams on the GPU); N > 1 runs config 4 (8192 streams in total, "
                                      "sharded, strong scaling).  The same-workload base of the N > 1 points is config.n1_strong_value of the "
                                      "N = 1 line (config 4's 8192 streams on ONE GPU); samples/s are comparable across N, ms_per_step are not",
                       "streams_total": total_streams, "streams_this_rank": count, "windows_per_stream": lay.n_windows, "bins": lay.n_bins,
                       "sharding": f"streams, {world} rank(s)",
                       "collective": ({"lib": "none", "nranks": 1} if comm is None else {"lib": comm.transport, "nranks": comm.size, "ncclCommCount": comm.size if comm.transport == "rccl" else None,
                                                                                              "rccl_version": comm.library_version, "call": "ncclAllReduce(2000, ncclUint64, ncclSum) per step" if comm.transport == "rccl" else "host-staged sum over loopback TCP"}),
                       "mode": ["sequential (spectrum kernel, then the time-domain chain)",
                                "overlap (spectrum kernel on a second HIP stream beside the time-domain chain)",
                                "time-domain kernel, then the spectrum kernel on a second HIP stream beside the chain's tail (gating / histograms)"][ov_mode],
                       "geometry": {"fft_windows_per_block": geo.fft_windows_per_block, "fft_blocks": geo.fft_blocks,
                                    "td_segments": geo.td_segments, "td_segment_subblocks": geo.td_segment_subblocks,
                                    "td_handover": ("whole-stream workgroups" if geo.td_split == 1 else
                                                    f"segments on eight waves, {geo.td_warm_subblocks} sub-block filter run-in inside the launch" if geo.td_split == 2 else
                                                    f"exact: fix-up launch over the first {geo.td_fixup_subblocks} sub-blocks of segments > 0" if geo.td_fixup_subblocks else
                                                    f"{geo.td_warm_subblocks} sub-block run-in" if geo.td_warm_subblocks else "one segment"),
                                    "waveform_fused": geo.waveform_fused},
                       "sustained": sustained,
                       "corpus_integrated_lufs": corpus_i, "corpus_lra": corpus_lra,
                       "kernel_ms": kernels, "kernel_ms_note": ("HIP events on the batch's stream around every kernel of the K timed steps themselves (ring of event sets, no host "
                                                              "synchronisation inside the region)" if timed_in_region else "separate sequential pass, HIP events on the batch's stream"
                                                              if kernels_timed else "not measured: an overlap mode's separate sequential pass runs with --full"),
                       "sequential_gpu_ms": round(seq_ms, 4) if kernels_timed else None,
                       "step_hbm_frac": step_alg / (dt / args.steps) / 1e9 / HBM_PEAK_GBS,
                       "time_domain_kernel": td},
            "roofline": {"bound": "hbm", "kernel": lib.ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT).decode(),
                         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": (achieved / HBM_PEAK_GBS) if achieved else None, "traffic": traffic, "traffic_source": traffic_src,
                         "traffic_note": "committed-profile data (PMC counters cannot be read inside this run); not an input of frac",
                         "algorithmic_bytes_per_launch": alg_bytes,
                         # context, measured in this run: the same loads and stores with no arithmetic in between
                         "io_floor": ({"ms": io_floor_ms, "GBps": alg_bytes / (io_floor_ms * 1e-3) / 1e9,
                                       "kernel_over_floor": (fft_ms / max(fft_n_launch, 1)) / io_floor_ms,
                                       "what": "k_fft4096_traffic: this kernel's grid, occupancy and addresses, loads + stores only"}
                                      if io_floor_ms else None)},
        }
        # PCIe-inclusive rate (informational, never `value`): host f32 -> HBM upload of a slice + its share of a pass
        host = None
        if args.full:
            try:
                k = min(count, 64)
                host = np.concatenate([b.download_input(i) for i in range(k)])
                t0 = time.perf_counter()
                b.upload(0, host)
                up = time.perf_counter() - t0
                out["config"]["pcie_inclusive_samples_per_s"] = host.size / (up + dt / args.steps * k / count)
                out["config"]["h2d_GBps"] = host.nbytes / up / 1e9
            except Exception:
                pass
        if args.full and world == 1 and not args.no_cpu:
            cb, check = cpu_baseline(b, args.rate, args.fft_n, args.hop)
            out["cpu_baseline"] = cb
            out["config"]["self_check_vs_oracle"] = check
            out["config"]["gpu_over_cpu_1core"] = value / cb["value"]
        else:
            out["cpu_baseline"] = None
        # what the driver's record keeps of `config` are its scalar entries: the facts a reader of BENCH / SCALE files needs are
        # repeated flat beside the nested objects
        cfgd = out["config"]
        cfgd["collective_lib"] = "none" if comm is None else comm.transport
        cfgd["collective_nranks"] = 1 if comm is None else comm.size
        cfgd["ncclCommCount"] = comm.size if (comm is not None and comm.transport == "rccl") else None
        cfgd["rccl_version"] = comm.library_version if comm is not None else None
        cfgd["td_segments"] = geo.td_segments
        cfgd["td_handover"] = cfgd["geometry"]["td_handover"]
        for kname, kms in kernels.items():
            cfgd["kernel_ms_" + kname] = kms
        if sustained:
            cfgd["sustained_value"] = sustained["value"]
            cfgd["sustained_ms_per_step"] = sustained["ms_per_step"]
            cfgd["sustained_sclk_mhz_under_load"] = sustained["sclk_mhz_under_load"]
        if io_floor_ms:
            out["roofline"]["io_floor_ms"] = io_floor_ms
            out["roofline"]["kernel_over_io_floor"] = (fft_ms / max(fft_n_launch, 1)) / io_floor_ms
        if args.full and world == 1 and not args.no_extra:
            b.close()
            extra = []
            if not strong:
                # The same-workload base of the scaling curve: N > 1 runs BASELINE config 4 (8192 streams in total, sharded), so N = 1
                # ALSO times config 4's whole corpus on this one GPU (85 GB of the 288 fit) — the step of the N > 1 runs, rank count 1.
                # `value` stays config 3 (the metric's configuration); this is the figure the N >= 2 points divide by.
                try:
                    b8 = ssa.Batch(args.rate, 2, CONFIG4_TOTAL_STREAMS, frames, args.fft_n, args.hop, flags=L.SS_BATCH_ALL)
                    b8.synthesize(0x5EED0000, 0)
                    b8.set_overlap(ov_mode)
                    for _ in range(2):
                        b8.run(); b8.corpus_gate_enqueue(None)
                    lib.ss_device_synchronize()
                    n8 = 5
                    t8 = time.perf_counter()
                    for _ in range(n8):
                        b8.run(); b8.corpus_gate_enqueue(None)
                    lib.ss_device_synchronize()
                    d8 = time.perf_counter() - t8
                    b8.sync()
                    cfgd["n1_strong_value"] = CONFIG4_TOTAL_STREAMS * frames * 2 * n8 / d8
                    cfgd["n1_strong_ms_per_step"] = d8 / n8 * 1e3
                    cfgd["n1_strong_streams"] = CONFIG4_TOTAL_STREAMS
                    cfgd["n1_strong_corpus_integrated_lufs"] = b8.corpus_gate_read()[0]
                    b8.close()
                except Exception as ex:                                   # noqa: BLE001 — (a smaller card: the line says so)
                    cfgd["n1_strong_value"] = None
                    cfgd["n1_strong_error"] = repr(ex)
            if host is not None and not strong:
                # The boundary hands over HOST buffers: the same full path fed over PCIe by the pipelined runner (soundscope_amd/pipeline.py:
                # the host corpus page-locked in place, two batches as a double buffer — chunk k + 1 uploads on the copy engine while
                # chunk k is analysed — results read back per chunk), wall clock of the whole call, second of two calls.  Informational.
                try:
                    corpus_h = np.tile(host, max(1, 512 * frames * 2 // host.size))
                    for _ in range(2):
                        tp0 = time.perf_counter()
                        res_p, _hist_p = ssa.analyze_corpus(corpus_h, args.rate, 2, frames, chunk_streams=128, flags=L.SS_BATCH_ALL,
                                                            fft_n=args.fft_n, hop_frames=args.hop)
                        dtp = time.perf_counter() - tp0
                    cfgd["pcie_inclusive_pipelined_samples_per_s"] = corpus_h.size / dtp
                    cfgd["pcie_inclusive_pipelined_h2d_GBps"] = corpus_h.nbytes / dtp / 1e9
                    cfgd["pcie_inclusive_pipelined_streams"] = len(res_p)
                    cfgd["pcie_inclusive_pipelined_what"] = ("soundscope_amd.analyze_corpus: host f32 corpus page-locked in place, chunks of 128 streams double-buffered "
                                                             "(upload of chunk k + 1 beside the full pass of chunk k), per-chunk read-back of the results; PCIe-bound")
                    del corpus_h, res_p
                except Exception as ex:                               # noqa: BLE001
                    cfgd["pcie_inclusive_pipelined_error"] = repr(ex)
            try:
                # config 3 as BASELINE.json words it ("4096-pt FFT + LUFS"): the headline step additionally carries the
                # 4x true peak and the decimation that north_star puts on the path
                e = time_config(ssa, L, args.rate, 2, count, frames, args.fft_n, args.hop, 0, steps=5, flags=L.SS_BATCH_FFT | L.SS_BATCH_LUFS)
                e["workload"] = f"config 3 without true peak and decimation: {count} streams x {args.seconds:g} s, spectrum + K-weighted gated LUFS / LRA only"
                extra.append(e)
                # the headline step with the true peak as the opt-in f16x3 split instead of the f32 product
                e = time_config(ssa, L, args.rate, 2, count, frames, args.fft_n, args.hop, 0, steps=5, tp_arith=L.SS_TP_ARITH_F16X3)
                e["workload"] = f"config 3, full path, true peak as the opt-in f16x3 split (ss_batch_set_true_peak_arith): {count} streams x {args.seconds:g} s"
                extra.append(e)
                # the headline step in columns-only mode (N3 fused into the spectrum epilogue): no row is stored, 160 chart columns
                # per row leave the chip — the compute-bound face of the spectrum kernel (its fp32 fraction is the figure to read)
                e = time_config(ssa, L, args.rate, 2, count, frames, args.fft_n, args.hop, 0, steps=5, cols=160)
                e["workload"] = (f"config 3, full path, columns-only spectrum (SS_BATCH_FFT_COLUMNS, 160 columns, reference gain): {count} streams x "
                                 f"{args.seconds:g} s; algorithmic bytes = 4 B per input sample + 160 x 2 x 4 B per window")
                extra.append(e)
                # config 2: one stream (10 s and the 600 s steady-state variant)
                for secs in (10, 600):
                    e = time_config(ssa, L, 48000, 2, 1, 48000 * secs, 4096, 1024, 0, steps=5)
                    e["workload"] = f"config 2: 1 stream x {secs} s, 48 kHz stereo, N=4096 hop 1024, full path"
                    extra.append(e)
                extra.append(reference_tick_workload(ssa, L))
                # config 5: 96 kHz 8-channel, N = 16384 per channel; forced 4x (benchmark) and the crate rule's 2x
                for tp, name in ((4, "forced 4x true peak"), (0, "rule 2x true peak")):
                    e = time_config(ssa, L, 96000, 8, 64, 960000, 16384, 1024, tp, steps=3)
                    e["workload"] = f"config 5: 64 streams x 10 s, 96 kHz 8 ch, N=16384 hop 1024 per channel, {name}"
                    extra.append(e)
                    tag = "config5_tp4x" if tp == 4 else "config5_tp2x"
                    cfgd[tag + "_samples_per_s"] = e.get("samples_per_s")
                    for kname, kms in (e.get("kernel_ms") or {}).items():
                        cfgd[tag + "_ms_" + kname] = kms
            except Exception as ex:
                extra.append({"error": repr(ex)})
            out["config"]["extra"] = extra
        sys.stdout.flush()
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if comm is not None:
        comm.barrier()
        comm.close()


if __name__ == "__main__":
    main()
