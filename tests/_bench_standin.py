"""Runs bench.main() in this process with a stand-in for the package, on a machine without a GPU (a helper of
tests/test_bench_full_option.py, started as a child process: bench.main() re-points file descriptor 1).  The stand-in has the
names bench.py uses of soundscope_amd, soundscope_amd._lib and soundscope_amd.distributed; every method of its batch appends
its own name to a list, which goes to stderr as one `CALLS [...]` line behind the run.  No value it returns means anything."""
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = []
GATE = (-23.0, 7.5)
CLOCK = [0.0]                   # bench's clock here: 5 ms a pass, 1 ms an upload, so that no figure depends on this machine


def recorded(fn):
    def wrapper(self, *a, **k):
        CALLS.append(fn.__name__)
        return fn(self, *a, **k)
    return wrapper


class Lib:
    def ss_device_count(self): return 1
    def ss_set_device(self, dev): return 0
    def ss_last_device_error(self): return b""
    def ss_device_synchronize(self): return 0
    def ss_batch_kernel_name(self, h, k): return b"k_%d" % k


class Batch:
    def __init__(self, rate, channels, streams, frames, fft_n, hop, flags=0, **kw):
        CALLS.append("Batch")
        self._h = None
        self.frames = frames
        self.cfg = types.SimpleNamespace(n_streams=streams, channels=channels)
        self.layout = types.SimpleNamespace(n_windows=max(1, (frames - fft_n) // hop + 1), fft_channels=2, n_bins=fft_n // 2 + 1,
                                            n_wave_points=40, n_subblocks=max(1, frames * 10 // rate))
        self.geometry = types.SimpleNamespace(fft_windows_per_block=1, fft_blocks=streams, td_segments=1, td_segment_subblocks=0,
                                              td_split=0, td_warm_subblocks=0, td_fixup_subblocks=0, td_true_peak_factor=4,
                                              waveform_fused=1)
        self.arith = 0
        self.passes = 0

    @property
    def true_peak_arith(self): return self.arith

    @recorded
    def synthesize(self, seed, first): pass

    @recorded
    def set_overlap(self, mode): pass

    @recorded
    def traffic_floor(self, reps): return 1.0

    @recorded
    def run(self):
        self.passes += 1
        CLOCK[0] += 5e-3

    @recorded
    def corpus_gate_enqueue(self, comm): pass

    @recorded
    def sync(self): pass

    @recorded
    def timing_enable(self, on): pass

    @recorded
    def timing_read(self, k): return (2.0 * self.passes, self.passes)

    @recorded
    def corpus_gate_read(self): return GATE

    @recorded
    def histograms(self): return np.zeros(1000, np.uint64), np.zeros(1000, np.uint64)

    @recorded
    def set_true_peak_arith(self, arith): self.arith = arith

    @recorded
    def download_input(self, i): return np.linspace(-0.5, 0.5, 2 * self.frames).astype(np.float32)

    @recorded
    def peaks(self, i): return np.full(2, 0.5), np.full(2, 0.5)

    @recorded
    def upload(self, first, pcm): CLOCK[0] += 1e-3

    @recorded
    def results(self):
        return [types.SimpleNamespace(integrated_lufs=-20.0, loudness_range=1.0, true_peak=[0.5, 0.5], sample_peak=[0.5, 0.5],
                                      n_gating_blocks=1, n_st_blocks=1) for _ in range(self.cfg.n_streams)]

    @recorded
    def fft(self, s): return np.zeros((self.layout.n_windows, 2, self.layout.n_bins), np.float32)

    @recorded
    def waveform(self, s): return np.zeros((self.layout.n_wave_points // 2, 2), np.float32)

    @recorded
    def subblocks(self, s): return np.zeros((self.layout.n_subblocks, self.cfg.channels), np.float64)

    @recorded
    def close(self): pass


def main():
    ssa = types.ModuleType("soundscope_amd")
    ssa.__path__ = []
    ssa.Batch = Batch
    L = types.ModuleType("soundscope_amd._lib")
    L.lib = lambda: Lib()
    L.SS_BATCH_ALL, L.SS_KERNEL_COUNT, L.SS_KERNEL_FFT, L.SS_KERNEL_TIME_DOMAIN = 0xFF, 4, 0, 1
    L.SS_TP_ARITH_F32, L.SS_TP_ARITH_F16X3 = 0, 1
    dist = types.ModuleType("soundscope_amd.distributed")
    dist.Comm = None
    dist.corpus_gate = lambda hist: GATE
    dist.shard_streams = lambda total, rank, world: (0, total)
    ssa._lib, ssa.distributed = L, dist
    sys.modules.update({"soundscope_amd": ssa, "soundscope_amd._lib": L, "soundscope_amd.distributed": dist})
    sys.path.insert(0, ROOT)
    import bench
    bench.gpu_sclk_mhz = lambda dev=0: None       # (no clock to read, and no tool to start for it)
    bench.time = types.SimpleNamespace(perf_counter=lambda: CLOCK[0], sleep=lambda s: None)
    try:
        bench.main()
    finally:
        sys.stderr.write("CALLS " + json.dumps(CALLS) + "\n")


if __name__ == "__main__":
    main()
