#!/usr/bin/env python3
"""Recorded rows of the N = 4096 spectrum kernels at the smallest shapes that walk every line of the window loop and of the
shared dB epilogue (tests/golden/spectrum_window_loop_v1.npz, checked bit for bit by tests/test_gpu_spectrum_window_loop.py):

    python tests/golden/make_spectrum_window_loop.py <commit the library was built from>      (needs the GPU)

The fixture pins the bits of the commit it was recorded at, named in its `commit` entry: a change of the kernels that is meant
to leave every output bit alone is held to it.  Every entry is the result's u32 bit patterns as four byte planes ([4][count]
u8, plane b = byte b of every word: the high planes of dB rows repeat and compress, the low ones do not); `planes` is what the
test applies to its own result.

Cases (every batch at N = 4096 with SS_BATCH_FFT alone; `plans` records kernel, windows per workgroup, workgroups):
  run6      k_fft4096_ms1, 48 kHz stereo, six windows walked by ONE workgroup: first window (full load), slid windows that
            prefetch the next hop, the last window, which prefetches nothing.  The plan gives runs of six only from 512 streams on
            (fewer streams get runs of two, see ragged), so the batch has 512 and the first and the last stream are recorded:
            stream 0 with an onset inside its first windows (the exact-energy exponent and a rescale), stream 511 steady.
  ragged    two streams, runs of two: one stream of two windows and one shorter than a window (no row at all).
  zeros-*   squared magnitudes that are exactly zero INSIDE a non-empty row: a sine at amplitude 2^-68 on mid and one at 2^-72
            on side — a handful of bins around either tone square to a normal number, the transform's rounding noise everywhere
            else squares to zero and reads -150 dB (+ pink).  zeros-ms: both rows mixed.  zeros-dual: L = R, the side row is
            empty and takes the floor-row path behind a mid row that is mixed.  zeros-raw: the mid signal through
            Analyzer.get_fft, whose rows carry no pink table (k_fft4096_pairw on the offset-only table).
  r96k, r44k  96 kHz (853 bins: no thread owns a second group of four) and 44.1 kHz (the most bins of the common rates), stereo,
            three windows.
  cols      run6 as columns-only, 160 columns, fixed gain 0 dB.
  mono, hop512, hop768   the siblings on the shared epilogue, one stream of six windows each: k_fft4096_pairw, k_fft4096_ms<2>,
            k_fft4096_ms_anyhop.
The maker asserts the kernel of every case and, for the zeros cases, that a recorded row holds both floor bins and others."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "spectrum_window_loop_v1.npz")
MAX_BYTES = 512 * 1024
N = 4096
NAMES = ["run6", "ragged", "zeros-ms", "zeros-dual", "zeros-raw", "r96k", "r44k", "cols", "mono", "hop512", "hop768"]


def planes(a):
    """[4][count] u8: byte b of every u32 word of `a` (f32 as it stands, f64 as two words)"""
    words = np.ascontiguousarray(a).reshape(-1).view(np.uint32)
    return np.ascontiguousarray(words.view(np.uint8).reshape(-1, 4).T)


def frames_for(hop, nw):
    return (N // hop + 1) * hop + (nw - 1) * hop


def programme(seed, frames, channels, rate, onset=0):
    """[frames][channels] f32: a tone and quiet noise per channel at their own levels; the first `onset` frames 60 dB down"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)
    x = np.empty((frames, channels), np.float64)
    for c in range(channels):
        f = (310.0 + 1730.0 * c + 97.0 * (seed % 7)) / rate
        x[:, c] = (0.4 / (1 + 3 * c)) * np.sin(2 * np.pi * f * t + 0.5 * c) + 0.004 * rng.uniform(-1, 1, frames)
    if onset:
        x[:onset] *= 1e-3
    return x.astype(np.float32)


def tiny_mid_side(frames):
    """(mid, side) f64: sines on bins 300 and 700 at amplitudes 2^-68 and 2^-72"""
    t = np.arange(frames, dtype=np.float64)
    m = np.sin(2 * np.pi * 300 * t / N).astype(np.float32).astype(np.float64) * 2.0 ** -68
    s = np.sin(2 * np.pi * 700 * t / N + 1.0).astype(np.float32).astype(np.float64) * 2.0 ** -72
    return m, s


def _batch(ssa, L, rate, ch, ns, frames, hop, kernel, nw, cols=0):
    b = ssa.Batch(rate, ch, ns, frames, N, hop, flags=L.SS_BATCH_FFT, spectrum_columns=cols)
    g = b.geometry
    plan = (L.lib().ss_batch_kernel_name(b._h, L.SS_KERNEL_FFT).decode(), int(g.fft_windows_per_block), int(g.fft_blocks))
    assert plan[0] == kernel and b.layout.n_windows == nw, (plan, b.layout.n_windows)
    return b, plan


def _mixed(row, floor):
    """the row holds floor bins (-150 + pink) and bins well away from the floor"""
    at = np.abs(row.astype(np.float64) - floor) <= 1e-3
    return bool(at.any()) and bool((np.abs(row.astype(np.float64) - floor)[~at] > 1.0).any())


def run_case(name):
    """-> (result array, plan or None)"""
    import soundscope_amd as ssa
    from soundscope_amd import _lib as L
    if name in ("run6", "cols"):
        ns, F = 512, frames_for(1024, 6)
        b, plan = _batch(ssa, L, 48000, 2, ns, F, 1024, "k_fft4096_ms1", 6, cols=160 if name == "cols" else 0)
        assert plan[1] == 6 and plan[2] == ns, plan                      # one run of six windows per stream
        x = np.zeros((ns, F, 2), np.float32)
        x[0] = programme(11, F, 2, 48000, onset=4096 + 700)
        x[1:ns - 1] = programme(12, F, 2, 48000)
        x[ns - 1] = programme(13, F, 2, 48000)
        b.upload(0, x.reshape(-1))
        if name == "cols":
            b.set_columns_gain(0.0)
        b.run(); b.sync()
        get = b.spectrum_columns if name == "cols" else b.fft
        out = np.stack([get(0), get(ns - 1)])
        b.close()
        return out, plan
    if name == "ragged":
        F = frames_for(1024, 6)
        b, plan = _batch(ssa, L, 48000, 2, 2, F, 1024, "k_fft4096_ms1", 6)
        lengths = [frames_for(1024, 2) + 100, 3000]
        b.set_lengths(lengths)
        x = np.stack([programme(21, F, 2, 48000), programme(22, F, 2, 48000)])
        for i, n in enumerate(lengths):
            x[i, n:] = 0.0
        b.upload(0, x.reshape(-1)); b.run(); b.sync()
        assert b.stream_shape(0).n_windows == 2 and b.stream_shape(1).n_windows == 0
        out = b.fft(0).copy()
        assert out.shape[0] == 2 and b.fft(1).shape[0] == 0
        b.close()
        return out, plan
    if name in ("zeros-ms", "zeros-dual"):
        F = frames_for(1024, 2)
        m, s = tiny_mid_side(F)
        if name == "zeros-dual":
            s = np.zeros(F)
        x = np.stack([m + s, m - s], 1).astype(np.float32)
        b, plan = _batch(ssa, L, 48000, 2, 1, F, 1024, "k_fft4096_ms1", 2)
        b.upload(0, x.reshape(-1)); b.run(); b.sync()
        out = b.fft(0).copy()
        floor = -150.0 + b.bin_tables()[2]
        b.close()
        for w in range(2):
            assert _mixed(out[w, 0], floor), (name, w, "mid")
            if name == "zeros-ms":
                assert _mixed(out[w, 1], floor), (name, w, "side")
            else:
                assert np.all(np.abs(out[w, 1] - floor) <= 1e-3), (name, w, "side is the floor row")
        return out, plan
    if name == "zeros-raw":
        m, _ = tiny_mid_side(N)
        a = ssa.Analyzer(2, 48000)
        out = np.asarray(a.get_fft(m.astype(np.float32))).copy()
        a.close()
        b = ssa.Batch(48000, 1, 1, frames_for(1024, 1), N, 1024, flags=L.SS_BATCH_FFT)
        floor = -150.0 + b.bin_tables()[2]
        b.close()
        assert out.shape == (floor.size, 2) and _mixed(out[:, 1], floor), name
        return out, None
    shapes = {"r96k": (96000, 2, 1024, 3, "k_fft4096_ms1"), "r44k": (44100, 2, 1024, 3, "k_fft4096_ms1"),
              "mono": (48000, 1, 1024, 6, "k_fft4096_pairw"), "hop512": (48000, 2, 512, 6, "k_fft4096_ms"),
              "hop768": (48000, 2, 768, 6, "k_fft4096_ms_anyhop")}
    rate, ch, hop, nw, kernel = shapes[name]
    F = frames_for(hop, nw)
    b, plan = _batch(ssa, L, rate, ch, 1, F, hop, kernel, nw)
    b.upload(0, programme(31 + NAMES.index(name), F, ch, rate, onset=N // 2 + 300).reshape(-1)); b.run(); b.sync()
    out = b.fft(0).copy()
    if name == "r96k":
        assert out.shape[2] == 853
    if name == "r44k":
        assert out.shape[2] > 1705                       # more groups of four than at 48 kHz
    b.close()
    return out, plan


def main():
    commit = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else PATH
    entries, plans = {}, []
    for name in NAMES:
        res, plan = run_case(name)
        entries[name] = planes(res)
        plans.append("%s: %s %s" % (name, plan, res.shape))
        print(plans[-1], flush=True)
    np.savez_compressed(out_path, commit=np.array(commit), plans=np.array(plans), **entries)
    size = os.path.getsize(out_path)
    print("%s: %d bytes, recorded at %s" % (out_path, size, commit))
    assert size < MAX_BYTES, size


if __name__ == "__main__":
    main()
