#!/usr/bin/env python3
"""Randomised ragged meter-bank programmes against the product's own handles: random rate, channel count and stream count, a
dozen ragged calls in which every stream draws its own length (none, a few frames, up to a tile of the kernel, beyond it, beyond
32 sub-blocks), selective resets between calls, one NaN / +Inf / -Inf planted in one stream, and the three input forms (f32,
raw s16 / s24, device-resident).  After every call every stream against an `Analyzer` fed the same blocks: integrated loudness,
range and all peaks bit for bit, momentary and short-term within 1e-9 LU, the frame count.
      python tools/fuzz_bank_ragged.py [programmes] [first seed]"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundscope_amd as ssa
from soundscope_amd import _lib as L
from oracle import pyoracle as po


def same_bits(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def close9(a, b):
    return same_bits(a, b) or abs(a - b) <= 1e-9


def stream_against_handle(bank, s, rec, h, fed):
    """None, or what differs between stream s of the bank (its record `rec`) and the handle `h` fed the same blocks"""
    if int(rec["frames"]) != fed:
        return f"frames {rec['frames']} vs {fed}"
    if not same_bits(rec["integrated"], h.get_integrated_lufs()):
        return f"integrated {rec['integrated']!r} vs {h.get_integrated_lufs()!r}"
    if not same_bits(rec["loudness_range"], h.get_loudness_range()):
        return f"range {rec['loudness_range']!r} vs {h.get_loudness_range()!r}"
    if not close9(rec["momentary"], h.get_momentary_lufs()):
        return f"momentary {rec['momentary']!r} vs {h.get_momentary_lufs()!r}"
    if not close9(rec["shortterm"], h.get_shortterm_lufs()):
        return f"short-term {rec['shortterm']!r} vs {h.get_shortterm_lufs()!r}"
    tp, sp = bank.peaks(s)
    for c in range(bank.channels):
        if not same_bits(sp[c], h.get_sample_peak_channel(c)):
            return f"sample peak {c}: {sp[c]!r} vs {h.get_sample_peak_channel(c)!r}"
        if not same_bits(tp[c], h.get_true_peak_channel(c)):
            return f"true peak {c}: {tp[c]!r} vs {h.get_true_peak_channel(c)!r}"
    return None


def draw_length(rng, rate, S, big_left):
    kind = int(rng.integers(0, 8))
    if kind == 0: return 0
    if kind == 1: return int(rng.integers(1, 64))
    if kind == 2: return int(rng.integers(64, 2000))
    if kind == 3: return int(S + rng.integers(-1, 2))
    if kind == 4 and big_left: return int(32 * S + rng.integers(-2, 3 * S))
    if kind == 5: return int(rng.integers(2000, rate // 3))
    return int(rng.integers(400, 560))


def programme(seed):
    rng = np.random.default_rng(seed)
    rate = int(rng.choice([32000, 44100, 48000, 48000, 96000]))
    ch = int(rng.choice([1, 2, 2, 2, 3, 5, 6]))
    n = int(rng.integers(2, 10))
    S = (rate + 5) // 10
    n_calls = int(rng.integers(6, 15))
    tag = f"seed {seed} ({rate} Hz, {ch} ch, {n} streams)"
    bank = ssa.MeterBank(n, ch, rate)
    def fresh():
        a = ssa.Analyzer(); a.create_loudness_meter(ch, rate)
        return a
    handles = [fresh() for _ in range(n)]
    fed = [0] * n
    big_left = [True] * n                                   # one call beyond 32 sub-blocks per stream: the programmes stay short
    bad_call = int(rng.integers(0, n_calls)) if rng.random() < 0.35 else -1
    scratch, cap = None, 0
    for k in range(n_calls):
        frames = []
        for s in range(n):
            f = draw_length(rng, rate, S, big_left[s])
            if f > 32 * S - 2: big_left[s] = False
            frames.append(f)
        form = "f32" if k == bad_call else str(rng.choice(["f32", "f32", "s16", "s24", "device"]))
        level = 10.0 ** (rng.uniform(-40, -3) / 20.0)
        blocks = []
        for s, f in enumerate(frames):
            t = (np.arange(f) + fed[s]) / rate
            x = np.empty((f, ch), np.float32)
            for c in range(ch):
                x[:, c] = level * (np.sin(2 * np.pi * rng.uniform(40, 5000) * t + c) + 0.3 * rng.standard_normal(f))
            blocks.append(np.clip(x, -1.0, 1.0).reshape(-1))
        if k == bad_call and max(frames) > 0:
            s = int(rng.choice([i for i, f in enumerate(frames) if f]))
            blocks[s][int(rng.integers(0, blocks[s].size))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
        if form in ("s16", "s24"):
            fmt = L.SS_PCM_S16 if form == "s16" else L.SS_PCM_S24
            raws = []
            for s in range(n):
                if form == "s16":
                    raw = np.round(blocks[s] * 32767.0).astype("<i2").view(np.uint8)
                else:
                    q = np.round(blocks[s].astype(np.float64) * 8388607.0).astype(np.int32)
                    raw = np.stack([q & 0xFF, (q >> 8) & 0xFF, (q >> 16) & 0xFF], axis=-1).astype(np.uint8).reshape(-1)
                raws.append(raw if frames[s] else None)
                blocks[s] = po.pcm_to_f32(raw.tobytes(), fmt) if frames[s] else blocks[s]
            bank.add_ragged_pcm(raws, fmt)
        elif form == "device" and max(frames) > 0:
            longest = max(frames)
            if longest > cap:
                if scratch is not None: scratch.close()
                cap = longest
                scratch = ssa.Batch(rate, ch, n, cap, flags=L.SS_BATCH_LUFS)
            padded = np.zeros((n, cap * ch), np.float32)
            for s in range(n): padded[s, :blocks[s].size] = blocks[s]
            scratch.upload(0, padded)
            scratch.sync()
            bank.add_ragged_device(scratch.input_device_ptr(), frames, cap * ch)
        else:
            bank.add_ragged([b if f else None for b, f in zip(blocks, frames)])
        for s in range(n):
            if frames[s]: handles[s].add_samples(blocks[s])
            fed[s] += frames[s]
        rec = bank.read()
        for s in range(n):
            why = stream_against_handle(bank, s, rec[s], handles[s], fed[s])
            if why: return False, f"{tag} call {k} ({form}, frames {frames}) stream {s}: {why}"
        if rng.random() < 0.15:
            which = [s for s in range(n) if rng.random() < 0.4]
            if which:
                bank.reset(which)
                for s in which:                                  # (a fresh handle: what a reset stream must equal)
                    handles[s] = fresh(); fed[s] = 0
    if scratch is not None: scratch.close()
    return True, tag


if __name__ == "__main__":
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    bad = 0
    for seed in range(first, first + count):
        ok, msg = programme(seed)
        if not ok:
            print("FAIL", msg, flush=True); bad += 1
    print(f"{count} programmes, {bad} failed")
    sys.exit(1 if bad else 0)
