"""The streaming plants of tests/_td_plants.py can fail (CPU only: f64 models, no device).

For every handle shape of the table test_gpu_streaming_td_forms.py runs, and every boundary class its schedule reaches, four
deliberately wrong f64 models — the interpolator history zeroed at the boundary, the history one frame late, the filter state
zeroed at the boundary, two channels swapped — must read at least 100x the GPU test's bar away from the true f64 reference, at
the read behind a boundary of that class: 1e-4 relative in a true peak, 1e-4 LU in the momentary reading.  Not every anchor can
show a history model: with the boundary behind the burst's tenth frame or in front of its third the peak does not move
(_td_plants.d_order).  Counted per class: of the anchors where some channel's offset d is 3 ... 9 — alone, such a burst moves by 1 %
and more under either history model — at least three quarters meet the margin (the others are masked: the next anchor's higher
burst of that channel already stands in the call that is read), and at least one anchor does for every model.  The same for the
ticks' material, per tick class.  A condition on the material (seeds, amplitudes, offsets), checked on the reference alone."""
import os
import subprocess
import sys
import collections

import numpy as np
import pytest

import _td_plants as P

TP_MARGIN = 100 * 1e-6          # 100 x the true-peak bar (relative)
LU_MARGIN = 100 * 1e-6          # 100 x the reading bar (LU)

SHAPES = sorted({(rate, ch) for _, rate, ch, _, k in P.HANDLE_SHAPES if k is None})


def test_plan_answers_with_no_device_visible():
    """a fresh process that sees no device gets the plan, and still sees no device afterwards"""
    code = ("import soundscope_amd as ssa; from soundscope_amd import _lib as L; p = ssa.streaming_plan(2, 48000, 8192); "
            "print(p.form, p.waves, p.tile_frames, p.chunk_frames, p.true_peak_factor, p.subblock_frames, p.piece_frames, L.lib().ss_device_count())")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["1", "8", "1200", "40", "4", "4800", "153600", "0"], (out.stdout, out.stderr)


def test_plan_forms_meet_at_one_tile():
    """the two forms meet at one tile of the one-wave form"""
    for rate, ch in SHAPES:
        one, shared = P.forms(ch, rate)
        assert one.tile >= 1 and shared.tile >= 1 and shared.waves in (4, 8) and one.factor == shared.factor == {44100: 4, 48000: 4, 96000: 2, 192000: 0}[rate]


def test_burst_material():
    """noise within 1e-3, amplitudes rising by at least 2 % per anchor, every channel its own offsets and amplitudes"""
    for rate, ch in ((48000, 2), (96000, 2), (48000, 5)):
        factor = P.forms(ch, rate)[0].factor
        for seg in P.handle_segments(ch, rate):
            assert P.growth(len(seg.anchors)) >= 1.02
            x, starts = P.plant(seg, ch, factor, 1)
            planted = np.zeros(x.shape, bool)
            for i, a in enumerate(seg.anchors):
                for c in range(ch):
                    if starts[i, c] >= 0:
                        assert not planted[starts[i, c]:starts[i, c] + P.SPAN, c].any(), (a, c)       # bursts never overlap
                        planted[starts[i, c]:starts[i, c] + P.SPAN, c] = True
            assert np.abs(x[~planted]).max() <= P.NOISE
            live = [i for i, a in enumerate(seg.anchors) if a.cls != P.RESET]
            assert len({tuple(a.b - starts[i]) for i, a in zip(live, (seg.anchors[i] for i in live))}) > 1
            if ch > 1:
                assert all(len(set(seg.anchors[i].b - starts[i])) == ch for i in live)              # channel c: its own offset
    # a class with enough anchors sweeps every offset
    seg = P.handle_segments(2, 48000)[0]
    _, starts = P.plant(seg, 2, 4, 1)
    seen = {int(a.b - s) for a, st in zip(seg.anchors, starts) for s in st if a.cls != P.RESET}
    assert seen == set(range(-2, P.SPAN + 12 + 3)), sorted(seen)


def enough(tag, n_telling, n_hit):
    assert n_hit >= max(1, -(-3 * n_telling // 4)), (tag, n_telling, n_hit)


@pytest.mark.parametrize("rate,ch", SHAPES, ids=["%d-%d" % s for s in SHAPES])
def test_wrong_models_are_caught(rate, ch):
    segs = P.handle_stream(ch, rate)
    starts = P.handle_starts(ch, rate)
    factor = segs[0][2].factor
    hits, telling = collections.Counter(), collections.Counter()
    reached = set()
    for si, (seg, x, ref) in enumerate(segs):
        for i, a in enumerate(seg.anchors):
            reached.add(a.cls)
            k = a.read
            tp = ref.true_peak(k)
            if a.cls == P.RESET:
                # the wrong model of a reset: none happened — the peaks and the filtered signal of the segment in front stand
                prev = segs[si - 1]
                stale = np.maximum(tp, prev[2].true_peak(len(prev[0].sizes) - 1))
                for m in ("zero", "shift", "swap"):
                    hits[a.cls, m] += float((np.abs(stale - tp) / tp).max()) >= TP_MARGIN
                both = P.SegRef(np.vstack([prev[1], x]), rate, factor, prev[0].sizes + seg.sizes)
                hits[a.cls, "state"] += abs(both.momentary(len(prev[0].sizes) + k) - ref.momentary(k)) >= LU_MARGIN
                continue
            telling[a.cls] += any(3 <= d <= 9 for d in a.b - starts[si][i])
            if factor:
                for m in ("zero", "shift"):
                    hits[a.cls, m] += float((np.abs(ref.wrong_history(a.b, k, m) - tp) / tp).max()) >= TP_MARGIN
            if ch > 1:
                hits[a.cls, "swap"] += float((np.abs(ref.wrong_swapped(k) - tp) / tp).max()) >= TP_MARGIN
            hits[a.cls, "state"] += abs(ref.wrong_filter_state(a.b, k) - ref.momentary(k)) >= LU_MARGIN
    # a one-wave tile of 50 frames (56 channels) is shorter than the sweep of d with its ringing: no anchor fits inside such a call
    must = set(P.CLASSES) - ({P.TILE_ONE} if P.forms(ch, rate)[0].tile < 100 else set())
    assert reached >= must, (must - reached)
    for cls in sorted(reached):
        for m in ("zero", "shift", "swap", "state"):
            if (m in ("zero", "shift") and not factor) or (m == "swap" and ch == 1):
                continue                                    # no interpolator at 192 kHz; one channel has none to swap with
            enough((rate, ch, cls, m), telling[cls] if m in ("zero", "shift") else 0, hits[cls, m])


def test_uniform_bank_sweep_is_caught():
    """the uniform bank's material (stream s: offset d_order[s + 7 c + anchor]): at EVERY anchor of every class, each history model
    is caught in at least 5 of the 29 burst streams (7 offsets of 29 lie in 3 ... 9), a zeroed state and a swap in at least one"""
    rate, ch, n, nt = 48000, 2, 32, 3
    segs = P.handle_segments(ch, rate, light=True)
    for i, seg in enumerate(segs):
        refs = []
        for s in range(nt, n):
            x = P.plant(seg, ch, 4, 7000 + 10 * s + i, turn=lambda a, c, s=s: s + 7 * c + a)[0]
            refs.append(P.SegRef(x, rate, 4, seg.sizes))
        for a in seg.anchors:
            if a.cls == P.RESET:
                continue
            tps = [r.true_peak(a.read) for r in refs]
            for m in ("zero", "shift"):
                n_hit = sum(float((np.abs(r.wrong_history(a.b, a.read, m) - tp) / tp).max()) >= TP_MARGIN for r, tp in zip(refs, tps))
                assert n_hit >= 5, (a, m, n_hit)
            assert any(abs(r.wrong_filter_state(a.b, a.read) - r.momentary(a.read)) >= LU_MARGIN for r in refs), a
            assert any(float((np.abs(r.wrong_swapped(a.read) - tp) / tp).max()) >= TP_MARGIN for r, tp in zip(refs, tps)), a


@pytest.mark.parametrize("rate", [48000, 44100, 96000, 192000])
def test_tick_material_catches_wrong_models(rate):
    """the file ticks' material, over the concatenated 8192-frame slices of each part (a restart between them): per tick class — a
    tile boundary of the fed stream's grid inside the slice, the slice's end — the four wrong models at the planted boundary, read
    behind that tick (the state model in the short-term reading, which is what a tick returns)"""
    n_ticks, restart_at = P.TICK_CASE
    x, pos, anchors = P.tick_file(rate, n_ticks, 11, restart_at)
    factor = P.forms(2, rate)[0].factor
    parts = [(0, restart_at), (restart_at, n_ticks)]
    refs = [P.SegRef(np.vstack([x[p - P.SLICE:p] for p in pos[a:b]]), rate, factor, [P.SLICE] * (b - a)) for a, b in parts]
    hits, telling, count = collections.Counter(), collections.Counter(), collections.Counter()
    order = P.d_order(factor)
    turn = collections.Counter()
    for a in anchors:
        part = a.tick >= restart_at
        ref, k = refs[part], a.tick - parts[part][0]
        ds = [order[(turn[a.cls] * 2 + c) % len(order)] for c in range(2)]
        turn[a.cls] += 1
        count[a.cls] += 1
        if a.b >= int(ref.ends[-1]):
            continue                                        # (the end of a part's last slice: nothing is fed behind it)
        read = k if a.cls == P.TICK_TILE else k + 1          # a slice's end is read behind the NEXT tick
        tp = ref.true_peak(read)
        telling[a.cls] += any(3 <= d <= 9 for d in ds)
        if factor:
            for m in ("zero", "shift"):
                hits[a.cls, m] += float((np.abs(ref.wrong_history(a.b, read, m) - tp) / tp).max()) >= TP_MARGIN
        hits[a.cls, "swap"] += float((np.abs(ref.wrong_swapped(read) - tp) / tp).max()) >= TP_MARGIN
        hits[a.cls, "state"] += abs(ref.wrong_filter_state(a.b, read, 30) - ref.shortterm(read)) >= LU_MARGIN
    # A slice's end: whatever stands there stands again, whole, 1024 frames further in the next slice — the history models show only
    # where the cut burst reads higher than the whole one: at least one anchor.  A tile boundary inside the slice: three quarters.
    for cls in (P.TICK_TILE, P.TICK_END):
        assert count[cls] >= len(order) // 2, (cls, count[cls])             # two channels: every offset has its turn
        for m in ("zero", "shift", "swap", "state"):
            if m in ("zero", "shift") and not factor:
                continue
            enough((rate, cls, m), telling[cls] if m in ("zero", "shift") and cls == P.TICK_TILE else 0, hits[cls, m])
