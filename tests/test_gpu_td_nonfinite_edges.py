"""An infinity in the last frames of a sub-block, of a tile and of a chunk, through the batch forms of `k_time_domain`, against the
oracle's meter.

Where an infinity turns into a NaN inside the K-weighting decides which 100 ms sub-block carries a NaN energy and which +Inf: with
the sample at frame p the state v_p is an infinity, and the output of the NEXT step is b0 v_{p+1} + b1 v_p = Inf - Inf = NaN — so
an infinity in the second-to-last frame of a sub-block makes THAT sub-block's energy NaN (the gating block that ends with it is
dropped), one in the very last frame leaves it +Inf (a block counted in the highest histogram bin, which then dominates the
integrated loudness).  The batch kernels' unit-gain output taps (y / b0 = x + g1 v1 + ...) would stay an infinity one step longer;
tiles with a non-finite value in reach run the gained taps, and this file holds them to the crate's placement: S - 2 and S - 1 of
a sub-block, the last two frames of a tile inside a sub-block (the state another tile — in the shared forms another wave —
starts from), of a 30-frame chunk, of a segment and of the stream, either sign, either channel, in the one-wave segments with the
fix-up launch, the eight-wave segments of a few files and whole-stream workgroups."""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from conftest import make_stereo

pytestmark = pytest.mark.gpu

RATE, S, TILE, CHUNK = 48000, 4800, 960, 30
FLAGS = L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK | L.SS_BATCH_WAVEFORM
TOL = 1e-9

# (frame inside the stream, what it is)
def _positions(frames, seg):
    sb = 27 * S                       # a sub-block well inside the stream (segment 1 or later of every geometry below)
    p = [sb + S - 2, sb + S - 1,                         # the sub-block's last two frames
         sb + 2 * TILE - 2, sb + 2 * TILE - 1,           # a tile's, inside the sub-block
         sb + TILE + 7 * CHUNK - 2, sb + TILE + 7 * CHUNK - 1,   # a chunk's, inside a tile
         seg - 2, seg - 1, seg + S - 2, seg + S - 1,     # a segment's, and its first (fix-up) sub-block's
         frames - 2, frames - 1]
    return [q for q in p if 0 <= q < frames]


def _same(a, b):
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= TOL


def _run(oracle, ns, frames, mode, want, shift=0):
    b = ssa.Batch(RATE, 2, ns, frames, 4096, 1024, flags=FLAGS)
    try:
        b.set_time_domain_mode(mode)
        g = b.geometry
        want(g)
        seg = g.td_segment_subblocks * S if g.td_segments > 1 else 13 * S
        pos = _positions(frames, seg)
        xs = []
        for i in range(ns):
            x = make_stereo(900 + i, frames, RATE, level=0.8)
            k = i + shift
            q = pos[k % len(pos)]
            x[2 * q + ((k // len(pos)) & 1)] = np.float32(np.inf if k % 2 == 0 else -np.inf)
            xs.append(x)
        b.upload(0, np.concatenate(xs))
        b.run(); b.sync()
        res = b.results()
        bad = []
        for i in range(ns):
            m = oracle.Meter(2, RATE)
            m.add_frames(xs[i])
            if not (_same(res[i].integrated_lufs, m.integrated()) and _same(res[i].loudness_range, m.loudness_range())):
                bad.append((i, pos[(i + shift) % len(pos)], res[i].integrated_lufs, m.integrated(), res[i].loudness_range, m.loudness_range()))
        assert not bad, bad
    finally:
        b.close()


def test_fixup_segments(oracle):
    def want(g):
        assert g.td_split == 0 and g.td_segments > 1 and g.td_fixup_subblocks > 0, (g.td_split, g.td_segments, g.td_fixup_subblocks)
    _run(oracle, 24, 5 * RATE, L.SS_TD_AUTO, want)


def test_eight_wave_segments_of_a_few_files(oracle):
    def want(g):
        assert g.td_split == 2 and g.td_segments > 1, (g.td_split, g.td_segments)
    _run(oracle, 8, 5 * RATE, L.SS_TD_AUTO, want)
    _run(oracle, 8, 5 * RATE, L.SS_TD_AUTO, want, shift=16)


def test_whole_stream_workgroups(oracle):
    def want(g):
        assert (g.td_split, g.td_segments) == (1, 1), (g.td_split, g.td_segments)
    _run(oracle, 24, 5 * RATE, L.SS_TD_WHOLE_STREAMS, want)
