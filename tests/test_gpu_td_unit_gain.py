"""The batch instantiations of `k_time_domain` run the K-weighting's output taps with the gain b0 taken out and referred to the
input (y / b0 = x + g1 v1 + ... + g4 v4, g_k = (b_k - b0 a_k) / b0) and scale a tile's energy by b0^2 where it joins the sub-block's.
Energies may move by rounding, nothing else.

Reference: the sequential f64 filter of tests/_f64ref.py (not the oracle), and — from its sub-block energies — ebur128's gating in
histogram mode restated here from the published definitions (1000 bins of 0.1 LU from -70 LUFS; integrated: 400 ms blocks every
100 ms, -70 LUFS absolute and -10 LU relative gate; range: 3 s blocks every second, -20 LU relative gate, the 10th and 95th
percentile).

Bounds.  Integrated loudness and loudness range: within 1e-9 LU, what tests/test_gpu_parity.py holds them to (measured here:
3.6e-15 LU, parent and new).  Sub-block energies, relative to the sub-block's own energy: the parity tests' 1e-10
(tests/test_gpu_time_domain_forms.py, `_e(48000)`) is for stationary material; this file's material steps its level by up to 30 dB
every 0.7 s so that the relative gates cut, and a quiet sub-block behind a loud one carries the loud one's rounding — the parent
kernel itself reads 1.18e-10 / 1.60e-10 / 3.76e-10 on the first three shapes below, the new one 1.12e-10 / 1.57e-10 / 3.60e-10 (one
MI355X; also in profiles/td_tile_ledger.txt).  The bound is the larger worst value with a factor two: 2 x 3.76e-10 -> 7.6e-10.

Shapes: 2 streams x 1.0 s (one segment per stream); 8 streams x 10 s cut into segments; 16 streams x 10 s, where the planner takes
one-wave segments with the fix-up launch (asserted from the geometry: at 8 streams it deals a segment's tiles to eight waves and runs
the filter in over the segment in front instead, no second launch — both hand-overs are batch instantiations); 1 stream x 0.35 s (a
trailing partial sub-block); and the two forms side by side on one handle: streaming `add_samples`, a one-shot batch pass
(`calculate_integrated_lufs`) in between, `add_samples` again.  (No entry point runs a streaming call on a state a batch launch
wrote — a batch zeroes its meter in front of every pass and a handle's launches all publish y — so TdState::acc is never read
across the two forms; it is in y's units in both.)"""
import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
import _f64ref as R

pytestmark = pytest.mark.gpu

RATE = 48000
E_REL = 7.6e-10        # sub-block energies, relative: see the docstring
LU_ABS = 1e-9          # integrated loudness and loudness range (test_gpu_parity)
FLAGS = L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK | L.SS_BATCH_WAVEFORM

# worst values over the cases of this file on one MI355X: (sub-block energy rel, integrated LU, range LU)
MEASURED_PARENT = (3.76e-10, 3.6e-15, 3.6e-15)
MEASURED_NEW = (3.60e-10, 3.6e-15, 3.6e-15)


def _material(seed, frames, ch=2):
    """programme-like: two sines and noise per channel under a level that steps every 0.7 s over 30 dB (so that the relative
    gates cut and the range is not zero)"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / RATE
    steps = 10.0 ** (rng.uniform(-32.0, -2.0, frames // int(0.7 * RATE) + 1) / 20.0)
    g = np.repeat(steps, int(0.7 * RATE))[:frames]
    x = np.empty((frames, ch))
    for c in range(ch):
        f1, f2 = np.exp(rng.uniform(np.log(60.0), np.log(9000.0), 2))
        x[:, c] = g * (0.5 * np.sin(2 * np.pi * f1 * t + c) + 0.3 * np.sin(2 * np.pi * f2 * t) + 0.1 * rng.uniform(-1, 1, frames))
    return x.astype(np.float32)


_BOUNDS = 10.0 ** ((np.arange(1001) / 10.0 - 70.0 + 0.691) / 10.0)
_ENERGIES = 10.0 ** ((np.arange(1000) / 10.0 - 69.95 + 0.691) / 10.0)


def _hist(e):
    e = e[e >= _BOUNDS[0]]
    idx = np.clip(np.searchsorted(_BOUNDS, e, side="right") - 1, 0, 999)
    return np.bincount(idx, minlength=1000).astype(np.float64)


def _gate_start(level):
    if level < _BOUNDS[0]:
        return 0
    i = int(np.clip(np.searchsorted(_BOUNDS, level, side="right") - 1, 0, 999))
    return i + 1 if level > _ENERGIES[i] else i


def _integrated(sub):
    """(integrated LUFS, loudness range) from [sub-block][channel] energies of stereo material (weights 1, 1)"""
    S = R.subblock_frames(RATE)
    c = np.concatenate([[0.0], np.cumsum(sub.sum(axis=1))])
    n = sub.shape[0]
    blocks = (c[4:] - c[:-4]) / (4 * S) if n >= 4 else np.zeros(0)
    ends = np.arange(30, n + 1, 10)
    st = (c[ends] - c[ends - 30]) / (30 * S) if ends.size else np.zeros(0)
    h = _hist(blocks)
    integ = -np.inf
    if h.sum():
        start = _gate_start(0.1 * (h @ _ENERGIES) / h.sum())
        if h[start:].sum():
            integ = 10.0 * np.log10((h[start:] @ _ENERGIES[start:]) / h[start:].sum()) - 0.691
    h = _hist(st)
    lra = 0.0
    if h.sum():
        start = _gate_start(0.01 * (h @ _ENERGIES) / h.sum())
        size = int(h[start:].sum())
        if size:
            cum = np.cumsum(h[start:])
            lo = start + int(np.searchsorted(cum, int((size - 1) * 0.1 + 0.5), side="right"))
            hi = start + int(np.searchsorted(cum, int((size - 1) * 0.95 + 0.5), side="right"))
            lra = 10.0 * np.log10(_ENERGIES[hi]) - 10.0 * np.log10(_ENERGIES[lo])
    return integ, lra


@pytest.fixture(scope="module")
def worst():
    w = {"energy": 0.0, "integrated": 0.0, "range": 0.0}
    yield w
    print("\nunit-gain taps, worst over the cases run: sub-block energy %.3g (relative), integrated %.3g LU, range %.3g LU"
          % (w["energy"], w["integrated"], w["range"]))


def _run_batch(ns, frames, seed, worst, want):
    x = np.stack([_material(seed + i, frames) for i in range(ns)])
    refs = [R.kweighted_subblocks(x[i].reshape(-1), RATE, 2) for i in range(ns)]
    b = ssa.Batch(RATE, 2, ns, frames, 4096, 1024, flags=FLAGS)
    try:
        g = b.geometry
        want(g)
        b.upload(0, x.reshape(-1))
        b.run(); b.sync()
        res = b.results()
        bad = []                                               # every figure is taken (and printed) before anything is asserted
        for i in range(ns):
            ref = refs[i]
            got = b.subblocks(i)[:ref.shape[0]]
            assert got.shape == ref.shape, (i, got.shape, ref.shape)
            if ref.size:
                rel = float((np.abs(got - ref) / ref).max())
                worst["energy"] = max(worst["energy"], rel)
                if not rel <= E_REL:
                    bad.append(("energy", i, rel))
            integ, lra = _integrated(ref)
            if np.isfinite(integ):
                d = abs(res[i].integrated_lufs - integ)
                worst["integrated"] = max(worst["integrated"], d)
                if not d <= LU_ABS:
                    bad.append(("integrated", i, res[i].integrated_lufs, integ))
            elif res[i].integrated_lufs != integ:
                bad.append(("integrated", i, res[i].integrated_lufs, integ))
            d = abs(res[i].loudness_range - lra)
            worst["range"] = max(worst["range"], d)
            if not d <= LU_ABS:
                bad.append(("range", i, res[i].loudness_range, lra))
        print("\n%d x %d frames: worst so far energy %.3g, integrated %.3g LU, range %.3g LU" % (ns, frames, worst["energy"], worst["integrated"], worst["range"]))
        assert not bad, bad
    finally:
        b.close()


def test_one_segment(worst):
    def want(g):
        assert g.td_segments == 1, g.td_segments
    _run_batch(2, RATE, 100, worst, want)


def test_segments_of_eight_streams(worst):
    def want(g):
        assert g.td_segments > 1, g.td_segments
    _run_batch(8, 10 * RATE, 200, worst, want)


def test_segments_with_the_fixup_launch(worst):
    def want(g):
        assert g.td_segments > 1 and g.td_fixup_subblocks > 0 and g.td_split == 0, (g.td_segments, g.td_fixup_subblocks, g.td_split)
    _run_batch(16, 10 * RATE, 300, worst, want)


def test_trailing_partial_subblock(worst):
    def want(g):
        assert g.td_segments == 1, g.td_segments
    _run_batch(1, int(0.35 * RATE), 400, worst, want)


def test_streaming_and_batch_forms_on_one_handle(worst):
    frames = 5 * RATE + 1234
    x = _material(500, frames).reshape(-1)
    other = _material(501, 3 * RATE + 77).reshape(-1)
    cut = 2 * (2 * RATE + 4321)                              # inside a sub-block
    an = ssa.Analyzer()
    try:
        an.create_loudness_meter(2, RATE)
        an.add_samples(x[:cut])
        got_other = an.calculate_integrated_lufs(2, other)   # a batch pass between the two streaming calls
        an.add_samples(x[cut:])
        integ, lra = _integrated(R.kweighted_subblocks(x, RATE, 2))
        d = abs(an.get_integrated_lufs() - integ)
        worst["integrated"] = max(worst["integrated"], d)
        print("handle: integrated %.9f (f64 %.9f)" % (an.get_integrated_lufs(), integ))
        assert d <= LU_ABS, (an.get_integrated_lufs(), integ)
        assert abs(an.get_loudness_range() - lra) <= LU_ABS, (an.get_loudness_range(), lra)
        io, _ = _integrated(R.kweighted_subblocks(other, RATE, 2))
        d = abs(got_other - io)
        worst["integrated"] = max(worst["integrated"], d)
        print("one-shot: integrated %.9f (f64 %.9f)" % (got_other, io))
        assert d <= LU_ABS, (got_other, io)
    finally:
        an.close()
