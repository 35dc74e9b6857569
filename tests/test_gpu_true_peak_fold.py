"""The folded VALU true peak (factor 4) where one of its two terms cancels, against the f64 interpolator.

The kernels take max(|y1|, |y3|) as |s| + |d| with s = (y1 + y3) / 2 and d = (y1 - y3) / 2 (sst::true_peak_fold4).  A burst that is
symmetric about a point half-way between two samples gives y1 = y3 there (d cancels); an antisymmetric one gives y1 = -y3 (s
cancels).  Bursts of twelve frames of either kind are picked so that the true peak lies on branch 1 or 3, at least 1.2x the sample
peak, and one is planted per (stream, channel) over silence, walking across tile and lane-run boundaries.  2 and 8 channels run
the packed form, 3 channels the plain one."""
import numpy as np
import pytest
from scipy import signal

import soundscope_amd as ssa
from soundscope_amd import _lib as L
import _f64ref as R

pytestmark = pytest.mark.gpu

RATE, NS, FRAMES = 48000, 64, 48000
TP_REL = 1e-6


def _bursts(kind, n, seed):
    """n bursts of twelve frames, mirrored (kind 'sym') or mirrored and negated ('anti') about their middle, whose true peak lies
    on branch 1 or 3 and is at least 1.2x their sample peak; with that true peak in f64"""
    h = R.interpolator_taps(4)
    rng = np.random.default_rng(seed)
    out, tps = [], []
    while len(out) < n:
        half = rng.uniform(-1, 1, 6)
        burst = np.concatenate([half[::-1], half if kind == "sym" else -half]).astype(np.float32)
        y = signal.upfirdn(h, np.concatenate([np.zeros(16), burst, np.zeros(16)]).astype(np.float64), up=4)
        i = int(np.argmax(np.abs(y)))
        if i % 4 in (1, 3) and abs(y[i]) >= 1.2 * float(np.abs(burst).max()):
            out.append(burst)
            tps.append(float(np.abs(y).max()))
    return out, np.array(tps)


@pytest.mark.parametrize("channels", [2, 3, 8])
@pytest.mark.parametrize("kind", ["sym", "anti"])
def test_folded_true_peak_where_a_term_cancels(channels, kind):
    n = NS * channels
    bursts, want = _bursts(kind, n, 11 + channels + (kind == "anti"))
    x = np.zeros((NS, FRAMES, channels), np.float32)
    for j in range(n):
        i, c = divmod(j, channels)
        pos = 960 * (1 + j % 40) + (j * 7) % 61 - 30           # both sides of a tile boundary, every lane-run phase
        x[i, pos:pos + 12, c] = bursts[j]
    b = ssa.Batch(RATE, channels, NS, FRAMES, 4096, 1024, flags=L.SS_BATCH_LUFS | L.SS_BATCH_TRUE_PEAK, true_peak_factor=0)
    try:
        b.set_true_peak_arith(L.SS_TP_ARITH_F32)
        assert b.geometry.td_true_peak_factor == 4
        for i in range(NS):
            b.upload(i, x[i].reshape(-1))
        b.run()
        b.sync()
        worst = 0.0
        for i in range(NS):
            tp, sp = b.peaks(i)
            ref = want[i * channels:(i + 1) * channels]
            assert np.array_equal(sp, np.abs(x[i]).max(axis=0).astype(np.float64))
            rel = np.abs(tp - ref) / ref
            worst = max(worst, float(rel.max()))
            assert rel.max() <= TP_REL, (channels, kind, i, tp, ref)
        print("%d channels, %s: worst true-peak error %.2e" % (channels, kind, worst))
    finally:
        b.close()
