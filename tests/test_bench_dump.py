"""bench.py --dump-outputs on CPU: the files it writes from a batch (a stand-in with the batch's getters and layout), their
dtypes, the 64 MB cap, the seeded sample being the same from run to run, and the index arrays naming the rows written."""
import importlib
import os
import sys
import types
from unittest import mock

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    with mock.patch.dict(os.environ):              # bench.py sets RCCL / HSA defaults at import: keep them out of this session
        return importlib.import_module("bench")


class StandInBatch:
    """Batch's layout and getters, with every value a function of (stream, position) so that misplaced rows show."""

    def __init__(self, streams, windows, bins, wave_points, subblocks, channels=2):
        self.layout = types.SimpleNamespace(n_windows=windows, fft_channels=2, n_bins=bins, n_wave_points=wave_points,
                                            n_subblocks=subblocks)
        self.cfg = types.SimpleNamespace(n_streams=streams, channels=channels)

    def results(self):
        return [types.SimpleNamespace(integrated_lufs=-20.0 - s, loudness_range=float(s), true_peak=[0.5, 0.25 + s],
                                      sample_peak=[0.4, 0.2], n_gating_blocks=s, n_st_blocks=2 * s)
                for s in range(self.cfg.n_streams)]

    def fft(self, s):
        L = self.layout
        return (np.arange(L.n_windows * 2 * L.n_bins, dtype=np.float64).reshape(L.n_windows, 2, L.n_bins) + 1e6 * int(s)).astype(np.float32)

    def waveform(self, s):
        return (np.arange(self.layout.n_wave_points, dtype=np.float64) + 1e7 * int(s)).astype(np.float32).reshape(-1, 2)

    def subblocks(self, s):
        return np.arange(self.layout.n_subblocks * self.cfg.channels, dtype=np.float64).reshape(-1, self.cfg.channels) + 1e7 * int(s)

    def histograms(self):
        return np.arange(1000, dtype=np.uint64), 2 * np.arange(1000, dtype=np.uint64)


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("shape", [(1024, 465, 1705, 20000, 100),        # the bench's step: 1024 x 10 s at 48 kHz, N = 4096
                                   (16, 28000, 1705, 1200000, 6000)])    # 600 s streams: every per-stream kind is sampled
def test_dump_is_capped_seeded_and_indexed(bench, tmp_path, shape):
    b = StandInBatch(*shape)
    first = 4096
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(b, first, (-23.5, 6.25), a_dir)
    bench.dump_outputs(StandInBatch(*shape), first, (-23.5, 6.25), b_dir)
    assert sum(os.path.getsize(os.path.join(a_dir, f)) for f in os.listdir(a_dir)) <= 64 * 10**6
    A, B = load(a_dir), load(b_dir)
    assert A.keys() == B.keys()
    for name in A:
        assert A[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(A[name], B[name]), name
    streams = A["streams"].astype(np.int64) - first
    assert 0 < streams.size <= 64 and np.all(np.diff(streams) > 0)
    win, wbin, sub = (A[k].astype(np.int64) for k in ("spectrum_windows", "waveform_bins", "subblocks_index"))
    for i, s in enumerate(streams):
        assert np.array_equal(A["spectrum"][i], b.fft(s)[win])
        assert np.array_equal(A["waveform"][i], b.waveform(s)[wbin])
        assert np.array_equal(A["subblocks"][i], b.subblocks(s)[sub])
    rs = A["results_streams"].astype(np.int64) - first
    assert np.array_equal(A["results"][:, 0], -20.0 - rs) and np.array_equal(A["results"][:, 7], 2.0 * rs)
    assert np.array_equal(A["histograms"][1], 2.0 * np.arange(1000))
    assert list(A["corpus_gate"]) == [-23.5, 6.25]
