"""The N = 4096 spectrum kernels give, bit for bit, the rows recorded in tests/golden/spectrum_window_loop_v1.npz at the commit
named in its `commit` entry — the parent of the change that took the launch constants and the dead moves out of k_fft4096_ms1's
window loop and the shared dB epilogue, which was to leave every output bit where it was.  The cases are the smallest shapes that
walk every line that change touched (tests/golden/make_spectrum_window_loop.py describes them and records the file): a run of six
windows (first, slid, last), a ragged batch, exactly-zero squared magnitudes inside a non-empty row with and without the pink
table and beside an empty row, 96 kHz and 44.1 kHz, columns-only, and the siblings on the shared epilogue (mono, hop 512, hop 768)."""
import os

import numpy as np
import pytest

from golden import make_spectrum_window_loop as M

pytestmark = pytest.mark.gpu

G = np.load(M.PATH)


def test_fixture_is_whole():
    assert os.path.getsize(M.PATH) < M.MAX_BYTES
    assert set(M.NAMES) <= set(G.files) and len(str(G["commit"])) == 40
    assert all(G[n].dtype == np.uint8 and G[n].shape[0] == 4 for n in M.NAMES)


@pytest.mark.parametrize("name", M.NAMES)
def test_rows_equal_the_recorded_bits(name):
    res, _ = M.run_case(name)
    got, want = M.planes(res), G[name]
    assert got.shape == want.shape, (name, got.shape, want.shape)
    words = np.flatnonzero((got != want).any(axis=0))
    assert words.size == 0, (name, "%d of %d words differ, the first at %d" % (words.size, got.shape[1], words[0]))
