"""Meter-bank spectra on the MI355X: every row of every stream against the oracle's get_fft on the stream's newest 16384 frames
(after every call of an irregular feed), bit for bit against the product's own ss_get_fft, the crate's refusals per row, the
fused chart columns against the rows and the oracle's render rule, the history's semantics, and 1024 live stereo inputs."""
import ctypes as C

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L
from soundscope_amd.meter_bank import MeterBank

from conftest import db_close, make_multich, make_stereo
from oracle.render import spectrum_columns_f32

pytestmark = pytest.mark.gpu

N = 16384
FEEDS = [1, 127, 4801, 16384, 16385, 0, 48000, 3, 480]


def material(seed, frames, channels, rate, level=0.5):
    """[frames, channels] f32"""
    if channels == 2:
        return make_stereo(seed, frames, rate, level=level).reshape(frames, 2)
    return make_multich(seed, frames, channels, rate, level=level).reshape(frames, channels)


class History:
    """The host's copy of every stream's input: [stream] lists of [frames, channels] blocks."""

    def __init__(self, n, channels):
        self.blocks = [[] for _ in range(n)]
        self.channels = channels

    def add(self, data):                                  # data [n, frames, channels]
        for s in range(len(self.blocks)):
            self.blocks[s].append(np.asarray(data[s], np.float32))

    def window(self, s):
        """The newest N frames of stream s with zeros in front: [N, channels] f32."""
        x = np.concatenate([np.zeros((N, self.channels), np.float32)] + self.blocks[s], axis=0)
        return x[-N:]


def signals(win):
    """The rows' signals of one window: mid, side for stereo (the oracle's mid_side), otherwise the channels."""
    from oracle import pyoracle as po
    if win.shape[1] == 2:
        return list(po.mid_side(win.reshape(-1)))
    return [np.ascontiguousarray(win[:, c]) for c in range(win.shape[1])]


def handle_fft(an, x):
    """ss_get_fft on the product's own handle: (status, [bins, 2] f64)."""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty((N // 2 + 1, 2), np.float64)
    n = C.c_size_t(0)
    rc = L.lib().ss_get_fft(an._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, out.ctypes.data_as(C.POINTER(C.c_double)),
                            out.shape[0], C.byref(n))
    return rc, out[:n.value].copy()


def oracle_fft(rate, x):
    """(status, [bins, 2] f64) of the oracle's get_fft."""
    from oracle import pyoracle as po
    try:
        return L.SS_OK, po.get_fft(rate, x)
    except po.OracleError as e:
        return e.code, None


def check_rows(bank, hist, rate, tag):
    rows, st = bank.spectrum()
    pink = bank.spectrum_pink()
    _, nb, chart_x = bank.spectrum_layout()
    for s in range(bank.n_streams):
        for r, sig in enumerate(signals(hist.window(s))):
            rc, ref = oracle_fft(rate, sig)
            assert st[s, r] == rc, (tag, s, r, st[s, r], rc)
            if rc:
                assert np.isnan(rows[s, r]).all(), (tag, s, r)
                continue
            assert ref.shape[0] == nb and np.array_equal(ref[:, 0], chart_x), tag
            assert db_close(rows[s, r].astype(np.float64) + pink, ref[:, 1]), (tag, s, r)
    return rows, st


@pytest.mark.parametrize("rate", [44100, 48000, 96000])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_oracle_parity_irregular_feeds(rate, channels):
    n = 3
    bank = MeterBank(n, channels, rate)
    bank.enable_spectrum()
    r, _, _ = bank.spectrum_layout()
    assert r == (2 if channels == 2 else channels)
    hist = History(n, channels)
    check_rows(bank, hist, rate, "empty")
    for i, f in enumerate(FEEDS):
        data = np.stack([material(100 * i + s + channels, f, channels, rate) if f else np.zeros((0, channels), np.float32)
                         for s in range(n)])
        bank.add(data)
        hist.add(data)
        check_rows(bank, hist, rate, (rate, channels, i, f))


@pytest.mark.parametrize("channels", [1, 2, 6])
def test_rows_bit_equal_to_the_handle(channels):
    """(double)row + pink is ss_get_fft's value bit for bit, chart_x its x: window starts even, odd, at a multiple of 16384, and
    the first 16383 frames (windows partly zero)."""
    rate, n = 48000, 2
    bank = MeterBank(n, channels, rate)
    bank.enable_spectrum()
    an = ssa.Analyzer(2, rate)
    pink = bank.spectrum_pink()
    _, _, chart_x = bank.spectrum_layout()
    hist = History(n, channels)
    for i, f in enumerate([1000, 3, 12380, 1, N - 1, 7, 4096 * 3 + 1]):      # totals: 1000 1003 13383 13384 (+N-1) ... (+7) ...
        data = np.stack([material(7 * i + s, f, channels, rate) for s in range(n)])
        bank.add(data)
        hist.add(data)
        rows, st = bank.spectrum()
        for s in range(n):
            for r, sig in enumerate(signals(hist.window(s))):
                rc, ref = handle_fft(an, sig)
                assert rc == L.SS_OK and st[s, r] == L.SS_OK
                assert np.array_equal(ref[:, 0], chart_x)
                got = rows[s, r].astype(np.float64) + pink
                assert np.array_equal(got, ref[:, 1]), (i, s, r, np.abs(got - ref[:, 1]).max())
    assert sum(b.shape[0] for b in hist.blocks[0]) > N


def test_refusals_per_row():
    """NaN, +-inf, inf under the zero window weight, L = +inf with R = -inf, finite samples that overflow the mid, and finite
    samples loud enough that the magnitude's square overflows: each row's status is what ss_get_fft and the oracle return; the
    other streams are unaffected; the row returns to SS_OK once the sample has left the window."""
    rate = 48000
    big = np.float32(3.0e38)
    plants = {0: (100, (np.nan, 0.0)), 1: (200, (np.inf, 0.0)), 2: (300, (-np.inf, 0.0)), 3: (300, (np.inf, -np.inf)),
              4: (400, (big, big)), 5: (None, None), 6: (500, (0.0, np.nan))}
    n = 8
    bank = MeterBank(n, 2, rate)
    bank.enable_spectrum()
    an = ssa.Analyzer(2, rate)
    hist = History(n, 2)
    # stream 5: a full-scale-ish DC-free square wave whose bins overflow f32 squares: samples of 1e19 alternate in sign
    block = N
    data = np.stack([material(s, block, 2, rate) for s in range(n)])
    data[5] = np.float32(1.5e19) * np.where((np.arange(block) // 2) % 2, 1.0, -1.0).astype(np.float32)[:, None]
    for s, (off, v) in plants.items():
        if off is not None:
            data[s, off] = v
    data[7, 0] = (np.inf, np.inf)                        # the window's first frame: zero weight -> NaN
    bank.add(data)
    hist.add(data)
    rows, st = bank.spectrum()
    for s in range(n):
        for r, sig in enumerate(signals(hist.window(s))):
            rc_h, _ = handle_fft(an, sig)
            rc_o, _ = oracle_fft(rate, sig)
            assert st[s, r] == rc_h == rc_o, (s, r, st[s, r], rc_h, rc_o)
            if st[s, r]:
                assert np.isnan(rows[s, r]).all()
    assert st[0, 0] == st[0, 1] == L.SS_ERR_NAN
    assert st[1, 0] == st[1, 1] == L.SS_ERR_INFINITY and st[2, 0] == L.SS_ERR_INFINITY
    assert st[3, 0] == L.SS_ERR_NAN and st[3, 1] == L.SS_ERR_INFINITY
    assert st[4, 0] == L.SS_ERR_INFINITY and st[4, 1] == L.SS_OK
    assert L.SS_ERR_SCALING in st[5]
    assert st[7, 0] == st[7, 1] == L.SS_ERR_NAN
    # columns carry the refusal as NaN
    cols, cst = bank.spectrum_columns(160, 0.0)
    assert np.array_equal(cst, st)
    assert np.isnan(cols[st != 0]).all()
    # the meters read as on a bank without the spectrum fed the same samples
    twin = MeterBank(n, 2, rate)
    twin.add(data)
    assert bank.read().tobytes() == twin.read().tobytes()
    # a clean block of N frames pushes every planted sample out of the window
    clean = np.stack([material(50 + s, N, 2, rate) for s in range(n)])
    bank.add(clean)
    hist.add(clean)
    rows, st = bank.spectrum()
    assert (st == L.SS_OK).all()
    for s in range(n):
        for r, sig in enumerate(signals(hist.window(s))):
            rc, ref = handle_fft(an, sig)
            assert rc == L.SS_OK and np.array_equal(rows[s, r].astype(np.float64) + bank.spectrum_pink(), ref[:, 1])


@pytest.mark.parametrize("cols", [1, 7, 160, 512])
def test_columns(cols):
    """Fixed and reference gain (one stream silent: integrated -inf): bit-equal to the header's rule on the bank's own rows,
    within 0.01 dB of the oracle's render rule where both lie inside (-100, 0)."""
    from oracle import pyoracle as po
    from oracle import render
    rate, n = 48000, 4
    bank = MeterBank(n, 2, rate)
    bank.enable_spectrum()
    hist = History(n, 2)
    pink = bank.spectrum_pink()
    _, _, chart_x = bank.spectrum_layout()
    for i, f in enumerate([4800, 20000, 481]):
        data = np.stack([material(11 * i + s, f, 2, rate, level=0.5 if s != 3 else 0.0) for s in range(n)])
        bank.add(data)
        hist.add(data)
        rows, st = bank.spectrum()
        assert (st == 0).all()
        integ = bank.read()["integrated"]
        assert integ[3] == -np.inf
        for gain in (0.0, 17.5, "reference"):
            got, cst = bank.spectrum_columns(cols, gain)
            assert (cst == 0).all()
            for s in range(n):
                g = np.float32(-13.0) - np.float32(integ[s]) if gain == "reference" else np.float32(gain)
                for r, sig in enumerate(signals(hist.window(s))):
                    v = (rows[s, r].astype(np.float64) + pink).astype(np.float32)
                    want = spectrum_columns_f32(v, chart_x, g, cols)
                    assert np.array_equal(got[s, r], want, equal_nan=True), (i, gain, s, r)
                    ref = render.spectrum_columns(po.get_fft(rate, sig), float(g), cols)
                    inside = (ref > -100) & (ref < 0) & (got[s, r] > -100) & (got[s, r] < 0)
                    assert np.all(np.abs(got[s, r][inside] - ref[inside]) <= 0.01), (i, gain, s, r)
                    assert np.array_equal(np.isnan(got[s, r]), np.isnan(ref))


def test_history_semantics():
    """A reset leaves the spectra alone; disabling and enabling again starts from zeros; a spectrum-off bank refuses; the device
    and PCM inputs feed the history like add; bad arguments and small capacities are refused."""
    from oracle import pyoracle as po
    rate, n = 48000, 3
    bank = MeterBank(n, 2, rate)
    for call in (lambda: bank.spectrum(), lambda: bank.spectrum_columns(10), lambda: bank.spectrum_layout()):
        with pytest.raises(ssa.AnalyzerError) as e:
            call()
        assert e.value.code == L.SS_ERR_INVALID_MODE
    bank.enable_spectrum()
    data = np.stack([material(s, 20000, 2, rate) for s in range(n)])
    bank.add(data)
    before, _ = bank.spectrum()
    bank.reset([1])
    bank.reset()
    after, _ = bank.spectrum()
    assert np.array_equal(before, after, equal_nan=True)
    bank.enable_spectrum(False)
    with pytest.raises(ssa.AnalyzerError):
        bank.spectrum()
    bank.enable_spectrum()
    zero, st = bank.spectrum()
    assert (st == 0).all() and (zero == np.float32(-150.0)).all()
    # device and PCM input against add on a twin bank
    twin = MeterBank(n, 2, rate)
    twin.enable_spectrum()
    a = np.stack([material(20 + s, 7001, 2, rate) for s in range(n)])
    b = np.stack([material(30 + s, 999, 2, rate) for s in range(n)])
    twin.add(a)
    src = ssa.Batch(rate, 2, n, 7001, flags=L.SS_BATCH_LUFS)             # a device buffer: stream s at s * 7001 * 2 floats
    src.upload(0, a.reshape(n, -1))
    bank.add_device(src.input_device_ptr(), 7001, 7001 * 2)
    pcm16 = np.clip(np.round(b * 32768.0), -32768, 32767).astype("<i2").reshape(n, -1)
    twin.add(np.stack([po.pcm_to_f32(pcm16[s].tobytes(), L.SS_PCM_S16) for s in range(n)]))
    bank.add_pcm(pcm16.tobytes(), L.SS_PCM_S16)
    x, sx = bank.spectrum()
    y, sy = twin.spectrum()
    assert np.array_equal(x, y) and np.array_equal(sx, sy)
    assert bank.read().tobytes() == twin.read().tobytes()
    # refusals
    lib = L.lib()
    f = np.empty(4, np.float32)
    s4 = np.empty(4, np.int32)
    fp, sp = f.ctypes.data_as(C.POINTER(C.c_float)), s4.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ss_meter_bank_spectrum(bank._h, fp, 4, sp, 4) == L.SS_ERR_CAPACITY
    assert lib.ss_meter_bank_spectrum_columns(bank._h, 0, 0, 0.0, fp, 4, sp, 4) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_columns(bank._h, 513, 0, 0.0, fp, 4, sp, 4) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_columns(bank._h, 2, 5, 0.0, fp, 4, sp, 4) == L.SS_ERR_INVALID_ARG
    assert lib.ss_meter_bank_spectrum_columns(bank._h, 2, 0, 0.0, fp, 4, sp, 4) == L.SS_ERR_CAPACITY
    x = np.empty(4, np.float64)
    assert lib.ss_meter_bank_spectrum_layout(bank._h, None, None, x.ctypes.data_as(C.POINTER(C.c_double)), None, 4) == \
        L.SS_ERR_CAPACITY
    low = MeterBank(1, 2, 32000)
    with pytest.raises(ssa.AnalyzerError) as e:
        low.enable_spectrum()
    assert e.value.code == L.SS_ERR_FREQ_LIMIT


def test_scale_1024_streams():
    """1024 stereo 48 kHz streams fed 10 ms blocks past 16384 frames: every status SS_OK, 8 sampled streams match the oracle,
    the columns of all streams equal the rows reduced on the host."""
    from oracle import pyoracle as po
    rate, n, blk = 48000, 1024, 480
    bank = MeterBank(n, 2, rate)
    bank.enable_spectrum()
    rng = np.random.default_rng(5)
    base = np.stack([material(s % 16, 40 * blk, 2, rate) for s in range(16)])
    gains = rng.uniform(0.1, 1.0, n).astype(np.float32)
    pieces = []
    for k in range(36):                                   # 17280 frames
        blockdata = base[np.arange(n) % 16, k * blk % (40 * blk - blk):][:, :blk] * gains[:, None, None]
        bank.add(blockdata)
        pieces.append(blockdata)
    rows, st = bank.spectrum()
    assert (st == 0).all()
    pink = bank.spectrum_pink()
    _, _, chart_x = bank.spectrum_layout()
    for s in rng.choice(n, 8, replace=False):
        win = np.concatenate([p[s] for p in pieces], axis=0)[-N:]
        for r, sig in enumerate(po.mid_side(win.reshape(-1))):
            ref = po.get_fft(rate, sig)
            assert db_close(rows[s, r].astype(np.float64) + pink, ref[:, 1]), (s, r)
    integ = bank.read()["integrated"]
    cols, cst = bank.spectrum_columns(160, "reference")
    assert (cst == 0).all()
    v = (rows.astype(np.float64) + pink).astype(np.float32)
    for s in range(n):
        g = np.float32(-13.0) - np.float32(integ[s])
        for r in range(2):
            assert np.array_equal(cols[s, r], spectrum_columns_f32(v[s, r], chart_x, g, 160), equal_nan=True), (s, r)
