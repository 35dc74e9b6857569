"""PCM export (ss_batch_download_pcm): the resident f32 corpus in a delivery format, the inverse of ss_batch_upload_pcm.

The reference is the header's recipe restated in numpy, in this file: v = x * scale in f32 (exact), with dither one rounded f32
addition of the counter-based TPDF value, q = rint(v) (halves to even) saturated to [-scale, scale - 1], NaN -> 0, unsigned 8-bit
stores q + 128.  Everything must be EQUAL byte for byte.  The round trip holds for every integer an f32 sample can carry: all of
U8, S16 and S24, and for S32 the integers of 24 significant bits (random 24-bit values times 256: the full range, the corpus
itself is f32)."""
import ctypes
import math

import numpy as np
import pytest

import soundscope_amd as ssa
from soundscope_amd import _lib as L

pytestmark = pytest.mark.gpu

SCALE = {L.SS_PCM_U8: 128.0, L.SS_PCM_S16: 32768.0, L.SS_PCM_S24: 8388608.0, L.SS_PCM_S32: 2147483648.0}
M32 = np.uint64(0xFFFFFFFF)


def make_batch(channels, streams, frames):
    return ssa.Batch(48000, channels, streams, frames, 4096, 1024, flags=L.SS_BATCH_TRUE_PEAK)


# ------------------------------------------------------------------------------------------------------------ reference
def mix(v):
    v = v & M32
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & M32
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & M32
    return v ^ (v >> np.uint64(16))


def tpdf(seed, stream, n):
    """the dither of samples i = frame * channels + channel = 0 .. n - 1 of `stream`, f32"""
    i = np.arange(n, dtype=np.uint64)
    hi, lo = np.uint64(seed >> 32), np.uint64(seed & 0xFFFFFFFF)
    k = mix(mix(mix(np.full(1, hi ^ np.uint64(stream), np.uint64)) ^ lo) ^ (i >> np.uint64(32))) ^ (i & M32)
    u1, u2 = mix(k) >> np.uint64(8), mix(k ^ np.uint64(0x80000000)) >> np.uint64(8)
    d = (u1.astype(np.int64) - u2.astype(np.int64)).astype(np.float32) * np.float32(2.0 ** -24)
    assert (np.abs(d) < 1).all()
    return d


def quantise(x, fmt, d=None):
    """x f32 (any shape) -> int64 q"""
    scale = SCALE[fmt]
    with np.errstate(over="ignore", invalid="ignore"):
        v = x.astype(np.float32) * np.float32(scale)
        if d is not None:
            v = v + d.astype(np.float32)
        r = np.rint(v).astype(np.float64)
    r[np.isnan(r)] = 0.0
    return np.clip(r, -scale, scale - 1).astype(np.int64)


def encode(q, fmt):
    """int64 q -> the format's bytes as download_pcm hands them back"""
    if fmt == L.SS_PCM_U8:
        return (q + 128).astype(np.uint8)
    if fmt == L.SS_PCM_S16:
        return q.astype(np.int16)
    if fmt == L.SS_PCM_S32:
        return q.astype(np.int32)
    u = (q & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 0xFF, (u >> 8) & 0xFF, u >> 16], axis=-1).astype(np.uint8)


def upload_pcm(b, raw, fmt):
    raw = np.ascontiguousarray(raw)
    rc = L.lib().ss_batch_upload_pcm(b._h, 0, int(b.cfg.n_streams), raw.ctypes.data_as(ctypes.c_void_p), fmt)
    assert rc == L.SS_OK, rc


# ------------------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("channels,frames", [(2, 1000), (3, 1001)])          # (the second: the samples are no multiple of four)
def test_round_trip(channels, frames):
    rng = np.random.default_rng(10 + channels)
    b = make_batch(channels, 2, frames)
    shape = (2, frames, channels)
    raws = {L.SS_PCM_U8: rng.integers(0, 256, shape).astype(np.uint8),
            L.SS_PCM_S16: rng.integers(-32768, 32768, shape).astype(np.int16),
            L.SS_PCM_S24: rng.integers(0, 256, shape + (3,)).astype(np.uint8),
            L.SS_PCM_S32: (rng.integers(-(1 << 23), 1 << 23, shape) * 256).astype(np.int32)}
    for fmt, raw in raws.items():
        upload_pcm(b, raw, fmt)
        got = b.download_pcm(0, 2, fmt)
        assert got.dtype == raw.dtype and got.shape == raw.shape and got.tobytes() == raw.tobytes(), fmt
        assert b.download_pcm(1, 1, fmt).tobytes() == raw[1:].tobytes(), fmt
    b.close()


def test_round_trip_extremes():
    b = make_batch(1, 1, 8)
    # (step: the distance of neighbouring integers an f32 sample can tell apart at full scale)
    for fmt, dt, lo, hi, step in ((L.SS_PCM_U8, np.uint8, 0, 255, 1), (L.SS_PCM_S16, np.int16, -32768, 32767, 1),
                                  (L.SS_PCM_S32, np.int32, -(1 << 31), (1 << 31) - 256, 256)):
        raw = np.array([lo, hi, lo + step, hi - step, 0, step, lo, hi], np.int64).astype(dt).reshape(1, 8, 1)
        upload_pcm(b, raw, fmt)
        assert b.download_pcm(0, 1, fmt).tobytes() == raw.tobytes(), fmt
    b.close()


# ------------------------------------------------------------------------------------------------------------ plants
def test_plants():
    x = np.array([0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768, 1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf,
                  32766.5 / 32768, 32767.5 / 32768, 0.0, -0.0], np.float32).reshape(1, -1, 1)
    b = make_batch(1, 1, x.shape[1])
    b.upload(0, x)
    s16 = b.download_pcm(0, 1, L.SS_PCM_S16).reshape(-1)
    assert list(s16) == [0, 2, 2, 0, -2, 32767, -32768, 32767, -32768, 0, 32767, -32768, 32766, 32767, 0, 0]
    for fmt in SCALE:
        assert b.download_pcm(0, 1, fmt).tobytes() == encode(quantise(x, fmt), fmt).tobytes(), fmt
    one = b.download_pcm(0, 1, L.SS_PCM_S32).reshape(-1)
    assert one[5] == (1 << 31) - 1 and one[6] == -(1 << 31) and one[9] == 0 and one[10] == (1 << 31) - 1 and one[11] == -(1 << 31)
    assert list(b.download_pcm(0, 1, L.SS_PCM_U8).reshape(-1)[5:12]) == [255, 0, 255, 0, 128, 255, 0]
    # F32 copies, F64 widens
    f32, f64 = b.download_pcm(0, 1, L.SS_PCM_F32), b.download_pcm(0, 1, L.SS_PCM_F64)
    assert f32.dtype == np.float32 and f32.tobytes() == b.download_input(0).tobytes() == x.tobytes()
    assert f64.dtype == np.float64 and np.array_equal(f64, x.astype(np.float64), equal_nan=True)
    assert np.signbit(f64.reshape(-1)[15]) and not np.signbit(f64.reshape(-1)[14])
    b.close()


def test_float_formats_on_noise():
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.2, 1.2, (3, 1001, 3)).astype(np.float32)
    b = make_batch(3, 3, 1001)
    b.upload(0, x)
    assert b.download_pcm(0, 3, L.SS_PCM_F32).tobytes() == x.tobytes()
    assert b.download_pcm(1, 2, L.SS_PCM_F64).tobytes() == x[1:].astype(np.float64).tobytes()
    assert b.download_pcm(1, 2, L.SS_PCM_F64, dither_seed=5).tobytes() == x[1:].astype(np.float64).tobytes()      # dither is ignored
    for fmt in SCALE:
        assert b.download_pcm(0, 3, fmt).tobytes() == encode(quantise(x, fmt), fmt).tobytes(), fmt
    b.close()


# ------------------------------------------------------------------------------------------------------------ ragged tail
def test_ragged_tail_reads_the_formats_zero():
    rng = np.random.default_rng(12)
    frames, lengths = 999, [600, 0, 999]
    x = rng.uniform(-1.0, 1.0, (3, frames, 2)).astype(np.float32)
    b = make_batch(2, 3, frames)
    b.upload(0, x)
    b.set_lengths(lengths)
    own = x.copy()
    for s, F in enumerate(lengths):
        own[s, F:] = 0.0
    for fmt in SCALE:
        want = encode(quantise(own, fmt), fmt)
        got = b.download_pcm(0, 3, fmt)
        assert got.tobytes() == want.tobytes(), fmt
    assert (b.download_pcm(0, 3, L.SS_PCM_U8)[0, 600:] == 128).all() and (b.download_pcm(1, 1, L.SS_PCM_S24) == 0).all()
    assert b.download_pcm(0, 3, L.SS_PCM_F32).tobytes() == own.tobytes()
    assert b.download_pcm(0, 3, L.SS_PCM_F64).tobytes() == own.astype(np.float64).tobytes()
    assert b.download_input(0).tobytes() == x[0].tobytes()                    # (the corpus itself is as it was)
    b.close()


# ------------------------------------------------------------------------------------------------------------ TPDF
@pytest.mark.parametrize("fmt", [L.SS_PCM_S16, L.SS_PCM_S24])
def test_tpdf(fmt):
    rng = np.random.default_rng(13)
    frames, C = 1000, 2
    x = rng.uniform(-1.0, 1.0, (2, frames, C)).astype(np.float32)
    x[0, :16] = 0.0                                                            # (silence shows the dither alone)
    b = make_batch(C, 2, frames)
    b.upload(0, x)
    seed = 0x0123456789ABCDEF
    d = np.stack([tpdf(seed, s, frames * C).reshape(frames, C) for s in range(2)])
    want = encode(quantise(x, fmt, d), fmt)
    got = b.download_pcm(0, 2, fmt, dither_seed=seed)
    assert got.tobytes() == want.tobytes()
    assert b.download_pcm(0, 2, fmt, dither_seed=seed).tobytes() == got.tobytes()                      # reproducible
    other = b.download_pcm(0, 2, fmt, dither_seed=seed + 1)
    assert other.tobytes() != got.tobytes()                                                            # two seeds differ
    assert b.download_pcm(1, 1, fmt, dither_seed=seed).tobytes() == got[1:].tobytes()                  # a stream's dither is its own
    plain = b.download_pcm(0, 2, fmt)
    assert plain.tobytes() == encode(quantise(x, fmt), fmt).tobytes() and plain.tobytes() != got.tobytes()
    # triangular, +-1 LSB: on silence the dithered values are -1, 0 or 1
    q = quantise(x[0, :16], fmt, d[0, :16])
    assert set(np.unique(q)) <= {-1, 0, 1}
    # the dither itself over many samples: mean 0, variance 1/6 (two uniforms of variance 1/12 each)
    big = tpdf(seed, 0, 1 << 16).astype(np.float64)
    assert abs(big.mean()) < 0.01 and abs(big.var() - 1.0 / 6.0) < 0.01
    b.close()


def test_tpdf_uses_the_high_seed_word_and_u8_s32():
    rng = np.random.default_rng(14)
    x = rng.uniform(-1.0, 1.0, (1, 257, 1)).astype(np.float32)
    b = make_batch(1, 1, 257)
    b.upload(0, x)
    for seed in (1, 1 << 32, (1 << 64) - 1):
        d = tpdf(seed, 0, 257).reshape(1, 257, 1)
        for fmt in (L.SS_PCM_U8, L.SS_PCM_S32):
            assert b.download_pcm(0, 1, fmt, dither_seed=seed).tobytes() == encode(quantise(x, fmt, d), fmt).tobytes(), (seed, fmt)
    b.close()


# ------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes():
    lib = L.lib()
    b = make_batch(2, 2, 100)
    out = np.zeros(2 * 100 * 2, np.int16)
    ptr, cap = out.ctypes.data_as(ctypes.c_void_p), out.nbytes
    INVALID = L.SS_ERR_INVALID_ARG
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, L.SS_PCM_S16, None) == L.SS_OK
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, 0, None) == INVALID and lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, 7, None) == INVALID
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, L.SS_PCM_S16, ctypes.byref(L.PcmDither(1, 2, 0))) == INVALID     # unknown kind
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, L.SS_PCM_S16, ctypes.byref(L.PcmDither(1, 1, 1))) == INVALID     # reserved
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, L.SS_PCM_S16, ctypes.byref(L.PcmDither(1, L.SS_DITHER_NONE, 0))) == L.SS_OK
    assert lib.ss_batch_download_pcm(b._h, 1, 2, ptr, cap, L.SS_PCM_S16, None) == INVALID                                    # first + count
    assert lib.ss_batch_download_pcm(b._h, 0xFFFFFFFF, 2, ptr, cap, L.SS_PCM_S16, None) == INVALID
    assert lib.ss_batch_download_pcm(b._h, 0, 2, None, cap, L.SS_PCM_S16, None) == INVALID
    assert lib.ss_batch_download_pcm(None, 0, 2, ptr, cap, L.SS_PCM_S16, None) == INVALID
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap - 1, L.SS_PCM_S16, None) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_pcm(b._h, 0, 2, ptr, cap, L.SS_PCM_S24, None) == L.SS_ERR_CAPACITY
    assert lib.ss_batch_download_pcm(b._h, 0, 1, ptr, cap // 2, L.SS_PCM_S16, None) == L.SS_OK
    assert lib.ss_batch_download_pcm(b._h, 2, 0, None, 0, L.SS_PCM_S16, None) == L.SS_OK                                     # nothing asked
    b.close()
