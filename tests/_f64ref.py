"""Plain f64 restatements, from the published definitions, that the time-domain, gating and spectrum tests hold the device path
to (a helper module, not a test file): none of it calls the product or the oracle.

  * K-weighting: libebur128's design (ebur128_init_filter: a high shelf, then the 38 Hz high-pass, each by bilinear transform,
    numerators and denominators convolved into one 4th-order section) for any rate, run as a sequential f64 filter;
  * the crate's true-peak interpolator: 49 Hann-windowed sinc taps rounded to f32, a zero-stuffed polyphase convolution in f64;
  * ebur128's channel weights, and the momentary / short-term series as `loudness_momentary()` / `loudness_shortterm()` return
    them after every 100 ms sub-block (zeros before the start);
  * the gate (BS.1770-4, EBU Tech 3342, ebur128's histogram mode): the bin tables, gating and short-term block energies from
    sub-block energies with the additions in a fixed order, their histograms, integrated loudness and loudness range of a
    histogram, and the reading of a sliding window;
  * get_waveform's min-max decimation (analyzer.rs:107-137);
  * the spectrum rows (analyzer.rs:11-27, :55-105): the retained-bin rule, mid / side formed in f32, one row of any mono window
    with the transform in f64, and `row_error`, the metric the spectrum forms are held to.
"""
import numpy as np
from scipy import signal


def subblock_frames(rate):
    return (rate + 5) // 10


def kweight_coeffs(rate):
    """(b[5], a[5]) of the K-weighting filter at `rate` (libebur128 ebur128_init_filter)."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    pb = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    pa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / rate)
    rb = np.array([1.0, -2.0, 1.0])
    ra = np.array([1.0, 2.0 * (K * K - 1.0) / (1.0 + K / Q + K * K), (1.0 - K / Q + K * K) / (1.0 + K / Q + K * K)])
    return np.convolve(pb, rb), np.convolve(pa, ra)


def kweighted_subblocks(x, rate, channels, frames=None):
    """[sub-block][channel] sums of y^2 of a sequential f64 K-weighting of interleaved `x` (its first `frames` frames), over the
    whole sub-blocks of (rate + 5) // 10 frames."""
    b, a = kweight_coeffs(rate)
    x = np.asarray(x).reshape(-1, channels)
    if frames is not None:
        x = x[:frames]
    S = subblock_frames(rate)
    n = x.shape[0] // S
    y = signal.lfilter(b, a, x[:n * S].astype(np.float64), axis=0)
    return (y * y).reshape(n, S, channels).sum(axis=1)


def channel_weights(channels):
    """ebur128's default channel map as weights: L / R / C 1.0, LFE (the fourth of five and more) 0, the surrounds 1.41,
    channels past the sixth unused; four channels are L R Ls Rs, five L R C Ls Rs."""
    if channels == 4:
        return np.array([1.0, 1.0, 1.41, 1.41])
    if channels == 5:
        return np.array([1.0, 1.0, 1.0, 1.41, 1.41])
    w = np.zeros(channels)
    for i, v in enumerate((1.0, 1.0, 1.0, 0.0, 1.41, 1.41)):
        if i < channels:
            w[i] = v
    return w


def _window_loudness(e, k, S):
    """-0.691 + 10 log10 of the mean square over the last k sub-blocks after each sub-block (zeros before the start)."""
    c = np.concatenate([np.zeros(k), np.cumsum(e)])
    win = (c[k:] - c[:-k]) / (k * S)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(win > 0.0, 10.0 * np.log10(np.where(win > 0.0, win, 1.0)) - 0.691, -np.inf)


def loudness_series(sub, rate, channels):
    """(momentary, short-term) after every sub-block from [sub-block][channel] energies: 4 and 30 sub-blocks, channel-weighted."""
    S = subblock_frames(rate)
    e = sub @ channel_weights(channels)
    return _window_loudness(e, 4, S), _window_loudness(e, 30, S)


# ---- the gate: BS.1770-4 gating blocks, EBU Tech 3342 short-term blocks, ebur128's histogram mode
HIST_BINS = 1000


def histogram_tables():
    """(energies[1000], bounds[1001]) of ebur128's histogram mode: bin i spans [-70 + i / 10, -70 + (i + 1) / 10) LUFS and stands
    for the energy of its centre."""
    i = np.arange(HIST_BINS + 1, dtype=np.float64)
    return 10.0 ** ((-69.95 + i[:-1] / 10.0 + 0.691) / 10.0), 10.0 ** ((-70.0 + i / 10.0 + 0.691) / 10.0)


def _window_energies(sub, w, k, ends, S):
    """Energy of the k sub-blocks that end with each sub-block of `ends`: over the weighted channels in order, w_c times the
    channel's k sub-blocks added oldest first, the channels' terms added in order, then one division by k S — every step one
    rounded f64 operation, so the same inputs give the same bits wherever these operations run in this order."""
    ends = np.asarray(ends, np.int64)
    total = np.zeros(ends.size)
    for c in np.flatnonzero(w):
        cs = sub[ends - (k - 1), c].astype(np.float64)
        for q in range(k - 2, -1, -1):
            cs = cs + sub[ends - q, c]
        total = total + w[c] * cs
    return total / (float(k) * S)


def gate_blocks(sub, rate, channels, first=0, n=None):
    """(gating-block energies, short-term energies) of the sub-blocks [first, first + n) of `sub` ([sub-block][channel] energies;
    n=None: all from `first` on).  A gating block ends with every sub-block j >= first + 3 (400 ms, 75 % overlap), a short-term
    block with j = first + 29 + 10 m (3 s every second: the crate's cadence, its phase at the start of the range)."""
    sub = np.asarray(sub, np.float64).reshape(-1, channels)
    n = sub.shape[0] - first if n is None else n
    assert 0 <= first and n >= 0 and first + n <= sub.shape[0], (first, n, sub.shape)
    S = float(subblock_frames(rate))
    w = channel_weights(channels)
    return (_window_energies(sub, w, 4, np.arange(first + 3, first + n), S),
            _window_energies(sub, w, 30, np.arange(first + 29, first + n, 10), S))


def hist_bins_of(energies):
    """bin of every energy: i with bounds[i] <= e < bounds[i + 1], the top bin open above; -1 for what is never counted (an
    energy under bounds[0], a NaN)"""
    _, bd = histogram_tables()
    e = np.asarray(energies, np.float64).reshape(-1)
    idx = np.minimum(np.searchsorted(bd, e, side="right") - 1, HIST_BINS - 1)      # (NaN sorts behind every bound: excluded below)
    return np.where(e >= bd[0], idx, -1)


def gate_histograms(blocks, st):
    """(block histogram, short-term histogram), u64[1000] each, of the energies gate_blocks returns"""
    out = []
    for e in (blocks, st):
        idx = hist_bins_of(e)
        out.append(np.bincount(idx[idx >= 0], minlength=HIST_BINS).astype(np.uint64))
    return out[0], out[1]


def hist_moments(h):
    """(count, mean energy) of a histogram, its bins standing for their centre energies; the sum is exact (fsum)"""
    import math
    en, _ = histogram_tables()
    h = np.asarray(h, np.uint64)
    cnt = int(h.sum(dtype=np.uint64))
    return cnt, (math.fsum(h.astype(np.float64) * en) / cnt if cnt else 0.0)


def gate_start_bin(threshold):
    """First bin a relative threshold (an energy) admits: the bin that holds it, plus one if it exceeds that bin's energy — a
    bin counts only if the energy it stands for reaches the threshold.  (holding bin, start bin); (0, 0) under the first bound."""
    en, bd = histogram_tables()
    if threshold < bd[0]:
        return 0, 0
    i = int(hist_bins_of([threshold])[0])
    return i, i + 1 if threshold > en[i] else i


def integrated_from_hist(hb, start=None):
    """Gated loudness of a block histogram (BS.1770-4 in the crate's histogram mode): the mean of the bins from the relative
    gate's start bin on — 0.1 x the mean of all counted blocks; -inf for an empty histogram or an empty gate.  `start`: another
    start bin, for telling two readings of the gate rule apart."""
    import math
    en, _ = histogram_tables()
    cnt, mean = hist_moments(hb)
    if cnt == 0:
        return -np.inf
    if start is None:
        start = gate_start_bin(0.1 * mean)[1]
    cnt, mean = hist_moments(np.concatenate([np.zeros(start, np.uint64), np.asarray(hb, np.uint64)[start:]]))
    return 10.0 * math.log10(mean) - 0.691 if cnt else -np.inf


def lra_entries_from_hist(hs, start=None):
    """(gate start bin, gated count, bin of the 10 % entry, bin of the 95 % entry) of a short-term histogram, None for the bins
    of an empty gate: EBU Tech 3342 in the crate's histogram mode — relative gate 0.01 x the mean of all counted values, the
    entries of ranks floor((n - 1) p + 0.5) among the n gated ones (the product in f64, as the crate forms it).  `start`: another
    start bin, as integrated_from_hist takes one."""
    hs = np.asarray(hs, np.uint64)
    cnt, mean = hist_moments(hs)
    if cnt == 0:
        return 0, 0, None, None
    if start is None:
        start = gate_start_bin(0.01 * mean)[1]
    cum = np.cumsum(hs[start:], dtype=np.uint64)
    n = int(cum[-1]) if cum.size else 0
    if n == 0:
        return start, 0, None, None
    lo, hi = (int(float(n - 1) * p + 0.5) for p in (0.1, 0.95))
    return (start, n, start + int(np.searchsorted(cum, np.uint64(lo), side="right")),
            start + int(np.searchsorted(cum, np.uint64(hi), side="right")))


def lra_from_hist(hs, start=None):
    """Loudness range of a short-term histogram: the 95 % entry's bin over the 10 % entry's, in LU; 0 where nothing is gated"""
    import math
    en, _ = histogram_tables()
    _, n, lo, hi = lra_entries_from_hist(hs, start)
    return 10.0 * math.log10(en[hi]) - 10.0 * math.log10(en[lo]) if n else 0.0


def window_reading(y, weights, F, frames):
    """The reading of a sliding window at frame F: -0.691 + 10 log10 of the channel-weighted mean square of the filtered signal
    y ([frame][channel]) over the frames [F - frames, F), zeros in front of frame 0 (the divisor is `frames` throughout, as a
    meter's zeroed ring has it); -inf for silence."""
    import math
    y = np.asarray(y, np.float64)
    seg = y[max(F - frames, 0):F]
    e = float(((seg * seg).sum(axis=0) * np.asarray(weights, np.float64)).sum()) / frames
    return 10.0 * math.log10(e) - 0.691 if e > 0.0 else -np.inf


def interpolator_taps(factor):
    """The 49 taps of the crate's interpolator (sinc at 1/factor, Hann over 48 intervals), rounded to f32 like the crate's."""
    j = np.arange(49, dtype=np.float64)
    m = j - 24.0
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.where(np.abs(m) > 1e-6, np.sin(m * np.pi / factor) / (m * np.pi / factor), 1.0)
    c *= 0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0))
    c[np.abs(c) <= 1e-6] = 0.0                          # the crate keeps only taps above 1e-6
    return c.astype(np.float32).astype(np.float64)


def true_peak(ch, factor):
    """One channel's true peak in f64: max(|upfirdn(taps, x, factor)|[:factor n], |x|); the sample peak at factor 0."""
    ch = np.asarray(ch, np.float64)
    if factor == 0:
        return float(np.abs(ch).max())
    up = signal.upfirdn(interpolator_taps(factor), ch, up=factor)
    return float(max(np.abs(up[:factor * ch.size]).max(), np.abs(ch).max()))


def tap_bound(factor):
    """max over the phases of sum |taps|: no interpolated output exceeds this times the largest |sample| it reads"""
    t = np.abs(interpolator_taps(factor))
    return float(max(t[p::factor].sum() for p in range(factor)))


def event_windows(x, starts, span, pad=40):
    """frames [start - pad, start + span + pad) of every row of x ([k][n]), zeros outside [0, n)"""
    x = np.asarray(x)
    k, n = x.shape
    idx = np.asarray(starts, np.int64)[:, None] - pad + np.arange(span + 2 * pad)[None, :]
    return np.where((idx >= 0) & (idx < n), x[np.arange(k)[:, None], np.clip(idx, 0, n - 1)], 0).astype(np.float64)


def event_true_peak(win, starts, n, span, factor, pad=40):
    """True peaks of many channels of n frames, each holding one event at frames [start, start + span), from the frames around
    it alone (win = event_windows(...)).  The outputs whose taps reach into the event read only frames of the window
    (pad >= 48 / factor) and are computed exactly; every other output reads only background and is at most
    tap_bound(factor) * max|background|.  Returns the event's peak, [k], its own samples included: the channel's true peak is
    max(that, its sample peak) wherever the caller's background bound lies below it.  (An event in the last 48 / factor frames
    rings past the end of the stream: the outputs there are never made.)"""
    k, W = win.shape
    starts = np.asarray(starts, np.int64)
    span = W - 2 * pad
    taps = interpolator_taps(factor)
    up = np.zeros((k, W * factor))
    up[:, ::factor] = win
    y = np.zeros_like(up)
    for j in np.nonzero(taps)[0]:                       # y[m] = sum_j taps[j] up[m - j]
        y[:, j:] += taps[j] * up[:, :up.shape[1] - j]
    m = (starts[:, None] - pad) * factor + np.arange(W * factor)[None, :]   # the outputs' positions in the whole stream
    exact = (np.arange(W * factor)[None, :] >= 48) & (m >= 0) & (m < factor * np.reshape(n, (-1, 1)))
    return np.maximum(np.where(exact, np.abs(y), 0.0).max(axis=1), np.abs(win[:, pad:pad + span]).max(axis=1))


def waveform_numpy(x, window_s):
    """analyzer.rs:107-137 with numpy: W = window_s * 1000 bins, spp = len / W in f64, bin i = [floor(i spp),
    min(ceil((i + 1) spp), len)), points (i, min), (i, max); stops at the first bin that starts past the end."""
    w = int(window_s * 1000.0)
    spp = len(x) / w
    out = []
    for i in range(w):
        bs = int(np.floor(i * spp))
        be = min(int(np.ceil((i + 1) * spp)), len(x))
        if bs >= len(x):
            break
        seg = x[bs:be]
        out += [np.nanmin(seg) if seg.size and not np.all(np.isnan(seg)) else (np.nan if seg.size else 0.0),
                np.nanmax(seg) if seg.size and not np.all(np.isnan(seg)) else (np.nan if seg.size else 0.0)]
    return np.array(out, np.float32)


def retained_bins(rate, n):
    """(first bin, count) of the bins a row keeps: f32 frequencies k * (rate / n), both in f32, within [20, 20000]"""
    f = np.arange(n // 2 + 1, dtype=np.float32) * (np.float32(rate) / np.float32(n))
    keep = np.nonzero((f >= np.float32(20.0)) & (f <= np.float32(20000.0)))[0]
    return (int(keep[0]), int(keep.size)) if keep.size else (0, 0)


def pink_db(rate, n):
    """the pink compensation the retained bins carry: 10 log10(f / 1000), f the f32 bin frequency, in f64"""
    first, count = retained_bins(rate, n)
    f = (np.arange(first, first + count, dtype=np.float32) * (np.float32(rate) / np.float32(n))).astype(np.float64)
    return 10.0 * np.log10(f / 1000.0)


def mid_side_f32(lr):
    """mid and side of [frames][2] stereo as the crate forms them: (l + r) / 2 and (l - r) / 2 in f32"""
    lr = np.asarray(lr, np.float32)
    two = np.float32(2.0)
    return ((lr[:, 0] + lr[:, 1]) / two).astype(np.float32), ((lr[:, 0] - lr[:, 1]) / two).astype(np.float32)


def hann_f32(n):
    """the crate's periodic Hann window, its weights rounded to f32"""
    i = np.arange(n, dtype=np.float64)
    return (0.5 * (1.0 - np.cos(2.0 * np.pi * i / n))).astype(np.float32).astype(np.float64)


def spectrum_row_f64(x, rate, n=None, pink=True):
    """One row of get_fft for the mono window x (n samples, taken as they are: pass f32 data as f32): f32 Hann weights, the
    product and the rfft in f64, 20 log10(|X| 4 / N) on the retained bins, -150 for an exact zero, + 10 log10(f / 1000)."""
    x = np.asarray(x)
    n = x.size if n is None else n
    mag = np.abs(np.fft.rfft(x.astype(np.float64) * hann_f32(n)))
    first, count = retained_bins(rate, n)
    m = mag[first:first + count]
    with np.errstate(divide="ignore"):
        db = np.where(m == 0.0, -150.0, 20.0 * np.log10(np.where(m == 0.0, 1.0, m) * 4.0 / n))
    return db + pink_db(rate, n) if pink else db


def spectrum_f64(x, rate, n):
    """One window of the reference's get_fft restated with numpy in f64 (window values rounded to f32 as the crate's)."""
    return spectrum_row_f64(x, rate, n)


def row_error(got_db, ref_db, pink):
    """max_k |a_got - a_ref| / max_k a_ref: a row's error as a fraction of its own peak amplitude, pink taken out of both rows
    (a = 10^(dB / 20)).  Each bin is first allowed the rounding of its stored f32 dB value (two ulps of it), so that a quiet
    row is bounded by its transform and not by how its output is stored."""
    got = np.asarray(got_db, np.float64)
    ref = np.asarray(ref_db, np.float64)
    assert got.shape == ref.shape and got.ndim == 1, (got.shape, ref.shape)
    a_got = 10.0 ** ((got - pink) / 20.0)
    a_ref = 10.0 ** ((ref - pink) / 20.0)
    ulp2 = 2.0 * np.abs(np.spacing(got.astype(np.float32))).astype(np.float64)
    allow = a_got * (10.0 ** (ulp2 / 20.0) - 1.0)
    return float(np.maximum(np.abs(a_got - a_ref) - allow, 0.0).max() / a_ref.max())


def floor_error(got_db, ref_db, pink, below_db=40.0):
    """row_error over the bins at least `below_db` under the row's peak only: the transform's rounding noise, apart from what the
    dB conversion rounds in proportion to each bin (that sets row_error at the peak; this sees the twiddles and the butterflies)"""
    got = np.asarray(got_db, np.float64)
    ref = np.asarray(ref_db, np.float64)
    a_got = 10.0 ** ((got - pink) / 20.0)
    a_ref = 10.0 ** ((ref - pink) / 20.0)
    quiet = a_ref <= a_ref.max() * 10.0 ** (-below_db / 20.0)
    if not quiet.any():
        return 0.0
    allow = a_got * (10.0 ** (2.0 * np.abs(np.spacing(got.astype(np.float32))).astype(np.float64) / 20.0) - 1.0)
    return float(np.maximum(np.abs(a_got - a_ref) - allow, 0.0)[quiet].max() / a_ref.max())
