"""Batch extension: many equal-length streams resident in HBM, analysed in one pass.

Not part of the reference API (soundscope analyses one file at a time); it is the
data-parallel form of receive_audio_file + analyze_audio_file_samples
(reference src/tui.rs:1207-1241, :1482-1552) over a corpus.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .analyzer import _check


def _region_rows(regions):
    """A region list as contiguous u32 [n][4] rows: a u32 array [n][4] as it is, else rows of three or four integers (a missing
    group is L.SS_REGION_NO_GROUP)."""
    rows = regions
    if not (isinstance(rows, np.ndarray) and rows.dtype == np.uint32 and rows.ndim == 2 and rows.shape[1] == 4):   # (else: as it is)
        a = np.asarray(regions, dtype=np.int64).reshape(-1, 4 if len(regions) and len(regions[0]) == 4 else 3)
        if ((a < 0) | (a > 0xFFFFFFFF)).any():
            raise ValueError("region fields are u32")
        rows = np.full((a.shape[0], 4), L.SS_REGION_NO_GROUP, np.uint32)
        rows[:, :a.shape[1]] = a
    return np.ascontiguousarray(rows)


# The structured arrays' dtypes are the ctypes records' (_lib.py, Python's one definition of what crosses the C ABI).
PEAK_ENTRY_DTYPE = np.dtype(L.PeakEntry)
# the signal scan's records (ss_stream_scan, ss_channel_scan, ss_signal_event)
STREAM_SCAN_DTYPE = np.dtype(L.StreamScan)
CHANNEL_SCAN_DTYPE = np.dtype(L.ChannelScan)
SIGNAL_EVENT_DTYPE = np.dtype(L.SignalEvent)
SIGNAL_SILENCE, SIGNAL_CLIP = L.SS_SIGNAL_SILENCE, L.SS_SIGNAL_CLIP
# the pair series' records (ss_pair_entry, ss_region_pair, ss_group_pair)
PAIR_ENTRY_DTYPE = np.dtype(L.PairEntry)
REGION_PAIR_DTYPE = np.dtype(L.RegionPair)
GROUP_PAIR_DTYPE = np.dtype(L.GroupPair)


# what a caller reads off pair records (entries, regions or groups: anything with s_aa, s_bb, s_ab), as plain numpy
def pair_correlation(rec):
    """s_ab / sqrt(s_aa s_bb): +1 in phase, -1 out of phase; NaN where a power is 0."""
    aa, bb, ab = (np.asarray(rec[n], np.float64) for n in ("s_aa", "s_bb", "s_ab"))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((aa > 0) & (bb > 0), ab / np.sqrt(aa * bb), np.nan)


def pair_balance_db(rec):
    """10 log10(s_bb / s_aa): positive where channel b is the louder."""
    aa, bb = np.asarray(rec["s_aa"], np.float64), np.asarray(rec["s_bb"], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(bb / aa)


def pair_mono_loss_db(rec):
    """10 log10((s_aa + 2 s_ab + s_bb) / (2 (s_aa + s_bb))): the power of the fold-down (a + b) / 2 against the mean channel power —
    0 for b = a, -inf for b = -a, about -3 for unrelated channels."""
    aa, bb, ab = (np.asarray(rec[n], np.float64) for n in ("s_aa", "s_bb", "s_ab"))
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10((aa + 2.0 * ab + bb) / (2.0 * (aa + bb)))


# batch gain (ss_gain_point, ss_gain_channel) and what normalise() hands back per stream
GAIN_POINT_DTYPE = np.dtype(L.GainPoint)
GAIN_CHANNEL_DTYPE = np.dtype(L.GainChannel)
NORMALISE_DTYPE = np.dtype([("loudness", np.float64), ("peak", np.float64), ("gain_db", np.float64), ("gain", np.float32),
                            ("limited_by", np.uint32)])
_PCM_DTYPES = {L.SS_PCM_U8: np.uint8, L.SS_PCM_S16: np.int16, L.SS_PCM_S24: np.uint8, L.SS_PCM_S32: np.int32,
               L.SS_PCM_F32: np.float32, L.SS_PCM_F64: np.float64}


def _gain_points(points):
    """A point list as a contiguous GAIN_POINT_DTYPE array: such an array as it is, else rows (stream, frame, gain)."""
    if isinstance(points, np.ndarray) and points.dtype == GAIN_POINT_DTYPE:
        return np.ascontiguousarray(points).reshape(-1)
    out = np.zeros(len(points), GAIN_POINT_DTYPE)
    for i, (stream, frame, gain) in enumerate(points):
        out[i] = (frame, stream, gain)
    return out


def gain_envelope(points, frames):
    """ss_gain_envelope of ONE stream's points (frames strictly ascending) at every frame of `frames`, as f64: g_0 at or before the
    first point, g_last at or behind the last, g_k + (frame - f_k) * d_k for f_k <= frame < f_(k+1) with d_k = (g_(k+1) - g_k) /
    (f_(k+1) - f_k) — numpy rounds every operation on its own, as the library does.  No point: 1."""
    p, n = _gain_points(points), np.asarray(frames, dtype=np.uint64)
    if p.size == 0:
        return np.ones(n.shape, np.float64)
    f, g = p["frame"], p["gain"].astype(np.float64)
    out = np.full(n.shape, g[0], np.float64)
    if f.size > 1:
        k = np.clip(np.searchsorted(f, n, side="right").astype(np.int64) - 1, 0, f.size - 2)      # f_k <= frame < f_(k+1) where it counts
        d = (g[1:] - g[:-1]) / (f[1:] - f[:-1]).astype(np.float64)
        ramp = g[k] + (n - f[k]).astype(np.float64) * d[k]      # (frames in front of f_0 wrap here and are replaced below)
        out = np.where(n <= f[0], g[0], np.where(n >= f[-1], g[-1], ramp))
    return out


# batch limiter (ss_limit_item, ss_limit_stream); the per-channel records are GAIN_CHANNEL_DTYPE
LIMIT_ITEM_DTYPE = np.dtype(L.LimitItem)
LIMIT_STREAM_DTYPE = np.dtype(L.LimitStream)


def _limit_items(items):
    """An item list as a contiguous LIMIT_ITEM_DTYPE array: such an array as it is, else rows (stream, gain)."""
    if isinstance(items, np.ndarray) and items.dtype == LIMIT_ITEM_DTYPE:
        return np.ascontiguousarray(items).reshape(-1)
    out = np.zeros(len(items), LIMIT_ITEM_DTYPE)
    for i, (stream, gain) in enumerate(items):
        out[i] = (stream, gain)
    return out


def limit_curve(level, gain, ceiling, lookahead, hold, advance=0):
    """ss_limit_curve: the limiter's gain curve of ONE stream from its frames' levels (f32), on the host — (r_q u32, S u64, c f64)
    per frame: the required gain floor(ceiling / (level |gain|) 2^30) where the product is finite and over the ceiling (else 2^30),
    its minimum over [k - hold, k + lookahead + advance] summed over the lookahead + 1 windows that hold the frame, and that sum
    over (lookahead + 1) 2^30.  lookahead and hold are frames."""
    m = np.ascontiguousarray(level, dtype=np.float32).reshape(-1)
    cfg = L.LimitConfig(0, float(ceiling), 1.0, int(lookahead), int(hold), 0, 0, 0)
    r_q, s, c = np.zeros(m.size, np.uint32), np.zeros(m.size, np.uint64), np.zeros(m.size, np.float64)
    _check(L.lib().ss_limit_curve(m.ctypes.data_as(C.POINTER(C.c_float)), m.size, float(gain), C.byref(cfg), int(advance),
                                  r_q.ctypes.data_as(C.POINTER(C.c_uint32)), s.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  c.ctypes.data_as(C.POINTER(C.c_double))))
    return r_q, s, c


# batch resampler (ss_resample_plan): the plan rule, the table, the output length and the reference chain are host arithmetic
def resample_plan(in_rate, out_rate, attenuation_db=0.0, passband=0.0):
    """ss_resample_plan_make: the L.ResamplePlan of a conversion in_rate -> out_rate (up = L, down = M, taps = T per phase, beta,
    cutoff); attenuation_db 0 means 100, passband 0 means 20000 / 22050 of the lower Nyquist."""
    plan = L.ResamplePlan()
    _check(L.lib().ss_resample_plan_make(int(in_rate), int(out_rate), float(attenuation_db), float(passband), C.byref(plan)))
    return plan


def resample_taps(plan):
    """ss_resample_taps: the plan's polyphase table [L][T] f32; tap k of phase p weighs input frame base - T/2 + 1 + k."""
    out = np.zeros((int(plan.up), int(plan.taps)), np.float32)
    _check(L.lib().ss_resample_taps(C.byref(plan), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
    return out


def resample_length(plan, frames_in):
    """ss_resample_length: the outputs of a stream of frames_in frames, ceil(frames_in * L / M)."""
    return int(L.lib().ss_resample_length(C.byref(plan), int(frames_in)))


def resample_host(plan, x, channels=1, first_out=0, n_out=None, taps=None):
    """ss_resample_host: outputs [first_out, first_out + n_out) of ONE stream x ([frames][channels] f32, or flat) on the host, as
    [n_out][channels] f32 — the definition of Batch.resample_into in bits: one fmaf chain per output over the phase's taps in order."""
    a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    ch = int(channels)
    frames = a.size // ch
    assert frames * ch == a.size
    t = resample_taps(plan) if taps is None else np.ascontiguousarray(taps, dtype=np.float32)
    if n_out is None:
        n_out = resample_length(plan, frames) - int(first_out)
    out = np.zeros((int(n_out), ch), np.float32)
    f32p = C.POINTER(C.c_float)
    _check(L.lib().ss_resample_host(C.byref(plan), t.ctypes.data_as(f32p), a.ctypes.data_as(f32p), frames, ch, int(first_out), int(n_out),
                                    out.ctypes.data_as(f32p)))
    return out


def normalisation_gain(loudness_lufs, peak_linear, target_lufs, max_true_peak_dbtp=np.inf, max_gain_db=np.inf, min_gain_db=-np.inf):
    """ss_normalisation_gain over arrays: (gain_db f64, gain f32, limited_by u32) for every (loudness, linear peak).  The law: an
    unmeasured loudness (NaN, +-inf) gives 0 dB and SS_GAIN_UNMEASURED; else target - loudness, cut to the headroom under the
    ceiling (finite ceiling, finite peak > 0), then clamped to [min_gain_db, max_gain_db]; gain = (f32)10^(dB / 20), one f32 down
    where the ceiling bound and the rounding went up."""
    lu, pk = np.broadcast_arrays(np.asarray(loudness_lufs, np.float64), np.asarray(peak_linear, np.float64))
    t, ceiling, g_max, g_min = float(target_lufs), float(max_true_peak_dbtp), float(max_gain_db), float(min_gain_db)
    if any(np.isnan(v) for v in (t, ceiling, g_max, g_min)) or np.isnan(pk).any() or g_min > g_max:
        raise ValueError("normalisation target: NaN, or min_gain_db above max_gain_db")
    measured = np.isfinite(lu)
    with np.errstate(all="ignore"):
        g = t - lu
        capped = np.isfinite(ceiling) & np.isfinite(pk) & (pk > 0)
        headroom = ceiling - 20.0 * np.log10(np.where(capped, pk, 1.0))
        by_peak = measured & capped & (g > headroom)
        g = np.where(by_peak, headroom, g)
        by_max = measured & (g > g_max)
        g = np.where(by_max, g_max, g)
        by_min = measured & (g < g_min)
        g = np.where(by_min, g_min, g)
        g = np.where(measured, g, 0.0)
        exact = np.power(10.0, g / 20.0)
        lin = exact.astype(np.float32)
        down = by_peak & (g == headroom) & (lin.astype(np.float64) > exact)
        lin = np.where(down, np.nextafter(lin, np.float32(-np.inf)), lin).astype(np.float32)
    why = (by_peak * L.SS_GAIN_LIMITED_PEAK + by_max * L.SS_GAIN_LIMITED_MAX + by_min * L.SS_GAIN_LIMITED_MIN +
           ~measured * L.SS_GAIN_UNMEASURED).astype(np.uint32)
    return g, lin, why


class Batch:
    def __init__(self, sample_rate=48000, channels=2, n_streams=1, frames_per_stream=480000,
                 fft_n=4096, hop_frames=1024, flags=L.SS_BATCH_ALL, true_peak_factor=0,
                 waveform_window=0.0, spectrum_columns=0):
        """spectrum_columns > 0 (with L.SS_BATCH_FFT_COLUMNS in flags, added here if missing): columns-only spectrum — the
        render-side reduction runs inside the spectrum kernel and only that many chart columns per row are kept."""
        self._ragged = False                # set_lengths() has been called
        self._listed = {"loudness": (0, 0), "peak": (0, 0), "spectrum": (0, 0), "pair": (0, 0)}   # (regions, groups) of the last accepted list of each kind
        if spectrum_columns:
            flags |= L.SS_BATCH_FFT_COLUMNS
            self._render_cols = int(spectrum_columns)
        cfg = L.BatchConfig(sample_rate, channels, n_streams, fft_n, hop_frames, flags, true_peak_factor, int(spectrum_columns),
                            frames_per_stream, waveform_window)
        self.cfg = cfg
        self._h = C.c_void_p()
        rc = L.lib().ss_batch_create(C.byref(cfg), C.byref(self._h))
        if rc != L.SS_OK:
            self._h = None
            _check(rc)
        lay = L.BatchLayout()
        _check(L.lib().ss_batch_layout_get(self._h, C.byref(lay)))
        self.layout = lay

    def close(self):
        if getattr(self, "_h", None):
            L.lib().ss_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def samples_per_stream(self):
        return int(self.cfg.frames_per_stream) * int(self.cfg.channels)

    def upload(self, first, pcm):
        a = np.ascontiguousarray(pcm, dtype=np.float32)
        count = a.size // self.samples_per_stream
        assert count * self.samples_per_stream == a.size
        _check(L.lib().ss_batch_upload(self._h, first, count, a.ctypes.data_as(C.POINTER(C.c_float))))

    def download_input(self, stream):
        out = np.empty(self.samples_per_stream, np.float32)
        _check(L.lib().ss_batch_download_input(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def input_device_ptr(self):
        return L.lib().ss_batch_input_device_ptr(self._h)

    def synthesize(self, seed=0x5EED0000, first_stream_id=0):
        _check(L.lib().ss_batch_synthesize(self._h, seed, first_stream_id))

    def run(self):
        _check(L.lib().ss_batch_run(self._h))
        self._ran = True

    def sync(self):
        _check(L.lib().ss_batch_sync(self._h))

    # -- ragged batches: every stream its own length inside its frames_per_stream slot
    def set_lengths(self, frames):
        a = np.ascontiguousarray(frames, dtype=np.uint64)
        _check(L.lib().ss_batch_set_lengths(self._h, a.ctypes.data_as(C.POINTER(C.c_uint64)), a.size))
        self._ragged = True

    def stream_shape(self, stream):
        sh = L.StreamShape()
        _check(L.lib().ss_batch_stream_shape(self._h, stream, C.byref(sh)))
        return sh

    def results(self):
        n = int(self.cfg.n_streams)
        arr = (L.StreamResult * n)()
        _check(L.lib().ss_batch_results(self._h, arr, n))
        return arr

    def peaks(self, stream):
        """Every channel's (true_peak, sample_peak) of one stream, linear: arrays [channels] f64."""
        ch = int(self.cfg.channels)
        tp, sp = np.empty(ch, np.float64), np.empty(ch, np.float64)
        dp = C.POINTER(C.c_double)
        _check(L.lib().ss_batch_peaks(self._h, stream, tp.ctypes.data_as(dp), sp.ctypes.data_as(dp), ch))
        return tp, sp

    @property
    def geometry(self):
        g = L.BatchGeometry()
        _check(L.lib().ss_batch_geometry_get(self._h, C.byref(g)))
        return g

    def set_overlap(self, mode=True):
        """0 / False: sequential; 1 / True: spectrum kernel on a second HIP stream beside the time-domain chain;
        2: beside the chain's tail only (time-domain kernel first and alone).  Same results in every mode."""
        _check(L.lib().ss_batch_set_overlap(self._h, int(mode)))

    def set_time_domain_mode(self, mode):
        """L.SS_TD_AUTO (time segments with the exact state hand-over), L.SS_TD_RUN_IN (segments with the 0.1 s run-in of earlier
        rounds, for comparison), L.SS_TD_WHOLE_STREAMS (a workgroup per stream, where the shape allows)."""
        _check(L.lib().ss_batch_set_time_domain_mode(self._h, int(mode)))

    def set_true_peak_arith(self, arith):
        """L.SS_TP_ARITH_F32 (default: f32 MFMA, the width of the crate's interpolator) or L.SS_TP_ARITH_F16X3 (opt-in: f16x3
        split on the matrix cores, within 2^-21 of the tile peak of the f32 result, faster)."""
        _check(L.lib().ss_batch_set_true_peak_arith(self._h, int(arith)))

    @property
    def true_peak_arith(self):
        return int(L.lib().ss_batch_get_true_peak_arith(self._h))

    def allreduce_histograms(self, comm):
        """The corpus gate's exchange: in-place SUM all-reduce of this batch's corpus histograms over `comm`
        (soundscope_amd.distributed.Comm).  Returns (block_hist, shortterm_hist) of the whole corpus."""
        out = np.empty(2000, np.uint64)
        _check(L.lib().ss_batch_allreduce_histograms(self._h, comm._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:1000].copy(), out[1000:].copy()

    def corpus_gate_enqueue(self, comm=None):
        """Queue the corpus gate on the device behind run(): all-reduce over `comm` (if any) + gate + LRA; no wait."""
        _check(L.lib().ss_batch_corpus_gate_enqueue(self._h, comm._h if comm is not None else None))

    def corpus_gate_read(self):
        """(integrated LUFS, LRA) of the last queued corpus gate (waits for the batch's stream)."""
        i, r = C.c_double(), C.c_double()
        _check(L.lib().ss_batch_corpus_gate_read(self._h, C.byref(i), C.byref(r)))
        return i.value, r.value

    def traffic_floor(self, reps=5):
        """ms per launch of the spectrum kernel's loads and stores alone (measurement utility; clobbers the spectra)."""
        ms = C.c_double()
        _check(L.lib().ss_batch_traffic_floor(self._h, reps, C.byref(ms)))
        return ms.value

    def checksums(self):
        """[n_streams][3] u64, computed on the device: order-independent checksums of every stream's whole spectrum block,
        decimation bins and sub-block energies (bit patterns).  Equal checksums <=> bit-equal data (up to 2^-64)."""
        n = int(self.cfg.n_streams)
        out = np.zeros((n, 3), np.uint64)
        _check(L.lib().ss_batch_checksums(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n))
        return out

    def fft(self, stream):
        lay = self.layout
        out = np.empty((lay.n_windows, lay.fft_channels, lay.n_bins), np.float32)
        _check(L.lib().ss_batch_download_fft(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out[:self.stream_shape(stream).n_windows] if self._ragged else out

    def bin_tables(self):
        n = self.layout.n_bins
        x, f, p = (np.empty(n, np.float64) for _ in range(3))
        dp = C.POINTER(C.c_double)
        _check(L.lib().ss_batch_bin_tables(self._h, x.ctypes.data_as(dp), f.ctypes.data_as(dp), p.ctypes.data_as(dp)))
        return x, f, p

    def waveform(self, stream):
        pts = self.layout.n_wave_points
        out = np.empty(pts, np.float32)
        _check(L.lib().ss_batch_download_waveform(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        if self._ragged:
            out = out[:self.stream_shape(stream).n_wave_points]
        return out.reshape(-1, 2)          # [bin] -> (min, max)

    # -- render-side reductions (tui.rs:49-51, :801-821, :664-681)
    def render_spectrum(self, cols, gain_db=None):
        """Reduce every spectrum row to `cols` chart columns on the device.  gain_db=None uses the
        reference's per-file rule -13 - integrated (tui.rs:1234)."""
        mode = L.SS_GAIN_REFERENCE if gain_db is None else L.SS_GAIN_FIXED
        _check(L.lib().ss_batch_render_spectrum(self._h, cols, mode, 0.0 if gain_db is None else float(gain_db)))
        self._render_cols = cols

    def set_columns_gain(self, gain_db=None):
        """columns-only batches: None = the reference's per-file rule -13 - integrated (needs the meter pass), else a fixed gain"""
        mode = L.SS_GAIN_REFERENCE if gain_db is None else L.SS_GAIN_FIXED
        _check(L.lib().ss_batch_set_columns_gain(self._h, mode, 0.0 if gain_db is None else float(gain_db)))

    def spectrum_columns(self, stream):
        lay = self.layout
        out = np.empty((lay.n_windows, lay.fft_channels, self._render_cols), np.float32)
        _check(L.lib().ss_batch_download_spectrum_columns(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    # -- one curve per stream: long-term average (power mean) and peak-hold spectrum over the stream's own windows
    def spectrum_stats(self):
        """Queue the reduction of every stream's rows behind run() (no copy, no wait)."""
        _check(L.lib().ss_batch_spectrum_stats(self._h))

    @property
    def spectrum_stats_plan(self):
        """(chunks, chunk_windows): how spectrum_stats() cuts the windows of this batch (chunks > 1: partial sums and a second launch)."""
        c, w = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_spectrum_stats_plan(self._h, C.byref(c), C.byref(w)))
        return c.value, w.value

    def _stats_triple(self, count_dtype):
        lay = self.layout
        shape = (lay.fft_channels, lay.n_bins)
        return np.empty(shape, np.float32), np.empty(shape, np.float32), np.empty(lay.fft_channels, count_dtype)

    def spectrum_stats_of(self, stream):
        """(mean_db[R][n_bins], max_db[R][n_bins], windows_counted[R]) of one stream after spectrum_stats(): NaN values (refused
        windows) are skipped; nothing counted gives NaN with count 0."""
        mean, mx, cnt = self._stats_triple(np.uint32)
        fp = C.POINTER(C.c_float)
        _check(L.lib().ss_batch_download_spectrum_stats(self._h, stream, mean.ctypes.data_as(fp), mx.ctypes.data_as(fp), mean.size,
                                                        cnt.ctypes.data_as(C.POINTER(C.c_uint32)), cnt.size))
        return mean, mx, cnt

    def corpus_spectrum(self):
        """The same triple for the whole batch pooled (every counted window of every stream weighs the same; counts are u64)."""
        mean, mx, cnt = self._stats_triple(np.uint64)
        fp = C.POINTER(C.c_float)
        _check(L.lib().ss_batch_corpus_spectrum(self._h, mean.ctypes.data_as(fp), mx.ctypes.data_as(fp), mean.size,
                                                cnt.ctypes.data_as(C.POINTER(C.c_uint64)), cnt.size))
        return mean, mx, cnt

    # -- one picture per stream: time columns x chart columns, the maximum of every cell's windows and bins
    def _spectrogram_view(self, t_cols, f_cols, w_min, w_max, gain_db):
        mode = L.SS_GAIN_REFERENCE if gain_db is None else L.SS_GAIN_FIXED
        return L.SpectrogramView(int(t_cols), int(f_cols), int(w_min), int(self.layout.n_windows if w_max is None else w_max),
                                 mode, 0.0 if gain_db is None else float(gain_db))

    def spectrogram(self, t_cols, f_cols, w_min=0, w_max=None, gain_db=None):
        """Queue the reduction of the windows [w_min, w_max) of every stream to t_cols x f_cols cells behind run() (no copy, no
        wait): time column t owns the windows with floor((w - w_min) * t_cols / (w_max - w_min)) == t, frequency column c the bins
        render_spectrum(f_cols) gives it; a cell is the maximum of clamp(dB + gain, -100, 0), NaN where it holds no value.
        w_max=None: the layout's n_windows; gain_db=None: the reference's per-file rule -13 - integrated.  Columns-only batches:
        f_cols must be spectrum_columns, and the gain is the pass's own."""
        v = self._spectrogram_view(t_cols, f_cols, w_min, w_max, gain_db)
        _check(L.lib().ss_batch_spectrogram(self._h, C.byref(v)))
        self._spectrogram_shape = (int(self.layout.fft_channels), int(t_cols), int(f_cols))

    def spectrogram_plan(self, t_cols, f_cols, w_min=0, w_max=None, gain_db=None):
        """(runs, run_windows): how spectrogram() cuts the windows of a time column of this view (runs > 1: partial maxima and a
        second launch)."""
        v = self._spectrogram_view(t_cols, f_cols, w_min, w_max, gain_db)
        r, w = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_spectrogram_plan(self._h, C.byref(v), C.byref(r), C.byref(w)))
        return r.value, w.value

    def spectrograms(self, first=0, count=None):
        """[count][fft_channels][t_cols][f_cols] f32 of the last spectrogram(): `count` streams from `first` on (None: all that
        follow) in one copy.  Before any spectrogram() the library refuses."""
        count = int(self.cfg.n_streams) - int(first) if count is None else int(count)
        out = np.empty((max(count, 0),) + getattr(self, "_spectrogram_shape", (0, 0, 0)), np.float32)
        _check(L.lib().ss_batch_download_spectrogram(self._h, int(first), count, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def spectrogram_of(self, stream):
        """[fft_channels][t_cols][f_cols] f32 of one stream after spectrogram()."""
        return self.spectrograms(stream, 1)[0]

    def windows_between(self, t0_s, t1_s):
        """(w_min, w_max): the windows that lie wholly inside the time range [t0_s, t1_s] seconds — window w covers the frames
        [first + w * hop, first + w * hop + fft_n), first = (fft_n // hop + 1) * hop - fft_n (where the pass puts window 0) —
        cut to the layout's n_windows; w_max == w_min where none does."""
        rate, n, hop = int(self.cfg.sample_rate), int(self.cfg.fft_n), int(self.cfg.hop_frames)
        first = (n // hop + 1) * hop - n
        # whole frames inside the range (a millionth of a frame forgives the rounding of seconds x rate)
        f0, f1 = max(0, int(np.ceil(float(t0_s) * rate - 1e-6))), int(np.floor(float(t1_s) * rate + 1e-6))
        lo = max(0, -((first - f0) // hop))                                  # smallest w with first + w * hop >= f0
        hi = (f1 - n - first) // hop + 1 if f1 >= first + n else 0          # one past the largest w with first + w * hop + n <= f1
        lo, hi = min(lo, int(self.layout.n_windows)), min(hi, int(self.layout.n_windows))
        return lo, max(lo, hi)

    def render_waveform(self, cols, x_min, x_max):
        _check(L.lib().ss_batch_render_waveform(self._h, cols, int(x_min), int(x_max)))
        self._render_wave_cols = cols

    def waveform_columns(self, stream):
        out = np.empty((self._render_wave_cols, 2), np.float32)
        _check(L.lib().ss_batch_download_waveform_columns(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def subblocks(self, stream):
        n = self.layout.n_subblocks
        out = np.empty((n, int(self.cfg.channels)), np.float64)
        _check(L.lib().ss_batch_download_subblocks(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def loudness_series(self, stream):
        """(momentary, shortterm): the stream's loudness after every 100 ms sub-block, LUFS, two f64 arrays of its own
        n_subblocks entries — entry j is what EbuR128::loudness_momentary() / loudness_shortterm() returns after the first
        (j + 1) sub-blocks (batches made with L.SS_BATCH_LOUDNESS_SERIES)."""
        n = int(self.stream_shape(stream).n_subblocks)
        m, s = np.empty(n, np.float64), np.empty(n, np.float64)
        dp = C.POINTER(C.c_double)
        _check(L.lib().ss_batch_download_loudness_series(self._h, stream, m.ctypes.data_as(dp), s.ctypes.data_as(dp), n))
        return m, s

    def loudness_extremes(self):
        """Per stream: L.LoudnessExtremes (max_momentary, max_shortterm, max_momentary_at, max_shortterm_at) over the full
        windows of its series; -inf at 0xFFFFFFFF where there is none."""
        n = int(self.cfg.n_streams)
        arr = (L.LoudnessExtremes * n)()
        _check(L.lib().ss_batch_loudness_extremes(self._h, arr, n))
        return list(arr)

    # -- follow-up calls on a region list: one setter and two record getters per kind
    def _set_list(self, kind, call, regions, n_groups, *more):
        """Queue the library's list setter `call` on `regions` (as _region_rows takes them) and remember the list's counts."""
        rows = _region_rows(regions)
        _check(call(self._h, rows.ctypes.data_as(C.POINTER(L.LoudnessRegion)), rows.shape[0], int(n_groups), *more))
        self._listed[kind] = (rows.shape[0], int(n_groups))                  # (a refused call leaves the previous list)

    def _records(self, kind, per_group, record, call):
        """One `record` per region (per_group: group) of the last list of `kind`; before any list the library refuses."""
        arr = (record * self._listed[kind][per_group])()
        _check(call(self._h, arr, len(arr)))
        return arr

    # -- loudness regions: gated loudness of time ranges of the streams, and of groups of them
    def loudness_regions(self, regions, n_groups=0):
        """Queue the gate of `regions` behind the pass: rows (stream, first_subblock, n_subblocks[, group]) in 100 ms sub-blocks,
        group 0 .. n_groups - 1 or L.SS_REGION_NO_GROUP (the default of a three-column row); a u32 array [n][4] is passed as it is.
        Replaces the previous list."""
        self._set_list("loudness", L.lib().ss_batch_loudness_regions, regions, n_groups)

    def region_results(self):
        """Per region of the last list: L.RegionResult (integrated_lufs, loudness_range, max_momentary, max_shortterm and their
        absolute sub-block indices, n_gating_blocks, n_st_blocks)."""
        return self._records("loudness", 0, L.RegionResult, L.lib().ss_batch_download_region_results)

    def group_results(self):
        """Per group of the last list: L.GroupResult (integrated_lufs, loudness_range, n_gating_blocks, n_st_blocks)."""
        return self._records("loudness", 1, L.GroupResult, L.lib().ss_batch_download_group_results)

    def group_histograms(self, g):
        """(block, short-term) histograms of group g: the bin-wise sums of its regions' pairs, 1000 u64 bins each."""
        out = np.empty(2000, np.uint64)
        _check(L.lib().ss_batch_group_histograms(self._h, int(g), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:1000].copy(), out[1000:].copy()

    # -- peak series and peak regions: true and sample peak per 100 ms entry, and their maxima over ranges and groups
    def peak_series(self):
        """Queue the peak series of whatever is resident: per (stream, 100 ms entry, channel) the true and sample peak and the
        frame of each.  Needs no run() and no particular flag."""
        _check(L.lib().ss_batch_peak_series(self._h))

    def peak_series_plan(self):
        """(tile_frames, entries_cap): the frames of an entry a workgroup stages at a time, and the entry slots per stream."""
        t, e = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_peak_series_plan(self._h, C.byref(t), C.byref(e)))
        return t.value, e.value

    def peak_series_of(self, stream):
        """Stream's entries: a structured array [entries][channels] (true_peak, sample_peak, true_peak_frame, sample_peak_frame;
        the frames are offsets in the entry, 0xFFFFFFFF where nothing was captured)."""
        ch, cap = int(self.cfg.channels), self.peak_series_plan()[1]
        out = np.zeros((cap, ch), PEAK_ENTRY_DTYPE)
        n = C.c_uint32()
        _check(L.lib().ss_batch_download_peak_series(self._h, stream, out.ctypes.data_as(C.POINTER(L.PeakEntry)), cap, C.byref(n)))
        return out[:n.value].copy()

    def peak_regions(self, regions, n_groups=0, ceiling=float("inf")):
        """Queue the maxima of the peak series over `regions` (rows as loudness_regions takes them, in 100 ms entries; a region may
        reach the stream's tail entry) behind peak_series(); `ceiling` (linear) is what n_over / first_over count against.
        Replaces the previous list."""
        self._set_list("peak", L.lib().ss_batch_peak_regions, regions, n_groups, float(ceiling))

    def region_peaks(self):
        """Per region of the last peak list: L.RegionPeaks (true_peak, sample_peak, their absolute frames and channels, n_over,
        first_over)."""
        return self._records("peak", 0, L.RegionPeaks, L.lib().ss_batch_download_region_peaks)

    def group_peaks(self):
        """Per group of the last peak list: L.GroupPeaks (true_peak, sample_peak, the regions that attain them, n_over)."""
        return self._records("peak", 1, L.GroupPeaks, L.lib().ss_batch_download_group_peaks)

    def region_channel_peaks(self):
        """(true_peak, sample_peak) of every channel of every region of the last peak list: two f32 arrays [regions][channels]."""
        shape = (self._listed["peak"][0], int(self.cfg.channels))
        tp, sp = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        fp = C.POINTER(C.c_float)
        _check(L.lib().ss_batch_download_region_channel_peaks(self._h, tp.ctypes.data_as(fp), sp.ctypes.data_as(fp), tp.size))
        return tp, sp

    # -- spectrum regions: average and peak-hold spectrum of time ranges of the streams, and of groups of them
    def spectrum_regions(self, regions, n_groups=0):
        """Queue the reduction of `regions` (rows as loudness_regions takes them, on the peak series' grid: a region may reach the
        stream's tail entry) behind run(): each owns the windows that lie wholly inside it (region_windows).  Replaces the
        previous list."""
        self._set_list("spectrum", L.lib().ss_batch_spectrum_regions, regions, n_groups)

    def _spectra(self, per_group, call, count_dtype, first, count):
        lay = self.layout
        count = self._listed["spectrum"][per_group] - int(first) if count is None else int(count)
        shape = (max(count, 0), int(lay.fft_channels), int(lay.n_bins))
        mean, mx, cnt = np.empty(shape, np.float32), np.empty(shape, np.float32), np.empty(shape[:2], count_dtype)
        fp = C.POINTER(C.c_float)
        _check(call(self._h, int(first), count, mean.ctypes.data_as(fp), mx.ctypes.data_as(fp), mean.size,
                    cnt.ctypes.data_as(C.POINTER(C.c_uint32 if count_dtype == np.uint32 else C.c_uint64)), cnt.size))
        return mean, mx, cnt

    def region_spectra(self, first=0, count=None):
        """(mean_db[count][R][n_bins], max_db[count][R][n_bins], windows_counted[count][R]) of `count` regions of the last
        spectrum list from `first` on (None: all that follow): NaN values (refused windows) are skipped; nothing counted gives NaN
        with count 0."""
        return self._spectra(0, L.lib().ss_batch_download_region_spectra, np.uint32, first, count)

    def group_spectra(self, first=0, count=None):
        """The same triple per group of the last spectrum list: its regions pooled, every counted window of every region weighing
        the same; the counts are u64."""
        return self._spectra(1, L.lib().ss_batch_download_group_spectra, np.uint64, first, count)

    @property
    def spectrum_regions_plan(self):
        """(chunks, chunk_windows): how the last spectrum_regions() list was cut (chunks > 1: partial sums and a second launch)."""
        c, w = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_spectrum_regions_plan(self._h, C.byref(c), C.byref(w)))
        return c.value, w.value

    def region_windows(self, region):
        """(w_first, w_end): the windows region (stream, first_subblock, n_subblocks[, group]) owns — ss_region_windows, cut to the
        stream's own window count."""
        a, e = C.c_uint32(), C.c_uint32()
        cfg = self.cfg
        L.lib().ss_region_windows(cfg.sample_rate, cfg.fft_n, cfg.hop_frames, int(region[1]), int(region[2]), C.byref(a), C.byref(e))
        nw = int(self.stream_shape(int(region[0])).n_windows)
        return min(a.value, nw), min(e.value, nw)

    # -- signal scan: silence, clip runs, DC and non-finite samples of every stream, and the lists of the runs
    def signal_scan(self, silence_threshold=0.0, clip_level=1.0, silence_min_frames=None, clip_min_samples=3, max_events=256):
        """Queue the scan of whatever is resident (no run(), no particular flag): a frame is silent iff |x| <= silence_threshold on
        every channel, a sample is clipped iff |x| >= clip_level (both linear); runs of at least silence_min_frames frames (None:
        100 ms) and clip_min_samples samples are counted and listed, max_events per stream and kind.  Replaces the previous scan."""
        if silence_min_frames is None:
            silence_min_frames = (int(self.cfg.sample_rate) + 5) // 10
        cfg = L.SignalScanConfig(float(silence_threshold), float(clip_level), int(silence_min_frames), int(clip_min_samples),
                                 int(max_events), 0)
        _check(L.lib().ss_batch_signal_scan(self._h, C.byref(cfg)))
        self._scan_events = int(max_events)

    def signal_scan_plan(self):
        """(tile_frames, tiles_cap): the frames one workgroup scans (a multiple of 64), and the tile slots per stream."""
        t, n = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_signal_scan_plan(self._h, C.byref(t), C.byref(n)))
        return t.value, n.value

    def stream_scans(self):
        """One record per stream, a structured array [n_streams] of STREAM_SCAN_DTYPE (UINT64_MAX where there is no run)."""
        out = np.zeros(int(self.cfg.n_streams), STREAM_SCAN_DTYPE)
        _check(L.lib().ss_batch_download_stream_scans(self._h, out.ctypes.data_as(C.POINTER(L.StreamScan)), out.size))
        return out

    def channel_scans(self):
        """One record per channel of every stream, a structured array [n_streams][channels] of CHANNEL_SCAN_DTYPE: DC is
        sum / (frames - nonfinite)."""
        out = np.zeros((int(self.cfg.n_streams), int(self.cfg.channels)), CHANNEL_SCAN_DTYPE)
        _check(L.lib().ss_batch_download_channel_scans(self._h, out.ctypes.data_as(C.POINTER(L.ChannelScan)), out.size))
        return out

    def signal_events(self, stream, kind):
        """The stream's listed runs of `kind` (SIGNAL_SILENCE: by first_frame, channel 0xFFFFFFFF; SIGNAL_CLIP: by (channel,
        first_frame)): a structured array of SIGNAL_EVENT_DTYPE, the first max_events of them."""
        cap = getattr(self, "_scan_events", 0)
        out = np.zeros(cap, SIGNAL_EVENT_DTYPE)
        n = C.c_uint32()
        _check(L.lib().ss_batch_download_signal_events(self._h, int(stream), int(kind), out.ctypes.data_as(C.POINTER(L.SignalEvent)),
                                                       cap, C.byref(n)))
        return out[:n.value].copy()

    # -- pair series and pair regions: sums of x_a^2, x_b^2, x_a x_b per 100 ms entry, and over ranges and groups
    def pair_series(self, pairs=None):
        """Queue the pair series of whatever is resident (no run(), no particular flag): per (stream, 100 ms entry, pair) the f64
        sums over the frames in which both samples are finite.  `pairs`: up to 16 (a, b) channel pairs, None: the one pair (0, 1).
        Replaces the previous series, pair list included."""
        if pairs is None:
            _check(L.lib().ss_batch_pair_series(self._h, None, 0))
        else:
            a = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
            _check(L.lib().ss_batch_pair_series(self._h, a.ctypes.data_as(C.POINTER(L.ChannelPair)), a.shape[0]))

    def pair_series_plan(self):
        """(tile_frames, entries_cap, n_pairs): the frames a workgroup has in flight at a time, the entry slots per stream, the
        pairs of the last series."""
        t, e, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_pair_series_plan(self._h, C.byref(t), C.byref(e), C.byref(n)))
        return t.value, e.value, n.value

    def pair_entries(self, stream):
        """Stream's entries: a structured array [entries][pairs] of PAIR_ENTRY_DTYPE (pair_correlation and its neighbours read it)."""
        _, cap, pairs = self.pair_series_plan()
        out = np.zeros((cap, pairs), PAIR_ENTRY_DTYPE)
        n = C.c_uint32()
        _check(L.lib().ss_batch_download_pair_series(self._h, int(stream), out.ctypes.data_as(C.POINTER(L.PairEntry)), cap, C.byref(n)))
        return out[:n.value].copy()

    def pair_regions(self, regions, n_groups=0, threshold=0.0, power_floor=0.0, min_run=1):
        """Queue the reduction of the pair series over `regions` (rows as loudness_regions takes them, on the peak series' grid: a
        region may reach the stream's tail entry) behind pair_series().  An entry is active iff s_aa + s_bb > power_floor * frames
        and below iff its correlation < threshold; runs of at least min_run active below entries are counted.  Replaces the
        previous list."""
        cfg = L.PairRegionConfig(float(threshold), float(power_floor), int(min_run), 0)
        self._set_list("pair", L.lib().ss_batch_pair_regions, regions, n_groups, C.byref(cfg))
        self._listed_pairs = self.pair_series_plan()[2]

    def _pair_records(self, per_group, dtype, record, call):
        pairs = getattr(self, "_listed_pairs", 0)
        out = np.zeros((self._listed["pair"][per_group], pairs), dtype)
        _check(call(self._h, out.ctypes.data_as(C.POINTER(record)), out.size))
        return out

    def region_pairs(self):
        """Per region of the last pair list: a structured array [regions][pairs] of REGION_PAIR_DTYPE."""
        return self._pair_records(0, REGION_PAIR_DTYPE, L.RegionPair, L.lib().ss_batch_download_region_pairs)

    def group_pairs(self):
        """Per group of the last pair list: a structured array [groups][pairs] of GROUP_PAIR_DTYPE."""
        return self._pair_records(1, GROUP_PAIR_DTYPE, L.GroupPair, L.lib().ss_batch_download_group_pairs)

    # -- batch gain and PCM export: a gain curve per stream applied to the resident corpus, and the corpus in a delivery format
    def apply_gain(self, points, channel_mask=0, clip_level=1.0):
        """Queue the sweep that multiplies the resident corpus in place by every stream's gain curve (gain_envelope): `points` is a
        GAIN_POINT_DTYPE array or rows (stream, frame, gain), grouped by stream, frames strictly ascending.  channel_mask 0: every
        channel, else bit c selects channel c.  Lossy (one rounding per sample); results of earlier passes and series describe the
        corpus before the call."""
        p = _gain_points(points)
        cfg = L.GainConfig(int(channel_mask), float(clip_level), 0)
        _check(L.lib().ss_batch_apply_gain(self._h, p.ctypes.data_as(C.POINTER(L.GainPoint)) if p.size else None, p.size, C.byref(cfg)))

    def apply_gain_plan(self):
        """tile_frames: the frames one workgroup of the sweep covers."""
        t = C.c_uint32()
        _check(L.lib().ss_batch_apply_gain_plan(self._h, C.byref(t)))
        return t.value

    def gain_stats(self):
        """What the last apply_gain() left, a structured array [n_streams][channels] of GAIN_CHANNEL_DTYPE over every stream's own
        frames: the largest finite |y|, the samples at or over clip_level and the first such frame, the non-finite samples."""
        out = np.zeros((int(self.cfg.n_streams), int(self.cfg.channels)), GAIN_CHANNEL_DTYPE)
        _check(L.lib().ss_batch_download_gain_stats(self._h, out.ctypes.data_as(C.POINTER(L.GainChannel)), out.size))
        return out

    def download_pcm(self, first, count, format, dither_seed=None):
        """`count` slots from stream `first` on in a delivery format (L.SS_PCM_*), [count][frames_per_stream][channels] (24-bit: a
        last axis of the three little-endian bytes); frames behind a stream's own length read the format's zero.  dither_seed: TPDF
        dither of +-1 LSB from that seed on the integer formats."""
        shape = (int(count), int(self.cfg.frames_per_stream), int(self.cfg.channels)) + ((3,) if format == L.SS_PCM_S24 else ())
        out = np.empty(shape, _PCM_DTYPES.get(format, np.uint8))
        dither = None if dither_seed is None else C.byref(L.PcmDither(int(dither_seed) & 0xFFFFFFFFFFFFFFFF, L.SS_DITHER_TPDF, 0))
        _check(L.lib().ss_batch_download_pcm(self._h, int(first), int(count), out.ctypes.data_as(C.c_void_p), out.nbytes, int(format), dither))
        return out

    # -- batch limiter: the gain and a look-ahead gain curve that shapes only what would cross the ceiling, in one sweep
    def _limit_config(self, ceiling, lookahead_s, hold_s, true_peak, channel_mask, clip_level, scratch_bytes):
        rate = int(self.cfg.sample_rate)
        frames = [int(round(float(s) * rate)) for s in (lookahead_s, hold_s)]
        if not 0 <= frames[0] <= L.SS_LIMIT_LOOKAHEAD_MAX or not 0 <= frames[1] <= L.SS_LIMIT_HOLD_MAX:
            raise ValueError("limiter: a look-ahead of %d or a hold of %d frames is outside [0, %d] / [0, %d]"
                             % (frames[0], frames[1], L.SS_LIMIT_LOOKAHEAD_MAX, L.SS_LIMIT_HOLD_MAX))
        return L.LimitConfig(int(channel_mask), float(ceiling), float(clip_level), frames[0], frames[1],
                             L.SS_LIMIT_TRUE_PEAK if true_peak else L.SS_LIMIT_SAMPLE_PEAK, 0, int(scratch_bytes))

    def limit(self, items, ceiling, lookahead_s=0.0015, hold_s=0.010, true_peak=True, channel_mask=0, clip_level=1.0, scratch_bytes=0):
        """Queue the limiter's sweep over the resident corpus, in place: `items` is a LIMIT_ITEM_DTYPE array or rows (stream, gain),
        each stream at most once; a stream's samples become x * gain * c[n] with the gain curve c of limit_curve from the linked
        level of the selected channels (true_peak: the batch's interpolator, else the samples' magnitudes), so that every finite
        |y| <= ceiling.  Seconds become frames by round(s * rate); a value beyond the maxima is refused.  Lossy; results of earlier
        passes and series describe the corpus before the call."""
        it = _limit_items(items)
        cfg = self._limit_config(ceiling, lookahead_s, hold_s, true_peak, channel_mask, clip_level, scratch_bytes)
        _check(L.lib().ss_batch_limit(self._h, it.ctypes.data_as(C.POINTER(L.LimitItem)) if it.size else None, it.size, C.byref(cfg)))

    def limit_plan(self, n_items, ceiling=1.0, lookahead_s=0.0015, hold_s=0.010, true_peak=True, channel_mask=0, clip_level=1.0, scratch_bytes=0):
        """(tile_frames, group_streams, scratch_bytes) of a limit() call with n_items items: the frames one workgroup sweeps, the
        streams whose required gains the scratch buffer holds at a time (the sweep runs group after group), and that buffer's bytes."""
        cfg = self._limit_config(ceiling, lookahead_s, hold_s, true_peak, channel_mask, clip_level, scratch_bytes)
        t, g, sb = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(L.lib().ss_batch_limit_plan(self._h, C.byref(cfg), int(n_items), C.byref(t), C.byref(g), C.byref(sb)))
        return t.value, g.value, sb.value

    def limit_stats(self):
        """What the last limit() left: (LIMIT_STREAM_DTYPE [n_streams], GAIN_CHANNEL_DTYPE [n_streams][channels]) — the frames whose
        gain was lowered, the first of them and the lowest window sum per stream, and gain_stats()' records of the corpus behind it."""
        n = int(self.cfg.n_streams)
        streams, channels = np.zeros(n, LIMIT_STREAM_DTYPE), np.zeros((n, int(self.cfg.channels)), GAIN_CHANNEL_DTYPE)
        _check(L.lib().ss_batch_download_limit_stats(self._h, streams.ctypes.data_as(C.POINTER(L.LimitStream)), streams.size,
                                                     channels.ctypes.data_as(C.POINTER(L.GainChannel)), channels.size))
        return streams, channels

    # -- batch resampler: every stream of this batch converted to another rate, into the same slot of another batch
    def resample_into(self, dst, plan):
        """Queue the conversion of every stream, each at its own length, into the same slot of `dst` (a batch at plan.out_rate with
        the same channels and streams, and a slot that holds the longest output): dst gets the lengths resample_length(F_s) as
        dst.set_lengths() would give them, floats behind them keep their bytes, and every output equals resample_host in bits.
        Queued on dst's stream behind what this batch's stream holds; work queued on this batch later runs behind the read."""
        _check(L.lib().ss_batch_resample(self._h, dst._h, C.byref(plan)))
        dst._ragged = True

    def resample_tiles(self, plan):
        """(tile_out_frames, tile_in_frames): the outputs one workgroup of resample_into converts and the input frames they span."""
        o, i = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_batch_resample_plan(self._h, C.byref(plan), C.byref(o), C.byref(i)))
        return o.value, i.value

    def resample(self, out_rate, attenuation_db=0.0, passband=0.0, **batch_kwargs):
        """A new Batch at out_rate holding this batch's streams converted (resample_plan, resample_into): this batch's other
        settings unless batch_kwargs (Batch's keywords) says otherwise, and a slot as long as the longest output needs."""
        cfg = self.cfg
        plan = resample_plan(int(cfg.sample_rate), out_rate, attenuation_db, passband)
        longest = max(resample_length(plan, self.stream_shape(s).frames) for s in range(int(cfg.n_streams)))
        kw = dict(fft_n=int(cfg.fft_n), hop_frames=int(cfg.hop_frames), flags=int(cfg.flags), true_peak_factor=int(cfg.true_peak_factor),
                  waveform_window=float(cfg.waveform_window), spectrum_columns=int(cfg.spectrum_columns))
        kw.update(batch_kwargs)
        dst = Batch(int(out_rate), int(cfg.channels), int(cfg.n_streams), max(1, longest), **kw)
        self.resample_into(dst, plan)
        return dst

    def normalise(self, target_lufs, max_true_peak_dbtp=float("inf"), max_gain_db=float("inf"), min_gain_db=float("-inf"), album=False,
                  limiter=None):
        """Bring every stream to `target_lufs` under a true-peak ceiling (normalisation_gain) and apply the gains on the device, one
        constant gain per stream; album: ONE gain for all streams, from the loudness and the peak of all of them pooled.  Needs
        L.SS_BATCH_LUFS; runs a pass if none has run, then peak_series(), and replaces the peak (album: and loudness) region list.
        limiter: a dict of limit()'s keywords (lookahead_s, hold_s, true_peak, ...) — the law is then evaluated with no peak ceiling
        (limited_by never reads SS_GAIN_LIMITED_PEAK) and the one sweep is limit() with those gains under the ceiling
        10^(max_true_peak_dbtp / 20), which must be finite.
        Returns a NORMALISE_DTYPE array [n_streams]: the loudness and linear peak read, gain_db, gain, limited_by."""
        if not int(self.cfg.flags) & L.SS_BATCH_LUFS:
            raise ValueError("normalise needs a batch with SS_BATCH_LUFS")
        n, S = int(self.cfg.n_streams), (int(self.cfg.sample_rate) + 5) // 10
        if not getattr(self, "_ran", False):
            self.run()
        self.peak_series()
        shapes = [self.stream_shape(s) for s in range(n)]
        whole = [(s, 0, (int(sh.frames) + S - 1) // S, 0) for s, sh in enumerate(shapes)]          # every entry, the tail's included
        out = np.zeros(n, NORMALISE_DTYPE)
        if album:
            self.loudness_regions([(s, 0, int(sh.n_subblocks), 0) for s, sh in enumerate(shapes)], 1)
            self.peak_regions(whole, 1)
            out["loudness"], out["peak"] = self.group_results()[0].integrated_lufs, self.group_peaks()[0].true_peak
        else:
            self.peak_regions(whole, 1)
            out["loudness"] = [r.integrated_lufs for r in self.results()]
            out["peak"] = [r.true_peak for r in self.region_peaks()]
        if limiter is not None and not np.isfinite(max_true_peak_dbtp):
            raise ValueError("normalise with a limiter needs a finite max_true_peak_dbtp")
        out["gain_db"], out["gain"], out["limited_by"] = normalisation_gain(out["loudness"], out["peak"], target_lufs,
                                                                            max_true_peak_dbtp if limiter is None else float("inf"),
                                                                            max_gain_db, min_gain_db)
        if limiter is not None:
            items = np.zeros(n, LIMIT_ITEM_DTYPE)
            items["stream"], items["gain"] = np.arange(n), out["gain"]
            self.limit(items, 10.0 ** (float(max_true_peak_dbtp) / 20.0), **limiter)
            return out
        points = np.zeros(n, GAIN_POINT_DTYPE)
        points["stream"], points["gain"] = np.arange(n), out["gain"]
        self.apply_gain(points)
        return out

    def histograms(self):
        out = np.empty(2000, np.uint64)
        _check(L.lib().ss_batch_histograms(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:1000].copy(), out[1000:].copy()

    def histograms_to_device(self, dev_ptr):
        _check(L.lib().ss_batch_histograms_device(self._h, C.c_void_p(dev_ptr)))

    def timing_enable(self, on=True):
        _check(L.lib().ss_batch_timing_enable(self._h, 1 if on else 0))

    def timing_read(self, kernel):
        ms, n = C.c_double(), C.c_uint64()
        _check(L.lib().ss_batch_timing_read(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def corpus_integrated_lufs(block_hist):
    h = np.ascontiguousarray(block_hist, dtype=np.uint64)
    return L.lib().ss_corpus_integrated_lufs(h.ctypes.data_as(C.POINTER(C.c_uint64)))


def corpus_loudness_range(st_hist):
    h = np.ascontiguousarray(st_hist, dtype=np.uint64)
    return L.lib().ss_corpus_loudness_range(h.ctypes.data_as(C.POINTER(C.c_uint64)))


def waveform_view(playhead_ms, waveform_window_s, chart_points):
    """Player-mode x bounds of the waveform chart (tui.rs:664-681) -> (x_min, x_max)."""
    lo, hi = C.c_double(), C.c_double()
    L.lib().ss_waveform_view(float(playhead_ms), float(waveform_window_s), int(chart_points), C.byref(lo), C.byref(hi))
    return lo.value, hi.value
