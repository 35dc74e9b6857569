"""Meter banks (include/soundscope_hip.h, "Meter banks"): N live EBU R128 meters of one shape, advanced together.

Stream s of a bank behaves exactly like an `Analyzer` loudness meter fed the same blocks; a call advances every stream with a
time-domain launch and a gating launch, and `read()` returns every stream's readings behind one launch and one copy.
The streams need not move together: `add_ragged()` gives every stream its own number of frames per call, none included.
With `enable_spectrum()` the bank also keeps every stream's newest 16384 input frames, and `spectrum()` /
`spectrum_columns()` transform all of them (mid and side for stereo banks) in one launch.
With `enable_spectrum_tracking()` it keeps, per row, an exponentially averaged and a peak-hold curve on the device;
`track_spectrum()` advances them on each stream's own clock, `tracked_spectrum()` / `tracked_spectrum_columns()` read them.
With `enable_signal_watch()` every add also advances, per stream, the records `Batch.signal_scan` defines for everything the
stream was given: silence and since when, clip runs, DC sums and non-finite samples; `signal_watch()` reads them.
With `enable_pair_watch()` every add also advances, per stream and channel pair, the entries `Batch.pair_series` defines: the sums
of the newest window and of everything so far, and the runs of entries below a correlation threshold; `pair_watch()` reads them.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .analyzer import _check
from .batch import PAIR_ENTRY_DTYPE

# the structured arrays' dtypes are the ctypes records' (_lib.py), as batch.py's are
READING_DTYPE = np.dtype(L.MeterReading)
# ss_stream_watch / ss_channel_watch: the batch scan's records (batch.STREAM_SCAN_DTYPE / CHANNEL_SCAN_DTYPE), then the live fields
STREAM_WATCH_DTYPE = np.dtype(L.StreamWatch)
CHANNEL_WATCH_DTYPE = np.dtype(L.ChannelWatch)
# ss_pair_watch: `window` and `total` are records with the pair entries' field names, so that batch.pair_correlation, pair_balance_db
# and pair_mono_loss_db take rec["window"] or rec["total"] directly
PAIR_SUMS_DTYPE = np.dtype(L.PairSums)
PAIR_WATCH_DTYPE = np.dtype(L.PairWatch)


class MeterBank:
    """`n_streams` meters of `channels` channels at `rate`; true_peak_factor 0 = the crate's rule for the rate, or 2 / 4."""

    def __init__(self, n_streams, channels, rate, true_peak_factor=0):
        self._h = C.c_void_p()
        _check(L.lib().ss_meter_bank_create(n_streams, channels, rate, true_peak_factor, C.byref(self._h)))
        self.n_streams, self.channels, self.rate = int(n_streams), int(channels), int(rate)

    def __del__(self):
        if getattr(self, "_h", None):
            L.lib().ss_meter_bank_destroy(self._h)
            self._h = None

    def _frames(self, size, per_sample=1):
        per = self.n_streams * self.channels * per_sample
        if size % per:
            raise ValueError(f"{size} values are not whole frames of {self.n_streams} streams x {self.channels} channels")
        return size // per

    def add(self, pcm):
        """pcm: [n_streams][frames * channels] f32 (any shape with that many values, stream-major)."""
        a = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        _check(L.lib().ss_meter_bank_add(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), self._frames(a.size)))

    def add_device(self, ptr, frames, stream_stride_floats):
        """Device-resident f32 input: stream s at `ptr` + s * stream_stride_floats (an int device address, e.g. a tensor's
        data_ptr()).  Only queued: the buffer must stay unchanged until the next read."""
        _check(L.lib().ss_meter_bank_add_device(self._h, C.c_void_p(int(ptr)), int(frames), int(stream_stride_floats)))

    def add_pcm(self, raw, fmt):
        """Raw little-endian interleaved samples of an ss_pcm_format (bytes or a numpy array), [stream][frame][channel]."""
        b = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        sb = int(L.lib().ss_pcm_sample_bytes(int(fmt))) or 1
        frames = self._frames(b.size, sb)
        _check(L.lib().ss_meter_bank_add_pcm(self._h, b.ctypes.data_as(C.c_void_p), frames, int(fmt)))

    def _ragged(self, blocks, to_bytes, per_sample):
        """(pointer array, frames array, the arrays kept alive) of one block per stream; None or an empty block: no frames"""
        if len(blocks) != self.n_streams:
            raise ValueError(f"{len(blocks)} blocks for {self.n_streams} streams")
        keep, ptrs, frames = [], (C.c_void_p * self.n_streams)(), (C.c_uint64 * self.n_streams)()
        for s, blk in enumerate(blocks):
            if blk is None:
                continue
            a = to_bytes(blk)
            per = self.channels * per_sample
            if a.size % per:
                raise ValueError(f"stream {s}: {a.size} values are not whole frames of {self.channels} channels")
            if a.size:
                keep.append(a)
                ptrs[s], frames[s] = a.ctypes.data, a.size // per
        return ptrs, frames, keep

    def add_ragged(self, blocks):
        """blocks: one per stream, [frames_s * channels] f32 (any shape with that many values) or None for no frames.  Stream s
        advances by its own frames_s; a stream given nothing is not touched."""
        ptrs, frames, keep = self._ragged(blocks, lambda b: np.ascontiguousarray(b, dtype=np.float32).reshape(-1), 1)
        _check(L.lib().ss_meter_bank_add_ragged(self._h, ptrs, frames))

    def add_ragged_pcm(self, blocks, fmt):
        """The same for raw little-endian interleaved samples of an ss_pcm_format: bytes or a numpy array per stream, or None."""
        def raw(b):
            return np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b).view(np.uint8).reshape(-1)
        sb = int(L.lib().ss_pcm_sample_bytes(int(fmt))) or 1
        ptrs, frames, keep = self._ragged(blocks, raw, sb)
        _check(L.lib().ss_meter_bank_add_ragged_pcm(self._h, ptrs, frames, int(fmt)))

    def add_ragged_device(self, ptr, frames, stream_stride_floats):
        """Device-resident f32 input: stream s's frames[s] frames at `ptr` + s * stream_stride_floats.  Only queued, as add_device."""
        f = np.ascontiguousarray(frames, dtype=np.uint64).reshape(-1)
        if f.size != self.n_streams:
            raise ValueError(f"{f.size} frame counts for {self.n_streams} streams")
        _check(L.lib().ss_meter_bank_add_ragged_device(self._h, C.c_void_p(int(ptr)), f.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       int(stream_stride_floats)))

    def reset(self, streams=None):
        """Reset the listed streams (None: all), as EbuR128::reset; the others are untouched."""
        if streams is None:
            _check(L.lib().ss_meter_bank_reset(self._h, None, 0))
            return
        a = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
        _check(L.lib().ss_meter_bank_reset(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def read(self):
        """Every stream's readings: a structured array [n_streams] of READING_DTYPE (fields as ss_meter_reading)."""
        out = np.empty(self.n_streams, READING_DTYPE)
        _check(L.lib().ss_meter_bank_read(self._h, out.ctypes.data_as(C.c_void_p), self.n_streams))
        return out

    def peaks(self, stream):
        """Every channel's (true_peak, sample_peak) of one stream, linear: arrays [channels] f64."""
        tp, sp = np.empty(self.channels, np.float64), np.empty(self.channels, np.float64)
        dp = C.POINTER(C.c_double)
        _check(L.lib().ss_meter_bank_peaks(self._h, stream, tp.ctypes.data_as(dp), sp.ctypes.data_as(dp), self.channels))
        return tp, sp

    def histograms(self, stream):
        """(block, short-term) histograms of one stream: two arrays [1000] u64."""
        out = np.empty(2000, np.uint64)
        _check(L.lib().ss_meter_bank_histograms(self._h, stream, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out[:1000].copy(), out[1000:].copy()

    # ---- spectra (ss_meter_bank_spectrum_*) ------------------------------------------------------------------------------------
    def enable_spectrum(self, on=True):
        """Keep (on) or drop every stream's history of the newest 16384 frames; enabling starts from a zero window."""
        _check(L.lib().ss_meter_bank_spectrum_enable(self._h, 1 if on else 0))

    def spectrum_layout(self):
        """(rows per stream, n_bins, chart_x [n_bins] f64): chart_x is the first element of get_fft's pairs."""
        r, nb = C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_meter_bank_spectrum_layout(self._h, C.byref(r), C.byref(nb), None, None, 0))
        x = np.empty(nb.value, np.float64)
        _check(L.lib().ss_meter_bank_spectrum_layout(self._h, None, None, x.ctypes.data_as(C.POINTER(C.c_double)), None, nb.value))
        return r.value, nb.value, x

    def spectrum_pink(self):
        """The f64 pink compensation [n_bins] that get_fft adds to a row's dB values."""
        _, nb, _ = self.spectrum_layout()
        p = np.empty(nb, np.float64)
        _check(L.lib().ss_meter_bank_spectrum_layout(self._h, None, None, None, p.ctypes.data_as(C.POINTER(C.c_double)), nb))
        return p

    def spectrum(self):
        """(rows [n_streams, rows, n_bins] f32 dBFS before pink compensation, status [n_streams, rows] i32 ss_status)."""
        r, nb, _ = self.spectrum_layout()
        rows = np.empty((self.n_streams, r, nb), np.float32)
        st = np.empty((self.n_streams, r), np.int32)
        _check(L.lib().ss_meter_bank_spectrum(self._h, rows.ctypes.data_as(C.POINTER(C.c_float)), rows.size,
                                              st.ctypes.data_as(C.POINTER(C.c_int32)), st.size))
        return rows, st

    @staticmethod
    def _gain(gain):
        """(gain mode, gain_db) of a gain argument: None (0 dB), a float in dB, or 'reference'"""
        if isinstance(gain, str):
            if gain != "reference":
                raise ValueError(f"gain {gain!r}: None, a number or 'reference'")
            return L.SS_GAIN_REFERENCE, 0.0
        return L.SS_GAIN_FIXED, 0.0 if gain is None else float(gain)

    def spectrum_columns(self, cols, gain=None):
        """(columns [n_streams, rows, cols] f32, status [n_streams, rows] i32).  gain: None (0 dB), a float in dB, or "reference"
        (-13 - integrated loudness of each stream, tui.rs:1234)."""
        r, _, _ = self.spectrum_layout()
        mode, g = self._gain(gain)
        out = np.empty((self.n_streams, r, int(cols)), np.float32)
        st = np.empty((self.n_streams, r), np.int32)
        _check(L.lib().ss_meter_bank_spectrum_columns(self._h, int(cols), mode, g, out.ctypes.data_as(C.POINTER(C.c_float)), out.size,
                                                      st.ctypes.data_as(C.POINTER(C.c_int32)), st.size))
        return out, st

    # ---- tracked spectra (ss_meter_bank_spectrum_track*) -----------------------------------------------------------------------
    def enable_spectrum_tracking(self, average_tau_s, hold_s, decay_db_per_s):
        """Keep, per row, an exponentially averaged power spectrum (time constant average_tau_s; 0: the newest row) and a
        peak-hold spectrum (held hold_s seconds, inf: for ever, then falling decay_db_per_s) on the device.  Needs
        enable_spectrum(); enabling again starts from empty state."""
        cfg = L.SpectrumBallistics(float(average_tau_s), float(hold_s), float(decay_db_per_s))
        _check(L.lib().ss_meter_bank_spectrum_track_enable(self._h, C.byref(cfg)))

    def disable_spectrum_tracking(self):
        """Tracking off, its device memory freed."""
        _check(L.lib().ss_meter_bank_spectrum_track_enable(self._h, None))

    def track_spectrum(self):
        """Advance every row's curves to the windows as they stand, each stream by the frames it has had since its last update
        (a stream given nothing, or a refused row, is left alone).  Only queued: two launches, no copy, no wait."""
        _check(L.lib().ss_meter_bank_spectrum_track(self._h))

    def reset_spectrum_tracking(self, streams=None):
        """Empty the listed streams' curves (None: all); their next update starts them again."""
        if streams is None:
            _check(L.lib().ss_meter_bank_spectrum_track_reset(self._h, None, 0))
            return
        a = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
        _check(L.lib().ss_meter_bank_spectrum_track_reset(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def tracked_spectrum(self):
        """(avg [n_streams, rows, n_bins] f32 dB, hold [n_streams, rows, n_bins] f32 dB, updates [n_streams, rows] u32): both
        curves before pink compensation, like spectrum(); a row with updates == 0 is all NaN."""
        r, nb, _ = self.spectrum_layout()
        avg = np.empty((self.n_streams, r, nb), np.float32)
        hold = np.empty((self.n_streams, r, nb), np.float32)
        upd = np.empty((self.n_streams, r), np.uint32)
        fp = C.POINTER(C.c_float)
        _check(L.lib().ss_meter_bank_spectrum_tracked(self._h, avg.ctypes.data_as(fp), hold.ctypes.data_as(fp), avg.size,
                                                      upd.ctypes.data_as(C.POINTER(C.c_uint32)), upd.size))
        return avg, hold, upd

    def tracked_spectrum_columns(self, cols, gain=None):
        """(avg [n_streams, rows, cols] f32, hold [n_streams, rows, cols] f32, updates [n_streams, rows] u32): both curves reduced
        to chart columns on the device by spectrum_columns()'s rule; gain as there.  NaN: a column without a bin, a row without
        state."""
        r, _, _ = self.spectrum_layout()
        mode, g = self._gain(gain)
        avg = np.empty((self.n_streams, r, int(cols)), np.float32)
        hold = np.empty((self.n_streams, r, int(cols)), np.float32)
        upd = np.empty((self.n_streams, r), np.uint32)
        fp = C.POINTER(C.c_float)
        _check(L.lib().ss_meter_bank_spectrum_tracked_columns(self._h, int(cols), mode, g, avg.ctypes.data_as(fp),
                                                              hold.ctypes.data_as(fp), avg.size,
                                                              upd.ctypes.data_as(C.POINTER(C.c_uint32)), upd.size))
        return avg, hold, upd

    # ---- signal watch (ss_meter_bank_signal_watch*) ----------------------------------------------------------------------------
    def enable_signal_watch(self, silence_threshold=0.0, clip_level=1.0, silence_min_frames=None, clip_min_samples=3):
        """Watch every stream's input from now on: silent frames (|x| <= silence_threshold on every channel) and clipped samples
        (|x| >= clip_level), their runs of at least silence_min_frames (None: 100 ms, as Batch.signal_scan) / clip_min_samples, the
        DC sums and the non-finite samples.  Enabling again starts empty."""
        if silence_min_frames is None:
            silence_min_frames = (self.rate + 5) // 10
        cfg = L.SignalScanConfig(float(silence_threshold), float(clip_level), int(silence_min_frames), int(clip_min_samples), 0, 0)
        _check(L.lib().ss_meter_bank_signal_watch_enable(self._h, C.byref(cfg)))

    def disable_signal_watch(self):
        """The watch off, its device memory freed."""
        _check(L.lib().ss_meter_bank_signal_watch_enable(self._h, None))

    def signal_watch_plan(self):
        """Frames one tile of the watch kernel holds (a multiple of 64)."""
        t = C.c_uint32()
        _check(L.lib().ss_meter_bank_signal_watch_plan(self._h, C.byref(t)))
        return t.value

    def reset_signal_watch(self, streams=None):
        """Empty the listed streams' watch (None: all); the others are untouched."""
        if streams is None:
            _check(L.lib().ss_meter_bank_signal_watch_reset(self._h, None, 0))
            return
        a = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
        _check(L.lib().ss_meter_bank_signal_watch_reset(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def signal_watch(self):
        """(streams [n_streams] of STREAM_WATCH_DTYPE, channels [n_streams, channels] of CHANNEL_WATCH_DTYPE) for everything each
        stream was given since its watch reset; frame numbers count from there."""
        st = np.empty(self.n_streams, STREAM_WATCH_DTYPE)
        ch = np.empty((self.n_streams, self.channels), CHANNEL_WATCH_DTYPE)
        _check(L.lib().ss_meter_bank_signal_watch(self._h, st.ctypes.data_as(C.POINTER(L.StreamWatch)), st.size,
                                                  ch.ctypes.data_as(C.POINTER(L.ChannelWatch)), ch.size))
        return st, ch

    # ---- pair watch (ss_meter_bank_pair_watch*) --------------------------------------------------------------------------------
    def enable_pair_watch(self, pairs=None, window_s=3.0, threshold=0.0, power_floor=0.0, min_run=1):
        """Watch, from now on, how the channels of every stream relate: per `pairs` (up to 16 (a, b) channel pairs, None: the one
        pair (0, 1)) the f64 sums of every complete 100 ms entry as Batch.pair_series defines them, the newest window_s seconds of
        them (1 .. 600 entries), the totals, and the runs of active entries whose correlation is below `threshold`
        (Batch.pair_regions' predicates).  Enabling again starts empty."""
        cfg = L.PairWatchConfig(float(threshold), float(power_floor), int(min_run), int(round(float(window_s) * 10.0)))
        if pairs is None:
            _check(L.lib().ss_meter_bank_pair_watch_enable(self._h, None, 0, C.byref(cfg)))
        else:
            a = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
            _check(L.lib().ss_meter_bank_pair_watch_enable(self._h, a.ctypes.data_as(C.POINTER(L.ChannelPair)), a.shape[0], C.byref(cfg)))

    def disable_pair_watch(self):
        """The pair watch off, its device memory freed."""
        _check(L.lib().ss_meter_bank_pair_watch_enable(self._h, None, 0, None))

    def pair_watch_plan(self):
        """(lanes, window_entries, n_pairs): frame i of an entry belongs to lane i mod lanes (256); the window in entries; the pairs."""
        ln, w, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(L.lib().ss_meter_bank_pair_watch_plan(self._h, C.byref(ln), C.byref(w), C.byref(n)))
        return ln.value, w.value, n.value

    def reset_pair_watch(self, streams=None):
        """Empty the listed streams' pair watch (None: all); the others are untouched."""
        if streams is None:
            _check(L.lib().ss_meter_bank_pair_watch_reset(self._h, None, 0))
            return
        a = np.ascontiguousarray(streams, dtype=np.uint32).reshape(-1)
        _check(L.lib().ss_meter_bank_pair_watch_reset(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))

    def pair_watch(self):
        """Records [n_streams, n_pairs] of PAIR_WATCH_DTYPE for everything each stream was given since its pair-watch reset;
        entry numbers count from there."""
        out = np.empty((self.n_streams, self.pair_watch_plan()[2]), PAIR_WATCH_DTYPE)
        _check(L.lib().ss_meter_bank_pair_watch(self._h, out.ctypes.data_as(C.POINTER(L.PairWatch)), out.size))
        return out

    def pair_watch_entries(self, stream):
        """(first_entry, entries [n, n_pairs] of batch.PAIR_ENTRY_DTYPE): the ring of one stream, its newest min(window, E) complete
        entries in ascending order."""
        _, w, pairs = self.pair_watch_plan()
        out = np.zeros((w, pairs), PAIR_ENTRY_DTYPE)
        first, n = C.c_uint64(), C.c_uint32()
        _check(L.lib().ss_meter_bank_pair_watch_entries(self._h, int(stream), out.ctypes.data_as(C.POINTER(L.PairEntry)), w,
                                                        C.byref(first), C.byref(n)))
        return first.value, out[:n.value].copy()
