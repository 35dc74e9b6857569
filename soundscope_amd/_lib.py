"""ctypes loader for the C-ABI library (include/soundscope_hip.h).

The library is built in-tree by soundscope_amd/csrc/Makefile (hipcc, gfx950).
There is no fallback of any kind: a missing library raises ImportError at load,
and a missing GPU makes every compute entry point return SS_ERR_DEVICE, which
the wrappers turn into DeviceError.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# SOUNDSCOPE_HIP_LIB: load another build of the same library (A/B runs of kernel variants, tools/ab_libs.sh)
LIB_PATH = os.environ.get("SOUNDSCOPE_HIP_LIB") or os.path.join(_HERE, "lib", "libsoundscope_hip.so")
CSRC = os.path.join(_HERE, "csrc")

# every symbol include/soundscope_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "ss_status_string", "ss_abi_version", "ss_device_count", "ss_set_device", "ss_last_device_error",
    "ss_analyzer_create", "ss_analyzer_destroy", "ss_analyzer_configure", "ss_get_fft", "ss_get_fft_error_values", "ss_get_waveform",
    "ss_add_samples", "ss_reset", "ss_get_shortterm_lufs", "ss_get_integrated_lufs", "ss_get_loudness_range",
    "ss_get_true_peak", "ss_sample_rate", "ss_calculate_integrated_lufs", "ss_mid_side",
    "ss_get_momentary_lufs", "ss_get_true_peak_channel", "ss_get_sample_peak_channel",
    "ss_analyzer_set_true_peak_factor", "ss_analyzer_set_true_peak_arith",
    "ss_batch_create", "ss_batch_destroy", "ss_batch_layout_get", "ss_batch_upload", "ss_batch_download_input",
    "ss_batch_input_device_ptr", "ss_batch_synthesize", "ss_batch_run", "ss_batch_sync", "ss_batch_results",
    "ss_batch_download_fft", "ss_batch_bin_tables", "ss_batch_download_waveform", "ss_batch_download_subblocks",
    "ss_batch_histograms", "ss_batch_histograms_device", "ss_corpus_integrated_lufs", "ss_corpus_loudness_range",
    "ss_batch_timing_enable", "ss_batch_timing_read", "ss_kernel_name",
    "ss_wav_parse", "ss_pcm_sample_bytes", "ss_pcm_decode", "ss_batch_upload_pcm",
    "ss_session_open_file", "ss_session_open_capture", "ss_session_close", "ss_session_analyzer",
    "ss_session_waveform", "ss_session_gain_db", "ss_session_duration_ms", "ss_session_tick_file",
    "ss_session_tick_capture", "ss_session_capture_push", "ss_session_tick_capture_resident", "ss_session_restart",
    "ss_session_lufs_history",
    "ss_batch_render_spectrum", "ss_batch_download_spectrum_columns", "ss_batch_render_waveform",
    "ss_batch_download_waveform_columns", "ss_waveform_view", "ss_batch_kernel_name",
    "ss_host_register", "ss_host_unregister", "ss_batch_upload_pcm_async",
    "ss_batch_set_lengths", "ss_batch_stream_shape", "ss_batch_upload_samples",
    "ss_device_synchronize", "ss_batch_peaks", "ss_batch_geometry_get", "ss_batch_set_overlap",
    "ss_comm_init", "ss_comm_init_on_device", "ss_comm_init_from_env", "ss_comm_destroy", "ss_comm_rank", "ss_comm_size",
    "ss_comm_transport_name", "ss_comm_library_version", "ss_comm_barrier", "ss_comm_allreduce_u64_sum", "ss_comm_allreduce_f64_max",
    "ss_batch_allreduce_histograms", "ss_batch_traffic_floor",
    "ss_batch_corpus_gate_enqueue", "ss_batch_corpus_gate_read", "ss_batch_checksums", "ss_inspect_filter_state", "ss_batch_set_true_peak_arith", "ss_batch_get_true_peak_arith", "ss_batch_set_time_domain_mode", "ss_batch_set_columns_gain",
    "ss_release_caches", "ss_batch_geometry_get_sized",
    "ss_inspect_kweight", "ss_inspect_true_peak", "ss_inspect_true_peak_fold", "ss_inspect_hann", "ss_inspect_bins", "ss_inspect_histogram",
    "ss_batch_download_loudness_series", "ss_batch_loudness_extremes",
    "ss_meter_bank_create", "ss_meter_bank_destroy", "ss_meter_bank_add", "ss_meter_bank_add_device", "ss_meter_bank_add_pcm",
    "ss_meter_bank_add_ragged", "ss_meter_bank_add_ragged_pcm", "ss_meter_bank_add_ragged_device",
    "ss_meter_bank_reset", "ss_meter_bank_read", "ss_meter_bank_peaks", "ss_meter_bank_histograms",
    "ss_meter_bank_spectrum_enable", "ss_meter_bank_spectrum_layout", "ss_meter_bank_spectrum", "ss_meter_bank_spectrum_columns",
    "ss_meter_bank_spectrum_track_enable", "ss_meter_bank_spectrum_track", "ss_meter_bank_spectrum_track_reset",
    "ss_meter_bank_spectrum_tracked", "ss_meter_bank_spectrum_tracked_columns",
    "ss_meter_bank_signal_watch_enable", "ss_meter_bank_signal_watch_plan", "ss_meter_bank_signal_watch_reset",
    "ss_meter_bank_signal_watch",
    "ss_meter_bank_pair_watch_enable", "ss_meter_bank_pair_watch_plan", "ss_meter_bank_pair_watch_reset",
    "ss_meter_bank_pair_watch", "ss_meter_bank_pair_watch_entries",
    "ss_batch_spectrum_stats", "ss_batch_download_spectrum_stats", "ss_batch_corpus_spectrum", "ss_batch_spectrum_stats_plan",
    "ss_batch_loudness_regions", "ss_batch_download_region_results", "ss_batch_download_group_results", "ss_batch_group_histograms",
    "ss_batch_peak_series", "ss_batch_peak_series_plan", "ss_batch_download_peak_series", "ss_batch_peak_regions",
    "ss_batch_download_region_peaks", "ss_batch_download_group_peaks", "ss_batch_download_region_channel_peaks",
    "ss_batch_spectrogram", "ss_batch_spectrogram_plan", "ss_batch_download_spectrogram", "ss_spectrogram_column_windows",
    "ss_batch_signal_scan", "ss_batch_signal_scan_plan", "ss_batch_download_stream_scans", "ss_batch_download_channel_scans",
    "ss_batch_download_signal_events",
    "ss_batch_spectrum_regions", "ss_batch_download_region_spectra", "ss_batch_download_group_spectra",
    "ss_batch_spectrum_regions_plan", "ss_region_windows",
    "ss_batch_pair_series", "ss_batch_pair_series_plan", "ss_batch_download_pair_series", "ss_batch_pair_regions",
    "ss_batch_download_region_pairs", "ss_batch_download_group_pairs",
    "ss_normalisation_gain", "ss_gain_envelope", "ss_batch_apply_gain", "ss_batch_apply_gain_plan", "ss_batch_download_gain_stats",
    "ss_batch_download_pcm",
    "ss_limit_curve", "ss_batch_limit", "ss_batch_limit_plan", "ss_batch_download_limit_stats",
    "ss_resample_plan_make", "ss_resample_taps", "ss_resample_length", "ss_resample_host", "ss_batch_resample", "ss_batch_resample_plan",
    "ss_td_streaming_plan", "ss_session_last_tick_forms",
]

SS_ABI_VERSION = 2          # include/soundscope_hip.h; checked at load
SS_OK = 0
SS_ERR_NOMEM, SS_ERR_INVALID_MODE, SS_ERR_INVALID_CHANNEL = 1, 2, 3
SS_ERR_TOO_FEW_SAMPLES, SS_ERR_NAN, SS_ERR_INFINITY, SS_ERR_NOT_POW2, SS_ERR_FREQ_LIMIT, SS_ERR_SCALING = 10, 11, 12, 13, 14, 15
SS_ERR_CAPACITY, SS_ERR_UNSUPPORTED, SS_ERR_INVALID_ARG, SS_ERR_DEVICE = 20, 21, 22, 30

SS_BATCH_FFT, SS_BATCH_LUFS, SS_BATCH_TRUE_PEAK, SS_BATCH_WAVEFORM, SS_BATCH_ALL = 1, 2, 4, 8, 15
SS_BATCH_FFT_COLUMNS = 16
SS_BATCH_LOUDNESS_SERIES = 32
SS_REGION_NO_GROUP = 0xFFFFFFFF
SS_SIGNAL_SILENCE, SS_SIGNAL_CLIP = 0, 1
SS_PCM_U8, SS_PCM_S16, SS_PCM_S24, SS_PCM_S32, SS_PCM_F32, SS_PCM_F64 = 1, 2, 3, 4, 5, 6
SS_GAIN_LIMITED_PEAK, SS_GAIN_LIMITED_MAX, SS_GAIN_LIMITED_MIN, SS_GAIN_UNMEASURED = 1, 2, 4, 8
SS_DITHER_NONE, SS_DITHER_TPDF = 0, 1
SS_LIMIT_SAMPLE_PEAK, SS_LIMIT_TRUE_PEAK = 0, 1
SS_LIMIT_LOOKAHEAD_MAX, SS_LIMIT_HOLD_MAX = 2048, 8192
SS_RESAMPLE_TAPS_MAX = 24576
SS_GAIN_FIXED, SS_GAIN_REFERENCE = 0, 1
SS_COMM_RCCL, SS_COMM_HOST_TCP = 0, 1
SS_TP_ARITH_F16X3, SS_TP_ARITH_F32 = 0, 1
SS_TD_AUTO, SS_TD_RUN_IN, SS_TD_WHOLE_STREAMS = 0, 1, 2
SS_TD_FORM_ONE_WAVE, SS_TD_FORM_SHARED = 0, 1
SS_KERNEL_FFT, SS_KERNEL_TIME_DOMAIN, SS_KERNEL_FINALIZE, SS_KERNEL_WAVEFORM, SS_KERNEL_COUNT = 0, 1, 2, 3, 4


class BatchConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("channels", C.c_uint32), ("n_streams", C.c_uint32),
                ("fft_n", C.c_uint32), ("hop_frames", C.c_uint32), ("flags", C.c_uint32),
                ("true_peak_factor", C.c_int32), ("spectrum_columns", C.c_uint32),
                ("frames_per_stream", C.c_uint64), ("waveform_window", C.c_double)]


class StreamResult(C.Structure):
    _fields_ = [("integrated_lufs", C.c_double), ("loudness_range", C.c_double),
                ("true_peak", C.c_double * 2), ("sample_peak", C.c_double * 2),
                ("n_gating_blocks", C.c_uint32), ("n_st_blocks", C.c_uint32)]


class WavInfo(C.Structure):
    _fields_ = [("format", C.c_uint32), ("channels", C.c_uint32), ("sample_rate", C.c_uint32),
                ("bits_per_sample", C.c_uint32), ("data_offset", C.c_uint64), ("data_bytes", C.c_uint64),
                ("frames", C.c_uint64)]


class TickResult(C.Structure):
    _fields_ = [("playhead", C.c_uint64), ("fft_ran", C.c_int32), ("mid_status", C.c_int32),
                ("side_status", C.c_int32), ("n_mid", C.c_uint32), ("n_side", C.c_uint32),
                ("lufs_ran", C.c_int32), ("fed", C.c_int32), ("add_status", C.c_int32),
                ("shortterm_status", C.c_int32), ("reserved", C.c_uint32), ("shortterm", C.c_double)]


class StreamShape(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("n_windows", C.c_uint32), ("n_subblocks", C.c_uint32),
                ("n_wave_points", C.c_uint32), ("reserved", C.c_uint32)]


class BatchGeometry(C.Structure):
    _fields_ = [("fft_windows_per_block", C.c_uint32), ("fft_blocks", C.c_uint32), ("td_segments", C.c_uint32),
                ("td_segment_subblocks", C.c_uint32), ("td_warm_subblocks", C.c_uint32),
                ("td_true_peak_factor", C.c_uint32), ("waveform_fused", C.c_uint32), ("overlap", C.c_uint32),
                ("td_split", C.c_uint32), ("td_fixup_subblocks", C.c_uint32)]


class LoudnessExtremes(C.Structure):
    _fields_ = [("max_momentary", C.c_double), ("max_shortterm", C.c_double),
                ("max_momentary_at", C.c_uint32), ("max_shortterm_at", C.c_uint32)]


class LoudnessRegion(C.Structure):
    _fields_ = [("stream", C.c_uint32), ("first_subblock", C.c_uint32), ("n_subblocks", C.c_uint32), ("group", C.c_uint32)]


class RegionResult(C.Structure):
    _fields_ = [("integrated_lufs", C.c_double), ("loudness_range", C.c_double),
                ("max_momentary", C.c_double), ("max_shortterm", C.c_double),
                ("max_momentary_at", C.c_uint32), ("max_shortterm_at", C.c_uint32),
                ("n_gating_blocks", C.c_uint32), ("n_st_blocks", C.c_uint32)]


class GroupResult(C.Structure):
    _fields_ = [("integrated_lufs", C.c_double), ("loudness_range", C.c_double),
                ("n_gating_blocks", C.c_uint64), ("n_st_blocks", C.c_uint64)]


class PeakEntry(C.Structure):
    _fields_ = [("true_peak", C.c_float), ("sample_peak", C.c_float), ("true_peak_frame", C.c_uint32), ("sample_peak_frame", C.c_uint32)]


class RegionPeaks(C.Structure):
    _fields_ = [("true_peak", C.c_double), ("sample_peak", C.c_double),
                ("true_peak_frame", C.c_uint64), ("sample_peak_frame", C.c_uint64),
                ("true_peak_channel", C.c_uint32), ("sample_peak_channel", C.c_uint32),
                ("n_over", C.c_uint32), ("first_over", C.c_uint32)]


class GroupPeaks(C.Structure):
    _fields_ = [("true_peak", C.c_double), ("sample_peak", C.c_double),
                ("true_peak_region", C.c_uint32), ("sample_peak_region", C.c_uint32), ("n_over", C.c_uint64)]


class SignalScanConfig(C.Structure):
    _fields_ = [("silence_threshold", C.c_float), ("clip_level", C.c_float), ("silence_min_frames", C.c_uint32),
                ("clip_min_samples", C.c_uint32), ("max_events", C.c_uint32), ("reserved", C.c_uint32)]


class StreamScan(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("silent_frames", "leading_silence", "trailing_silence", "longest_silence",
                                          "longest_silence_at", "silence_runs", "clip_runs")]


class ChannelScan(C.Structure):
    _fields_ = [("sum", C.c_double), ("sum_sq", C.c_double)] + [(n, C.c_uint64) for n in (
        "nonfinite", "first_nonfinite", "clipped_samples", "longest_clip", "longest_clip_at", "clip_runs")]


class StreamWatch(C.Structure):            # ss_stream_watch: the batch record, then the live field
    _fields_ = StreamScan._fields_ + [("frames", C.c_uint64)]


class ChannelWatch(C.Structure):           # ss_channel_watch
    _fields_ = ChannelScan._fields_ + [("trailing_clip", C.c_uint64), ("last_clip_frame", C.c_uint64)]


class SignalEvent(C.Structure):
    _fields_ = [("first_frame", C.c_uint64), ("frames", C.c_uint64), ("channel", C.c_uint32), ("reserved", C.c_uint32)]


class ChannelPair(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32)]


class PairEntry(C.Structure):
    _fields_ = [("s_aa", C.c_double), ("s_bb", C.c_double), ("s_ab", C.c_double), ("frames", C.c_uint32), ("skipped", C.c_uint32)]


class PairRegionConfig(C.Structure):
    _fields_ = [("threshold", C.c_double), ("power_floor", C.c_double), ("min_run", C.c_uint32), ("reserved", C.c_uint32)]


class RegionPair(C.Structure):
    _fields_ = [("s_aa", C.c_double), ("s_bb", C.c_double), ("s_ab", C.c_double), ("frames", C.c_uint64), ("skipped", C.c_uint64)] + [
        (n, C.c_uint32) for n in ("n_active", "n_below", "first_below", "longest_below", "longest_below_at", "below_runs")]


class GroupPair(C.Structure):
    _fields_ = [("s_aa", C.c_double), ("s_bb", C.c_double), ("s_ab", C.c_double)] + [
        (n, C.c_uint64) for n in ("frames", "skipped", "n_active", "n_below", "below_runs")]


class NormaliseTarget(C.Structure):        # ss_normalise_target
    _fields_ = [("target_lufs", C.c_double), ("max_true_peak_dbtp", C.c_double), ("max_gain_db", C.c_double), ("min_gain_db", C.c_double)]


class GainPoint(C.Structure):              # ss_gain_point
    _fields_ = [("frame", C.c_uint64), ("stream", C.c_uint32), ("gain", C.c_float)]


class GainConfig(C.Structure):             # ss_gain_config
    _fields_ = [("channel_mask", C.c_uint64), ("clip_level", C.c_float), ("reserved", C.c_uint32)]


class GainChannel(C.Structure):            # ss_gain_channel
    _fields_ = [("sample_peak", C.c_float), ("touched", C.c_uint32), ("n_over", C.c_uint64), ("first_over", C.c_uint64),
                ("n_nonfinite", C.c_uint64)]


class PcmDither(C.Structure):              # ss_pcm_dither
    _fields_ = [("seed", C.c_uint64), ("kind", C.c_uint32), ("reserved", C.c_uint32)]


class LimitItem(C.Structure):              # ss_limit_item
    _fields_ = [("stream", C.c_uint32), ("gain", C.c_float)]


class LimitConfig(C.Structure):            # ss_limit_config
    _fields_ = [("channel_mask", C.c_uint64), ("ceiling", C.c_float), ("clip_level", C.c_float), ("lookahead", C.c_uint32),
                ("hold", C.c_uint32), ("detector", C.c_uint32), ("reserved", C.c_uint32), ("scratch_bytes", C.c_uint64)]


class LimitStream(C.Structure):            # ss_limit_stream
    _fields_ = [("n_limited", C.c_uint64), ("first_limited", C.c_uint64), ("min_sum", C.c_uint64), ("touched", C.c_uint32),
                ("reserved", C.c_uint32)]


class ResamplePlan(C.Structure):           # ss_resample_plan
    _fields_ = [("in_rate", C.c_uint32), ("out_rate", C.c_uint32), ("up", C.c_uint32), ("down", C.c_uint32), ("taps", C.c_uint32),
                ("reserved", C.c_uint32), ("attenuation_db", C.c_double), ("passband", C.c_double), ("beta", C.c_double),
                ("cutoff", C.c_double)]


class PairSums(C.Structure):               # ss_pair_sums
    _fields_ = [("s_aa", C.c_double), ("s_bb", C.c_double), ("s_ab", C.c_double), ("frames", C.c_uint64), ("skipped", C.c_uint64)]


class PairWatchConfig(C.Structure):        # ss_pair_watch_config
    _fields_ = [("threshold", C.c_double), ("power_floor", C.c_double), ("min_run", C.c_uint32), ("window_entries", C.c_uint32)]


class PairWatch(C.Structure):              # ss_pair_watch
    _fields_ = [("window", PairSums), ("total", PairSums)] + [(n, C.c_uint64) for n in (
        "entries", "n_active", "n_below", "first_below", "longest_below", "longest_below_at", "below_runs", "trailing_below")] + [
        ("open_frames", C.c_uint32), ("window_count", C.c_uint32), ("reserved", C.c_uint64)]


class SpectrogramView(C.Structure):
    _fields_ = [("t_cols", C.c_uint32), ("f_cols", C.c_uint32), ("w_min", C.c_uint32), ("w_max", C.c_uint32),
                ("gain_mode", C.c_int32), ("gain_db", C.c_float)]


class MeterReading(C.Structure):
    _fields_ = [("momentary", C.c_double), ("shortterm", C.c_double), ("integrated", C.c_double),
                ("loudness_range", C.c_double), ("true_peak", C.c_double * 2), ("sample_peak", C.c_double * 2),
                ("frames", C.c_uint64)]


class SpectrumBallistics(C.Structure):
    _fields_ = [("average_tau_s", C.c_double), ("hold_s", C.c_double), ("decay_db_per_s", C.c_double)]


class StreamingPlan(C.Structure):           # ss_streaming_plan
    _fields_ = [(n, C.c_uint32) for n in ("form", "waves", "tile_frames", "chunk_frames", "true_peak_factor", "subblock_frames")] + [
        ("piece_frames", C.c_uint64)]


assert C.sizeof(StreamingPlan) == 32 and StreamingPlan.piece_frames.offset == 24


class BatchLayout(C.Structure):
    _fields_ = [("n_windows", C.c_uint32), ("fft_channels", C.c_uint32), ("n_bins", C.c_uint32),
                ("first_bin", C.c_uint32), ("n_wave_points", C.c_uint32), ("n_subblocks", C.c_uint32),
                ("fft_bin_stride", C.c_uint32), ("reserved", C.c_uint32),
                ("input_bytes", C.c_uint64), ("fft_bytes", C.c_uint64)]


def build(force: bool = False) -> str:
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.run(["make", "-C", CSRC], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def _bind(lib):
    vp, f32p, f64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double)
    szp, u64p = C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)
    sig = {
        "ss_status_string": (C.c_char_p, [C.c_int]),
        "ss_abi_version": (C.c_int, []),
        "ss_device_count": (C.c_int, []),
        "ss_set_device": (C.c_int, [C.c_int]),
        "ss_last_device_error": (C.c_char_p, []),
        "ss_analyzer_create": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "ss_analyzer_destroy": (None, [vp]),
        "ss_analyzer_configure": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
        "ss_get_fft": (C.c_int, [vp, f32p, C.c_size_t, f64p, C.c_size_t, szp]),
        "ss_get_fft_error_values": (C.c_int, [vp, f32p, f32p]),
        "ss_get_waveform": (C.c_int, [f32p, C.c_size_t, C.c_double, f64p, C.c_size_t, szp]),
        "ss_add_samples": (C.c_int, [vp, f32p, C.c_size_t]),
        "ss_reset": (None, [vp]),
        "ss_get_shortterm_lufs": (C.c_int, [vp, f64p]),
        "ss_get_integrated_lufs": (C.c_int, [vp, f64p]),
        "ss_get_loudness_range": (C.c_int, [vp, f64p]),
        "ss_get_momentary_lufs": (C.c_int, [vp, f64p]),
        "ss_get_true_peak": (C.c_int, [vp, f64p, f64p]),
        "ss_get_true_peak_channel": (C.c_int, [vp, C.c_uint32, f64p]),
        "ss_get_sample_peak_channel": (C.c_int, [vp, C.c_uint32, f64p]),
        "ss_analyzer_set_true_peak_factor": (C.c_int, [vp, C.c_int]),
        "ss_sample_rate": (C.c_uint32, [vp]),
        "ss_calculate_integrated_lufs": (C.c_int, [vp, C.c_uint32, f32p, C.c_size_t, f64p]),
        "ss_mid_side": (C.c_int, [f32p, C.c_size_t, f32p, f32p, szp]),
        "ss_batch_create": (C.c_int, [C.POINTER(BatchConfig), C.POINTER(vp)]),
        "ss_batch_destroy": (None, [vp]),
        "ss_batch_layout_get": (C.c_int, [vp, C.POINTER(BatchLayout)]),
        "ss_batch_upload": (C.c_int, [vp, C.c_uint32, C.c_uint32, f32p]),
        "ss_batch_download_input": (C.c_int, [vp, C.c_uint32, f32p, C.c_size_t]),
        "ss_batch_input_device_ptr": (vp, [vp]),
        "ss_batch_synthesize": (C.c_int, [vp, C.c_uint64, C.c_uint32]),
        "ss_batch_run": (C.c_int, [vp]),
        "ss_batch_sync": (C.c_int, [vp]),
        "ss_batch_results": (C.c_int, [vp, C.POINTER(StreamResult), C.c_uint32]),
        "ss_batch_download_fft": (C.c_int, [vp, C.c_uint32, f32p, C.c_size_t]),
        "ss_batch_bin_tables": (C.c_int, [vp, f64p, f64p, f64p]),
        "ss_batch_download_waveform": (C.c_int, [vp, C.c_uint32, f32p, C.c_size_t]),
        "ss_batch_download_subblocks": (C.c_int, [vp, C.c_uint32, f64p, C.c_size_t]),
        "ss_batch_histograms": (C.c_int, [vp, u64p]),
        "ss_batch_histograms_device": (C.c_int, [vp, vp]),
        "ss_corpus_integrated_lufs": (C.c_double, [u64p]),
        "ss_corpus_loudness_range": (C.c_double, [u64p]),
        "ss_batch_timing_enable": (C.c_int, [vp, C.c_int]),
        "ss_batch_timing_read": (C.c_int, [vp, C.c_int, f64p, u64p]),
        "ss_kernel_name": (C.c_char_p, [C.c_int]),
        "ss_wav_parse": (C.c_int, [vp, C.c_size_t, C.POINTER(WavInfo)]),
        "ss_pcm_sample_bytes": (C.c_size_t, [C.c_int]),
        "ss_pcm_decode": (C.c_int, [vp, C.c_size_t, C.c_int, f32p]),
        "ss_batch_upload_pcm": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, C.c_int]),
        "ss_session_open_file": (C.c_int, [f32p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "ss_session_open_capture": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "ss_session_close": (None, [vp]),
        "ss_session_analyzer": (vp, [vp]),
        "ss_session_waveform": (C.c_int, [vp, f64p, C.c_size_t, szp]),
        "ss_session_gain_db": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "ss_session_duration_ms": (C.c_int, [vp, u64p]),
        "ss_session_tick_file": (C.c_int, [vp, C.c_size_t, f64p, f64p, C.c_size_t, C.POINTER(TickResult)]),
        "ss_session_tick_capture": (C.c_int, [vp, f32p, C.c_size_t, f64p, f64p, C.c_size_t, f64p, C.c_size_t,
                                              szp, C.POINTER(TickResult)]),
        "ss_session_capture_push": (C.c_int, [vp, f32p, C.c_size_t]),
        "ss_session_tick_capture_resident": (C.c_int, [vp, f64p, f64p, C.c_size_t, f64p, C.c_size_t, szp, C.POINTER(TickResult)]),
        "ss_session_restart": (C.c_int, [vp]),
        "ss_session_lufs_history": (C.c_int, [vp, f64p]),
        "ss_batch_render_spectrum": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_float]),
        "ss_batch_download_spectrum_columns": (C.c_int, [vp, C.c_uint32, f32p, C.c_size_t]),
        "ss_batch_render_waveform": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_uint32]),
        "ss_batch_download_waveform_columns": (C.c_int, [vp, C.c_uint32, f32p, C.c_size_t]),
        "ss_waveform_view": (None, [C.c_double, C.c_double, C.c_size_t, f64p, f64p]),
        "ss_batch_kernel_name": (C.c_char_p, [vp, C.c_int]),
        "ss_host_register": (C.c_int, [vp, C.c_size_t]),
        "ss_host_unregister": (C.c_int, [vp]),
        "ss_batch_upload_pcm_async": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, C.c_int]),
        "ss_batch_set_lengths": (C.c_int, [vp, u64p, C.c_uint32]),
        "ss_batch_upload_samples": (C.c_int, [vp, C.c_uint32, vp, C.c_size_t, C.c_int]),
        "ss_batch_stream_shape": (C.c_int, [vp, C.c_uint32, C.POINTER(StreamShape)]),
        "ss_device_synchronize": (C.c_int, []),
        "ss_batch_peaks": (C.c_int, [vp, C.c_uint32, f64p, f64p, C.c_uint32]),
        "ss_batch_geometry_get": (C.c_int, [vp, C.POINTER(BatchGeometry)]),
        "ss_batch_set_overlap": (C.c_int, [vp, C.c_int]),
        "ss_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]),
        "ss_comm_init_on_device": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]),
        "ss_comm_init_from_env": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "ss_comm_destroy": (None, [vp]),
        "ss_comm_rank": (C.c_int, [vp]),
        "ss_comm_size": (C.c_int, [vp]),
        "ss_comm_transport_name": (C.c_char_p, [vp]),
        "ss_comm_library_version": (C.c_int, [vp]),
        "ss_comm_barrier": (C.c_int, [vp]),
        "ss_comm_allreduce_u64_sum": (C.c_int, [vp, u64p, C.c_size_t]),
        "ss_comm_allreduce_f64_max": (C.c_int, [vp, f64p, C.c_size_t]),
        "ss_batch_allreduce_histograms": (C.c_int, [vp, vp, u64p]),
        "ss_batch_traffic_floor": (C.c_int, [vp, C.c_uint32, f64p]),
        "ss_batch_corpus_gate_enqueue": (C.c_int, [vp, vp]),
        "ss_batch_corpus_gate_read": (C.c_int, [vp, f64p, f64p]),
        "ss_batch_checksums": (C.c_int, [vp, u64p, C.c_uint32]),
        "ss_inspect_filter_state": (C.c_int, [vp, C.c_uint32, f64p]),
        "ss_batch_set_true_peak_arith": (C.c_int, [vp, C.c_int]),
        "ss_analyzer_set_true_peak_arith": (C.c_int, [vp, C.c_int]),
        "ss_batch_get_true_peak_arith": (C.c_int, [vp]),
        "ss_batch_set_time_domain_mode": (C.c_int, [vp, C.c_int]),
        "ss_batch_set_columns_gain": (C.c_int, [vp, C.c_int, C.c_float]),
        "ss_release_caches": (C.c_int, []),
        "ss_batch_geometry_get_sized": (C.c_int, [vp, vp, C.c_size_t]),
        "ss_inspect_kweight": (C.c_int, [C.c_uint32, f64p, f64p]),
        "ss_inspect_true_peak": (C.c_int, [C.c_int, f32p, C.c_uint32, C.POINTER(C.c_uint32)]),
        "ss_inspect_true_peak_fold": (C.c_int, [f32p]),
        "ss_inspect_hann": (C.c_int, [C.c_uint32, f32p]),
        "ss_inspect_bins": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_inspect_histogram": (C.c_int, [f64p, f64p]),
        "ss_batch_download_loudness_series": (C.c_int, [vp, C.c_uint32, f64p, f64p, C.c_size_t]),
        "ss_batch_loudness_extremes": (C.c_int, [vp, C.POINTER(LoudnessExtremes), C.c_uint32]),
        "ss_meter_bank_create": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(vp)]),
        "ss_meter_bank_destroy": (None, [vp]),
        "ss_meter_bank_add": (C.c_int, [vp, f32p, C.c_uint64]),
        "ss_meter_bank_add_device": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64]),
        "ss_meter_bank_add_pcm": (C.c_int, [vp, vp, C.c_uint64, C.c_int]),
        "ss_meter_bank_add_ragged": (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
        "ss_meter_bank_add_ragged_pcm": (C.c_int, [vp, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_int]),
        "ss_meter_bank_add_ragged_device": (C.c_int, [vp, vp, C.POINTER(C.c_uint64), C.c_uint64]),
        "ss_meter_bank_reset": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_meter_bank_read": (C.c_int, [vp, vp, C.c_uint32]),
        "ss_meter_bank_peaks": (C.c_int, [vp, C.c_uint32, f64p, f64p, C.c_uint32]),
        "ss_meter_bank_histograms": (C.c_int, [vp, C.c_uint32, u64p]),
        "ss_meter_bank_spectrum_enable": (C.c_int, [vp, C.c_int]),
        "ss_meter_bank_spectrum_layout": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), f64p, f64p, C.c_uint32]),
        "ss_meter_bank_spectrum": (C.c_int, [vp, f32p, C.c_size_t, C.POINTER(C.c_int32), C.c_uint32]),
        "ss_meter_bank_spectrum_columns": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_float, f32p, C.c_size_t, C.POINTER(C.c_int32), C.c_uint32]),
        "ss_meter_bank_spectrum_track_enable": (C.c_int, [vp, C.POINTER(SpectrumBallistics)]),
        "ss_meter_bank_spectrum_track": (C.c_int, [vp]),
        "ss_meter_bank_spectrum_track_reset": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_meter_bank_spectrum_tracked": (C.c_int, [vp, f32p, f32p, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_meter_bank_spectrum_tracked_columns": (C.c_int, [vp, C.c_uint32, C.c_int, C.c_float, f32p, f32p, C.c_size_t,
                                                             C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_batch_loudness_regions": (C.c_int, [vp, C.POINTER(LoudnessRegion), C.c_uint32, C.c_uint32]),
        "ss_batch_download_region_results": (C.c_int, [vp, C.POINTER(RegionResult), C.c_uint32]),
        "ss_batch_download_group_results": (C.c_int, [vp, C.POINTER(GroupResult), C.c_uint32]),
        "ss_batch_group_histograms": (C.c_int, [vp, C.c_uint32, u64p]),
        "ss_batch_peak_series": (C.c_int, [vp]),
        "ss_batch_peak_series_plan": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_batch_download_peak_series": (C.c_int, [vp, C.c_uint32, C.POINTER(PeakEntry), C.c_size_t, C.POINTER(C.c_uint32)]),
        "ss_batch_peak_regions": (C.c_int, [vp, C.POINTER(LoudnessRegion), C.c_uint32, C.c_uint32, C.c_double]),
        "ss_batch_download_region_peaks": (C.c_int, [vp, C.POINTER(RegionPeaks), C.c_uint32]),
        "ss_batch_download_group_peaks": (C.c_int, [vp, C.POINTER(GroupPeaks), C.c_uint32]),
        "ss_batch_download_region_channel_peaks": (C.c_int, [vp, f32p, f32p, C.c_size_t]),
        "ss_batch_spectrum_stats": (C.c_int, [vp]),
        "ss_batch_download_spectrum_stats": (C.c_int, [vp, C.c_uint32, f32p, f32p, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_batch_corpus_spectrum": (C.c_int, [vp, f32p, f32p, C.c_size_t, u64p, C.c_uint32]),
        "ss_batch_spectrum_stats_plan": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_batch_spectrogram": (C.c_int, [vp, C.POINTER(SpectrogramView)]),
        "ss_batch_spectrogram_plan": (C.c_int, [vp, C.POINTER(SpectrogramView), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_batch_download_spectrogram": (C.c_int, [vp, C.c_uint32, C.c_uint32, f32p, C.c_size_t]),
        "ss_spectrogram_column_windows": (None, [C.POINTER(SpectrogramView), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_meter_bank_signal_watch_enable": (C.c_int, [vp, C.POINTER(SignalScanConfig)]),
        "ss_meter_bank_signal_watch_plan": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "ss_meter_bank_signal_watch_reset": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_meter_bank_signal_watch": (C.c_int, [vp, C.POINTER(StreamWatch), C.c_uint32, C.POINTER(ChannelWatch), C.c_size_t]),
        "ss_meter_bank_pair_watch_enable": (C.c_int, [vp, C.POINTER(ChannelPair), C.c_uint32, C.POINTER(PairWatchConfig)]),
        "ss_meter_bank_pair_watch_plan": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_meter_bank_pair_watch_reset": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_uint32]),
        "ss_meter_bank_pair_watch": (C.c_int, [vp, C.POINTER(PairWatch), C.c_size_t]),
        "ss_meter_bank_pair_watch_entries": (C.c_int, [vp, C.c_uint32, C.POINTER(PairEntry), C.c_size_t, C.POINTER(C.c_uint64),
                                                       C.POINTER(C.c_uint32)]),
        "ss_batch_signal_scan": (C.c_int, [vp, C.POINTER(SignalScanConfig)]),
        "ss_batch_signal_scan_plan": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_batch_download_stream_scans": (C.c_int, [vp, C.POINTER(StreamScan), C.c_uint32]),
        "ss_batch_download_channel_scans": (C.c_int, [vp, C.POINTER(ChannelScan), C.c_size_t]),
        "ss_batch_download_signal_events": (C.c_int, [vp, C.c_uint32, C.c_int, C.POINTER(SignalEvent), C.c_size_t, C.POINTER(C.c_uint32)]),
        "ss_batch_spectrum_regions": (C.c_int, [vp, C.POINTER(LoudnessRegion), C.c_uint32, C.c_uint32]),
        "ss_batch_download_region_spectra": (C.c_int, [vp, C.c_uint32, C.c_uint32, f32p, f32p, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t]),
        "ss_batch_download_group_spectra": (C.c_int, [vp, C.c_uint32, C.c_uint32, f32p, f32p, C.c_size_t, u64p, C.c_size_t]),
        "ss_batch_spectrum_regions_plan": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_region_windows": (None, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_batch_pair_series": (C.c_int, [vp, C.POINTER(ChannelPair), C.c_uint32]),
        "ss_batch_pair_series_plan": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_batch_download_pair_series": (C.c_int, [vp, C.c_uint32, C.POINTER(PairEntry), C.c_size_t, C.POINTER(C.c_uint32)]),
        "ss_batch_pair_regions": (C.c_int, [vp, C.POINTER(LoudnessRegion), C.c_uint32, C.c_uint32, C.POINTER(PairRegionConfig)]),
        "ss_batch_download_region_pairs": (C.c_int, [vp, C.POINTER(RegionPair), C.c_size_t]),
        "ss_batch_download_group_pairs": (C.c_int, [vp, C.POINTER(GroupPair), C.c_size_t]),
        "ss_normalisation_gain": (C.c_int, [C.POINTER(NormaliseTarget), C.c_double, C.c_double, f64p, f32p, C.POINTER(C.c_uint32)]),
        "ss_gain_envelope": (C.c_double, [C.POINTER(GainPoint), C.c_uint32, C.c_uint64]),
        "ss_batch_apply_gain": (C.c_int, [vp, C.POINTER(GainPoint), C.c_uint32, C.POINTER(GainConfig)]),
        "ss_batch_apply_gain_plan": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
        "ss_batch_download_gain_stats": (C.c_int, [vp, C.POINTER(GainChannel), C.c_size_t]),
        "ss_batch_download_pcm": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.c_int, C.POINTER(PcmDither)]),
        "ss_limit_curve": (C.c_int, [f32p, C.c_uint64, C.c_float, C.POINTER(LimitConfig), C.c_uint32, C.POINTER(C.c_uint32), u64p, f64p]),
        "ss_batch_limit": (C.c_int, [vp, C.POINTER(LimitItem), C.c_uint32, C.POINTER(LimitConfig)]),
        "ss_batch_limit_plan": (C.c_int, [vp, C.POINTER(LimitConfig), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64p]),
        "ss_batch_download_limit_stats": (C.c_int, [vp, C.POINTER(LimitStream), C.c_size_t, C.POINTER(GainChannel), C.c_size_t]),
        "ss_resample_plan_make": (C.c_int, [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.POINTER(ResamplePlan)]),
        "ss_resample_taps": (C.c_int, [C.POINTER(ResamplePlan), f32p, C.c_size_t]),
        "ss_resample_length": (C.c_uint64, [C.POINTER(ResamplePlan), C.c_uint64]),
        "ss_resample_host": (C.c_int, [C.POINTER(ResamplePlan), f32p, f32p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, f32p]),
        "ss_batch_resample": (C.c_int, [vp, vp, C.POINTER(ResamplePlan)]),
        "ss_batch_resample_plan": (C.c_int, [vp, C.POINTER(ResamplePlan), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "ss_td_streaming_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int32, C.c_uint64, C.POINTER(StreamingPlan)]),
        "ss_session_last_tick_forms": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


_LIB = None


def lib():
    """The loaded library.  Raises ImportError if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            try:                      # build on demand (hipcc cross-compiles gfx950 without a GPU)
                build()
            except Exception:
                pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C soundscope_amd/csrc`). "
                "soundscope_amd has no CPU fallback.")
        cand = _bind(C.CDLL(LIB_PATH))
        got = cand.ss_abi_version()
        if got != SS_ABI_VERSION:
            raise ImportError(f"{LIB_PATH} reports ABI version {got}, this binding was written for {SS_ABI_VERSION}: rebuild "
                              "(make -C soundscope_amd/csrc)")
        _LIB = cand
    return _LIB
