/*
 * soundscope_hip.h — C ABI of the MI355X-native soundscope analyzer hot path.
 *
 * This is the drop-in boundary for `pub struct Analyzer`
 * (/root/reference/src/analyzer.rs:29-183).  Every Rust method of that type has
 * exactly one entry point here with the same argument meaning and the same
 * error behaviour; a Rust `analyzer.rs` that keeps the reference's signatures
 * and forwards to these symbols is shown in INTEGRATION.md.  The arithmetic
 * underneath runs in hand-written HIP kernels for gfx950 (soundscope_amd/csrc).
 *
 * Conventions
 *   - plain C types only; host pointers unless a name says `_device`.
 *   - every fallible call returns an `ss_status`; SS_OK == 0.  Nothing aborts.
 *   - `(f64,f64)` vectors of the reference are written as interleaved doubles
 *     `out_xy[2*i] = x, out_xy[2*i+1] = y` into caller-allocated storage.
 *   - a handle is used by one thread at a time (the reference only ever calls
 *     from the single TUI thread, src/main.rs:67-77); different handles are
 *     independent (two coexist in the reference, src/tui.rs:459-460).
 *   - there is NO CPU fallback: without a HIP device every compute entry point
 *     returns SS_ERR_DEVICE.
 */
#ifndef SOUNDSCOPE_HIP_H
#define SOUNDSCOPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: ss_add_samples returns behind its launch (a device fault surfaces at the next getter), ss_get_fft_error_values,
 *    ss_batch_get_true_peak_arith; the batch true peak defaults to SS_TP_ARITH_F32 */
#define SS_ABI_VERSION 2

typedef enum ss_status {
    SS_OK = 0,
    /* ebur128::Error (returned by add_samples / getters / create_loudness_meter) */
    SS_ERR_NOMEM = 1,
    SS_ERR_INVALID_MODE = 2,
    SS_ERR_INVALID_CHANNEL = 3,
    /* spectrum_analyzer::SpectrumAnalyzerError (returned by get_fft) */
    SS_ERR_TOO_FEW_SAMPLES = 10,
    SS_ERR_NAN = 11,
    SS_ERR_INFINITY = 12,
    SS_ERR_NOT_POW2 = 13,
    SS_ERR_FREQ_LIMIT = 14,
    SS_ERR_SCALING = 15,
    /* this library */
    SS_ERR_CAPACITY = 20,      /* caller buffer too small */
    SS_ERR_UNSUPPORTED = 21,   /* e.g. FFT length > 32768 (the reference panics there) */
    SS_ERR_INVALID_ARG = 22,
    SS_ERR_DEVICE = 30         /* no HIP device / HIP runtime error */
} ss_status;

const char *ss_status_string(int status);
int ss_abi_version(void);
/* number of visible HIP devices (0 if none); ss_set_device binds the calling
 * process's subsequent handle/batch creations to a device. */
int ss_device_count(void);
/* Tables and scratch are cached PER DEVICE; every handle / batch / session / communicator remembers the device
 * that was current when it was created and makes it current again at each of its entry points, so one process
 * may drive several GPUs from several threads.  (The one-process-per-GPU flow calls ss_set_device once.) */
int ss_set_device(int device);
/* hipDeviceSynchronize on the calling thread's current device (bench fences) */
int ss_device_synchronize(void);
/* last HIP runtime error text seen by this library on this thread ("" if none) */
const char *ss_last_device_error(void);

/* ------------------------------------------------------------------------ *
 *  Inspection of the constant tables the kernels consume, exactly as the library designs them on the host (no device
 *  needed).  They exist so that the PRODUCT's tables can be checked against published numbers (BS.1770-4 coefficient
 *  table, EBU histogram definition, SURVEY's bin counts) independently of the test oracle.  Any pointer may be NULL.
 * ------------------------------------------------------------------------ */
/* K-weighting of ebur128 0.1.10 at `rate` (one 4th-order section: b[0..4], a[0..4], a[0] = 1) */
int ss_inspect_kweight(uint32_t rate, double b5[5], double a5[5]);
/* true-peak interpolator (49-tap Hann-windowed sinc, `factor` 2 or 4): taps[(f - 1) * len + t] = coefficient of x[n - t] in
 * polyphase branch f = 1 .. factor - 1 (branch 0 is the identity tap); *len = taps per branch (12 or 24) */
int ss_inspect_true_peak(int factor, float *taps, uint32_t cap, uint32_t *len);
/* the factor-4 branches folded about their centre, as the VALU true-peak forms hold them: fold18[0..5] = (a[k] + c[k]) / 2,
 * [6..11] = (a[k] - c[k]) / 2, [12..17] = b[k], k = 0 .. 5, for branches a = 1, b = 2, c = 3 of ss_inspect_true_peak */
int ss_inspect_true_peak_fold(float fold18[18]);
/* spectrum-analyzer's periodic Hann window in f32 (n values) */
int ss_inspect_hann(uint32_t n, float *w);
/* retained bins of FrequencyLimit::Range(20, 20000) for (rate, n): FFT index of the first one and their number */
int ss_inspect_bins(uint32_t rate, uint32_t n, uint32_t *first_bin, uint32_t *n_bins);
/* ebur128 histogram: 1000 representative energies and 1001 bin boundaries */
int ss_inspect_histogram(double energies1000[1000], double bounds1001[1001]);

/* ------------------------------------------------------------------------ *
 *  Analyzer mirror (one entry point per Rust method)
 * ------------------------------------------------------------------------ */
typedef struct ss_analyzer ss_analyzer;

/* Analyzer::default() is ss_analyzer_create(2, 44100, &h)   analyzer.rs:34-45 */
int ss_analyzer_create(uint32_t channels, uint32_t rate, ss_analyzer **out);
/* Drop                                                                      */
void ss_analyzer_destroy(ss_analyzer *h);
/* create_loudness_meter(&mut self, channels, rate)           analyzer.rs:49-53
 * sample_rate is updated BEFORE the fallible meter creation (rate sticks on error). */
int ss_analyzer_configure(ss_analyzer *h, uint32_t channels, uint32_t rate);
/* get_fft(&self, samples) -> Vec<(chart_x, dB)>              analyzer.rs:55-105
 * n must be a power of two in [2, 32768]; cap_pairs >= n/2+1 is always enough. */
int ss_get_fft(const ss_analyzer *h, const float *samples, size_t n,
               double *out_xy, size_t cap_pairs, size_t *out_n);
/* payload of the LAST failed ss_get_fft on this handle, so that the binding can rebuild the reference's error value and the
 * text the TUI prints from it (analyzer.rs:60-65 `?` -> tui.rs:1439-1442):
 *   SS_ERR_SCALING    -> SpectrumAnalyzerError::ScalingError(a = original magnitude, b = scaled value) of the first bin
 *   SS_ERR_FREQ_LIMIT -> InvalidFrequencyLimit(ValueAboveNyquist(a = 20000.0)); b = the Nyquist frequency it exceeds */
int ss_get_fft_error_values(const ss_analyzer *h, float *a, float *b);
/* get_waveform(samples, waveform_window) — associated fn, no handle
 *                                                            analyzer.rs:107-137
 * out_xy receives (i,min),(i,max) pairs; cap_pairs >= 2*floor(window*1000). */
int ss_get_waveform(const float *samples, size_t n, double waveform_window,
                    double *out_xy, size_t cap_pairs, size_t *out_n);
/* add_samples(&mut self, samples)                            analyzer.rs:139-141
 * `samples` is copied before the call returns (the caller may reuse it at once).  A call of tick size (n <= 32768) returns
 * behind its launches, without waiting for the device: the status covers the arguments and the meter's state (the reference's
 * own error cases); every getter waits for the samples fed before it, and a device fault surfaces there as SS_ERR_DEVICE. */
int ss_add_samples(ss_analyzer *h, const float *samples, size_t n);
/* reset(&mut self)                                           analyzer.rs:143-145 */
void ss_reset(ss_analyzer *h);
/* get_shortterm_lufs / get_integrated_lufs / get_loudness_range
 *                                                            analyzer.rs:147-157
 * -inf is a valid SS_OK result (no blocks above the gate / silence). */
int ss_get_shortterm_lufs(ss_analyzer *h, double *out);
int ss_get_integrated_lufs(ss_analyzer *h, double *out);
int ss_get_loudness_range(ss_analyzer *h, double *out);
/* get_true_peak(&mut self) -> (left, right), linear amplitude analyzer.rs:159-164
 * SS_ERR_INVALID_CHANNEL when the meter has fewer than 2 channels. */
int ss_get_true_peak(ss_analyzer *h, double *left, double *right);
/* sample_rate(&self)                                         analyzer.rs:166-168 */
uint32_t ss_sample_rate(const ss_analyzer *h);
/* calculate_integrated_lufs(&mut self, channels, samples) -> Option<f64>
 *                                                            analyzer.rs:170-182
 * SS_OK => Some(*out); any other status => None.  Uses the handle's
 * sample_rate only; does not touch the handle's meter. */
int ss_calculate_integrated_lufs(ss_analyzer *h, uint32_t channels,
                                 const float *samples, size_t n, double *out);
/* Process-wide caches.  calculate_integrated_lufs (and ss_session_open_file, which calls it) keeps ONE loudness-only batch per
 * process for inputs of up to 64 MB — sized by its first caller with a quarter of headroom, up to ~80 MB of HBM plus the batch's
 * side buffers — and runs under a lock: concurrent calls from several threads are serialised.  The way an input is cut into
 * time segments follows the input's own length, not the kept batch's size, so a reading does not depend on what the process
 * analysed before.  ss_release_caches frees the kept batch (the next call builds a new one); always SS_OK. */
int ss_release_caches(void);
/* get_mid_and_side_samples(samples)                   audio_player.rs:400-419
 * mid/side need n/2 floats each; *out_frames = n/2. */
int ss_mid_side(const float *interleaved, size_t n, float *mid, float *side,
                size_t *out_frames);

/* extensions that the reference's ebur128 meter has under Mode::all() but the
 * app does not surface */
int ss_get_momentary_lufs(ss_analyzer *h, double *out);
int ss_get_true_peak_channel(ss_analyzer *h, uint32_t channel, double *out);
int ss_get_sample_peak_channel(ss_analyzer *h, uint32_t channel, double *out);
/* true-peak oversampling: 0 = ebur128's rule (<96 kHz: 4x, <192 kHz: 2x, else
 * off); 2 or 4 = forced (BASELINE config 5 asks for 4x at 96 kHz).  Takes
 * effect at the next ss_analyzer_configure or ss_reset (both start a fresh meter). */
int ss_analyzer_set_true_peak_factor(ss_analyzer *h, int factor);
/* arithmetic of the handle's 4x true-peak interpolator: SS_TP_ARITH_F32 (default, ebur128's width) or SS_TP_ARITH_F16X3
 * (see ss_batch_set_true_peak_arith below); takes effect with the next ss_add_samples / session tick. */
int ss_analyzer_set_true_peak_arith(ss_analyzer *h, int arith);
/* inspection (tests): the K-weighting filter's carried DF-II state v1..v4 of one channel, as ebur128's Filter keeps it
 * between add_frames calls — sub-normal values flushed to zero at the end of every internal filter call like the crate
 * does.  Waits for the handle's stream. */
int ss_inspect_filter_state(ss_analyzer *h, uint32_t channel, double v4[4]);
/* inspection (tests): how ONE streaming call of `frames` frames to a meter of this shape is launched — the handle's ss_add_samples,
 * a session tick's loudness call, every stream of a meter bank's add.  Host arithmetic only: no device is touched, and the
 * answer comes from the functions the launch itself calls.  A call longer than piece_frames is cut into calls of piece_frames
 * first; the tiles of every form lie on the stream's absolute grid (multiples of tile_frames inside every 100 ms sub-block,
 * counted from the meter's last reset), not on the call. */
enum { SS_TD_FORM_ONE_WAVE = 0, SS_TD_FORM_SHARED = 1 };
typedef struct ss_streaming_plan {
    uint32_t form;             /* SS_TD_FORM_ONE_WAVE: one wave walks the call; SS_TD_FORM_SHARED: the waves of a workgroup share its tiles */
    uint32_t waves;            /* 1; shared: 8, or 4 where eight LDS slices do not fit                */
    uint32_t tile_frames;      /* frames of one tile of that form                                      */
    uint32_t chunk_frames;     /* frames one lane filters sequentially in a tile of that form         */
    uint32_t true_peak_factor; /* resolved: 4, 2 or 0 (off)                                            */
    uint32_t subblock_frames;  /* (rate + 5) / 10                                                      */
    uint64_t piece_frames;     /* 32 sub-blocks                                                        */
} ss_streaming_plan;           /* 32 bytes */
/* true_peak_factor: 0 = ebur128's rule for the rate, or 2 / 4.  SS_ERR_NOMEM for a shape no meter takes, SS_ERR_INVALID_ARG. */
int ss_td_streaming_plan(uint32_t channels, uint32_t rate, int32_t true_peak_factor, uint64_t frames, ss_streaming_plan *out);

/* ------------------------------------------------------------------------ *
 *  PCM ingest: the step before the path.  The reference decodes a
 *  file with symphonia into one interleaved Vec<f32> (audio_player.rs:169-267,
 *  SampleBuffer::<f32>::copy_interleaved_ref); for RIFF/WAVE PCM that is a
 *  sample-format conversion, done here on the device:
 *    u8: s/128 - 1   s16: s/32768   s24: s/8388608   s32: (f32)(s/2147483648.0)
 *    f32: as is      f64: (f32)s          (all divisions are exact powers of two)
 * ------------------------------------------------------------------------ */
typedef enum ss_pcm_format {
    SS_PCM_U8 = 1, SS_PCM_S16 = 2, SS_PCM_S24 = 3, SS_PCM_S32 = 4, SS_PCM_F32 = 5, SS_PCM_F64 = 6
} ss_pcm_format;

typedef struct ss_wav_info {
    uint32_t format;        /* ss_pcm_format */
    uint32_t channels;
    uint32_t sample_rate;
    uint32_t bits_per_sample;
    uint64_t data_offset;   /* byte offset of the first sample in the file image */
    uint64_t data_bytes;    /* bytes of sample data actually present            */
    uint64_t frames;        /* whole frames in the data chunk                   */
} ss_wav_info;

/* Parse a RIFF/WAVE image held in memory (little-endian PCM / IEEE float, incl.
 * WAVE_FORMAT_EXTENSIBLE).  Host logic only; no device needed.
 * SS_ERR_INVALID_ARG: not a WAVE file / truncated header; SS_ERR_UNSUPPORTED: other codecs. */
int ss_wav_parse(const void *file_bytes, size_t len, ss_wav_info *out);
/* bytes per sample of a format (0 if unknown) */
size_t ss_pcm_sample_bytes(int format);
/* interleaved little-endian PCM -> interleaved f32 (host in, host out, converted on the device) */
int ss_pcm_decode(const void *pcm, size_t n_samples, int format, float *out);

/* ------------------------------------------------------------------------ *
 *  Batch extension (NOT in the reference): many independent streams of equal
 *  length analysed in one pass — the data-parallel form of
 *  receive_audio_file + analyze_audio_file_samples (tui.rs:1207-1241,
 *  :1482-1552) over a corpus.  Streams stay resident in HBM.
 * ------------------------------------------------------------------------ */
typedef struct ss_batch ss_batch;

enum {
    SS_BATCH_FFT = 1u,       /* per-window mid/side (2 ch) or per-channel spectrum */
    SS_BATCH_LUFS = 2u,      /* K-weighting, gating blocks, histograms, I, LRA    */
    SS_BATCH_TRUE_PEAK = 4u, /* sample peak + oversampled true peak               */
    SS_BATCH_WAVEFORM = 8u,  /* min-max decimation of the interleaved buffer      */
    SS_BATCH_ALL = 15u,
    /* with SS_BATCH_FFT: columns-only spectrum.  The render-side reduction (below: gain, chart bounds, chart columns) runs
     * INSIDE the spectrum kernel's epilogue, on the window's spectrum while it is still in LDS: the full rows are never
     * stored (nor allocated: 6.5 GB at the bench shape) and only `spectrum_columns` values per row leave the chip — what a
     * terminal can show.  Results equal ss_batch_render_spectrum's bit for bit.  Stereo, fft_n = 4096, hop 1024 only
     * (SS_ERR_UNSUPPORTED otherwise); ss_batch_download_fft is not available (SS_ERR_INVALID_MODE).
     * What the mode buys is BYTES, not kernel time: 5.9 GB less HBM footprint at the bench shape (1024 x 10 s: 0.61 GB of columns
     * instead of 6.49 GB of rows), the second pass over the rows gone, and 10.6x less to download over PCIe.  The kernel itself is
     * no faster than the full-row one (3.0-3.2 ms against 2.9): the spectrum kernel is bound by VALU issue, not by its stores, and
     * folding 1705 bins into columns costs about as many instructions as storing them saves waiting. */
    SS_BATCH_FFT_COLUMNS = 16u,
    /* with SS_BATCH_LUFS (SS_ERR_INVALID_ARG otherwise): the momentary and short-term loudness series of every stream and their
     * maxima, formed on the device behind the gating pass (ss_batch_download_loudness_series, ss_batch_loudness_extremes below).
     * Allocates [n_streams][n_subblocks][2] f64 plus one ss_loudness_extremes per stream; a pass with the flag off launches
     * nothing more. */
    SS_BATCH_LOUDNESS_SERIES = 32u
};

typedef struct ss_batch_config {
    uint32_t sample_rate;
    uint32_t channels;          /* 2 => spectrum of mid/side (audio_player.rs:400-419);
                                   otherwise per-channel spectrum */
    uint32_t n_streams;
    uint32_t fft_n;             /* window length (power of two, <= 32768) */
    uint32_t hop_frames;        /* 1024 in the reference (audio_player.rs:65) */
    uint32_t flags;             /* SS_BATCH_* */
    int32_t true_peak_factor;   /* 0 = ebur128 rule, 2 / 4 = forced */
    uint32_t spectrum_columns;  /* SS_BATCH_FFT_COLUMNS: chart columns per spectrum row, 1 .. 512 (otherwise 0) */
    uint64_t frames_per_stream;
    double waveform_window;     /* seconds; <= 0 => frames_per_stream / sample_rate */
} ss_batch_config;

typedef struct ss_stream_result {
    double integrated_lufs;     /* loudness_global(), may be -inf            */
    double loudness_range;      /* loudness_range()                          */
    double true_peak[2];        /* channels 0,1: max(true, sample), linear   */
    double sample_peak[2];
    uint32_t n_gating_blocks;   /* 400 ms blocks evaluated                   */
    uint32_t n_st_blocks;       /* 3 s blocks evaluated                      */
} ss_stream_result;

typedef struct ss_batch_layout {
    uint32_t n_windows;         /* per stream */
    uint32_t fft_channels;      /* 2 (mid, side) or channels */
    uint32_t n_bins;            /* retained bins, 20 Hz..20 kHz */
    uint32_t first_bin;         /* FFT bin index of retained bin 0 */
    uint32_t n_wave_points;     /* per stream: 2 per decimation bin */
    uint32_t n_subblocks;       /* complete 100 ms sub-blocks per stream */
    uint32_t fft_bin_stride;    /* floats between spectrum rows on the device (n_bins rounded up to 4) */
    uint32_t reserved;
    uint64_t input_bytes;       /* device bytes of the input corpus */
    uint64_t fft_bytes;         /* device bytes of the spectrum output */
} ss_batch_layout;

int ss_batch_create(const ss_batch_config *cfg, ss_batch **out);
void ss_batch_destroy(ss_batch *b);
int ss_batch_layout_get(const ss_batch *b, ss_batch_layout *out);
/* copy host PCM into streams [first, first+count): interleaved f32,
 * count*frames_per_stream*channels floats */
int ss_batch_upload(ss_batch *b, uint32_t first, uint32_t count, const float *pcm);
int ss_batch_download_input(ss_batch *b, uint32_t stream, float *pcm, size_t cap_floats);
/* same as ss_batch_upload for raw PCM of `format`: the bytes are copied to the GPU and converted
 * there straight into the resident f32 corpus (no host-side f32 copy) */
int ss_batch_upload_pcm(ss_batch *b, uint32_t first, uint32_t count, const void *pcm, int format);
/* Ragged batches: streams of different lengths in one batch.  Create the batch for the longest stream
 * (frames_per_stream is the slot size), then give every stream its own length; each gets its own window count,
 * sub-block count and decimation geometry by the rules ss_batch_create applies to a uniform batch.  Rows beyond a
 * stream's own counts in the downloads are unspecified; ss_batch_stream_shape says how many are valid. */
typedef struct ss_stream_shape {
    uint64_t frames;
    uint32_t n_windows, n_subblocks, n_wave_points, reserved;
} ss_stream_shape;              /* 24 bytes */
int ss_batch_set_lengths(ss_batch *b, const uint64_t *frames, uint32_t n_streams);
int ss_batch_stream_shape(const ss_batch *b, uint32_t stream, ss_stream_shape *out);
/* the first n_samples interleaved samples of one stream's slot (raw PCM of any ss_pcm_format), queued on the batch's
 * stream; `pcm` must stay valid until the next ss_batch_sync */
int ss_batch_upload_samples(ss_batch *b, uint32_t stream, const void *pcm, size_t n_samples, int format);
/* Pipelined ingest.  A batch owns its HIP stream, so two batches are a double buffer: while one runs, the other's
 * upload is in flight — provided the host memory is page-locked (ss_host_register pins caller memory in place) and
 * the upload does not wait: ss_batch_upload_pcm_async only queues the copy and the conversion; `pcm` must stay
 * valid until the next ss_batch_sync / ss_batch_results on that batch.  soundscope_amd/pipeline.py is the loop. */
int ss_host_register(void *ptr, size_t bytes);
int ss_host_unregister(void *ptr);
int ss_batch_upload_pcm_async(ss_batch *b, uint32_t first, uint32_t count, const void *pcm, int format);
/* device pointer of the resident corpus ([stream][frame][channel] f32) for
 * producers that already hold data on the GPU */
void *ss_batch_input_device_ptr(ss_batch *b);
/* fill the corpus with the documented synthetic signal: utility
 * for benchmarks, not part of the measured path */
int ss_batch_synthesize(ss_batch *b, uint64_t seed, uint32_t first_stream_id);
/* measurement utility (like ss_batch_synthesize, not part of the measured path): run ONLY the HBM traffic of this batch's
 * spectrum kernel — same grid, workgroup size, LDS footprint (occupancy) and addresses, loads and stores, no arithmetic —
 * `reps` times and return the average milliseconds per launch: the floor the memory system sets for that access pattern
 * on this device, next to which the kernel's time can be read.  Overwrites the batch's spectrum buffer.
 * SS_ERR_UNSUPPORTED unless the batch takes the N = 4096 stereo kernel at hop 1024. */
int ss_batch_traffic_floor(ss_batch *b, uint32_t reps, double *ms_per_launch);
/* enqueue one pass of the hot path over the whole batch; asynchronous */
int ss_batch_run(ss_batch *b);
int ss_batch_sync(ss_batch *b);
/* results (after ss_batch_sync) */
int ss_batch_results(ss_batch *b, ss_stream_result *out, uint32_t cap);
/* every channel's peaks of one stream (ss_stream_result only carries channels 0 and 1, like
 * Analyzer::get_true_peak, analyzer.rs:159-164; ebur128 keeps them per channel and the app leaves the rest as
 * "TODO: channels", tui.rs:1217-1221): true_pk[c] = max(true, sample) like EbuR128::true_peak(c), sample_pk[c]
 * = EbuR128::sample_peak(c), linear.  Either array may be NULL; cap_channels >= the batch's channel count. */
int ss_batch_peaks(ss_batch *b, uint32_t stream, double *true_pk, double *sample_pk, uint32_t cap_channels);
/* the launch geometry this batch's shape selected (tests assert that the benchmark geometry is the one they check) */
typedef struct ss_batch_geometry {
    uint32_t fft_windows_per_block;  /* windows one spectrum workgroup walks                          */
    uint32_t fft_blocks;             /* spectrum workgroups per pass                                  */
    uint32_t td_segments;            /* time segments per stream in the time-domain kernel            */
    uint32_t td_segment_subblocks;   /* 100 ms sub-blocks per segment (0: one segment)                */
    uint32_t td_warm_subblocks;      /* filter run-in of segments > 0 (SS_TD_RUN_IN: 1; td_split == 2: 2) */
    uint32_t td_true_peak_factor;    /* 0, 2, 4                                                       */
    uint32_t waveform_fused;         /* 1: decimation runs inside the time-domain kernel              */
    uint32_t overlap;                /* ss_batch_set_overlap mode: 0, 1 or 2                          */
    uint32_t td_split;               /* 1: a stream is one segment walked by the four waves of a workgroup, the filter state handed
                                      *    from tile to tile (the whole recurrence: no run-in); td_segments is 1 then.  2: a handful of
                                      *    streams: every SEGMENT's tiles dealt to the eight waves of a workgroup (latency); a segment
                                      *    then runs the filter over the td_warm_subblocks (2) in front of it inside the one launch —
                                      *    the state the second launch would start from — and td_fixup_subblocks is 0              */
    uint32_t td_fixup_subblocks;     /* sub-blocks at the head of every segment > 0 re-run from the exact state by the second launch */
} ss_batch_geometry;                 /* 40 bytes (32 up to ABI version 1) */
int ss_batch_geometry_get(const ss_batch *b, ss_batch_geometry *out);
/* the same for a caller built against an older (shorter) or newer (longer) struct: writes min(out_bytes, sizeof(ss_batch_geometry))
 * bytes, never more than the caller has — a client compiled against the 32-byte struct of ABI version 1 passes 32 and gets the
 * fields it knows (ss_batch_geometry_get itself writes the whole 40-byte struct and is for callers that check ss_abi_version()) */
int ss_batch_geometry_get_sized(const ss_batch *b, void *out, size_t out_bytes);
/* how the time-domain kernel walks a stream.  The K-weighting recurrence has a long memory (poles at |z| = 0.995): a stream cut
 * into time segments for parallelism must hand the filter state from one segment to the next.
 *   SS_TD_AUTO (default)   time segments, one wave each, EXACT hand-over: every segment starts at its boundary from a zero state,
 *                          leaves its end state behind, and a second light launch re-runs the first 0.2 s of every segment > 0 from
 *                          the state the segment in front of it left, overwriting those sub-blocks' energies (after 0.2 s the
 *                          zero start differs from the true trajectory by e^-48 of the state: 1e-13 of the filtered signal on
 *                          DC-offset material, under the 2e-11 at which any two evaluation orders of this recurrence differ).
 *                          Segment 0 and the re-run head of segment 1 equal the one-segment path bit for bit; elsewhere the
 *                          difference is the rounding noise of the recurrence (3e-10 at worst on the bench corpus, the same as
 *                          for the exact-by-construction SS_TD_WHOLE_STREAMS), not a dropped term (tests pin both).
 *                          A handful of streams (one file; td_split == 2 in the geometry): the same segments on eight waves each,
 *                          and every segment runs the filter over the 0.2 s in front of it, from zero, inside the ONE launch —
 *                          the state the second launch would have started from, without a second launch.
 *   SS_TD_RUN_IN           the form of rounds 1-4, kept for comparison: a segment > 0 starts its filter 0.1 s early from a zero
 *                          state and drops that run-in (3e-10 on sub-block energies of DC-offset material: a truncation).
 *   SS_TD_WHOLE_STREAMS    stereo / eight channels, equal lengths: a stream is ONE segment walked by the four waves of a
 *                          workgroup, the state handed from tile to tile through LDS — exact by construction, but the waves of a
 *                          workgroup wait for each other: 16 % slower at the bench shape than independent segment waves. */
enum { SS_TD_AUTO = 0, SS_TD_RUN_IN = 1, SS_TD_WHOLE_STREAMS = 2 };
int ss_batch_set_time_domain_mode(ss_batch *b, int mode);
/* how a pass is laid over the batch's two HIP streams; results are identical in every mode.
 *   0  sequential: spectrum kernel, then the time-domain chain (default);
 *   1  the spectrum kernel on a second stream beside the whole time-domain chain (they use different pipes: packed f32
 *      VALU + LDS vs f64 VALU + matrix cores);
 *   2  the time-domain kernel alone first, then the spectrum kernel on the second stream beside the chain's short
 *      latency-bound tail (per-stream gating / histograms, a standalone decimation).
 * Per-kernel event timing (ss_batch_timing_enable) always runs sequentially. */
int ss_batch_set_overlap(ss_batch *b, int mode);
/* arithmetic of the 4x true-peak interpolator in batches (the Analyzer handle and the sessions: ss_analyzer_set_true_peak_arith, same default):
 *   SS_TP_ARITH_F32 (default)    an f32 fmaf chain per output, the width of ebur128's interpolator (its 12 products per phase
 *                                summed in f32; analyzer.rs:139-141,159-164).  2, 6 or 8 channels: on the packed-f32 VALU
 *                                (v_pk_fma_f32; a frame's pair of adjacent channels is one packed operand, round 6; at factor 2
 *                                the 24-tap branch's halves on neighbouring lanes — in the four-waves register builds with plain
 *                                v_fma_f32 instead); channel counts that do not divide 16 (3, 5, 7 ...): plain v_fma_f32, a lane
 *                                per channel; mono, 4 and 16 channels: v_mfma_f32_16x16x4_f32 as a banded-Toeplitz product
 *                                (measured the faster form there);
 *   SS_TP_ARITH_F16X3 (opt-in)   three-term f16 split on the matrix cores with f32 accumulation, scaled per tile by a
 *                                power of two from the tile's own peak: within 2^-21 of the tile peak of the f32 result
 *                                (measured 2.0e-7 relative on the bench corpus against 1.1e-7 for the f32 product; north_star's
 *                                bar is 1e-4), 3-5 % less time-domain kernel time since the f32 form left the matrix pipe
 *                                (it was 25 %).  2 / 8 channels only: other shapes, and tiles with non-finite samples, take
 *                                the f32 form whatever the mode. */
enum { SS_TP_ARITH_F16X3 = 0, SS_TP_ARITH_F32 = 1 };
int ss_batch_set_true_peak_arith(ss_batch *b, int arith);
int ss_batch_get_true_peak_arith(const ss_batch *b);      /* SS_TP_ARITH_* */
/* verification utility: order-independent 64-bit checksums, computed on the device, of everything a pass left in HBM for
 * each stream: out[3 * s + 0] the stream's whole spectrum block ([n_windows][fft_channels][fft_bin_stride] f32 bit patterns),
 * out[3 * s + 1] its decimation bins, out[3 * s + 2] its sub-block energies (f64 bit patterns).  Two passes agree on a
 * checksum iff (up to 2^-64) they agree bit for bit on the data: a stress test can compare EVERY window of a multi-gigabyte
 * batch between launch modes (ss_batch_set_overlap) without downloading it.  Waits for the batch's stream. */
int ss_batch_checksums(ss_batch *b, uint64_t *out, uint32_t cap_streams);
/* spectrum of one stream: compact [n_windows][fft_channels][n_bins] f32 dB (pink-compensated);
 * on the device the rows are fft_bin_stride floats apart */
int ss_batch_download_fft(ss_batch *b, uint32_t stream, float *out, size_t cap_floats);
/* chart_x / frequency / pink compensation per retained bin (f64, n_bins each; any may be NULL) */
int ss_batch_bin_tables(const ss_batch *b, double *chart_x, double *freq, double *pink_db);
/* waveform of one stream: n_wave_points pairs (i, value) like get_waveform, as f32 values only:
 * out[2*i] = min, out[2*i+1] = max of decimation bin i */
int ss_batch_download_waveform(ss_batch *b, uint32_t stream, float *out, size_t cap_floats);
/* K-weighted energy of the 100 ms sub-blocks of one stream: [n_subblocks][channels] f64 */
int ss_batch_download_subblocks(ss_batch *b, uint32_t stream, double *out, size_t cap_doubles);
/* Loudness over time (SS_BATCH_LOUDNESS_SERIES batches; SS_ERR_INVALID_MODE otherwise).  Entry j of a stream's series is what
 * EbuR128::loudness_momentary() / loudness_shortterm() returns after the stream's first (j + 1) * s100 frames
 * (s100 = (rate + 5) / 10):  10 log10(E) - 0.691,  E = sum_c w_c (sum of the sub-block energies j - N + 1 ... j) / (N s100),
 * N = 4 (momentary) or 30 (short-term), w_c the meter's channel weights (weight-0 channels are never read).  Sub-blocks in front
 * of the stream count as zero (the crate's ring starts zeroed): entries j < N - 1 are its partial readings; E = 0 reads -inf.
 * A non-finite sample poisons the meter like the crate's: every window that ends behind the first sub-block holding one reads
 * NaN, the window that ends with it holds what the recurrence produced.  At rates whose thirty sub-blocks exceed the crate's
 * 3 s ring (loudness_shortterm fails there) the short-term entries are NaN.
 * ss_batch_download_loudness_series writes the stream's own n_subblocks entries (ss_batch_stream_shape for ragged batches) into
 * either array (either may be NULL); cap < n_subblocks: SS_ERR_CAPACITY. */
int ss_batch_download_loudness_series(ss_batch *b, uint32_t stream, double *momentary, double *shortterm, size_t cap);
/* the maxima of the series over the FULL windows only (j >= 3 momentary, j >= 29 short-term): NaN entries are skipped, an
 * infinity counts as a value, ties go to the lowest j; no such entry: -inf at 0xFFFFFFFF.  Waits for the batch's stream; cap_streams < n_streams: SS_ERR_CAPACITY. */
typedef struct ss_loudness_extremes {
    double max_momentary;       /* LUFS; -inf if the stream has no full 400 ms window                        */
    double max_shortterm;       /* LUFS; -inf if the stream has no full 3 s window                           */
    uint32_t max_momentary_at;  /* sub-block index j of the window that attains it first; 0xFFFFFFFF if none */
    uint32_t max_shortterm_at;
} ss_loudness_extremes;         /* 24 bytes */
int ss_batch_loudness_extremes(ss_batch *b, ss_loudness_extremes *out, uint32_t cap_streams);
/* Loudness regions: the gated loudness of time ranges of the streams of a batch, and of groups of such ranges (programme items in
 * a transmission log, tracks of a mix, scenes of a reel; a group of whole streams is an album, the loudness_global_multiple /
 * loudness_range_multiple case).  Not in the reference.  After ss_batch_run, on what the pass left on the device: nothing inside
 * the pass changes.  With S = s100 and P the stream's sub-block energies (ss_batch_download_subblocks), region (s, a, n):
 *   - owns the gating blocks of stream s that end with sub-block j, a + 3 <= j < a + n (all four sub-blocks inside the region),
 *     and the short-term blocks that end with j = a + 29 + 10 m < a + n: the phase is anchored at the region's start, as a meter
 *     started there would have it, not at the stream's start.  n_gating_blocks = max(n - 3, 0), n_st_blocks = (n - 30) / 10 + 1
 *     for n >= 30, else 0;
 *   - every energy is the weighted sum of the 4 (30) sub-block energies ending with j, each channel added oldest first, divided
 *     by 4 S (30 S): for a = 0 the same expressions and additions as the pass itself, hence the same bits;
 *   - the K-weighting filter is the stream's continuous one: a region is NOT a fresh meter fed the range, it is the stream's own
 *     blocks that lie inside the range (a fresh meter's filter would start from rest at a: its first blocks differ by what the
 *     filter still remembers of the frames in front of a);
 *   - non-finite input follows the stream: a block that ends behind the stream's first sub-block holding a non-finite sample of a
 *     weighted channel has a NaN energy; it is counted in n_gating_blocks / n_st_blocks and lands in no bin;
 *   - blocks at or above the absolute gate (-70 LUFS) are binned like the stream's own (1000 bins of 0.1 LU); integrated_lufs and
 *     loudness_range are the relative gate at -10 LU and the EBU 3342 percentile walk on the region's own histogram pair: -inf and
 *     0 where nothing is counted;
 *   - max_momentary runs over a + 3 <= j < a + n; max_shortterm over EVERY j with a + 29 <= j < a + n (every sub-block, as the
 *     loudness series has it, not only the histogram's phase).  Values are 10 log10(E) - 0.691 (E <= 0: -inf); NaN is skipped, an
 *     infinity counts, ties go to the lowest j; *_at is the ABSOLUTE sub-block index in the stream; no such value: -inf at
 *     0xFFFFFFFF.  At rates without short-term blocks (thirty sub-blocks exceed the crate's 3 s ring) n_st_blocks = 0 and
 *     max_shortterm is -inf at 0xFFFFFFFF.
 * Groups: a group's histogram pair is the bin-wise u64 sum of the pairs of the regions that name it, its counts the sums of their
 * counts, its results the same evaluation of that sum.  Regions may come from any streams, overlap and repeat: each one counts.
 * A group without regions reads -inf, 0, 0, 0.  Per-region histograms are not kept: give a region a group of its own to read its.
 * Only integer atomics touch shared histograms and there are no floating-point atomics: two calls on the same pass agree byte for
 * byte.
 * ss_batch_loudness_regions copies `regions` before it returns and queues its work on the batch's stream like
 * ss_batch_spectrum_stats: nothing is copied back or waited for.  A later call replaces the list and every result.  The downloads
 * and ss_batch_group_histograms (1000 block bins then 1000 short-term bins, as ss_batch_histograms) wait for the stream.
 * Device memory (16 bytes + 48 bytes per region, 16 KB + 32 bytes per group) is allocated at the first call and grows with a longer
 * list: a batch that never calls this allocates and launches exactly what it did before.
 * Status codes, all checked before anything is queued: a batch without SS_BATCH_LUFS, and a download before the first call,
 * SS_ERR_INVALID_MODE; stream >= n_streams, first_subblock + n_subblocks (in 64 bits) beyond the stream's own n_subblocks
 * (ss_batch_stream_shape for ragged batches), a group >= n_groups other than SS_REGION_NO_GROUP, a group index >= n_groups in
 * ss_batch_group_histograms, regions == NULL with n_regions > 0: SS_ERR_INVALID_ARG; a `cap` too small: SS_ERR_CAPACITY.
 * n_regions == 0 and n_subblocks == 0 are valid. */
#define SS_REGION_NO_GROUP 0xFFFFFFFFu
typedef struct ss_loudness_region {
    uint32_t stream;
    uint32_t first_subblock;    /* a: index of the region's first 100 ms sub-block in its stream */
    uint32_t n_subblocks;       /* n: may be 0 */
    uint32_t group;             /* 0 .. n_groups - 1, or SS_REGION_NO_GROUP */
} ss_loudness_region;           /* 16 bytes */
typedef struct ss_region_result {
    double integrated_lufs, loudness_range;
    double max_momentary, max_shortterm;            /* LUFS; -inf if none */
    uint32_t max_momentary_at, max_shortterm_at;    /* ABSOLUTE sub-block index in the stream; 0xFFFFFFFF if none */
    uint32_t n_gating_blocks, n_st_blocks;
} ss_region_result;             /* 48 bytes */
typedef struct ss_group_result {
    double integrated_lufs, loudness_range;
    uint64_t n_gating_blocks, n_st_blocks;
} ss_group_result;              /* 32 bytes */
int ss_batch_loudness_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups);
int ss_batch_download_region_results(ss_batch *b, ss_region_result *out, uint32_t cap_regions);
int ss_batch_download_group_results(ss_batch *b, ss_group_result *out, uint32_t cap_groups);
int ss_batch_group_histograms(ss_batch *b, uint32_t group, uint64_t *out2000);
/* Peak series and peak regions: the true and sample peak of every 100 ms of every stream of a batch, the frame that attains each,
 * and their maxima over time ranges and groups of ranges — the second half of a delivery specification (programme loudness and
 * maximum true peak per item), on the grid of the loudness regions, so one ss_loudness_region list reads both.  Not in the
 * reference.  ss_batch_peak_series reads the resident f32 corpus alone: it needs no ss_batch_run and no particular flag, and
 * nothing inside a pass changes.  With S = s100 = (sample_rate + 5) / 10 and F_s stream s's own frame count (ss_batch_set_lengths;
 * frames behind it are never read), stream s has E_s = ceil(F_s / S) entries; entry j covers frames [j S, min((j + 1) S, F_s)):
 * entries j < n_subblocks are the sub-blocks the loudness side indexes, a last partial entry covers the tail, so the maximum over
 * a stream's entries covers every frame.  Per (stream, entry, channel) one ss_peak_entry:
 *   - the interpolator is the batch's: y_f[n] = sum_t c_f[t] x[n - t] over the taps ss_inspect_true_peak lists (12 per branch at
 *     factor 4, 24 at factor 2), the factor ss_batch_config::true_peak_factor (0: the crate's rule for the rate; at 192 kHz and
 *     above there is no interpolation and true_peak equals sample_peak).  Branch 0 is x[n] itself.  One f32 chain of fused
 *     multiply-adds per output, oldest tap first; it need not equal a pass's true peak bit for bit (the pass's own forms do not
 *     equal each other either), and lies within the same distance of the exact sum;
 *   - x[n] = 0 for n < 0: a stream's history is its own, never the tail of the stream in front of it in memory;
 *   - an output belongs to the entry of its frame n and reaches back up to 11 (23) frames into the entry before;
 *   - capture is the crate's `if v > max` from 0: a NaN output is never captured (the other branches of its frame still are), an
 *     infinity is; an all-zero or all-NaN entry reads 0 at 0xFFFFFFFF; ties go to the lowest frame.
 * The series ([stream][entries_cap][channels] records, 16 * entries_cap * channels * n_streams bytes, entries_cap =
 * ceil(frames_per_stream / S)) is allocated at the first call; ss_batch_peak_series_plan reports entries_cap and tile_frames, the
 * frames of an entry one workgroup stages at a time (an entry of more frames is walked in tiles).
 * ss_batch_peak_regions takes the loudness regions' records, copies them before it returns, and reduces the series over entries
 * first_subblock <= j < first_subblock + n_subblocks; the bound is the stream's E_s, not n_subblocks, so a region may include the
 * tail entry.  `ceiling` is linear (+inf: nothing is over).  Ties between equal values: within a region the lowest entry, then the
 * lowest frame, then the lowest channel; across a group the lowest region index.  Regions may come from any streams, overlap and
 * repeat: each one counts.  A region or group in which nothing was captured reads 0 with the "none" marks below.  Group maxima use
 * integer atomics on (value bits, inverted index) words only and there are no floating-point atomics: two calls agree byte for byte.
 * ss_batch_download_region_channel_peaks returns every region's per-channel maxima, [region][channels] floats each; either pointer
 * may be NULL.
 * Both calls queue their work on the batch's stream like ss_batch_spectrum_stats: nothing is copied back or waited for.  A later
 * call replaces every result; the downloads wait for the stream.  ss_batch_peak_regions reads the series as it is when it runs:
 * call ss_batch_peak_series again after new input or new lengths.  A batch that never calls any of this allocates and launches
 * exactly what it did before.
 * Status codes, all checked before anything is queued: a download before the first computation of its kind, and
 * ss_batch_peak_regions before ss_batch_peak_series: SS_ERR_INVALID_MODE; stream >= n_streams, first_subblock + n_subblocks (in 64
 * bits) beyond the stream's E_s, a group >= n_groups other than SS_REGION_NO_GROUP, a NaN or negative ceiling, regions == NULL with
 * n_regions > 0: SS_ERR_INVALID_ARG; a `cap` too small: SS_ERR_CAPACITY.  n_regions == 0, n_subblocks == 0 and F_s == 0 (no
 * entries) are valid. */
typedef struct ss_peak_entry {
    float true_peak;            /* max over the entry's frames and ALL branches, branch 0 (the sample) included: max(true, sample)
                                 * like EbuR128::true_peak */
    float sample_peak;          /* max |x[n]| */
    uint32_t true_peak_frame;   /* offset in the entry of the frame that attains it first; 0xFFFFFFFF if nothing was captured */
    uint32_t sample_peak_frame;
} ss_peak_entry;                /* 16 bytes */
typedef struct ss_region_peaks {
    double true_peak, sample_peak;                      /* max over the region's entries and ALL channels (the f32 widened); 0 if none */
    uint64_t true_peak_frame, sample_peak_frame;        /* ABSOLUTE frame in the stream; UINT64_MAX if none */
    uint32_t true_peak_channel, sample_peak_channel;    /* 0xFFFFFFFF if none */
    uint32_t n_over;                                    /* entries whose true_peak of ANY channel is > ceiling */
    uint32_t first_over;                                /* absolute entry index of the first; 0xFFFFFFFF if none */
} ss_region_peaks;              /* 48 bytes */
typedef struct ss_group_peaks {
    double true_peak, sample_peak;                      /* max over the regions that name the group */
    uint32_t true_peak_region, sample_peak_region;      /* index into the list; 0xFFFFFFFF if none */
    uint64_t n_over;                                    /* sum of the regions' n_over (overlaps and repeats each count) */
} ss_group_peaks;               /* 32 bytes */
int ss_batch_peak_series(ss_batch *b);
int ss_batch_peak_series_plan(const ss_batch *b, uint32_t *tile_frames, uint32_t *entries_cap);
/* stream's entries, [entry][channel]; *n_entries (optional) = E_s; cap_entries counts entries (records / channels) */
int ss_batch_download_peak_series(ss_batch *b, uint32_t stream, ss_peak_entry *out, size_t cap_entries, uint32_t *n_entries);
int ss_batch_peak_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups, double ceiling);
int ss_batch_download_region_peaks(ss_batch *b, ss_region_peaks *out, uint32_t cap_regions);
int ss_batch_download_group_peaks(ss_batch *b, ss_group_peaks *out, uint32_t cap_groups);
int ss_batch_download_region_channel_peaks(ss_batch *b, float *true_pk, float *sample_pk, size_t cap_floats);
/* Signal scan: whether every stream of a batch holds sound at all, whether it is clipped, and whether it carries a DC offset or
 * non-finite samples — what an ingest or QC chain checks before it trusts the loudness and peak figures.  Not in the reference.
 * ss_batch_signal_scan reads the resident f32 corpus alone, like ss_batch_peak_series: it needs no ss_batch_run and no particular
 * flag, nothing inside a pass changes, and the corpus is only read.  F_s is stream s's own frame count (ss_batch_set_lengths);
 * frames behind it, and the neighbouring slots, are never read.  Predicates on single samples, f32 comparisons as written:
 *   - frame n is SILENT iff fabsf(x[n][c]) <= silence_threshold for every channel c: a NaN is never silent, threshold 0 is digital
 *     silence (-0.0 counts), and at threshold +inf an infinity is silent;
 *   - sample (n, c) is CLIPPED iff fabsf(x[n][c]) >= clip_level: an infinity is clipped, a NaN is not;
 *   - a RUN is a maximal sequence of consecutive frames of one stream on which a predicate holds.  Silence runs are counted per
 *     stream, clip runs per channel of a stream.
 * Every result except the two f64 sums is an integer defined by these predicates.  The sums widen every finite sample to f64 (its
 * square is formed in f64, so it is exact) and add in an order fixed by the kernel plan, not by timing; there are no floating-point
 * atomics: two calls agree byte for byte.  The caller forms DC = sum / (F_s - nonfinite) and RMS = sqrt(sum_sq / (F_s - nonfinite)).
 * Two lists per stream hold the runs themselves: the silence list has the runs of at least silence_min_frames, ascending by
 * first_frame, with channel = 0xFFFFFFFF; the clip list has the runs of at least clip_min_samples, ordered by (channel,
 * first_frame).  A list keeps its first max_events events in that order; the counts in the records are always the true totals, so
 * a caller sees truncation as count > max_events.
 * The call copies cfg, queues its work on the batch's stream and waits for nothing; a later call replaces every result; the
 * downloads wait for the stream.  Call it again after new input or new lengths.  Device memory is allocated at the first call:
 * 80 bytes per (tile, channel) and 48 per tile of ss_batch_signal_scan_plan's tile_frames frames (a multiple of 64), the records,
 * and 48 * max_events bytes of lists per stream, which grow with max_events.  A batch that never calls this allocates and launches
 * exactly what it did before.
 * Status codes, all checked before anything is queued, so a refused call leaves the previous results as they were: cfg == NULL, a
 * NaN or negative silence_threshold, clip_level NaN or <= 0, a minimum of 0, max_events > 65536, reserved != 0, stream >=
 * n_streams, an unknown kind: SS_ERR_INVALID_ARG; a download before the first scan: SS_ERR_INVALID_MODE; a `cap` too small:
 * SS_ERR_CAPACITY, with nothing written.  F_s == 0 is valid: every field is zero or "none" and both lists are empty. */
typedef struct ss_signal_scan_config {
    float    silence_threshold;   /* linear, >= 0, not NaN (+inf allowed) */
    float    clip_level;          /* linear, > 0, not NaN */
    uint32_t silence_min_frames;  /* >= 1: runs at least this long are counted and listed */
    uint32_t clip_min_samples;    /* >= 1 */
    uint32_t max_events;          /* list slots per stream and kind, 0 .. 65536 */
    uint32_t reserved;            /* 0 */
} ss_signal_scan_config;          /* 24 bytes */
typedef struct ss_stream_scan {
    uint64_t silent_frames;       /* every silent frame, in runs of any length */
    uint64_t leading_silence;     /* frames of the run that holds frame 0, else 0: any length, not subject to the minimum */
    uint64_t trailing_silence;    /* the same for the run that holds frame F_s - 1; in an all-silent stream both equal F_s */
    uint64_t longest_silence;     /* frames of the longest run of any length; ties go to the lowest frame; 0 if none */
    uint64_t longest_silence_at;  /* its first frame; UINT64_MAX if none */
    uint64_t silence_runs;        /* runs of at least silence_min_frames */
    uint64_t clip_runs;           /* the sum over channels of ss_channel_scan::clip_runs */
} ss_stream_scan;                 /* 56 bytes */
typedef struct ss_channel_scan {
    double   sum, sum_sq;         /* over the channel's finite samples of the stream */
    uint64_t nonfinite;           /* NaN and infinite samples */
    uint64_t first_nonfinite;     /* frame of the first; UINT64_MAX if none */
    uint64_t clipped_samples;
    uint64_t longest_clip;        /* any length; ties go to the lowest frame; 0 if none */
    uint64_t longest_clip_at;     /* UINT64_MAX if none */
    uint64_t clip_runs;           /* the channel's runs of at least clip_min_samples */
} ss_channel_scan;                /* 64 bytes */
typedef struct ss_signal_event {
    uint64_t first_frame;
    uint64_t frames;
    uint32_t channel;             /* 0xFFFFFFFF in the silence list */
    uint32_t reserved;            /* 0 */
} ss_signal_event;                /* 24 bytes */
enum { SS_SIGNAL_SILENCE = 0, SS_SIGNAL_CLIP = 1 };
int ss_batch_signal_scan(ss_batch *b, const ss_signal_scan_config *cfg);
/* tile_frames: the frames one workgroup scans (runs are carried across tiles); tiles_cap = ceil(frames_per_stream / tile_frames) */
int ss_batch_signal_scan_plan(const ss_batch *b, uint32_t *tile_frames, uint32_t *tiles_cap);
int ss_batch_download_stream_scans(ss_batch *b, ss_stream_scan *out, uint32_t cap_streams);
/* [stream][channel] */
int ss_batch_download_channel_scans(ss_batch *b, ss_channel_scan *out, size_t cap_records);
/* one list of one stream; *n_events (optional) = min(count, max_events) */
int ss_batch_download_signal_events(ss_batch *b, uint32_t stream, int kind, ss_signal_event *out, size_t cap_events, uint32_t *n_events);
/* Pair series and pair regions: how two channels of a stream relate in the time domain, per 100 ms and per time range — the
 * correlation (phase) meter, the channel balance and the level a mono fold-down loses.  A stereo item whose channels are out of
 * phase disappears in a mono fold-down; delivery specifications reject it.  Not in the reference.
 * ss_batch_pair_series reads the resident f32 corpus alone, like ss_batch_peak_series: it needs no ss_batch_run and no particular
 * flag, nothing inside a pass changes, and the corpus is only read.  The grid is the peak series': with S = s100 = (sample_rate +
 * 5) / 10 and F_s stream s's own frame count (ss_batch_set_lengths; frames behind it, and the neighbouring slots, are never read),
 * stream s has E_s = ceil(F_s / S) entries; entry j covers frames [j S, min((j + 1) S, F_s)), a last partial entry covers the tail.
 * Per (stream, entry, pair (a, b)) one ss_pair_entry: a frame in which x_a or x_b is NaN or infinite is SKIPPED and adds to no sum;
 * every other frame is counted, its two samples widened to f64, and x_a^2, x_b^2 and x_a x_b (exact in f64: 24 x 24 bits) added to
 * s_aa, s_bb and s_ab.  The additions follow an order fixed by the kernel plan, not by timing: a lane adds its own frames in
 * ascending order, the 64 lanes of a wave meet in a fixed tree, the four waves are added in wave order; there are no floating-point
 * atomics, so two calls agree byte for byte.  The caller forms, per entry or region,
 *   correlation  = s_ab / sqrt(s_aa s_bb)                              (NaN where a power is 0)
 *   balance (dB) = 10 log10(s_bb / s_aa)
 *   mono loss (dB) = 10 log10((s_aa + 2 s_ab + s_bb) / (2 (s_aa + s_bb)))   ((a + b) / 2 against the mean channel power: 0 for b = a)
 * pairs == NULL with n_pairs == 0 is the one pair (0, 1); a == b is allowed (s_ab == s_aa == s_bb).  The call copies `pairs`, queues
 * its work on the batch's stream and waits for nothing; a later call replaces every result (the pair list included); the downloads
 * wait for the stream.  Call it again after new input or new lengths.  Device memory, 32 * entries_cap * n_pairs * n_streams bytes
 * (entries_cap = ceil(frames_per_stream / S)), is allocated at the first call and grows with a longer pair list.
 * ss_batch_pair_series_plan reports tile_frames (the frames a workgroup has in flight at a time: it fixes which lane adds which
 * frame), entries_cap and the pairs of the last call that was queued (before the first: those of the default list, 1).
 * ss_batch_pair_regions takes the loudness regions' records under ss_batch_peak_regions' rules (the bound is the stream's E_s, so a
 * region may hold the tail entry; regions may overlap, repeat and come from any stream), copies them before it returns, and
 * reduces the series as it is when the call runs, per (region, pair):
 *   - the sums, frames and skipped of the region's entries, added in ascending entry order from 0;
 *   - an entry is ACTIVE iff s_aa + s_bb > power_floor * frames (one f64 addition, one f64 multiplication by the frames counted);
 *   - an entry is BELOW iff its correlation is under `threshold`, decided without a square root or a division: with p = s_aa * s_bb,
 *     q = s_ab, t = threshold, every product one rounded f64 multiplication (none contracted into a fused multiply-add),
 *         t >= 0:  BELOW iff q < 0 || q * q < (t * t) * p
 *         t <  0:  BELOW iff q < 0 && q * q > (t * t) * p
 *     so an entry with p == 0 is never BELOW when t <= 0, and when t > 0 only if q < 0 || q * q < 0 holds (it does not for a finite
 *     q >= 0; a silent entry is inactive anyway);
 *   - n_below, first_below and the runs take ACTIVE BELOW entries only: a run is a maximal sequence of consecutive entries of the
 *     region that are both, so an inactive entry ends a run as an entry that is not below does.
 * A group's record adds the records of the regions that name it in ascending region index order from 0 (ss_batch_spectrum_regions'
 * rule); its counts are integer sums.  Two calls agree byte for byte.  A batch that never calls any of this allocates and launches
 * exactly what it did before.
 * Status codes, all checked before anything is queued, so a refused call leaves the previous results as they were: a or b >=
 * channels, n_pairs > 16, pairs == NULL with n_pairs > 0, the default pair on a mono batch, stream >= n_streams, cfg == NULL, a NaN
 * threshold or |threshold| >= 1, a NaN or negative power_floor, min_run == 0, reserved != 0, and the list errors of
 * ss_batch_peak_regions: SS_ERR_INVALID_ARG; a download before the first computation of its kind, and ss_batch_pair_regions before
 * ss_batch_pair_series: SS_ERR_INVALID_MODE; a `cap` too small: SS_ERR_CAPACITY, with nothing written.  F_s == 0 (no entries),
 * n_regions == 0 and n_subblocks == 0 are valid. */
typedef struct ss_channel_pair { uint32_t a, b; } ss_channel_pair;      /* 8 bytes; a, b < channels */
typedef struct ss_pair_entry {
    double   s_aa, s_bb, s_ab;    /* sums of x_a^2, x_b^2, x_a x_b over the counted frames of the entry */
    uint32_t frames;              /* frames counted */
    uint32_t skipped;             /* frames of the entry in which x_a or x_b is NaN or infinite: they add to no sum */
} ss_pair_entry;                  /* 32 bytes */
typedef struct ss_pair_region_config {
    double   threshold;           /* an entry is BELOW iff its correlation < threshold; -1 < threshold < 1 */
    double   power_floor;         /* an entry is ACTIVE iff s_aa + s_bb > power_floor * frames (linear power per frame, >= 0) */
    uint32_t min_run;             /* >= 1: runs of consecutive active BELOW entries at least this long are counted */
    uint32_t reserved;            /* 0 */
} ss_pair_region_config;          /* 24 bytes */
typedef struct ss_region_pair {
    double   s_aa, s_bb, s_ab;    /* the entries' sums added in entry order */
    uint64_t frames, skipped;
    uint32_t n_active, n_below;   /* n_below counts active entries only */
    uint32_t first_below;         /* ABSOLUTE entry index of the first active BELOW entry; 0xFFFFFFFF if none */
    uint32_t longest_below;       /* entries of the longest run, of any length; ties go to the lowest entry; 0 if none */
    uint32_t longest_below_at;    /* ABSOLUTE entry index of its first entry; 0xFFFFFFFF if none */
    uint32_t below_runs;          /* runs of at least min_run */
} ss_region_pair;                 /* 64 bytes */
typedef struct ss_group_pair {
    double   s_aa, s_bb, s_ab;    /* the regions' sums added in region index order */
    uint64_t frames, skipped, n_active, n_below, below_runs;      /* overlaps and repeats each count */
} ss_group_pair;                  /* 64 bytes */
int ss_batch_pair_series(ss_batch *b, const ss_channel_pair *pairs, uint32_t n_pairs);
int ss_batch_pair_series_plan(const ss_batch *b, uint32_t *tile_frames, uint32_t *entries_cap, uint32_t *n_pairs);
/* stream's entries, [entry][pair]; *n_entries (optional) = E_s; cap_entries counts entries (records / n_pairs) */
int ss_batch_download_pair_series(ss_batch *b, uint32_t stream, ss_pair_entry *out, size_t cap_entries, uint32_t *n_entries);
int ss_batch_pair_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups, const ss_pair_region_config *cfg);
/* [region][pair] and [group][pair] of the last list, the pairs those of the series it read; cap_records counts records */
int ss_batch_download_region_pairs(ss_batch *b, ss_region_pair *out, size_t cap_records);
int ss_batch_download_group_pairs(ss_batch *b, ss_group_pair *out, size_t cap_records);
/* Batch gain and PCM export: the batch acts on what it measured — a gain per stream (or a gain curve: ramps, steps, fades) applied
 * to the resident corpus in one sweep, and the corpus handed back in a delivery format.  Not in the reference.
 *
 * Host arithmetic, no device needed.  ss_normalisation_gain is the gain law of a loudness target with a true-peak ceiling:
 *   - a loudness that is NaN or +-inf: gain_db = 0, gain = 1, limited_by = SS_GAIN_UNMEASURED;
 *   - else g = target_lufs - loudness_lufs;
 *   - the ceiling applies when max_true_peak_dbtp is finite and peak_linear is finite and > 0: with the headroom h =
 *     max_true_peak_dbtp - 20 log10(peak_linear), g > h makes g = h and sets SS_GAIN_LIMITED_PEAK;
 *   - then g > max_gain_db makes g = max_gain_db (SS_GAIN_LIMITED_MAX) and g < min_gain_db makes g = min_gain_db
 *     (SS_GAIN_LIMITED_MIN): the clamp comes last, so a positive min_gain_db can break the ceiling, and both bits then show;
 *   - gain = (float)pow(10, g / 20); where the ceiling bound the result (g is still the headroom) and the rounding to f32 went up,
 *     gain is the next f32 down, so that gain * peak exceeds the ceiling by no rounding of gain's.
 * +inf for max_true_peak_dbtp and max_gain_db and -inf for min_gain_db mean "none".  A NaN in a target field or in peak_linear,
 * min_gain_db > max_gain_db, or t == NULL: SS_ERR_INVALID_ARG.  The three outputs are optional.
 * ss_gain_envelope is the definition of the gain curve ss_batch_apply_gain follows: `pts` holds ONE stream's n points with strictly
 * ascending frames (the stream field is not read).  With g_k the gains widened to double and f_k the frames:
 *   - frame <= f_0: g_0;  frame >= f_(n-1): g_(n-1);
 *   - f_k <= frame < f_(k+1) otherwise: g_k + (double)(frame - f_k) * d_k, d_k = (g_(k+1) - g_k) / (double)(f_(k+1) - f_k),
 * every operation rounded on its own (no fused multiply-add).  One point is a constant gain, two points a ramp, two points on
 * adjacent frames a step, points of gain 0 fades.  n == 0 (or pts == NULL) gives 1.
 *
 * ss_batch_apply_gain multiplies the resident f32 corpus IN PLACE: sample x of frame n < F_s (the stream's own length,
 * ss_batch_set_lengths) in a selected channel of a stream that has at least one point becomes
 *     y = (float)((double)x * ss_gain_envelope(that stream's points, n))
 * one rounded f64 multiplication and one round-to-nearest conversion; where the envelope is constant that is the plain f32 product
 * x * g (the product of two f32 values is exact in f64).  THE OPERATION IS LOSSY, one rounding per sample: keep the source if the
 * gain may have to be taken back.  RESULTS OF EARLIER PASSES, SERIES AND SCANS DESCRIBE THE CORPUS BEFORE THE CALL: run them again
 * for the corpus behind it.  Streams without a point, unselected channels and frames at or behind F_s stay byte for byte (the latter
 * are neither read nor written); in a touched stream a frame whose envelope is exactly 1 may or may not be rewritten (its finite
 * samples are the same either way, a NaN stays a NaN with an unspecified payload).  NaN in gives NaN out, a finite product that
 * overflows gives +-inf.  Negative gains (polarity), gain 0 and points at or behind F_s are valid.
 * `points` lists the streams' points grouped by stream (each stream's points together, the streams in any order), frames strictly
 * ascending within a stream; the list is copied before the call returns, the work is queued on the batch's stream like the other
 * follow-up calls, and nothing is waited for.  channel_mask 0 means every channel, else bit c selects channel c.
 * Per (stream, channel) the call leaves one ss_gain_channel, taken over all frames [0, F_s) of the stream as they are behind the
 * call (unselected channels of a touched stream are measured as they are; untouched streams read touched = 0, zeros and first_over =
 * UINT64_MAX): n_over counts |y| >= clip_level, infinities included (clip_level = +inf: nothing is over).  Only integer atomics
 * meet across workgroups (a maximum of the float's bits, additions, a 64-bit minimum), so two calls on the same bytes leave the
 * same bytes.  ss_batch_download_gain_stats returns the records of the last call, [stream][channel], and waits for the stream.
 * ss_batch_apply_gain_plan reports tile_frames, the frames one workgroup sweeps: a tile that lies inside one constant stretch of the
 * envelope takes the f32 form, any other the f64 form.  A batch that never calls any of this allocates and launches exactly what it
 * did before.
 * Status codes, all checked before anything is queued: points == NULL with n_points > 0, cfg == NULL, points not grouped by stream,
 * frames not strictly ascending within a stream, stream >= n_streams, a NaN or infinite gain, a frame >= 2^52, a mask bit at or
 * above the channel count, a clip_level that is NaN or <= 0, reserved != 0: SS_ERR_INVALID_ARG; ss_batch_download_gain_stats before
 * the first call: SS_ERR_INVALID_MODE; a `cap` too small: SS_ERR_CAPACITY.  n_points == 0 is valid: it touches nothing and the
 * records read all untouched.
 *
 * ss_batch_download_pcm is the inverse of ss_batch_upload_pcm, in its layout: `count` slots of frames_per_stream * channels samples
 * from stream `first` on, converted on the device into a staging buffer of the call's own and copied out; it waits.  Frames at or
 * behind F_s are written as the format's zero (128 for SS_PCM_U8) and not read.  With scale = 128, 32768, 8388608 or 2^31:
 *     v = x * scale (exact in f32);  with dither v = v + d, one rounded f32 addition;  q = rint(v), halves to even, saturated to
 *     [-scale, scale - 1];  NaN gives 0, +-inf saturates;  SS_PCM_U8 stores q + 128.
 * SS_PCM_F32 copies and SS_PCM_F64 widens; dither is ignored for both.  dither == NULL or kind SS_DITHER_NONE: none.
 * SS_DITHER_TPDF is counter-based, so any sample's value is reproducible on its own; all of it is u32 arithmetic that wraps:
 *     mix(v):  v ^= v >> 16;  v *= 0x7FEB352D;  v ^= v >> 15;  v *= 0x846CA68B;  v ^= v >> 16
 *     i = frame * channels + channel (u64);  k = mix(mix(mix(seed_hi ^ stream) ^ seed_lo) ^ i_hi) ^ i_lo
 *     u1 = mix(k) >> 8;  u2 = mix(k ^ 0x80000000) >> 8;  d = (float)((int32_t)u1 - (int32_t)u2) * 2^-24
 * (seed_hi, seed_lo, i_hi, i_lo: the upper and lower 32 bits; stream: the absolute stream index).  d is exact, lies in (-1, 1) and
 * is triangular: +-1 LSB.  Status codes: an unknown format or dither kind, reserved != 0, first + count beyond the batch, pcm ==
 * NULL with count > 0: SS_ERR_INVALID_ARG; cap_bytes too small: SS_ERR_CAPACITY. */
enum { SS_GAIN_LIMITED_PEAK = 1, SS_GAIN_LIMITED_MAX = 2, SS_GAIN_LIMITED_MIN = 4, SS_GAIN_UNMEASURED = 8 };
enum { SS_DITHER_NONE = 0, SS_DITHER_TPDF = 1 };
typedef struct ss_normalise_target {
    double target_lufs;           /* e.g. -23 (broadcast), -14 (streaming) */
    double max_true_peak_dbtp;    /* the ceiling, e.g. -1; +inf: none */
    double max_gain_db;           /* +inf: no upper clamp */
    double min_gain_db;           /* -inf: no lower clamp */
} ss_normalise_target;            /* 32 bytes */
typedef struct ss_gain_point {
    uint64_t frame;               /* < 2^52 */
    uint32_t stream;
    float    gain;                /* linear, finite; negative flips the polarity */
} ss_gain_point;                  /* 16 bytes */
typedef struct ss_gain_config {
    uint64_t channel_mask;        /* 0: every channel; else bit c selects channel c */
    float    clip_level;          /* linear, > 0; +inf: nothing is over */
    uint32_t reserved;            /* 0 */
} ss_gain_config;                 /* 16 bytes */
typedef struct ss_gain_channel {
    float    sample_peak;         /* the largest finite |y| */
    uint32_t touched;             /* 1: the stream had a point */
    uint64_t n_over;              /* samples with |y| >= clip_level, infinities included */
    uint64_t first_over;          /* the lowest such frame; UINT64_MAX if none */
    uint64_t n_nonfinite;         /* NaN and +-inf */
} ss_gain_channel;                /* 32 bytes */
typedef struct ss_pcm_dither {
    uint64_t seed;
    uint32_t kind;                /* SS_DITHER_NONE, SS_DITHER_TPDF */
    uint32_t reserved;            /* 0 */
} ss_pcm_dither;                  /* 16 bytes */
int ss_normalisation_gain(const ss_normalise_target *t, double loudness_lufs, double peak_linear, double *gain_db, float *gain,
                          uint32_t *limited_by);
double ss_gain_envelope(const ss_gain_point *pts, uint32_t n, uint64_t frame);
int ss_batch_apply_gain(ss_batch *b, const ss_gain_point *points, uint32_t n_points, const ss_gain_config *cfg);
int ss_batch_apply_gain_plan(const ss_batch *b, uint32_t *tile_frames);
/* [stream][channel]; cap_records counts records */
int ss_batch_download_gain_stats(ss_batch *b, ss_gain_channel *out, size_t cap_records);
int ss_batch_download_pcm(ss_batch *b, uint32_t first, uint32_t count, void *pcm, size_t cap_bytes, int format, const ss_pcm_dither *dither);
/* Batch limiter: a look-ahead peak limiter over the resident corpus — the gain a loudness law asks for, applied in the same sweep
 * that shapes only the transients which would cross the ceiling.  Not in the reference.  Feed-forward: every reduction in it is a
 * minimum or a sum of integers, so any evaluation order, tiling or prefix scheme gives the same bits.
 *
 * For one stream of F frames (its own length), the item's f32 gain g, ceiling > 0 (f32), look-ahead L and hold H in frames,
 * ONE = 2^30:
 *  1. Level.  m[n] is an f32 over the SELECTED channels, which are linked: per channel |x[n][c]| (SS_LIMIT_SAMPLE_PEAK) or exactly
 *     what ss_batch_peak_series computes for that frame (SS_LIMIT_TRUE_PEAK: branch 0 and every interpolated branch, each one f32
 *     FMA chain, oldest tap first, fmaxf over the branches so that a NaN branch leaves the others standing, x[n] = 0 for n < 0, the
 *     batch's true_peak_factor rule — at 192 kHz and above there is no interpolation and the two detectors are the same bits).
 *     m[n] is the largest FINITE value among the selected channels, 0 where none is finite: a sample that is NaN or +-inf is not
 *     heard.  A = taps - 1 (11 at factor 4, 23 at factor 2) in true-peak mode with an interpolator, else 0.
 *  2. Required gain.  v = (double)m[n] * (double)fabsf(g), which is exact.  r_q[n] = (uint32)floor((double)ceiling / v * ONE) where
 *     v is finite and v > (double)ceiling, else ONE: a NaN or infinite level (ss_limit_curve takes any) never moves the gain, and
 *     non-finite samples pass through as x * g would leave them.
 *  3. Window minimum.  For any integer k, w_q[k] = min r_q[j] over j in [k - H, k + L + A] and [0, F); ONE over an empty range.
 *     The gain is already down at frame 0 when a peak lies within L frames of the start, and the A extra frames put every frame
 *     whose sample enters an over-ceiling interpolated output at or below that output's required gain.
 *  4. Window sum.  S[n] = sum of w_q[n - j] over j = 0 .. L, a u64 below 2^42; c[n] = (double)S[n] / (double)((L + 1) * ONE), one
 *     f64 division, so a full sum gives exactly 1.  Every window in the sum contains n, hence c[n] <= r_q[n] / ONE, and
 *     c[m] <= r_q[n] / ONE for m in [n - A, n].
 *  5. Output.  y = (float)((double)x * ((double)g * c[n])) for the selected channels of frames [0, F): every operation rounded on
 *     its own (no fused multiply-add).  Where c[n] = 1 this is the plain f32 product x * g, the bits ss_batch_apply_gain writes for
 *     one point of gain g, so a separate ss_batch_apply_gain is not needed.
 * In both detectors every finite |y| <= ceiling holds EXACTLY (floor quantisation, monotone rounding) — in true-peak mode with the
 * exception of the A frames behind an infinite sample of the same channel, whose value is infinite.  The TRUE peak behind the
 * call is not bounded by construction — the gain moves inside the interpolator's support; DESIGN.md section 3.3.6 has it measured.
 * ss_limit_curve is steps 2 to 4 on the host, no device needed: level[0 .. n) are the m[n], `advance` is A; it writes r_q[n], sum[n]
 * and curve[n] = c[n] where the pointer is not NULL.  NULL cfg, NULL level with n > 0, a NaN or infinite gain, a ceiling that is
 * NaN, <= 0 or infinite, lookahead or hold above its maximum, advance > 23: SS_ERR_INVALID_ARG (the other config fields are not
 * read).
 *
 * ss_batch_limit rewrites the resident f32 corpus IN PLACE.  THE OPERATION IS LOSSY: keep the source if the result may have to be
 * taken back.  RESULTS OF EARLIER PASSES, SERIES AND SCANS DESCRIBE THE CORPUS BEFORE THE CALL: run them again for the corpus behind
 * it.  Streams without an item, unselected channels and frames at or behind F stay byte for byte (the latter are never read); a
 * NaN stays a NaN with an unspecified payload.  Items name each stream at most once, in any order; the list is copied before the
 * call returns, the work is queued on the batch's stream like the other follow-up calls, and nothing is waited for.
 * channel_mask 0 means every channel.  The sweep is two launches per group of streams — the detector writes r_q of the tiles that
 * hold a frame over the ceiling to a scratch buffer of 4 bytes x frames_per_stream x group_streams (scratch_bytes bounds it, 0: 256
 * MiB; allocated at the first call, grown only), then the tiles are rewritten — and the groups follow one another when the items
 * do not fit.  ss_batch_limit_plan reports tile_frames, group_streams and the scratch bytes a call with n_items items would use.
 * Per stream the call leaves one ss_limit_stream (untouched streams: touched = 0, first_limited = UINT64_MAX, min_sum = (L + 1) *
 * 2^30) and per (stream, channel) one ss_gain_channel as ss_batch_apply_gain defines it, taken over [0, F) as the corpus stands
 * behind the call; they are the limiter's own (ss_batch_download_gain_stats keeps returning what the last ss_batch_apply_gain
 * left).  Only integer atomics meet across workgroups, so two calls on the same bytes leave the same bytes.
 * Status codes, all checked before anything is queued: cfg == NULL, items == NULL with n_items > 0, a duplicate stream or one >=
 * n_streams, a NaN or infinite gain, a ceiling that is NaN, <= 0 or infinite, a clip_level that is NaN or <= 0, lookahead or hold
 * above its maximum, an unknown detector, a mask bit at or above the channel count, reserved != 0: SS_ERR_INVALID_ARG;
 * ss_batch_download_limit_stats before the first call: SS_ERR_INVALID_MODE; a `cap` too small, a scratch_bytes that cannot hold one
 * stream: SS_ERR_CAPACITY.  n_items == 0 is valid.  A batch that never calls any of this allocates and launches exactly what it did
 * before. */
enum { SS_LIMIT_SAMPLE_PEAK = 0, SS_LIMIT_TRUE_PEAK = 1 };
#define SS_LIMIT_LOOKAHEAD_MAX 2048
#define SS_LIMIT_HOLD_MAX      8192
typedef struct ss_limit_item {
    uint32_t stream;
    float    gain;                /* linear, finite; negative flips the polarity */
} ss_limit_item;                  /* 8 bytes */
typedef struct ss_limit_config {
    uint64_t channel_mask;        /* 0: every channel; else bit c selects channel c */
    float    ceiling;             /* linear, > 0, finite */
    float    clip_level;          /* of the per-channel records: linear, > 0; +inf: nothing is over */
    uint32_t lookahead, hold;     /* L and H in frames */
    uint32_t detector;            /* SS_LIMIT_SAMPLE_PEAK, SS_LIMIT_TRUE_PEAK */
    uint32_t reserved;            /* 0 */
    uint64_t scratch_bytes;       /* 0: the default of 256 MiB */
} ss_limit_config;                /* 40 bytes */
typedef struct ss_limit_stream {
    uint64_t n_limited;           /* frames with S[n] < (L + 1) * 2^30 */
    uint64_t first_limited;       /* the lowest such frame; UINT64_MAX if none */
    uint64_t min_sum;             /* min S[n]; (L + 1) * 2^30 if none: the lowest gain is min_sum / ((L + 1) * 2^30) */
    uint32_t touched;             /* 1: the stream had an item */
    uint32_t reserved;
} ss_limit_stream;                /* 32 bytes */
/* host arithmetic; any output may be NULL */
int ss_limit_curve(const float *level, uint64_t n, float gain, const ss_limit_config *cfg, uint32_t advance,
                   uint32_t *r_q, uint64_t *sum, double *curve);
int ss_batch_limit(ss_batch *b, const ss_limit_item *items, uint32_t n_items, const ss_limit_config *cfg);
int ss_batch_limit_plan(const ss_batch *b, const ss_limit_config *cfg, uint32_t n_items,
                        uint32_t *tile_frames, uint32_t *group_streams, uint64_t *scratch_bytes);
/* streams [n_streams] and channels [stream][channel]; either may be NULL; waits */
int ss_batch_download_limit_stats(ss_batch *b, ss_limit_stream *streams, size_t cap_streams,
                                  ss_gain_channel *channels, size_t cap_records);
/* Batch resampler: sample-rate conversion of the resident corpus by a rational factor L / M, one batch into another — a centred
 * Kaiser-windowed-sinc polyphase FIR in f32.  Not in the reference.  Every output sample is ONE chain of fused multiply-adds in a
 * fixed order, so its bits do not depend on tile, slot, batch size or neighbouring streams; ss_resample_host is that chain with
 * libm's fmaf — the definition in bits — and needs no device.
 *
 * Plan rule (ss_resample_plan_make; all in f64, each operation as written):
 *   A = attenuation_db, 0 meaning 100; passband, 0 meaning 20000.0 / 22050.0;
 *   g = gcd(in_rate, out_rate), up = L = out_rate / g, down = M = in_rate / g;
 *   cutoff = fc = 0.5 * min(1.0, (double)L / (double)M)                       cycles per INPUT sample;
 *   delta = 2.0 * (1.0 - passband) * fc                                        the transition width: the response is flat up to
 *       passband x the lower Nyquist and stopped from (2 - passband) x it, so aliasing falls into the transition band only;
 *   beta = 0.1102 * (A - 8.7);
 *   taps = T = ceil((A - 7.95) / (14.36 * delta)), rounded up to a multiple of 4.
 *   Equal rates, a zero rate, A outside [40, 140], passband outside [0.5, 0.99], a NaN, out == NULL: SS_ERR_INVALID_ARG;
 *   L * T > SS_RESAMPLE_TAPS_MAX (24576 floats, 96 KB: the table and a tile share the 160 KiB of a CU's LDS): SS_ERR_UNSUPPORTED.
 * Taps (ss_resample_taps; [L][T] f32, computed in f64): tap k of phase p is h(t) at t = j / L input samples, j = (k - T/2 + 1) * L - p:
 *   h(t) = 2 fc * sinc(2 fc t) * I0(beta * sqrt(max(0, 1 - (2 t / T)^2))) / I0(beta),    sinc(x) = sin(pi x) / (pi x), 1 at 0.
 *   Where L >= M (2 fc = 1) the sinc is taken on the integer j: exactly 0 where j is a non-zero multiple of L, exactly 1 at j = 0 —
 *   PHASE 0 OF AN UPSAMPLING TABLE IS THE UNIT IMPULSE IN BITS.  Each phase is scaled to sum 1 in f64, then rounded to f32.
 *   cap_floats < L * T: SS_ERR_CAPACITY.
 * Output n of channel c of a stream of F_in frames x:  q = n * M (u64), base = q / L, p = q % L,
 *   acc = 0;  for k = 0 .. T - 1 in that order:  acc = fmaf(taps[p][k], x[base - T/2 + 1 + k][c], acc);   x outside [0, F_in) is 0.
 *   The filter is centred: no latency is added.  Non-finite samples follow IEEE through the chain; an output whose T-frame window
 *   holds none is unaffected.
 * Length (ss_resample_length): the number of n with n * M < F_in * L, ceil(F_in * L / M); 0 for 0.
 * ss_resample_host writes outputs [first_out, first_out + n_out) as [n_out][channels]; taps is what ss_resample_taps gave.  A null
 *   pointer (in: with frames_in > 0; out: with n_out > 0), channels == 0, first_out + n_out beyond the length: SS_ERR_INVALID_ARG.
 *
 * ss_batch_resample converts every stream of src, each at its own length (ss_batch_set_lengths respected), into the same slot of
 * dst and gives dst the lengths ss_resample_length(F_s), exactly as ss_batch_set_lengths(dst, ...) would (a stream of 0 frames
 * stays 0).  Floats of a dst slot at or behind the output length keep their bytes; src is read only, and no float outside [0, F_s)
 * of a stream's own slot is read.  Checked before anything is queued or changed: a null pointer, src == dst, different devices,
 * channel or stream counts, src's rate != in_rate, dst's rate != out_rate, reserved != 0, a plan that ss_resample_plan_make would
 * not have made from its own rates, attenuation_db and passband: SS_ERR_INVALID_ARG; dst's frames_per_stream below the longest
 * output: SS_ERR_CAPACITY.  The kernel is queued on dst's stream behind what src's stream holds, and src's stream then waits for
 * it, so work queued on src later (ss_batch_apply_gain ...) cannot overtake the read; the host waits for what ss_batch_set_lengths
 * on dst waits for (dst's stream), and the first call of dst with a plan other than its last also copies that plan's table to the
 * device before it returns: nothing else.  Two calls leave the same bytes.  There is no statistics record: dst is a batch, and its
 * peak series, signal scan and pass are the statistics.  The taps table of the last plan stays on the device with dst.
 * ss_batch_resample_plan reports how a call would cut the streams: a workgroup converts tile_out_frames = R * L outputs from
 * tile_in_frames = R * M inputs and their taps - 1 frames of surroundings. */
#define SS_RESAMPLE_TAPS_MAX 24576
typedef struct ss_resample_plan {
    uint32_t in_rate, out_rate;
    uint32_t up, down;            /* L = out_rate / g, M = in_rate / g, g = gcd */
    uint32_t taps;                /* T: taps per phase, a multiple of 4 */
    uint32_t reserved;            /* 0 */
    double   attenuation_db;      /* A */
    double   passband;            /* fraction of the lower Nyquist that is flat */
    double   beta, cutoff;        /* Kaiser beta; fc in cycles per INPUT sample */
} ss_resample_plan;               /* 56 bytes */
int ss_resample_plan_make(uint32_t in_rate, uint32_t out_rate, double attenuation_db, double passband, ss_resample_plan *out);
int ss_resample_taps(const ss_resample_plan *p, float *taps, size_t cap_floats);
uint64_t ss_resample_length(const ss_resample_plan *p, uint64_t frames_in);
int ss_resample_host(const ss_resample_plan *p, const float *taps, const float *in, uint64_t frames_in, uint32_t channels,
                     uint64_t first_out, uint64_t n_out, float *out);
int ss_batch_resample(ss_batch *src, ss_batch *dst, const ss_resample_plan *p);
int ss_batch_resample_plan(const ss_batch *src, const ss_resample_plan *p, uint32_t *tile_out_frames, uint32_t *tile_in_frames);
/* corpus histograms summed over this batch's streams: 1000 block-energy bins
 * followed by 1000 short-term bins (u64 each).  `_device` copies them into a
 * caller-owned device buffer (e.g. the send buffer of an RCCL all-reduce). */
int ss_batch_histograms(ss_batch *b, uint64_t *out2000);
int ss_batch_histograms_device(ss_batch *b, void *dst_device_2000_u64);
/* A7/A8 on a (summed / all-reduced) histogram: ebur128 loudness_global_multiple
 * and loudness_range_multiple semantics.  Host-side, O(1000). */
double ss_corpus_integrated_lufs(const uint64_t *block_hist1000);
double ss_corpus_loudness_range(const uint64_t *st_hist1000);

/* ------------------------------------------------------------------------- *
 *  Meter banks: N independent live EBU R128 meters (one channel count, rate and true-peak rule) advanced together.  Stream s
 *  of a bank behaves exactly like an ss_analyzer fed the same blocks (true peak in SS_TP_ARITH_F32, the handle's default); a
 *  call costs a time-domain launch and a gating launch for ALL streams (calls longer than 32 sub-blocks are cut into pieces,
 *  as ss_add_samples cuts them), a read one launch and one copy.  A non-finite sample poisons its own stream only.
 *  The streams need not move together: the _ragged calls give every stream its own frame count per call, none included.
 *  Device memory per stream, laid out as a handle holds its meter: the filter state (9.3 KB), a 96-slot sub-block ring, the
 *  filtered-sample ring of 3 s (rounded up to a whole 100 ms sub-block) x channels f64, two 1000-bin u64 histograms:
 *  about 2.33 MB at 48 kHz stereo — 2.4 GB for 1024 streams.
 *  Status codes: channels / rate outside EbuR128::new's range SS_ERR_NOMEM; a bad pointer, stream index, stride or format
 *  SS_ERR_INVALID_ARG; a `cap` too small SS_ERR_CAPACITY; no device SS_ERR_DEVICE.  frames == 0 is a no-op.
 * ------------------------------------------------------------------------- */
typedef struct ss_meter_bank ss_meter_bank;
typedef struct ss_meter_reading {
    double momentary;        /* loudness_momentary(), LUFS (-inf for silence)                                      */
    double shortterm;        /* loudness_shortterm(); NaN at rates where the crate's call fails (3 s < 30 sub-blocks) */
    double integrated;       /* loudness_global()                                                                  */
    double loudness_range;   /* loudness_range()                                                                   */
    double true_peak[2];     /* channels 0, 1: max(true, sample) like ss_get_true_peak; [1] NaN if mono           */
    double sample_peak[2];
    uint64_t frames;         /* frames fed since this stream's last reset                                          */
} ss_meter_reading;          /* 72 bytes */
/* true_peak_factor: 0 the crate's rule for the rate, 2 or 4 forced (ss_analyzer_set_true_peak_factor) */
int ss_meter_bank_create(uint32_t n_streams, uint32_t channels, uint32_t rate, int32_t true_peak_factor, ss_meter_bank **out);
void ss_meter_bank_destroy(ss_meter_bank *m);
/* every stream gets `frames` frames: pcm is [stream][frame][channel] f32, copied before the call returns */
int ss_meter_bank_add(ss_meter_bank *m, const float *pcm, uint64_t frames);
/* producers already on the GPU: stream s starts at pcm_device + s * stream_stride_floats (>= frames * channels); only
 * queued — the buffer must stay unchanged until the next call that waits (ss_meter_bank_read, _peaks, _histograms) */
int ss_meter_bank_add_device(ss_meter_bank *m, const float *pcm_device, uint64_t frames, uint64_t stream_stride_floats);
/* raw little-endian interleaved PCM of an ss_pcm_format, [stream][frame][channel], converted on the device */
int ss_meter_bank_add_pcm(ss_meter_bank *m, const void *pcm, uint64_t frames, int format);
/* Ragged adds: stream s gets frames[s] frames — inputs that arrive in packets of different sizes, pause, start, stop or drift
 * against each other.  `frames` is a host array of n_streams entries, copied before the call returns.  Afterwards stream s is in
 * the state an ss_analyzer of the bank's shape is in after one ss_add_samples of those frames[s] frames (the bank's contract, per
 * stream); a stream with frames[s] == 0 is not touched at all — its readings, histograms, peaks and spectrum history stay byte
 * for byte — and an all-zero call is a no-op.  A call launches the time domain at most twice per piece of 32 sub-blocks (the
 * streams that take up to one tile of the kernel, and the longer ones: each runs the form a handle runs for that length) and the
 * gating once where some stream completes a sub-block.
 * Checked before anything is advanced or copied: frames == NULL, pcm[s] == NULL where frames[s] > 0, an unknown format, a stride
 * below max(frames) * channels SS_ERR_INVALID_ARG; more than 2^40 samples in one stream or in all SS_ERR_NOMEM (ss_batch_create's rule).
 * stream s's frames are pcm[s], interleaved f32 (pcm[s] may be NULL where frames[s] == 0); the inputs are staged tightly packed
 * and copied, with the lengths, in one transfer before the call returns */
int ss_meter_bank_add_ragged(ss_meter_bank *m, const float *const *pcm, const uint64_t *frames);
/* the same for raw little-endian PCM of an ss_pcm_format, converted on the device */
int ss_meter_bank_add_ragged_pcm(ss_meter_bank *m, const void *const *pcm, const uint64_t *frames, int format);
/* producers on the GPU: stream s's frames[s] frames start at pcm_device + s * stream_stride_floats (stride >= max(frames) *
 * channels); only queued, as ss_meter_bank_add_device */
int ss_meter_bank_add_ragged_device(ss_meter_bank *m, const float *pcm_device, const uint64_t *frames, uint64_t stream_stride_floats);
/* resets the listed streams (streams == NULL: all of them), as EbuR128::reset; the others are untouched */
int ss_meter_bank_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count);
/* one record per stream for the state after the last add; waits; one device-to-host copy */
int ss_meter_bank_read(ss_meter_bank *m, ss_meter_reading *out, uint32_t cap_streams);
/* every channel of one stream: true_pk[c] = max(true, sample) peak, sample_pk[c] (either may be NULL); cap < channels: SS_ERR_CAPACITY */
int ss_meter_bank_peaks(ss_meter_bank *m, uint32_t stream, double *true_pk, double *sample_pk, uint32_t cap_channels);
/* one stream's histograms: 1000 block-energy bins followed by 1000 short-term bins */
int ss_meter_bank_histograms(ss_meter_bank *m, uint32_t stream, uint64_t *out2000);

/* Spectra of a bank: get_fft of every stream's newest SS_BANK_SPECTRUM_N frames, mid and side for stereo banks
 * (the reference's microphone tick, tui.rs:1427-1445), one row per channel otherwise (as ss_batch does; the reference's mono
 * device is a stereo bank fed a zero right channel, audio_capture.rs).  One launch transforms every row of every stream.
 *  - The history is the raw input, not the meter: ss_meter_bank_reset leaves it alone (so does the reference's
 *    analyzer.reset()), and a non-finite sample refuses a row only while it lies inside that row's window.  Every stream has
 *    its own frame counter, which places its window: [fed_s - 16384, fed_s) for what stream s itself was given, by uniform and
 *    ragged adds alike (a stream given nothing keeps its window); a call longer than the window keeps its newest
 *    SS_BANK_SPECTRUM_N frames.  The window starts full of zeros, as the reference's capture ring does (tui.rs:1783-1784).
 *  - Refusals follow the crate's order on the windowed signal (for stereo the f32 mid / side values): a windowed NaN (an
 *    infinite sample under a zero window weight included; +inf in L with -inf in R is a NaN mid) SS_ERR_NAN, else a windowed
 *    infinity (two finite samples near FLT_MAX overflow the mid) SS_ERR_INFINITY, else a non-finite dB value (the magnitude's
 *    square overflowed) SS_ERR_SCALING — each exactly what ss_get_fft returns for that window.  A refused row is all NaN.
 *  - Not enabled SS_ERR_INVALID_MODE; a `cap` too small SS_ERR_CAPACITY; bad cols / gain mode SS_ERR_INVALID_ARG. */
#define SS_BANK_SPECTRUM_N SS_TICK_WINDOW   /* 16384 frames: tui.rs:1431 / :1488 */
/* enable != 0: a zeroed history of the newest SS_BANK_SPECTRUM_N frames of every stream (4 * channels * 16384 bytes per
 * stream); frames added from now on enter it.  Enabling again starts from zeros; enable == 0 frees it.  SS_ERR_FREQ_LIMIT
 * where get_fft would refuse (20000 > rate / 2 as f32), before anything is allocated.  A bank without the spectrum launches
 * exactly what it did before. */
int ss_meter_bank_spectrum_enable(ss_meter_bank *m, int enable);
/* rows per stream (2 = mid, side for stereo banks, otherwise one per channel), retained bins, and per bin the chart x (the
 * first element of get_fft's pairs) and the f64 pink compensation (either array may be NULL) */
int ss_meter_bank_spectrum_layout(const ss_meter_bank *m, uint32_t *rows_per_stream, uint32_t *n_bins,
                                  double *chart_x, double *pink, uint32_t cap_bins);
/* the window [fed - 16384, fed) of every stream after the last add: rows [stream][row][n_bins] f32 = the dBFS value BEFORE pink
 * compensation, so that (double)row[i] + pink[i] is, bit for bit, the second element of the pair ss_get_fft returns for the same
 * samples; status[stream * rows + row] = SS_OK or the refusal above.  Waits; one launch and one copy. */
int ss_meter_bank_spectrum(ss_meter_bank *m, float *rows, size_t cap_floats, int32_t *status, uint32_t cap_rows);
/* the same windows reduced on the device to `cols` chart columns (1 .. 512) by ss_batch_render_spectrum's rule applied to
 * v[i] = (float)((double)row[i] + pink[i]): max over the column of clamp(v + gain, -100, 0) in f32, NaN for a column without
 * a bin or a refused row; gain_mode SS_GAIN_FIXED (gain_db) or SS_GAIN_REFERENCE (-13 - (float)integrated of each stream's
 * meter after the last add, as ss_meter_bank_read returns it).  out is [stream][row][cols]; the rows are never stored. */
int ss_meter_bank_spectrum_columns(ss_meter_bank *m, uint32_t cols, int gain_mode, float gain_db,
                                   float *out, size_t cap_floats, int32_t *status, uint32_t cap_rows);

/* Tracked spectra of a bank: the two curves every real-time analyser draws over the instantaneous row — an
 * exponentially averaged trace and a peak-hold trace that falls back after a hold time — kept on the device for every row of
 * every stream and advanced by ss_meter_bank_spectrum_track on each stream's OWN clock.  The live counterpart of
 * ss_batch_spectrum_stats.  Not in the reference.
 *  Definitions.  rate: the bank's sample rate.  v[i]: what ss_meter_bank_spectrum would return at this moment for row (s, r), bin
 *  i (f32 dBFS before pink compensation).  fed_s: stream s's own frame counter, the one that places its window (what uniform and
 *  ragged adds gave that stream).  Every row keeps last, the fed_s of its last accepted update, and updates, a u32 count of its
 *  accepted updates since its reset (it stays at 0xFFFFFFFF).  For one _track call, delta = fed_s - last.
 *  - Which rows a _track call touches.  A row with state and delta == 0 is not touched at all — nothing arrived for that stream,
 *    its state stays byte for byte ("a stream given nothing keeps its window").  A row whose status at this moment is a refusal
 *    (SS_ERR_NAN, SS_ERR_INFINITY, SS_ERR_SCALING) is not touched either: last stays, so the next accepted update decays over the
 *    whole gap.  Rows are independent: a refused channel row leaves the other rows of its stream alone.
 *  - First accepted update (updates == 0; delta plays no part): P[i] = p[i], peak[i] = v[i], age[i] = 0 for every bin.
 *  - Average.  p[i] = exp2f(v[i] * log2(10)/10), the f32 power as ss_batch_spectrum_stats forms it, widened to f64;
 *    alpha = -expm1(-delta / (rate * average_tau_s)) in f64 (exactly 1 for average_tau_s == 0); P[i] += alpha * (p[i] - P[i]) in
 *    f64; avg_db[i] = (float)(10 log10 P[i]), the logarithm in f64.
 *  - Peak hold.  age[i] counts frames in a u32 and stays at 0xFFFFFFFF; hold_frames = (uint64_t)(hold_s * rate + 0.5), and the peak
 *    never falls for hold_s = +inf.  hold_db[i] = (float)((double)peak - decay_db_per_s * ((double)over / (double)rate)) with
 *    over = max(0, age - hold_frames): f64, in exactly that order, without a fused multiply-add — the same IEEE expression on
 *    the host gives the same bits.  Update: age = sat(age + delta); D = hold_db of the new age; v[i] >= D captures (peak = v[i],
 *    age = 0), otherwise peak and the new age stay.  What is reported afterwards is hold_db of the state as it stands.
 *  - ss_meter_bank_reset resets the meters, not the display: it leaves the tracked state alone as it leaves the history alone.
 *    ss_meter_bank_spectrum_enable, with either argument, drops the tracked state and turns tracking off.
 *    ss_meter_bank_spectrum and _columns neither advance nor read the state: their results and launches are unchanged, and a bank
 *    that never enables tracking allocates and launches exactly what it did before.
 *  - Device memory: 16 bytes per bin (P f64, peak f32, age u32), bins rounded up to a multiple of four per row, plus one row
 *    buffer of the transform — 20 bytes per bin, 6820 bins at 48 kHz: about 224 MB of state and 56 MB of rows for 1024 stereo
 *    streams.
 *  - Status codes: before _track_enable SS_ERR_INVALID_MODE; a `cap` too small SS_ERR_CAPACITY; a bad stream index, cols outside
 *    1 .. 512 or an unknown gain mode SS_ERR_INVALID_ARG. */
typedef struct ss_spectrum_ballistics {
    double average_tau_s;    /* time constant of the exponential POWER average, >= 0, finite; 0: the average is the newest row */
    double hold_s;           /* how long a captured peak stays before it falls, >= 0; +inf: held for ever */
    double decay_db_per_s;   /* fall rate once the hold has run out, >= 0, finite */
} ss_spectrum_ballistics;   /* 24 bytes */
/* cfg != NULL: empty state for every row (enabling again, with the same or new parameters, starts from empty state);
 * SS_ERR_INVALID_ARG for a negative or NaN parameter, an infinite average_tau_s or decay_db_per_s, then SS_ERR_INVALID_MODE
 * without the spectrum history — both before anything is allocated.  cfg == NULL: tracking off, the state freed. */
int ss_meter_bank_spectrum_track_enable(ss_meter_bank *m, const ss_spectrum_ballistics *cfg);
/* advances every row's state to the windows as they stand: the transform's row launch into a device buffer and one elementwise
 * launch behind it.  Only queued: no copy, no wait. */
int ss_meter_bank_spectrum_track(ss_meter_bank *m);
/* empties the listed streams' rows (streams == NULL: all): updates = 0, the next accepted update seeds them */
int ss_meter_bank_spectrum_track_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count);
/* avg_db and hold_db as rows [stream][row][n_bins] f32, before pink compensation like ss_meter_bank_spectrum's (either may be
 * NULL: that curve is neither formed nor copied), and updates[stream * rows + row] (may be NULL).  A row with updates == 0
 * reads all NaN.  Waits; one launch and one copy. */
int ss_meter_bank_spectrum_tracked(ss_meter_bank *m, float *avg_rows, float *hold_rows, size_t cap_floats,
                                   uint32_t *updates, uint32_t cap_rows);
/* both curves reduced on the device to `cols` chart columns by ss_meter_bank_spectrum_columns' rule applied to
 * x = (float)((double)curve[i] + pink[i]): max over the column of clamp(x + gain, -100, 0) in f32, NaN for a column without a
 * bin or a row without state; gain_mode as there.  avg_cols / hold_cols are [stream][row][cols] (either may be NULL), updates
 * as above; the full rows never leave the device.  Waits; one launch (two with SS_GAIN_REFERENCE) and one copy. */
int ss_meter_bank_spectrum_tracked_columns(ss_meter_bank *m, uint32_t cols, int gain_mode, float gain_db,
                                           float *avg_cols, float *hold_cols, size_t cap_floats,
                                           uint32_t *updates, uint32_t cap_rows);

/* Signal watch of a bank: the live counterpart of ss_batch_signal_scan — is this input silent and since when, is
 * it clipping now, how often and for how long at a time, did a non-finite sample arrive, is a DC offset building up — kept on the
 * device for every stream and advanced by every add call, whichever of the six forms it has.  Not in the reference.
 *  The definition is the batch scan's, so there is one: after any sequence of adds, stream s's records equal what
 *  ss_batch_signal_scan defines for ONE stream that is the concatenation of every frame stream s was given since its watch was last
 *  reset, with F_s = frames.  The predicates, runs and minima are those of the batch scan's comment above, unchanged: a frame is
 *  silent iff fabsf(x) <= silence_threshold on every channel, a sample clipped iff fabsf(x) >= clip_level, f32 comparisons as
 *  written, a NaN holds neither predicate, a run is a maximal stretch of frames on which a predicate holds.  Frame numbers count
 *  from the stream's watch reset.  Consequences:
 *  - The run open at the newest frame is a run: it counts in silence_runs / clip_runs where it reaches the minimum, it is
 *    trailing_silence (the dead-air figure) / trailing_clip, and it takes part in longest_*; ties go to the lowest frame.
 *  - How the material was cut into calls changes no integer: one call, 10 ms blocks, one frame at a time and ragged calls agree.
 *  - The two f64 sums add the kernel's tiles (ss_meter_bank_signal_watch_plan's tile_frames frames of one call at most) in
 *    ascending order behind the state.  Their order is fixed by the call sequence and the plan, not by timing; there are no
 *    floating-point atomics: two banks fed the same calls agree byte for byte.  Differently cut feeds agree within the bound of
 *    f64 summation — (N - 1) u / (1 - (N - 1) u) times the sum of |x| (of x^2), u = 2^-53 — not in bits.
 *  - DC or RMS of the last interval: difference two reads (sum, sum_sq, frames and nonfinite are all running totals).
 *  - For the PCM forms the predicates see the f32 values the meter sees, ss_pcm_decode's.
 *  - A stream given 0 frames in a call is not touched, its state and records stay byte for byte, and an all-zero call launches
 *    nothing.  A non-finite sample touches its own stream's counters only.
 *  - ss_meter_bank_reset resets the meters, not the watch: it leaves the watch alone as it leaves the spectrum history and the
 *    tracked state alone.  The watch moves nothing else: readings, peaks, histograms and spectra are byte for byte what they are
 *    without it, and a bank that never enables it allocates and launches exactly what it did before.
 *  - Cost: one launch per add call (one workgroup per stream walks the stream's frames of that call tile by tile: a long call is
 *    walked serially), none for a read.  Device memory: 112 bytes of state per (stream, channels + 1), and the records.
 *  Configuration is ss_signal_scan_config with ss_batch_signal_scan's refusals; max_events must be 0 — there is no event list yet,
 *  a polling host reads trailing_*, last_clip_frame and the counters — a non-zero max_events is SS_ERR_INVALID_ARG.
 *  Status codes: _plan, _reset or the read before _enable SS_ERR_INVALID_MODE; a bad stream index SS_ERR_INVALID_ARG with nothing
 *  reset; a `cap` too small SS_ERR_CAPACITY with nothing written. */
typedef struct ss_stream_watch {
    uint64_t silent_frames;       /* the seven fields of ss_stream_scan, over the frames watched */
    uint64_t leading_silence;
    uint64_t trailing_silence;    /* frames of the silence run that holds the newest frame, else 0: dead air since then */
    uint64_t longest_silence;
    uint64_t longest_silence_at;
    uint64_t silence_runs;
    uint64_t clip_runs;
    uint64_t frames;              /* frames watched since this stream's watch reset */
} ss_stream_watch;                /* 64 bytes */
typedef struct ss_channel_watch {
    double   sum, sum_sq;         /* the eight fields of ss_channel_scan, over the frames watched */
    uint64_t nonfinite;
    uint64_t first_nonfinite;
    uint64_t clipped_samples;
    uint64_t longest_clip;
    uint64_t longest_clip_at;
    uint64_t clip_runs;
    uint64_t trailing_clip;       /* frames of the clip run that holds the newest frame, else 0 */
    uint64_t last_clip_frame;     /* frame of the newest clipped sample; UINT64_MAX if none */
} ss_channel_watch;               /* 80 bytes */
/* cfg != NULL: empty state for every stream (enabling again, with the same or new parameters, starts empty); cfg == NULL: the watch
 * off, its state freed.  Refusals before anything is allocated or changed, so a refused call leaves the previous watch as it was.
 * With frames == 0 every field of a record is zero or "none". */
int ss_meter_bank_signal_watch_enable(ss_meter_bank *m, const ss_signal_scan_config *cfg);
/* frames one tile of the kernel holds (ss_batch_signal_scan_plan's rule for the bank's channel count) */
int ss_meter_bank_signal_watch_plan(const ss_meter_bank *m, uint32_t *tile_frames);
/* empties the listed streams' watch (streams == NULL: all); the others are untouched */
int ss_meter_bank_signal_watch_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count);
/* the records for the state after the last add; either array may be NULL; channel records are [stream][channel].  Waits; no
 * launch (the adds leave the records behind) and one copy. */
int ss_meter_bank_signal_watch(ss_meter_bank *m, ss_stream_watch *streams_out, uint32_t cap_streams,
                               ss_channel_watch *channels_out, size_t cap_records);

/* Pair watch of a bank: the live counterpart of ss_batch_pair_series and ss_batch_pair_regions — are this input's
 * channels in phase, how is it balanced, what would a mono fold-down lose, and since when is it out of phase — kept on the device
 * for every stream and channel pair and advanced by every add call, whichever of the six forms it has.  Not in the reference.
 *  S = s100 = (rate + 5) / 10, as the batch series has it.  Frames and entries of a stream count from that stream's pair-watch reset.
 *  Entry j covers the stream's frames [j S, (j + 1) S), whichever calls they arrived in.  An entry is complete when its S-th frame
 *  has arrived; E is the number of complete entries.  The open_frames frames behind the last complete entry belong to no record
 *  yet: there is no partial tail entry in the live form.  A complete entry's ss_pair_entry for pair (a, b) is, bit for bit, what the
 *  batch series' general form computes for the same S frames: frame i of the entry belongs to lane i mod 256; a lane adds its frames
 *  in ascending order from +0 with one fused multiply-add per product; a frame in which x_a or x_b is NaN or infinite adds +0 and is
 *  counted in `skipped`; the 64 lanes of a wave meet in the xor butterfly at distances 32 .. 1; the four waves are added in wave
 *  order.  How the material was cut into calls changes no bit of any entry: one call, 10 ms blocks, one frame at a time and ragged
 *  calls agree, and two banks fed the same calls agree byte for byte.
 *  Lane state: per (stream, pair) the open entry's 256 lane sums x 3 f64 persist on the device between calls (6 KB per pair); a
 *  call loads them where open_frames > 0, each lane goes on adding its own frames, and lanes meet only when the entry completes.
 *  Ring: the newest R = window_entries complete entries per (stream, pair) stay on the device (32 R bytes), 1 <= R <=
 *  SS_BANK_PAIR_WINDOW_MAX (60 s).
 *  Record, per (stream, pair), as the state stands after the last add:
 *  - window: the sums, frames and skipped of the newest window_count = min(R, E) complete entries, added in ascending entry order
 *    from +0, one rounded f64 addition each: ss_batch_pair_regions' rule for the region [E - window_count, E);
 *  - total: the same over [0, E), kept as a running sequential sum (each entry added as it completes);
 *  - n_active, n_below, first_below, longest_below, longest_below_at, below_runs: ss_region_pair's fields for the region [0, E),
 *    with the ACTIVE and BELOW predicates of the comment above (threshold, power_floor, min_run), stepped once per completed entry;
 *  - trailing_below: the entries of the run that holds entry E - 1, else 0 — out of phase since then.  "None" is UINT64_MAX.
 *  The caller forms correlation, balance and mono loss from `window` or `total` as from a region's sums.
 *  - ss_meter_bank_reset resets the meters, not the pair watch.  A stream given 0 frames in a call keeps its state and records byte
 *    for byte, and an all-zero call launches nothing.  A non-finite sample touches its own stream's counters only.  The pair watch
 *    moves nothing else: readings, peaks, histograms, spectra and signal-watch records are byte for byte what they are without it,
 *    and a bank that never enables it allocates and launches exactly what it did before.  For the PCM forms the sums see the f32
 *    values the meter sees, ss_pcm_decode's.
 *  - Cost: one launch per add call (one workgroup per stream walks the stream's frames of that call entry by entry: a long call is
 *    walked serially), none for a read.
 *  Status codes, all checked before anything is allocated or queued, so a refused call leaves the previous watch as it was: a or b
 *  >= channels, n_pairs > 16, pairs == NULL with n_pairs > 0, the default pair on a mono bank, a NaN threshold or |threshold| >= 1, a
 *  NaN or negative power_floor, min_run == 0, window_entries == 0 or > SS_BANK_PAIR_WINDOW_MAX, a bad stream index:
 *  SS_ERR_INVALID_ARG; _plan, _reset or either read before _enable: SS_ERR_INVALID_MODE; a `cap` too small: SS_ERR_CAPACITY, with
 *  nothing written. */
#define SS_BANK_PAIR_WINDOW_MAX 600
typedef struct ss_pair_sums {
    double   s_aa, s_bb, s_ab;    /* the entries' sums added in entry order */
    uint64_t frames, skipped;
} ss_pair_sums;                   /* 40 bytes */
typedef struct ss_pair_watch_config {
    double   threshold;           /* an entry is BELOW iff its correlation < threshold; -1 < threshold < 1 */
    double   power_floor;         /* an entry is ACTIVE iff s_aa + s_bb > power_floor * frames (linear power per frame, >= 0) */
    uint32_t min_run;             /* >= 1: runs of consecutive active BELOW entries at least this long are counted */
    uint32_t window_entries;      /* R: 1 .. SS_BANK_PAIR_WINDOW_MAX complete entries in the window and the ring */
} ss_pair_watch_config;           /* 24 bytes */
typedef struct ss_pair_watch {
    ss_pair_sums window;          /* the newest window_count complete entries */
    ss_pair_sums total;           /* every complete entry since the stream's pair-watch reset */
    uint64_t entries;             /* E: complete entries */
    uint64_t n_active, n_below;   /* n_below counts active entries only */
    uint64_t first_below;         /* entry index of the first active BELOW entry; UINT64_MAX if none */
    uint64_t longest_below;       /* entries of the longest run, of any length; ties go to the lowest entry; 0 if none */
    uint64_t longest_below_at;    /* entry index of its first entry; UINT64_MAX if none */
    uint64_t below_runs;          /* runs of at least min_run */
    uint64_t trailing_below;      /* entries of the run that holds entry E - 1, else 0 */
    uint32_t open_frames;         /* frames behind the last complete entry: in no record yet */
    uint32_t window_count;        /* min(R, E) */
    uint64_t reserved;            /* 0 */
} ss_pair_watch;                  /* 160 bytes */
/* cfg != NULL: empty state for every stream (enabling again, with the same or new parameters, starts empty); cfg == NULL: the watch
 * off, its state freed.  pairs == NULL with n_pairs == 0 is the one pair (0, 1); the call copies `pairs`. */
int ss_meter_bank_pair_watch_enable(ss_meter_bank *m, const ss_channel_pair *pairs, uint32_t n_pairs, const ss_pair_watch_config *cfg);
/* *lanes = 256 (frame i of an entry belongs to lane i mod *lanes), the window and the pairs of the watch as enabled */
int ss_meter_bank_pair_watch_plan(const ss_meter_bank *m, uint32_t *lanes, uint32_t *window_entries, uint32_t *n_pairs);
/* empties the listed streams' pair watch (streams == NULL: all); the others are untouched */
int ss_meter_bank_pair_watch_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count);
/* the records for the state after the last add, [stream][pair]; cap_records counts records.  Waits; no launch (the adds leave the
 * records behind) and one copy through page-locked memory. */
int ss_meter_bank_pair_watch(ss_meter_bank *m, ss_pair_watch *out, size_t cap_records);
/* the ring of one stream: its newest *n_entries = min(R, E) complete entries in ascending order, [entry][pair], the first of them
 * entry *first_entry (both optional); cap_entries counts entries (records / n_pairs).  Waits; no launch and one copy. */
int ss_meter_bank_pair_watch_entries(ss_meter_bank *m, uint32_t stream, ss_pair_entry *out, size_t cap_entries,
                                     uint64_t *first_entry, uint32_t *n_entries);

/* ------------------------------------------------------------------------- *
 *  Multi-GPU: one process per GPU, streams sharded over the ranks, and exactly ONE exchange —
 *  the SUM all-reduce of the two 1000-bin u64 histograms for the corpus-level integrated-LUFS gate
 *  (ebur128 loudness_global_multiple semantics; the reference app has no collective).  The library talks to
 *  RCCL itself (librccl is opened at ss_comm_init; ncclAllReduce(buf, buf, 2000, ncclUint64, ncclSum) on the
 *  batch's stream, over xGMI) — no PyTorch, no MPI.
 *    SS_COMM_RCCL      device buffers, RCCL
 *    SS_COMM_HOST_TCP  the same calls staged through host memory over loopback TCP: CPU tests of the rank
 *                      logic, and ranks that share one GPU
 *  Rendezvous (one node): rank 0 publishes the RCCL unique id (and its TCP port) in `rendezvous_file`, the other
 *  ranks poll for it.  ss_comm_init_from_env derives rank / world from RANK / WORLD_SIZE and the file name from
 *  the launcher's process id and MASTER_PORT (torchrun as a launcher only), or takes SS_COMM_FILE.
 *  Environment: RCCL across processes needs HSA_ENABLE_IPC_MODE_LEGACY=0 on hosts whose driver has only dmabuf IPC, and
 *  the HSA runtime reads it at the process' first HIP call.  Loading the library changes nothing in the environment; the
 *  ss_comm_init* calls (RCCL, world > 1) set the variable if it is unset, which is in time only when they make the process'
 *  FIRST HIP call.  A rank therefore does NOT call ss_set_device first: ss_comm_init_on_device(…, device, …) and
 *  ss_comm_init_from_env (device = SS_COMM_DEVICE — explicit: it must parse as a number and name a visible device —, else
 *  LOCAL_RANK; where the launcher masks ONE GPU per rank, ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES per task as under
 *  SLURM, LOCAL_RANK still counts 0 .. n-1 against a single visible device: a LOCAL_RANK beyond the visible devices is
 *  taken modulo their count, i.e. device 0 there) make the rank's GPU current themselves, behind the
 *  setenv; plain ss_comm_init keeps whatever device is current (for callers that export the variable in the launcher, as
 *  bench.py does).  When the variable is wrong the failure surfaces as "hipIpcGetMemHandle: invalid argument" inside
 *  ncclCommInitRank; the error text of a failed init names the variable.
 *  Failure is all-or-nothing and prompt: what goes wrong on one rank before the ranks meet (no such device, no librccl, no
 *  memory) and the outcome of ncclCommInitRank are exchanged over the join sockets, so every rank returns SS_ERR_DEVICE within
 *  seconds and ss_last_device_error names the reason (the failing rank's own, "another rank ..." elsewhere).  Only a rank that
 *  never arrives (its process died) is waited for: SS_COMM_TIMEOUT_S seconds (default 180) at the rendezvous and again
 *  inside ncclCommInitRank.
 * ------------------------------------------------------------------------- */
typedef struct ss_comm ss_comm;
enum { SS_COMM_RCCL = 0, SS_COMM_HOST_TCP = 1 };
int ss_comm_init(int transport, int rank, int world, const char *rendezvous_file, ss_comm **out);
int ss_comm_init_on_device(int transport, int rank, int world, int device, const char *rendezvous_file, ss_comm **out);
int ss_comm_init_from_env(int transport, ss_comm **out);
void ss_comm_destroy(ss_comm *c);
int ss_comm_rank(const ss_comm *c);
/* number of ranks as the transport itself reports it (ncclCommCount for RCCL) */
int ss_comm_size(const ss_comm *c);
const char *ss_comm_transport_name(const ss_comm *c);
/* ncclGetVersion's code of the librccl this communicator runs on (e.g. 22707 = 2.27.7); 0 for the host transport */
int ss_comm_library_version(const ss_comm *c);
/* small host-buffer collectives (fences and the max-over-ranks clock of the benchmark) */
int ss_comm_barrier(ss_comm *c);
int ss_comm_allreduce_u64_sum(ss_comm *c, uint64_t *inout, size_t n);
int ss_comm_allreduce_f64_max(ss_comm *c, double *inout, size_t n);
/* the corpus gate's exchange: in-place SUM all-reduce of this batch's corpus histograms (block ++ short-term,
 * 2000 u64) across the ranks, queued on the batch's stream behind ss_batch_run; out2000 (nullable) receives
 * the reduced histograms after the stream has drained.  Afterwards ss_batch_histograms returns the corpus-wide
 * histograms on every rank, and ss_corpus_integrated_lufs / ss_corpus_loudness_range evaluate the gate. */
int ss_batch_allreduce_histograms(ss_batch *b, ss_comm *c, uint64_t *out2000);
/* the whole corpus gate on the device, asynchronously: [ss_batch_allreduce_histograms over `c` when c != NULL] + A7 / A8
 * (loudness_global_multiple, loudness_range_multiple) of the summed histograms into a device pair, queued on the batch's
 * stream behind ss_batch_run — no copy, no wait, so a loop of passes needs no host synchronisation per pass.
 * ss_batch_corpus_gate_read waits for the stream and returns the pair of the last pass. */
int ss_batch_corpus_gate_enqueue(ss_batch *b, ss_comm *c);
int ss_batch_corpus_gate_read(ss_batch *b, double *integrated_lufs, double *loudness_range);

/* ------------------------------------------------------------------------- *
 *  Render-side reductions: the step after the path.
 *  The reference adds fft_gain_compensation_db to every bin (tui.rs:801-821) and draws inside the chart
 *  bounds [FFT_LOWER_BOUND, FFT_UPPER_BOUND] = [-100, 0] dB (tui.rs:49-51, :890); the waveform chart shows
 *  the view [x_min, x_max] of the decimation bins (tui.rs:664-681).  Here both are reduced on the device to
 *  `cols` chart columns so that only what a terminal can show leaves HBM.  Gain and bounds are the
 *  reference's; the column rule is this library's (the reference hands every point to ratatui):
 *    spectrum column c = bins with floor(chart_x / 100 * cols) == c (last column closed), value =
 *                        max(clamp(dB + gain, -100, 0)); a column without a bin is NaN
 *    waveform column c = decimation bins i with floor((i - x_min) * cols / (x_max - x_min)) == c,
 *                        value = (min of mins, max of maxes); a column without a bin is (NaN, NaN)
 * ------------------------------------------------------------------------- */
enum { SS_GAIN_FIXED = 0,       /* gain_db as given                                                   */
       SS_GAIN_REFERENCE = 1 }; /* per stream FFT_TARGET_LUFS(-13) - integrated as f32 (tui.rs:1234) */
/* after ss_batch_run: [stream][window][fft_channel][cols] f32 into a device buffer of the batch */
int ss_batch_render_spectrum(ss_batch *b, uint32_t cols, int gain_mode, float gain_db);
/* SS_BATCH_FFT_COLUMNS batches: the gain of the fused reduction, for the passes that follow.  Default: SS_GAIN_REFERENCE
 * when the batch also runs the meter (SS_BATCH_LUFS: the pass then runs the time-domain chain first — the gain needs
 * every stream's integrated loudness), otherwise SS_GAIN_FIXED with 0 dB.  ss_batch_download_spectrum_columns reads
 * the result. */
int ss_batch_set_columns_gain(ss_batch *b, int gain_mode, float gain_db);
int ss_batch_download_spectrum_columns(ss_batch *b, uint32_t stream, float *out, size_t cap_floats);
/* One curve per stream instead of one row per window: the long-term average spectrum and the peak-hold spectrum of every
 * (stream s, fft channel r), reduced on the device from the rows a pass left — the v_w that ss_batch_download_fft returns, dB with
 * the pink compensation — over the stream's own windows w < n_windows_s (ss_batch_stream_shape for ragged batches; rows behind
 * that count are never read).  For retained bin i:
 *   - a NaN value is skipped: a refused window's row is all NaN and drops out of every bin of its row, and of no other row; an
 *     infinity counts as a value;
 *   - windows_counted[r] = the values not skipped at bin 0;
 *   - max_db[i] = the largest counted v_w, bit for bit the f32 that was stored;
 *   - mean_db[i] = the power mean (float)(10 log10((1 / n) sum_w 10^(v_w / 10))), n the values counted at bin i: powers formed in
 *     f32 (exp2f(v log2(10) / 10)), summed in f64, the logarithm taken in f64;
 *   - nothing counted (no window, or every window refused): mean_db = max_db = NaN, count 0.
 * The sums have one fixed order (windows by index, in chunks that are added by index; streams by index for the corpus form; no
 * floating-point atomics): two reductions of the same rows agree bit for bit, mean_db included.
 * Device memory (sums, means, maxima and counts per bin of every stream: 20 bytes per bin, 70 MB for 1024 stereo streams at
 * fft_n = 4096) is allocated at a batch's first ss_batch_spectrum_stats: a batch that never calls it allocates and launches
 * exactly what it did before.
 * Status codes: a batch without SS_BATCH_FFT or with SS_BATCH_FFT_COLUMNS (no rows), and a download or the corpus form before
 * the first reduction, SS_ERR_INVALID_MODE; a null batch or a bad stream index SS_ERR_INVALID_ARG.  n_windows == 0 is valid:
 * every result is NaN with count 0.
 * after ss_batch_run: reduce every stream's rows; queued on the batch's stream like ss_batch_render_spectrum, nothing is copied
 * or waited for */
int ss_batch_spectrum_stats(ss_batch *b);
/* one stream: mean_db / max_db are [fft_channels][n_bins] f32 (either may be NULL), windows_counted is [fft_channels] (may be
 * NULL); cap_floats < fft_channels * n_bins, or cap_channels < fft_channels with windows_counted given: SS_ERR_CAPACITY.  Waits
 * for the batch's stream. */
int ss_batch_download_spectrum_stats(ss_batch *b, uint32_t stream, float *mean_db, float *max_db, size_t cap_floats,
                                     uint32_t *windows_counted, uint32_t cap_channels);
/* the whole batch pooled, from the last reduction's per-stream sums: the same rule on the f64 power sums and counts of all streams
 * added up — every counted window of every stream weighs the same — max_db the maximum over the streams, windows_counted[r] the
 * u64 total of the streams' counts.  One more small launch; waits. */
int ss_batch_corpus_spectrum(ss_batch *b, float *mean_db, float *max_db, size_t cap_floats,
                             uint64_t *windows_counted, uint32_t cap_channels);
/* verification utility: how ss_batch_spectrum_stats cuts this batch's windows — `chunks` runs of `chunk_windows` consecutive
 * windows per stream (either may be NULL); chunks > 1: partial sums per run, added in run order by a second launch (one long file);
 * chunks == 1: one launch (many streams).  The results depend on it in the last bits of the f64 sums only. */
int ss_batch_spectrum_stats_plan(const ss_batch *b, uint32_t *chunks, uint32_t *chunk_windows);
/* A spectrogram per stream: time on one axis, the chart's log frequency on the other, reduced on the device from the rows a pass
 * left to a picture the size of the screen — [stream][fft_channel][t_cols][f_cols] f32.  Not in the reference (it shows one
 * spectrum at a time); the waveform side has this shape already (ss_batch_render_waveform).
 * Cell (s, r, t, c) is the maximum of clamp(v + gain, -100, 0), in f32, over
 *   - the windows w of stream s with w_min <= w < min(w_max, n_windows_s) and floor((w - w_min) * t_cols / (w_max - w_min)) == t
 *     (64-bit integers; the rule of the waveform columns), n_windows_s the stream's own count (ss_batch_stream_shape for ragged
 *     batches; rows behind that count are never read), and
 *   - the bins i of row (s, w, r) with floor(chart_x[i] / 100 * f_cols) == c, the last column closed: the column map of
 *     ss_batch_render_spectrum.
 * v is the value ss_batch_download_fft returns; gain is gain_db, or -13 - (float)integrated of stream s for SS_GAIN_REFERENCE, as
 * in ss_batch_render_spectrum.  A NaN value is skipped: a refused window's row is all NaN and drops out of its own row's cells and
 * of nothing else.  An infinity is clamped like any value.  A cell without a window, without a bin, or with only NaN values is
 * NaN.  x -> clamp(x + gain) is monotone, so the device takes the maxima first and applies the gain once per cell; a maximum is
 * exact in any order, so two calls (and the two plans below) agree value for value.
 * Beside ss_batch_render_spectrum: every cell equals the maximum over its windows of ss_batch_render_spectrum(f_cols, the same
 * gain)'s columns, NaN positions included — except for a refused window, whose NaN values ss_batch_render_spectrum draws at the
 * chart's floor (-100 in every column that owns a bin) and this call skips.
 * SS_BATCH_FFT_COLUMNS batches: the pass has reduced frequency and applied its gain (ss_batch_set_columns_gain), so the
 * spectrogram is the time maximum of the stored columns: f_cols must equal spectrum_columns (SS_ERR_INVALID_ARG otherwise),
 * gain_mode and gain_db are not read, and the result equals a full-row batch's of the same input under the same gain — except
 * that a refused window reads -100 there, as it does in the stored columns.
 * ss_batch_spectrogram copies the view and queues on the batch's stream like ss_batch_spectrum_stats: nothing is copied back or
 * waited for; a later call replaces the result.  The result's buffer is the call's own (not ss_batch_render_spectrum's), allocated
 * at a batch's first call and grown by a larger view: a batch that never calls it allocates and launches exactly what it did before.
 * Status codes, all checked before anything is queued: a null batch or view, t_cols or f_cols out of range, w_max <= w_min, an
 * unknown gain mode, first_stream + count > n_streams: SS_ERR_INVALID_ARG; a batch without SS_BATCH_FFT, SS_GAIN_REFERENCE
 * without SS_BATCH_LUFS, a download before the first call: SS_ERR_INVALID_MODE; cap_floats too small: SS_ERR_CAPACITY.
 * n_windows == 0 is valid: every cell is NaN. */
typedef struct ss_spectrogram_view {
    uint32_t t_cols;     /* time columns, 1 .. 4096                                                     */
    uint32_t f_cols;     /* frequency columns, 1 .. 512 (ss_batch_render_spectrum's chart columns)       */
    uint32_t w_min;      /* first window of the view                                                     */
    uint32_t w_max;      /* one past the last; > w_min; may lie beyond a stream's windows                */
    int32_t gain_mode;   /* SS_GAIN_FIXED / SS_GAIN_REFERENCE                                            */
    float gain_db;
} ss_spectrogram_view;   /* 24 bytes */
/* after ss_batch_run: reduce every stream's rows to the view's cells */
int ss_batch_spectrogram(ss_batch *b, const ss_spectrogram_view *v);
/* verification utility: how ss_batch_spectrogram cuts this view — `runs` workgroups of `run_windows` consecutive windows per time
 * column (either may be NULL); runs > 1: partial maxima per run, joined by a second launch (one long file, few time columns);
 * runs == 1: one launch (many streams).  The results do not depend on it. */
int ss_batch_spectrogram_plan(const ss_batch *b, const ss_spectrogram_view *v, uint32_t *runs, uint32_t *run_windows);
/* `count` streams from first_stream on, [count][fft_channels][t_cols][f_cols] of the last view, in one transfer.  Waits for the
 * batch's stream. */
int ss_batch_download_spectrogram(ss_batch *b, uint32_t first_stream, uint32_t count, float *out, size_t cap_floats);
/* the windows [*first, *end) time column t of a view owns, before the cut at a stream's own window count: the arithmetic of the
 * device; host arithmetic.  (0, 0) for a null view, t_cols out of range, w_max <= w_min and for t >= t_cols. */
void ss_spectrogram_column_windows(const ss_spectrogram_view *v, uint32_t t, uint32_t *first, uint32_t *end);
/* Spectrum regions: the average and the peak-hold spectrum of time ranges of the streams — each item of a transmission log, each
 * track of a continuous mix, each scene of a reel — and of groups of them (an album's pooled curve), reduced on the device from the
 * rows a pass left.  Not in the reference.  The list is the loudness regions' (ss_loudness_region: stream, first 100 ms sub-block,
 * count, group), so one list reads the loudness, the peaks and the tonal balance of a delivery.
 * Grid: S = (sample_rate + 5) / 10 frames and E_s = ceil(F_s / S) entries, the peak series' grid — every list that
 * ss_batch_peak_regions or ss_batch_loudness_regions accepts is accepted here, and a batch with SS_BATCH_FFT but without
 * SS_BATCH_LUFS works too.  The bound is first_subblock + n_subblocks <= E_s, in 64 bits.
 * Windows of a region: window w of a stream covers the frames [first + w hop, first + w hop + fft_n), first = (fft_n / hop + 1) hop
 * - fft_n (where a pass puts window 0).  Region (s, a, n) owns the windows that lie wholly inside [a S, (a + n) S), cut to the
 * stream's own n_windows_s (ss_batch_stream_shape); a window that straddles a boundary belongs to neither neighbour, like the
 * gating blocks of a loudness region.  With 64-bit integers, f0 = a S and f1 = (a + n) S:
 *   lo = f0 <= first ? 0 : ceil((f0 - first) / hop),  hi = f1 >= first + fft_n ? (f1 - fft_n - first) / hop + 1 : 0,
 *   end = max(lo, hi), then lo and end are cut to n_windows_s.
 * (48 kHz, fft_n 4096, hop 1024: region (16, 1) owns window 74 alone, (0, 1) owns none, (0, 20) of a 96 000-frame stream all 89.)
 * ss_region_windows is this rule before the cut, as host arithmetic: it saturates at 0xFFFFFFFF and gives (0, 0) for fft_n == 0
 * or hop_frames == 0; the device path runs on its arithmetic.
 * Per region, fft channel r and retained bin i, the rules of ss_batch_spectrum_stats on the region's windows: a NaN value is
 * skipped (a refused window's row drops out of its own row's bins and of nothing else), an infinity counts as a value; max_db is
 * the largest counted value, bit for bit the stored f32; mean_db = (float)(10 log10((1 / n) sum 10^(v / 10))), powers formed in f32
 * by exp2f, summed in f64, the logarithm taken in f64; windows_counted[r] = the values counted at bin 0; nothing counted
 * (n_subblocks == 0, a region too short to hold a window, every window refused): mean_db = max_db = NaN, count 0.
 * Groups: a group's power sums and counts are those of the regions that name it, added in region index order; its max_db is the
 * maximum of their maxima, its mean_db the same expression on the pooled sums, its windows_counted[r] a u64.  Regions may come from
 * any streams, may overlap and may repeat: each one counts.  A group without regions reads NaN, NaN, 0.
 * Order: windows by index inside a chunk, chunks by index, regions by index inside a group; no floating-point atomics — two calls
 * on the same rows agree byte for byte, mean_db included.  The results depend on the plan (below) in the last bits of the f64 sums
 * only; max_db, the counts and the NaN positions do not depend on it at all.
 * ss_batch_spectrum_regions runs after ss_batch_run on the rows the pass left: it copies the list before it returns, queues on the
 * batch's stream and waits for nothing; a later call replaces the list and every result.  The downloads wait for the stream.
 * Device memory, allocated at a batch's first call and grown by a longer list (a batch that never calls it allocates and launches
 * exactly what it did before): 20 bytes per bin of every (region, fft channel) — f64 sum, f32 mean, f32 max, u32 count — i.e.
 * 14 KB x 2 x 20 B = 68 KB per stereo region at fft_n = 4096, 700 MB for 10 240 regions; 8 bytes per bin of every (group, fft
 * channel) and a u64 per (group, fft channel); 16 bytes more per bin, region, fft channel and chunk where the plan has chunks.
 * Status codes, all checked before anything is queued or allocated, so a refused call leaves the previous list and results as they
 * were: a batch without SS_BATCH_FFT or with SS_BATCH_FFT_COLUMNS (no rows), a download or the plan before the first call:
 * SS_ERR_INVALID_MODE; a null batch, regions == NULL with n_regions > 0, stream >= n_streams, first_subblock + n_subblocks beyond
 * E_s, a group >= n_groups other than SS_REGION_NO_GROUP, first + count beyond the list: SS_ERR_INVALID_ARG; a cap too small:
 * SS_ERR_CAPACITY, with nothing written; a list whose grid or result size does not fit one launch (the limits of
 * ss_batch_spectrum_stats' own grid: about 1.2e9 (region, fft channel) pairs, or 1e9 (group, fft channel) pairs, at fft_n = 4096):
 * SS_ERR_UNSUPPORTED.  n_regions == 0 is valid. */
int ss_batch_spectrum_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups);
/* `count` regions of the last list from first_region on: mean_db / max_db [count][fft_channels][n_bins] f32 (device rows are
 * fft_bin_stride apart, these are dense), windows_counted [count][fft_channels]; any of the three may be NULL.  cap_floats counts
 * for mean_db and max_db each, cap_counts for windows_counted.  Waits for the batch's stream. */
int ss_batch_download_region_spectra(ss_batch *b, uint32_t first_region, uint32_t count, float *mean_db, float *max_db, size_t cap_floats,
                                     uint32_t *windows_counted, size_t cap_counts);
/* the same for `count` groups from first_group on; the counts are u64 */
int ss_batch_download_group_spectra(ss_batch *b, uint32_t first_group, uint32_t count, float *mean_db, float *max_db, size_t cap_floats,
                                    uint64_t *windows_counted, size_t cap_counts);
/* verification utility: how the last queued list was cut — ss_batch_spectrum_stats' rule on (regions x fft_channels) pairs and the
 * longest region's window count: `chunks` runs of `chunk_windows` consecutive windows per region (either may be NULL); chunks > 1:
 * partial sums per run, added in run order by a second launch (a few long regions); chunks == 1: one launch. */
int ss_batch_spectrum_regions_plan(const ss_batch *b, uint32_t *chunks, uint32_t *chunk_windows);
/* the windows [*first, *end) the sub-blocks [first_subblock, first_subblock + n_subblocks) own, before the cut at a stream's own
 * window count (either pointer may be NULL); host arithmetic */
void ss_region_windows(uint32_t sample_rate, uint32_t fft_n, uint32_t hop_frames, uint32_t first_subblock, uint32_t n_subblocks,
                       uint32_t *first, uint32_t *end);
/* [stream][cols][2] f32 (min, max) of the decimation bins x_min <= i < x_max */
int ss_batch_render_waveform(ss_batch *b, uint32_t cols, uint32_t x_min, uint32_t x_max);
int ss_batch_download_waveform_columns(ss_batch *b, uint32_t stream, float *out, size_t cap_floats);
/* the Player-mode view bounds of the waveform chart (tui.rs:664-681); host arithmetic, f64 */
void ss_waveform_view(double playhead_ms, double waveform_window_s, size_t chart_points,
                      double *x_min, double *x_max);

/* kernel timing with HIP events on the batch's own stream (for roofline
 * reporting): enable, run N passes, then read accumulated per-kernel time.
 * Timed passes queue back to back: the event pairs go into a ring of 32 passes'
 * sets and are read (one stream synchronisation) by ss_batch_timing_read /
 * ss_batch_sync / ss_batch_timing_enable — or by ss_batch_run itself when 32 passes
 * are pending — so a timed region of K passes measures its own kernels. */
enum { SS_KERNEL_FFT = 0, SS_KERNEL_TIME_DOMAIN = 1, SS_KERNEL_FINALIZE = 2, SS_KERNEL_WAVEFORM = 3, SS_KERNEL_COUNT = 4 };
int ss_batch_timing_enable(ss_batch *b, int enable);
int ss_batch_timing_read(ss_batch *b, int kernel, double *total_ms, uint64_t *launches);
const char *ss_kernel_name(int kernel);            /* the bench configuration's kernels */
const char *ss_batch_kernel_name(const ss_batch *b, int kernel);   /* the kernel this batch's shape selects */

/* ------------------------------------------------------------------------- *
 *  Tick drivers: the per-file / per-device state of the
 *  reference's App and its per-tick analysis, with the audio resident in HBM.
 *    ss_session_open_file     receive_audio_file            tui.rs:1207-1241
 *                             (+ AudioFile::from_file's mid/side and duration,
 *                              audio_player.rs:150-166)
 *    ss_session_tick_file     analyze_audio_file_samples    tui.rs:1482-1552
 *    ss_session_open_capture  device selection              tui.rs:1780-1808
 *    ss_session_tick_capture  analyze_microphone_input      tui.rs:1427-1480
 *    ss_session_restart       play / seek handlers          tui.rs:1586-1614
 *    ss_session_capture_push  the capture callback's extend audio_capture.rs:41-52
 *  A tick is ONE call: nothing is uploaded for a file tick (the file was
 *  uploaded at open; its spectrum, its loudness call and its short-term
 *  reading are one launch); the capture tick either uploads the 30*rate-sample snapshot it is given, or — the ring kept on the
 *  device, ss_session_capture_push + ss_session_tick_capture_resident — only what was captured since the last tick.  The session
 *  owns its analyzer (file_analyzer / device_analyzer) and the 300-entry short-term history (tui.rs:420,463).
 * ------------------------------------------------------------------------- */
typedef struct ss_session ss_session;

#define SS_LUFS_HISTORY 300
#define SS_TICK_WINDOW 16384      /* tui.rs:1488 / :1431: FFT window; :1529 / :1466: LUFS slice (samples) */

typedef struct ss_tick_result {
    uint64_t playhead;         /* pos / channels (tui.rs:1484-1485); capture: 0                     */
    int32_t fft_ran;           /* 0: the reference skips the FFT block (left bound == 0)            */
    int32_t mid_status;        /* status of get_fft(mid); != 0 => the reference stores [(0., 0.)]   */
    int32_t side_status;
    uint32_t n_mid, n_side;    /* pairs written to mid_xy / side_xy (1 = the (0,0) fallback)        */
    int32_t lufs_ran;          /* 0: LUFS block skipped (left bound == 0): history not shifted      */
    int32_t fed;               /* 1: add_samples + get_shortterm_lufs ran (bounds check passed)     */
    int32_t add_status;        /* status of add_samples                                             */
    int32_t shortterm_status;  /* status of get_shortterm_lufs; != 0 => lufs[299] = 0.0             */
    uint32_t reserved;
    double shortterm;          /* lufs[299] after this tick                                         */
} ss_tick_result;              /* 56 bytes */

/* interleaved: the decoded file (AudioFile::samples), n_samples floats; channels: the file's channel
 * count (AudioFile::channels — used only for pos / channels, mid/side always pair samples 2i, 2i+1);
 * the meter is created with 2 channels like the reference (tui.rs:1217-1221). */
int ss_session_open_file(const float *interleaved, size_t n_samples, uint32_t channels,
                         uint32_t sample_rate, ss_session **out);
/* device_analyzer.create_loudness_meter(channels, rate) + a 30*rate capture ring */
int ss_session_open_capture(uint32_t channels, uint32_t sample_rate, ss_session **out);
void ss_session_close(ss_session *s);
/* the session's Analyzer (for get_integrated_lufs / get_true_peak / get_loudness_range reads) */
ss_analyzer *ss_session_analyzer(ss_session *s);
/* waveform.audio_file_chart = get_waveform(samples, duration_s) (tui.rs:1213-1216) */
int ss_session_waveform(ss_session *s, double *out_xy, size_t cap_pairs, size_t *out_n);
/* fft_gain_compensation_db = FFT_TARGET_LUFS(-13) - integrated as f32, or 0 (tui.rs:1229-1238) */
int ss_session_gain_db(ss_session *s, float *out);
/* AudioFile::duration in ms (audio_player.rs:154) */
int ss_session_duration_ms(ss_session *s, uint64_t *out);
/* pos: the playback position in interleaved samples as passed to analyze_audio_file_samples */
int ss_session_tick_file(ss_session *s, size_t pos, double *mid_xy, double *side_xy,
                         size_t cap_pairs, ss_tick_result *res);
/* latest: the capture ring oldest-first (latest_captured_samples.to_vec()), n must be 30 * rate.
 * wave_xy receives waveform.microphone_input_chart = get_waveform(mid, 15.) */
int ss_session_tick_capture(ss_session *s, const float *latest, size_t n, double *mid_xy,
                            double *side_xy, size_t cap_pairs, double *wave_xy,
                            size_t wave_cap_pairs, size_t *wave_n, ss_tick_result *res);
/* The capture ring resident on the device (it starts full of zeros like the reference's, tui.rs:1783-1784):
 *   ss_session_capture_push           the capture callback's `audio_buf.extend(data)` (audio_capture.rs:41-52; mono devices push
 *                                     the zero-interleaved data the callback builds): host work only
 *   ss_session_tick_capture_resident  analyze_microphone_input on the ring as it stands after every push so far: the same results
 *                                     as ss_session_tick_capture on `latest_captured_samples.to_vec()`, without the snapshot
 * The two forms can be mixed (a snapshot tick replaces the ring).  One caller at a time per session: where the reference
 * locks its ring's mutex (audio_capture.rs:41, tui.rs:1428), lock around these calls. */
int ss_session_capture_push(ss_session *s, const float *samples, size_t n);
int ss_session_tick_capture_resident(ss_session *s, double *mid_xy, double *side_xy, size_t cap_pairs, double *wave_xy,
                                     size_t wave_cap_pairs, size_t *wave_n, ss_tick_result *res);
/* lufs = [-100.; 300]; analyzer.reset() */
int ss_session_restart(ss_session *s);
int ss_session_lufs_history(ss_session *s, double *out300);
/* inspection (tests): whether the last tick's spectrum (*spectrum_fused) and its short-term reading (*shortterm_fused) rode the
 * launch of its loudness call (one launch for the tick); 0 and 0 before the first tick and after a tick without a loudness call */
int ss_session_last_tick_forms(const ss_session *s, int32_t *spectrum_fused, int32_t *shortterm_fused);

#ifdef __cplusplus
}
#endif
#endif /* SOUNDSCOPE_HIP_H */
