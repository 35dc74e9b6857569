// ss_kernels.h — parameter blocks and launchers of the gfx950 kernels.
// Host code (ss_host.cpp, ss_analyzer.cpp, ss_batch.cpp, ss_session.cpp, ss_ingest.cpp, ss_meter_bank.cpp) sees only this header; device code lives in ss_fft.hip, ss_time_domain.hip, ss_loudness.hip, ss_spectrum_stats.hip, ss_spectrum_regions.hip, ss_spectrogram.hip, ss_peak_series.hip, ss_signal_scan.hip, ss_pair_series.hip, ss_apply_gain.hip, ss_limiter.hip, ss_bank_signal_watch.hip, ss_bank_pair_watch.hip, ss_util.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <cstddef>
#include <cstdint>

#include "../../include/soundscope_hip.h"

namespace ssk {

// The records that cross the C ABI have one definition, the public header's: the kernels write, and the host code copies out, the
// ss_* structs themselves under these names.  The sizes are the header's "/* N bytes */" comments.
using LoudnessExtremes = ss_loudness_extremes;
using LoudnessRegion = ss_loudness_region;
using RegionResult = ss_region_result;
using GroupResult = ss_group_result;
using RegionPeaks = ss_region_peaks;
using GroupPeaks = ss_group_peaks;
using StreamScan = ss_stream_scan;
using ChannelScan = ss_channel_scan;
using SignalEvent = ss_signal_event;
using ChannelPair = ss_channel_pair;
using PairEntry = ss_pair_entry;
using RegionPair = ss_region_pair;
using GroupPair = ss_group_pair;
using GainChannel = ss_gain_channel;
using MeterReading = ss_meter_reading;
using StreamWatch = ss_stream_watch;
using ChannelWatch = ss_channel_watch;
using PairWatchSums = ss_pair_sums;
using PairWatch = ss_pair_watch;
static_assert(sizeof(ss_loudness_extremes) == 24, "ss_loudness_extremes");
static_assert(sizeof(ss_loudness_region) == 16, "ss_loudness_region");
static_assert(sizeof(ss_region_result) == 48, "ss_region_result");
static_assert(sizeof(ss_group_result) == 32, "ss_group_result");
static_assert(sizeof(ss_peak_entry) == 16, "ss_peak_entry");
static_assert(sizeof(ss_region_peaks) == 48, "ss_region_peaks");
static_assert(sizeof(ss_group_peaks) == 32, "ss_group_peaks");
static_assert(sizeof(ss_stream_scan) == 56, "ss_stream_scan");
static_assert(sizeof(ss_channel_scan) == 64, "ss_channel_scan");
static_assert(sizeof(ss_signal_event) == 24, "ss_signal_event");
static_assert(sizeof(ss_channel_pair) == 8, "ss_channel_pair");
static_assert(sizeof(ss_pair_entry) == 32, "ss_pair_entry");
static_assert(sizeof(ss_region_pair) == 64, "ss_region_pair");
static_assert(sizeof(ss_group_pair) == 64, "ss_group_pair");
static_assert(sizeof(ss_gain_channel) == 32, "ss_gain_channel");
static_assert(sizeof(ss_meter_reading) == 72, "ss_meter_reading");
static_assert(sizeof(ss_stream_watch) == 64, "ss_stream_watch");
static_assert(sizeof(ss_channel_watch) == 80, "ss_channel_watch");
static_assert(sizeof(ss_pair_sums) == 40, "ss_pair_sums");
static_assert(sizeof(ss_pair_watch) == 160, "ss_pair_watch");
// the records count in uint64_t, HIP's 64-bit atomics take unsigned long long: the one cast of a kernel that adds to a record in place
__device__ __forceinline__ unsigned long long *atomic_u64(uint64_t *p) { return reinterpret_cast<unsigned long long *>(p); }

// hipFuncSetAttribute applies to the current device only: a launcher prepares its kernel once per device.  The bit of a
// device is set only AFTER the attribute call has succeeded there, under the launcher's mutex — a second thread on the
// same device cannot launch before the attribute exists, two threads cannot both act as "first", and a failure on one
// device leaves the other devices' bits alone.
struct DevicePrep {
    std::mutex mu;
    uint64_t done = 0;
};
template <class F>
inline hipError_t prepare_on_device(DevicePrep &p, F &&prepare)
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    const uint64_t bit = 1ull << (d & 63);
    std::lock_guard<std::mutex> lk(p.mu);
    if (p.done & bit) return hipSuccess;
    const hipError_t e = prepare();
    if (e == hipSuccess) p.done |= bit;
    return e;
}

constexpr int kHistBins = 1000;
constexpr int kMaxChannels = 64;
constexpr int kTpHistMax = 24;    // longest polyphase branch (factor 2)

// ---- spectrum ---------------------------------------------------------------
struct FftBatchParams {
    const float *pcm;            // [stream][frame][channels] f32
    float *out;                  // [stream][window][fft_channels][n_bins] f32 dB (+pink)
    const float *window;         // N (generic kernel) — full Hann
    const float *half_window;    // N (4096 kernel)   — 0.5 * Hann
    const float2 *tw_n;          // W_N^k, k < N  (4096 kernel uses k < 3841; generic k < N/2)
    const float2 *tw_256;        // W_256^k, k < 256 (4096 / 16384 kernels)
    const float2 *tw_core;       // W_4096^k, k < 4096 (16384 kernel)
    const float *pink;           // bin_stride f32 (zero padded), or nullptr for raw dBFS (generic / 16k kernels)
    const float *offpink;        // bin_stride f32: db_offset + pink[bin] (4096 kernels)
    uint64_t frames_per_stream;
    uint64_t first_start;        // frame index where window 0 starts
    uint32_t n_streams;
    uint32_t channels;
    uint32_t n_windows;
    uint32_t hop;
    uint32_t n;                  // FFT length
    uint32_t first_bin, n_bins;
    uint32_t bin_stride;         // floats between output rows (n_bins rounded up to 4: 16-B aligned rows)
    uint32_t windows_per_block;  // 4096 kernel
    float db_offset;             // 10*log10(4/N^2) (4096) or 20*log10(4/N) (generic)
    float lg0;                   // 4096 kernels: fft4096_lg0(db_offset), the log operand of an exactly-zero squared magnitude
    uint32_t publish_mask;       // 4096 kernels: bit kc set when bins [256kc, 256kc+255] hold a retained bin or a mirror
    const uint32_t *windows_of;   // ragged batches: windows of each stream (nullable = n_windows for all)
    // columns-only spectrum (N3 fused into the epilogue; N = 4096 stereo at hop 1024): the rows are never stored, each
    // is reduced to `cols` chart columns of max(clamp(dB + gain, -100, 0)) — out_cols[stream][window][mid, side][cols]
    float *out_cols;             // nullptr: ordinary rows into `out`
    const uint16_t *bin_col;     // bin_stride entries: chart column of every retained bin, 0xFFFF for the row padding
    const uint2 *col_groups;     // bin_stride / 4 entries, one per group of four bins: x = o0 | o3 << 16 (byte offsets, 4 x column, of the
                                 // first / last bin's column in a row's accumulators), y = n: n bins lie in the first column, the rest in the
                                 // last; n = 0: a general group (more columns inside it, or row padding)
    const uint2 *col_bins;       // the same per bin: four u16 byte offsets per group, 2048 (a spare slot) for the row padding
    const float *col_init;       // cols entries: -inf where the column owns a bin, NaN where it owns none
    const double *integrated;    // per stream: gain = -13 - (float)integrated (tui.rs:1234); nullptr: gain_db for all
    uint32_t cols;               // 1 .. 512
    float gain_db;
    // one-window N = 16384 kernel (a tick): when set, the workgroup of channel ch stores done_value into done_flag[ch] behind its
    // row — in host-visible memory, so that the host can take the row while the rest of the launch is still running
    uint32_t *done_flag;
    uint32_t done_value;
};

// N = 4096 kernels: the value that stands in for log2(q) where a squared magnitude q is exactly zero, so that the dB epilogue's
// fma(lg0, 10 log10(2), db_offset + pink) lands on -150 + pink.  A launch constant, formed once on the host: the correctly
// rounded f32 quotient (host code is built without fast-math), the bits the kernels' own division gave per window before.
inline float fft4096_lg0(float db_offset) { return (-150.0f - db_offset) / 3.01029995663981195f; }
// N = 4096 kernels: bit kc set when bins [256 kc, 256 kc + 255] hold a retained bin or the mirror 4096 - k of one (the other
// blocks of the transform are not published to LDS)
inline uint32_t fft4096_publish_mask(uint32_t first_bin, uint32_t n_bins)
{
    const uint32_t lo = first_bin, hi = first_bin + n_bins - 1;
    uint32_t mask = 0;
    for (uint32_t kc = 0; kc < 16; kc++) {
        const uint32_t a0 = 256 * kc, a1 = a0 + 255;
        const bool direct = a0 <= hi + 3 && a1 >= lo;                       // +3: the last group of four may run past
        const bool mirror = a0 <= 4096 - lo && a1 + 3 >= 4096 - hi - 3;
        if (direct || mirror) mask |= 1u << kc;
    }
    return mask;
}
// The spectrum kernels (ss_fft.hip), one per launch form:
//   ms1, ms, ms_anyhop  N = 4096 stereo -> mid/side packed as one complex FFT, hop a multiple of 256 (1024 / 512 or 2048 / other)
//   pairw               N = 4096, hop 1024, mono / per channel: one real channel per workgroup run, two windows per transform
//   fft16k_run          N = 16384, hop 1024, eight windows or more: runs of windows per workgroup
//   fft16k              N = 16384, one window per workgroup
//   generic             any other power-of-two N in [2, 32768]
enum class SpecKernel : uint32_t { ms1, ms, ms_anyhop, pairw, fft16k_run, fft16k, generic };
// what a window's rows are (the values are the kernels' `mode`)
enum class SpecRows : uint32_t { mono = 0, mid_side = 1, per_channel = 2 };
struct SpecPlan {
    SpecKernel kernel = SpecKernel::generic;
    SpecRows rows = SpecRows::mono;
    uint32_t fft_ch = 1;             // rows per window
    uint32_t windows_per_block = 1;  // consecutive windows a workgroup walks (FftBatchParams::windows_per_block)
    uint32_t blocks = 0;             // workgroups (pairw / fft16k_run launch this rounded up to a multiple of 8)
};
// which kernel runs n_streams x n_windows windows of N = n points of `channels`-channel input at `hop`, on what grid.  The one
// decision for batches and one-window callers alike (a handle's get_fft, a tick: one stream, one window at hop 1024).
SpecPlan plan_spectrum(uint32_t n, uint32_t channels, uint32_t hop, uint32_t n_streams, uint32_t n_windows);
// p: n_streams / n_windows as planned, windows_per_block = plan.windows_per_block
hipError_t launch_spectrum(const SpecPlan &plan, const FftBatchParams &p, hipStream_t s);
const char *spectrum_kernel_name(SpecKernel k);         // as rocprofv3 prints it, without template arguments

// ---- spectrum statistics (ss_spectrum_stats.hip): every (stream, fft_channel)'s rows reduced over the stream's windows ------------
struct SpecStatsPlan {
    uint32_t slices = 1;             // waves side by side on a row: 64 groups of four bins each
    uint32_t chunk_windows = 1;      // consecutive windows a wave walks
    uint32_t chunks = 1;             // chunks per stream slot; > 1: partial sums per chunk and a second launch that adds them in chunk order
};
// the one decision for every shape: pairs = n_streams x fft_channels, n_windows of the stream slot
SpecStatsPlan plan_spectrum_stats(uint32_t pairs, uint32_t bin_stride, uint32_t n_windows);
struct SpecStatsParams {
    const float *rows;               // [stream][n_windows][fft_ch][bin_stride] f32 dB: what a pass left (FftBatchParams::out)
    uint32_t bin_stride, n_bins;
    uint32_t n_streams, fft_ch, n_windows;
    const uint32_t *windows_of;      // ragged batches: windows of each stream (nullable = n_windows for all); rows behind it are never read
    SpecStatsPlan plan;
    // results, [stream][fft_ch][bin_stride] each; the row padding behind n_bins holds (0, NaN, NaN, 0)
    double *sums;                    // f64 sums of the counted values' powers 10^(v / 10)
    float *mean, *max;               // 10 log10(sum / count) and the largest counted value, NaN where nothing was counted
    uint32_t *counts;                // values counted (not NaN) per bin
    // plan.chunks > 1: [stream][fft_ch][chunk][bin_stride]
    double *part_sums;
    float *part_max;
    uint32_t *part_counts;
};
hipError_t launch_spectrum_stats(const SpecStatsParams &p, hipStream_t s);
// the batch pooled from p.sums / p.max / p.counts, streams in index order: mean / max [fft_ch][bin_stride], counts [fft_ch] (bin 0's)
hipError_t launch_spectrum_stats_corpus(const SpecStatsParams &p, float *mean, float *max, unsigned long long *counts, hipStream_t s);
// Spectrum regions (ss_batch_spectrum_regions; ss_spectrum_regions.hip): the same reduction over time ranges of the streams, pooled into groups.  The host
// resolves a region to the windows [w_first, w_end) of its stream, w_end no larger than the stream's own window count, so the kernels
// divide nothing and never read a row behind it.
struct SpecRegion { uint32_t stream, w_first, w_end, group; };
struct SpecRegionsParams {
    // the sweep's block with (region, fft_channel) for its pairs: rows, bin_stride, n_bins, fft_ch and n_windows (of the stream slot)
    // as in ss_batch_spectrum_stats; n_streams = the REGIONS, windows_of unused; plan = plan_spectrum_stats(regions x fft_ch,
    // bin_stride, the longest region's windows); sums / mean / max / counts [region][fft_ch][bin_stride], the parts
    // [region][fft_ch][chunk][bin_stride]
    SpecStatsParams s;
    const SpecRegion *regions;       // [regions]
    uint32_t n_groups;
    const uint32_t *member_start;    // [n_groups + 1]: group g's members are members[member_start[g] .. member_start[g + 1])
    const uint32_t *members;         // region indices, ascending inside a group
    float *group_mean, *group_max;   // [group][fft_ch][bin_stride]
    unsigned long long *group_counts;// [group][fft_ch]: the pooled count at bin 0
};
// whether a list fits the launch limits (launch_spectrum_stats' own, on the regions' and the groups' grids), and its plan
bool spectrum_regions_fit(uint64_t n_regions, uint64_t n_groups, uint32_t fft_ch, uint32_t bin_stride, uint32_t longest_windows, SpecStatsPlan *plan);
// k_spectrum_regions, k_spectrum_regions_combine where the plan has chunks, k_spectrum_region_groups where there are groups
hipError_t launch_spectrum_regions(const SpecRegionsParams &q, hipStream_t s);

// batch spectrogram (ss_spectrogram.hip): time x frequency chart tiles of the rows (or of a columns-only pass's columns)
constexpr uint32_t kSpectrogramMaxTCols = 4096, kSpectrogramMaxFCols = 512;
// first window of time column t of the view [w_min, w_min + span) cut into t_cols columns: the smallest w with
// floor((w - w_min) * t_cols / span) >= t; t == t_cols gives w_min + span.  (t <= 4096, span < 2^32: the product fits 64 bits.)
__host__ __device__ inline uint32_t spectrogram_column_first(uint32_t w_min, uint32_t span, uint32_t t_cols, uint32_t t)
{
    return w_min + (uint32_t)(((uint64_t)t * span + t_cols - 1u) / t_cols);
}
struct SpectrogramPlan {
    uint32_t runs = 1;               // workgroups side by side on a time column; > 1: partial maxima per run and a second launch that joins them
    uint32_t run_windows = 1;        // consecutive windows of a time column a run walks
};
// units = (stream, fft_channel) pairs x time columns; column_windows = the most windows a time column of the view holds inside the slot
SpectrogramPlan plan_spectrogram(uint64_t units, uint32_t column_windows);
struct SpectrogramParams {
    const float *rows;               // rows form: [stream][n_windows][fft_ch][bin_stride] f32 dB (FftBatchParams::out)
    const float *cols;               // columns form: [stream][n_windows][fft_ch][f_cols] f32, gain and clamp applied (FftBatchParams::out_cols)
    uint32_t columns_form;           // 0: reduce `rows`, 1: reduce `cols`
    uint32_t bin_stride;             // rows form
    uint32_t n_streams, fft_ch, n_windows;
    const uint32_t *windows_of;      // [stream], nullable: ragged batches read min(windows_of[s], n_windows) windows of stream s
    const uint16_t *bin_col;         // rows form: [bin_stride] chart column of every bin, 0xFFFF for the row padding
    uint32_t t_cols, f_cols, w_min, w_max;
    const double *integrated;        // rows form, SS_GAIN_REFERENCE: gain = -13 - (float)integrated[stream]; nullptr: gain_db
    float gain_db;
    SpectrogramPlan plan;
    float *out;                      // [stream][fft_ch][t_cols][f_cols]
    uint32_t *part;                  // plan.runs > 1: [stream][fft_ch][t_cols][run][f_cols] order-preserving images of the runs' maxima, 0 = none
};
hipError_t launch_spectrogram(const SpectrogramParams &p, hipStream_t s);

// ---- time domain ------------------------------------------------------------
struct TdConst {                 // one per (rate, true-peak factor), device resident
    double b[5], a[5];
    double bu[5];                // input-referred unit-gain output taps of the batch kernels (sst::kweight_unit_gain_taps):
                                 // bu[k] = (b[k] - b[0] a[k]) / b[0], k = 1 .. 4: y / b[0] = x + bu[1] v1 + ... + bu[4] v4; bu[0] = b[0]^2, the
                                 // factor an energy summed over y / b[0] takes where it leaves the lanes
    double m_pow[8][16];        // (A^L)^(2^k), A = zero-input transition, L = td_chunk_frames(C)
    double m_pow_split[8][16];   // the same for L = td_split_chunk_frames(C): streaming calls shared by a workgroup's waves (SPLIT)
    double m_step_split[68][16]; // A^n, n = 0 .. 67 (same coordinates): the partial last chunk of a SPLIT tile (n < L <= 65)
    double m_chunk_split[64][16];// (A^L)^(c + 1) for chunk c of a SPLIT tile: what the state in front of the tile adds to the state
                                 // behind chunk c — applied when that state arrives, behind a scan that ran without it
    double m_chunk[64][16];      // the same for L = td_chunk_frames(C): batches whose streams are walked by a whole workgroup (split_batch)
    float tp[3][kTpHistMax];     // polyphase branches 1..factor-1, coefficient of x[n - t]
    float tp_fold[3][6];         // factor 4: the branches folded about their centre (sst::true_peak_fold4), the VALU forms' taps
    int32_t tp_factor;           // 0, 2, 4
    int32_t tp_len;              // taps per branch (12 or 24)
    uint32_t s100;               // frames per 100 ms sub-block = (rate + 5) / 10
    uint32_t st_off;             // 1: no short-term blocks at this rate — thirty sub-blocks are more frames than ebur128's 3 s ring holds
                                 // (rates under 145 Hz that round UP to their sub-block: 16 Hz -> 60 > 48), its energy_shortterm fails
                                 // and add_frames skips the block; loudness range then reads 0
};

struct TdState {                 // per stream / per handle, device resident
    double v[kMaxChannels][4];           // DF-II state v1..v4
    double acc[kMaxChannels];            // energy of the current incomplete sub-block
    float tp_hist[kMaxChannels][kTpHistMax]; // last samples (newest first is index 0)
    float sample_peak[kMaxChannels];
    float true_peak[kMaxChannels];
    uint64_t frames_fed;                 // since reset
    // Non-finite input (NaN, +-Inf).  In the crate such a sample poisons the channel's DF-II state for good: every later filtered
    // sample, hence every later gating block, is NaN and `sum >= boundary` never holds again.  A wave notes the FIRST sub-block
    // in which it met one: bad_key[c] = ~index (0 = none yet, so the zero fill of a reset is "none" and atomicMax keeps the
    // earliest); the gating kernels read every sub-block of a weighted channel BEHIND that one as NaN — which a launch cut into
    // time segments (each starting from a zero state) would otherwise not know.
    uint32_t bad_key[kMaxChannels];
};
static_assert(offsetof(TdState, true_peak) == offsetof(TdState, sample_peak) + sizeof(float) * kMaxChannels,
              "sample_peak and true_peak are read as one block (ssh::peaks_of, ReadingsExtra)");

enum TdSplitBatch : uint32_t { kTdSplitNone = 0, kTdSplitStreams = 1, kTdSplitSegments = 2 };    // TdParams::split_batch

struct TdParams {
    const float *pcm;            // [stream][frame][channels]
    uint64_t stream_stride;      // floats between consecutive streams
    uint64_t n_frames;           // frames to consume from each stream this call
    uint32_t n_streams;
    uint32_t channels;
    const TdConst *k;
    TdState *state;              // [stream]
    double *subblocks;           // [stream][slot][channels] f64, slot = sub-block index % sub_cap
    uint64_t sub_stride;         // doubles between streams
    uint32_t sub_cap;            // ring capacity in sub-blocks
    double *ring;                // optional filtered-sample ring [stream][ring_frames][channels] (handle API, meter banks)
    uint64_t ring_frames;
    uint64_t ring_stride;        // doubles between the rings of consecutive streams (0: one stream, the handle)
    int32_t tp_factor;           // must equal k->tp_factor (selects the kernel instantiation)
    uint32_t s100;               // must equal k->s100
    uint32_t nseg;               // time segments per stream (1 for streaming calls)
    uint32_t seg_sub;            // sub-blocks per segment (nseg > 1)
    uint32_t warm_sub;           // run-in sub-blocks of segments > 0
    // fused min-max decimation (batch only; nullptr = off): out[stream][bin] = (min, max)
    union {                      // (one slot: decimation is a batch feature, per-stream bases one of the streaming launches — never both)
        float *wave_out;
        // streaming launches on the ring (meter banks' ragged adds): stream s's input starts at pcm + offset_of[s] floats instead of
        // pcm + s * stream_stride (nullable: the stride).  Read by the RING instantiations only.
        const uint64_t *offset_of;
    };
    uint64_t wave_stride;        // floats between streams
    uint32_t wave_window;        // number of decimation bins W
    uint32_t halo_frames;        // frames kept in front of each tile: >= longest bin, multiple of 4
    const uint64_t *frames_of;    // ragged batches: frames of each stream (nullable = n_frames for all).  Streaming launches on the
                                  // ring (meter banks' ragged adds) take it too: a stream of 0 frames is not touched at all, and
                                  // every other entry lies on n_frames' side of td_ring_tile_frames — the launch form is chosen from
                                  // n_frames, so the caller launches the short and the long streams of a call as two groups
    uint32_t tp_f32;              // 1: the factor-4 true peak as the f32 MFMA product everywhere (no f16 split)
    // Exact segment hand-over (batches, nseg > 1, warm_sub == 0): every segment's wave leaves the filter state behind its last frame in
    // seg_state[stream][segment][channel][4]; a second, light launch (fixup = 1: no true peak, no decimation) then re-runs the first
    // fix_sub sub-blocks of every segment > 0 from the state the segment in front of it left, and overwrites their energies.
    double *seg_state;
    uint32_t fixup, fix_sub;
    uint32_t split_batch;         // TdSplitBatch.  kTdSplitNone: one wave per stream / segment.  kTdSplitStreams (batches, nseg == 1):
                                  // a stream is ONE segment walked by the four waves of a workgroup, the filter state handed from tile to
                                  // tile through LDS (SPLIT with the batch's chunk length) — no run-in, nothing of the recurrence truncated.
                                  // kTdSplitSegments: the same with eight waves per (stream, SEGMENT) — a handful of streams cut into
                                  // short segments, where the length of the chain of tiles is what a pass takes
    // a tick's short-term reading inside the same launch (k_tick only; st_out == nullptr: off).  The window of st_frames frames
    // ends with this call; the st_old_total ring elements from st_begin_elem on are the part in front of the call.
    double *st_out;               // (energy, loudness): device or mapped host memory
    double *st_scratch;           // kRingTickBlocks partial sums + the count of finished workgroups (zero between launches)
    const double *st_weights;     // [channels]
    double st_frames;
    uint32_t st_begin_elem, st_old_total, st_blocks;
};
// tick_fft (streaming calls on the ring only): the one-window mid/side spectrum of a tick (N = 16384, out rows [mid, side]) to
// run in the SAME launch, beside the loudness call (k_tick), together with the short-term reading if p.st_out is set;
// *tick_fused tells whether that happened — if not, only the time-domain kernel was launched (p.st_out ignored) and the spectrum
// and the reading are the caller's to launch
hipError_t launch_time_domain(const TdParams &p, hipStream_t s, const FftBatchParams *tick_fft = nullptr, bool *tick_fused = nullptr);
// the second launch of the exact segment hand-over (see TdParams::seg_state): p as given to launch_time_domain
hipError_t launch_time_domain_fixup(const TdParams &p, hipStream_t s);
// frames per sequential chunk for a channel count (the constant block's m_pow must match)
uint32_t td_chunk_frames(uint32_t channels, uint32_t s100);
// the same for a streaming call whose tiles are shared by the waves of one workgroup (SPLIT): see ss_time_domain.hip
uint32_t td_split_chunk_frames(uint32_t channels, uint32_t s100);
uint32_t td_resident_waves_per_cu(uint32_t channels, uint32_t s100, uint32_t halo_frames);
// the longest streaming call (frames) that one wave walks; a longer one is shared by the eight waves of a workgroup (SPLIT), with
// another chunk length and hence other rounding — the one rule for handles, ticks and every stream of a meter bank
uint32_t td_ring_tile_frames(uint32_t channels, uint32_t s100);
// that rule itself: whether a streaming call of n_frames frames is shared (what launch_time_domain asks before it picks a form)
bool td_ring_call_shared(uint32_t channels, uint32_t s100, uint64_t n_frames);
// the form launch_time_domain gives a streaming call of n_frames frames, from the functions the launch calls (host arithmetic only)
struct TdRingPlan { bool shared; uint32_t waves, chunk_frames, tile_frames; };      // waves: of the workgroup that walk ONE stream
TdRingPlan td_ring_plan(uint32_t channels, uint32_t s100, uint64_t n_frames);

// a handle's readings in one launch: 2 * kMaxChannels floats copied from peaks_src to peaks_dst beside the evaluation of its
// histograms, then `seq` stored into *flag (host-visible memory: whoever sees the flag sees the evaluation and the peaks)
struct ReadingsExtra { const float *peaks_src; float *peaks_dst; uint32_t *flag; uint32_t seq; };

struct FinalizeParams {
    const TdConst *k;
    const double *subblocks; uint64_t sub_stride; uint32_t sub_cap;
    const double *hist_energies;     // 1000
    const double *hist_bounds;       // 1001
    const double *weights;           // [channels]
    uint64_t *hist;                  // [stream][2][1000] (block, short-term)
    uint64_t *corpus_hist;           // [2][1000] or nullptr
    uint32_t n_streams, channels;
    uint64_t sub_begin, sub_end;     // absolute sub-block index range completed by this call
    double *out_integrated;          // [stream] (nullable)
    double *out_lra;                 // [stream] (nullable)
    uint32_t *out_counts;            // [stream][2] gating / short-term blocks evaluated (nullable)
    const uint32_t *sub_end_of;   // ragged batches: sub-blocks of each stream (nullable = sub_end for all)
    const TdState *state;         // [stream]: bad_key (first sub-block with a non-finite sample per channel); nullable
    // launch_finalize_stream only (one handle): behind the histogram updates the same wave takes the handle's readings — (integrated,
    // range) into readings_out, the peaks and the flag as `readings` says (readings_out == nullptr: off)
    double *readings_out;
    ReadingsExtra readings;
};
// batches: the gating of every stream's sub-blocks [0, sub_end) into its own and the corpus histograms, the per-stream outputs
// (slot == sub-block index: hipErrorInvalidValue unless sub_begin == 0 and sub_end <= sub_cap, below 2^31)
hipError_t launch_finalize(const FinalizeParams &p, hipStream_t s);
// a handle (one stream, a few new sub-blocks per call): k_finalize_stream — the histograms updated in place and, when readings_out
// is set, the handle's readings taken behind them
// (hidden: not among the library's exported symbols)
__attribute__((visibility("hidden"))) hipError_t launch_finalize_stream(const FinalizeParams &p, hipStream_t s);
// Momentary / short-term loudness series of every stream of a batch and their maxima (SS_BATCH_LOUDNESS_SERIES), behind
// launch_finalize on the same stream: p as given there (batches: slot == sub-block index); series[stream][series_stride][2]
// (momentary, short-term) LUFS, extremes[stream] an ss_loudness_extremes.
hipError_t launch_loudness_series(const FinalizeParams &p, double *series, uint64_t series_stride, LoudnessExtremes *extremes,
                                  hipStream_t s);
// Loudness regions (ss_batch_loudness_regions), behind a pass on the same stream: the gated loudness of runs of one stream's
// sub-blocks, optionally pooled into groups.  The records are ss_loudness_region / ss_region_result / ss_group_result.
constexpr uint32_t kRegionNoGroup = SS_REGION_NO_GROUP;
struct RegionGateParams {
    const TdConst *k;
    const double *subblocks; uint64_t sub_stride; uint32_t sub_cap;      // batches: slot == sub-block index
    const double *hist_energies, *hist_bounds, *weights;
    const TdState *state;            // [stream]: bad_key
    uint32_t channels;
    const LoudnessRegion *regions;   // [n_regions], every one inside its stream (the caller has checked)
    RegionResult *results;           // [n_regions]
    uint32_t n_regions, n_groups;
    uint32_t longest;                // sub-blocks of the longest region: region_gate_threads
    GroupResult *group_results;      // [n_groups]; the launcher clears them and the histograms, the regions add their counts
    unsigned long long *group_hist;  // [n_groups][2][1000] (block, short-term)
};
// threads of a region's workgroup: launch_finalize's rule on the longest region of the list
constexpr uint32_t kRegionLongSub = 2048;
inline uint32_t region_gate_threads(uint32_t longest) { return longest > kRegionLongSub ? 1024u : 256u; }
// clears the groups, gates every region (k_region_gate) and evaluates every group (k_group_eval): three steps queued on s
hipError_t launch_region_gate(const RegionGateParams &p, hipStream_t s);
// Peak series (ss_batch_peak_series; ss_peak_series.hip): per (stream, 100 ms entry, channel) the true and sample peak and the
// frame of each, from the resident corpus alone — no pass, no tables.  A record is an ss_peak_entry: {f32 true_peak,
// f32 sample_peak, u32 true_peak_frame, u32 sample_peak_frame}, stored and loaded by the kernels as one 16-byte word.
struct PeakSeriesPlan { uint32_t tile_frames, entries_cap; };
// tile_frames: frames of an entry a workgroup stages at a time; entries_cap = ceil(n_frames / s100): record slots per stream
PeakSeriesPlan plan_peak_series(uint32_t channels, uint32_t s100, uint64_t n_frames);
struct PeakSeriesParams {
    const float *pcm;                // [stream][frame][channels] f32, 16-byte aligned
    uint64_t stream_stride;          // floats between streams
    uint64_t n_frames;               // frames of a slot
    const uint64_t *frames_of;       // ragged batches: each stream's own frames (nullable = n_frames for all)
    ss_peak_entry *series;           // [stream][entries_cap][channels]
    uint32_t n_streams, channels, s100;
    uint32_t tile_frames, entries_cap;      // plan_peak_series
    int factor;                      // 4, 2 or 0 (sample peak only)
    float taps[36];                  // [factor - 1][12 or 24]: branch f + 1's coefficient at delay d (ss_inspect_true_peak's layout)
};
hipError_t launch_peak_series(const PeakSeriesParams &p, hipStream_t s);
// Peak regions (ss_batch_peak_regions), behind a series on the same stream: its maxima over runs of one stream's entries, pooled
// into groups.  The records are ss_region_peaks / ss_group_peaks.
struct RegionPeaksParams {
    const ss_peak_entry *series; uint32_t entries_cap, channels, s100;
    double ceiling;                  // linear; an entry counts as over when any channel's true peak exceeds it
    const LoudnessRegion *regions;   // [n_regions], every one inside its stream's entries (the caller has checked)
    RegionPeaks *results;            // [n_regions]
    float *ch_true, *ch_sample;      // [n_regions][channels]
    uint32_t n_regions, n_groups;
    unsigned long long *group_acc;   // [n_groups][3]: (true bits, ~region), (sample bits, ~region), overs; the launcher clears them
    GroupPeaks *group_results;       // [n_groups]
};
// clears the groups' words, reduces every region (k_region_peaks) and writes every group's record (k_group_peaks)
hipError_t launch_region_peaks(const RegionPeaksParams &p, hipStream_t s);
// Signal scan (ss_batch_signal_scan; ss_signal_scan.hip): silence runs per stream, clip runs, sums and non-finite samples per
// channel, and the lists of the runs, from the resident corpus alone — no pass, no tables.  A stream has C + 1 predicate
// sequences: 0 is "the frame is silent", 1 + c is "the sample of channel c is clipped".  Three launches: k_signal_tiles (one
// workgroup per (stream, tile): the tile's sums and run summaries), k_signal_carry (one wave per stream: the runs that cross
// tiles, the records, every tile's place in the lists), k_signal_events (the lists; only with max_events > 0).
struct SignalScanPlan { uint32_t tile_frames, tiles_cap; };
// tile_frames: a multiple of 64 frames whose floats fit the peak series' tile; tiles_cap = ceil(n_frames / tile_frames) per stream
SignalScanPlan plan_signal_scan(uint32_t channels, uint64_t n_frames);
// one tile's view of one sequence: the run at its first frame, the run at its last frame, and the runs that touch neither edge
struct alignas(16) SignalTileRuns {
    uint32_t head, tail;             // frames of the run that holds the tile's first / last frame (both the tile's frames when all_true)
    uint32_t all_true;
    uint32_t count;                  // inner runs of at least the minimum
    uint32_t longest, longest_at;    // the longest inner run and its first frame in the tile (the lowest of equals); 0: none
    uint32_t total;                  // frames of the tile on which the predicate holds
    uint32_t pad;
};
struct alignas(16) SignalTileChannel {   // one tile's view of one channel
    double sum, sum_sq;              // over its finite samples
    uint32_t clipped, nonfinite;
    uint32_t first_nonfinite;        // frame in the tile, 0xFFFFFFFF: none
    uint32_t pad;
};
struct alignas(16) SignalTileCarry {     // what k_signal_carry tells k_signal_events about (tile, sequence)
    unsigned long long carry_in;     // frames of the run open at the tile's first frame that lie in front of the tile
    uint32_t ev_off;                 // qualifying runs of the sequence that end in earlier tiles (at most max_events)
    uint32_t owned;                  // ... that end in this tile (a run belongs to the tile that holds its last frame)
};
// (the records are ss_stream_scan / ss_channel_scan / ss_signal_event)
struct SignalScanParams {
    const float *pcm;                // [stream][frame][channels] f32, 16-byte aligned
    uint64_t stream_stride;          // floats between streams
    uint64_t n_frames;               // frames of a slot
    const uint64_t *frames_of;       // ragged batches: each stream's own frames (nullable = n_frames for all)
    uint32_t n_streams, channels;
    uint32_t tile_frames, tiles_cap; // plan_signal_scan
    float silence_threshold, clip_level;
    uint32_t silence_min, clip_min, max_events;
    SignalTileRuns *tile_runs;       // [stream][tiles_cap][channels + 1]
    SignalTileChannel *tile_channels;// [stream][tiles_cap][channels]
    SignalTileCarry *tile_carry;     // [stream][tiles_cap][channels + 1]
    uint32_t *list_base;             // [stream][channels + 1]: where a sequence's runs start in its list (at most max_events)
    StreamScan *streams;             // [stream]
    ChannelScan *channel_scans;      // [stream][channels]
    SignalEvent *events;             // [stream][2][max_events]: the silence list, the clip list (max_events == 0: unused)
};
hipError_t launch_signal_scan(const SignalScanParams &p, hipStream_t s);
// Pair series (ss_batch_pair_series; ss_pair_series.hip): per (stream, 100 ms entry, channel pair) the f64 sums of x_a^2, x_b^2 and
// x_a x_b over the entry's frames in which both samples are finite, from the resident corpus alone — no pass, no tables.  The grid
// is the peak series' (plan_peak_series' entries_cap).  The records are ss_channel_pair / ss_pair_entry.
constexpr uint32_t kMaxPairs = 16;
// sweep_frames: the frames a workgroup has in flight at a time (256 lanes, four loads each; a 16-byte load holds two stereo frames).
// It fixes which lane adds which frame, and with that the order of every sum.
struct PairSeriesPlan { uint32_t sweep_frames, entries_cap; bool stereo; };
// stereo: two channels and one pair of distinct channels — the form that reads the entry as 16-byte loads
PairSeriesPlan plan_pair_series(uint32_t channels, uint32_t s100, uint64_t n_frames, const ChannelPair *pairs, uint32_t n_pairs);
struct PairSeriesParams {
    const float *pcm;                // [stream][frame][channels] f32, 16-byte aligned
    uint64_t stream_stride;          // floats between streams
    uint64_t n_frames;               // frames of a slot
    const uint64_t *frames_of;       // ragged batches: each stream's own frames (nullable = n_frames for all)
    PairEntry *series;               // [stream][entries_cap][n_pairs]
    uint32_t n_streams, channels, s100;
    uint32_t entries_cap, n_pairs;   // plan_pair_series; 1 .. kMaxPairs
    uint32_t stereo;                 // plan_pair_series
    ChannelPair pairs[kMaxPairs];    // a, b < channels (the caller has checked)
};
hipError_t launch_pair_series(const PairSeriesParams &p, hipStream_t s);
// Pair regions (ss_batch_pair_regions), behind a series on the same stream: the entries' sums added in entry order, the entries
// below the correlation threshold and their runs, and the regions' records added per group in region index order.  The records are
// ss_region_pair / ss_group_pair.
struct RegionPairsParams {
    const PairEntry *series; uint32_t entries_cap, n_pairs;
    double threshold, power_floor; uint32_t min_run;       // ss_pair_region_config (the caller has checked)
    const LoudnessRegion *regions;   // [n_regions], every one inside its stream's entries (the caller has checked)
    RegionPair *results;             // [n_regions][n_pairs]
    uint32_t n_regions, n_groups;
    GroupPair *group_results;        // [n_groups][n_pairs]
};
// reduces every (region, pair) (k_region_pairs), then every (group, pair) over the regions' records (k_group_pairs)
hipError_t launch_region_pairs(const RegionPairsParams &p, hipStream_t s);
// Apply gain (ss_batch_apply_gain; ss_apply_gain.hip): the resident corpus times a gain curve per stream, in place, and per (stream,
// channel) what the result holds.  The host resolves the caller's points into a segment table per touched stream: segment j covers
// the frames [start_j, start_(j+1)) (the last one to the stream's end), and its value at frame n is
//     base == kGainConst:  g            else:  g + (double)(n - base) * d      (ss_gain_envelope, each operation rounded on its own)
// The first segment of a stream starts at frame 0.  The records are ss_gain_channel: the kernel keeps sample_peak as the bits of
// a non-negative f32, whose unsigned order is the values' order.
constexpr uint32_t kGainTileFrames = 4096;                       // frames one workgroup sweeps
constexpr unsigned long long kGainConst = ~0ull;
struct GainSegment { unsigned long long start, base; double g, d; };
struct GainStream { uint32_t stream, seg_first, n_seg, reserved; };       // a touched stream: its segments [seg_first, seg_first + n_seg)
static_assert(sizeof(GainSegment) == 32 && sizeof(GainStream) == 16, "gain table layouts");
struct ApplyGainParams {
    float *pcm;                      // [stream][frame][channels] f32, 16-byte aligned; read and written
    uint64_t stream_stride;          // floats between streams
    uint64_t n_frames;               // frames of a slot
    const uint64_t *frames_of;       // ragged batches: each stream's own frames (nullable = n_frames for all)
    const GainStream *touched;       // [n_touched]
    const GainSegment *segments;
    GainChannel *stats;              // [stream][channels], initialised by the caller (zeros, first_over = ~0)
    uint64_t channel_mask;           // bit c: channel c is multiplied (the caller has resolved 0 to all channels)
    uint32_t n_touched, channels, tiles_cap;      // tiles_cap = ceil(n_frames / kGainTileFrames)
    uint32_t clip_bits;              // the bits of clip_level; 0x7F800001 (above every |y| that is no NaN) for +inf
    uint32_t stereo;                 // two channels, both selected, an even stream_stride: the form with 16-byte accesses
};
// one workgroup per (touched stream, tile); untouched streams cost nothing
hipError_t launch_apply_gain(const ApplyGainParams &p, hipStream_t s);
// Limiter (ss_batch_limit; ss_limiter.hip): the resident corpus times an item's gain and a look-ahead gain curve, in place.  Per
// group of items two launches: k_limit_detect leaves every tile's minimum required gain in tile_min and the r_q of the tiles that
// hold a frame over the ceiling in the group's scratch rows, k_limit_apply rewrites the tiles.  The records are ss_limit_stream and
// ss_gain_channel, initialised by the caller; the kernels add to them with integer atomics.
constexpr uint32_t kLimitTileFrames = 4096;                      // frames one workgroup detects, and sweeps
constexpr uint32_t kLimitOne = 1u << 30;                         // the gain 1 as an integer
using LimitItem = ss_limit_item;
using LimitStream = ss_limit_stream;
static_assert(sizeof(ss_limit_item) == 8 && sizeof(ss_limit_stream) == 32 && sizeof(ss_limit_config) == 40, "limiter records");
struct LimitPlan { uint32_t tile_frames, tiles_cap, group_streams; uint64_t scratch_bytes; };
// tiles_cap = ceil(n_frames / tile_frames); group_streams: the items whose scratch rows (4 bytes x n_frames each) fit scratch_bytes
// together, n_items at most; scratch_bytes: what they take
LimitPlan plan_limit(uint64_t n_frames, uint32_t n_items, uint64_t scratch_bytes);
struct LimitParams {
    float *pcm;                      // [stream][frame][channels] f32, 16-byte aligned; read and written
    uint64_t stream_stride;          // floats between streams
    uint64_t n_frames;               // frames of a slot
    const uint64_t *frames_of;       // ragged batches: each stream's own frames (nullable = n_frames for all)
    const LimitItem *items;          // [items of the call]
    uint32_t *tile_min;              // [items of the call][tiles_cap]
    uint32_t *scratch;               // [group_streams][n_frames]: r_q of the launch's items, row = item - item_first
    LimitStream *streams;            // [stream], initialised by the caller (zeros, first_limited = ~0, min_sum = (L + 1) 2^30)
    GainChannel *stats;              // [stream][channels], initialised by the caller (zeros, first_over = ~0)
    uint64_t channel_mask;           // bit c: channel c is heard and multiplied (the caller has resolved 0 to all channels)
    uint32_t item_first, n_group;    // this launch's items [item_first, item_first + n_group)
    uint32_t channels, tiles_cap;    // tiles_cap: plan_limit
    uint32_t clip_bits;              // the bits of clip_level; 0x7F800001 (above every |y| that is no NaN) for +inf
    uint32_t stereo;                 // two channels, both selected, an even stream_stride: the form with 16-byte accesses
    uint32_t lookahead, hold;        // L, H <= the header's maxima
    uint32_t advance;                // A: taps - 1 where the detector interpolates, else 0
    float ceiling;                   // > 0, finite
    int factor;                      // of the detector: 4, 2 or 0 (the sample's magnitude)
    float taps[36];                  // PeakSeriesParams::taps
};
// the detector and the sweep of one group, queued on s in that order
hipError_t launch_limit(const LimitParams &p, hipStream_t s);
// Resampler (ss_batch_resample; ss_resample.hip): every stream of one corpus converted by L / M into the same slot of another.
// One workgroup per (stream, tile of tile_periods * L outputs); output n0 + i of a tile reads phase (i M) % L at the tile's input
// frame (i M) / L, so the tile's input run is tile_periods * M frames and taps - 1 frames of surroundings.  Three forms, equal in
// bits (each output is the header's one chain):
//   kResampleRegTaps   lane <-> output residue n mod L: its phase's taps stay in registers while it walks n, n + L, ...
//   kResampleLdsTaps   the table in LDS at an odd row stride beside the tile, lane <-> output: any L and T that fit
//   kResampleDirect    taps and samples from global memory, guarded: whatever fits neither
enum : uint32_t { kResampleAuto = 0, kResampleRegTaps = 1, kResampleLdsTaps = 2, kResampleDirect = 3 };
static_assert(sizeof(ss_resample_plan) == 56, "ss_resample_plan");
struct ResamplePlan {
    uint32_t form;                   // kResampleRegTaps ...
    uint32_t tile_periods;           // R: a tile is R * L outputs from R * M inputs
    uint32_t groups, threads;        // register form: residue groups G (lane = g * L + r), and the workgroup's size
    uint32_t lds_bytes;
};
// form: kResampleAuto, or the form to take where it can run the plan (else the next one down the list above)
ResamplePlan plan_resample(uint32_t up, uint32_t down, uint32_t taps, uint32_t channels, uint32_t form);
struct ResampleParams {
    const float *src;                // [stream][frame][channels] f32, 16-byte aligned; read only
    float *dst;                      // the same layout at dst_stride
    const float *taps;               // [L][T] f32, 16-byte aligned
    uint64_t src_stride, dst_stride; // floats between streams
    uint64_t n_frames;               // frames of a source slot
    const uint64_t *frames_of;       // ragged sources: each stream's own frames (nullable = n_frames for all)
    uint32_t n_streams, channels;
    uint32_t up, down, n_taps;       // L, M, T
    uint32_t tiles_cap;              // tiles of the longest output
    ResamplePlan plan;
};
hipError_t launch_resample(const ResampleParams &p, hipStream_t s);
// f32 corpus -> delivery PCM (ss_batch_download_pcm): samples [0, n_samples) of the slots from `first` on become `format` at out,
// frames at or behind a stream's own length the format's zero.  out holds n_samples rounded up to a multiple of 4 samples.
struct PcmOutParams {
    const float *pcm;                // the batch's input, stream 0
    uint64_t per_stream;             // samples of a slot (frames_per_stream * channels)
    uint64_t n_frames;
    const uint64_t *frames_of;       // nullable
    uint64_t n_samples;              // count * per_stream
    unsigned char *out;
    uint64_t seed;
    uint32_t first, channels;
    int format;                      // ss_pcm_format
    uint32_t tpdf;                   // 1: SS_DITHER_TPDF on the integer formats
};
hipError_t launch_f32_to_pcm(const PcmOutParams &p, hipStream_t s);
// gate + LRA on explicit histograms (corpus gate after the all-reduce; handle getters)
// `peaks` (optional): a handle's readings in one launch (ReadingsExtra above)
hipError_t launch_hist_eval(const uint64_t *hist2000, const double *energies, const double *bounds,
                            double *out2, hipStream_t s, const ReadingsExtra *peaks = nullptr);
// mean-square of the filtered ring over the last `frames` frames (handle getters)
constexpr int kRingScratchDoubles = 320;     // k_ring_energy: 256 partial sums + the completion counter; k_tick: kRingTickBlocks + 1 from kRingTickScratch on
constexpr int kRingTickScratch = 264;        // where a tick launch keeps ITS partial sums and count (the two kernels never share a slot)
constexpr int kRingTickBlocks = 32;          // workgroups of a tick launch that sum the ring (at most 64: one lane of the last wave each)
hipError_t launch_ring_energy(const double *ring, uint64_t ring_frames, uint32_t channels,
                              uint64_t end_frame, uint64_t frames, const double *weights,
                              double *out2 /* energy, loudness: device or mapped host memory */,
                              double *scratch /* kRingScratchDoubles, zero before the first launch */,
                              hipStream_t s);

// ---- meter banks (ss_meter_bank_*): N independent streaming meters advanced together --------------------------------------------
// Per stream, laid out as a handle holds its meter: TdState, a sub-block ring [sub_cap][C], the filtered-sample ring
// [ring_frames][C], histograms [2][1000], gating counts [2].
struct MeterBankParams {
    const TdConst *k;
    TdState *state;                  // [stream]
    double *subblocks; uint64_t sub_stride; uint32_t sub_cap;
    double *ring; uint64_t ring_stride; uint64_t ring_frames;
    const double *weights;           // [channels]
    uint64_t *hist;                  // [stream][2][1000]
    uint32_t *counts;                // [stream][2]
    const double *hist_energies;     // 1000
    const double *hist_bounds;       // 1001
    uint32_t n_streams, channels;
    uint32_t st_on;                  // 0: thirty sub-blocks are more than the crate's 3 s ring (the short-term reading is NaN)
};
// gating behind a time-domain launch of `frames` frames per stream (frames_of, device memory, nullable: frames_of[s] for stream s
// instead): stream s's new sub-blocks are [(fed - frames) / S, fed / S), fed = state[s].frames_fed (the streams' phases differ
// after a selective reset or a ragged add)
hipError_t launch_meter_bank_gate(const MeterBankParams &p, uint64_t frames, const uint64_t *frames_of, hipStream_t s);
// every stream's readings into out[stream] (an ss_meter_reading each; device or mapped host memory)
hipError_t launch_meter_bank_readings(const MeterBankParams &p, MeterReading *out, hipStream_t s);
// clears the listed streams' meters (streams == nullptr: streams 0 .. count - 1)
hipError_t launch_meter_bank_reset(const MeterBankParams &p, const uint32_t *streams, uint32_t count, hipStream_t s);

// meter-bank spectra (ss_fft.hip): every stream's newest 16384 frames, kept in a ring, transformed in one launch
constexpr uint32_t kBankSpecN = SS_BANK_SPECTRUM_N;
// the column fold of a bank kernel (the rule: ss_chart_dev.h): the tables of ssh::column_tables with stride = n_bins, and the gain
struct ChartFold {
    const double *pink;              // n_bins f64 pink compensation
    const uint16_t *bin_col;         // n_bins: chart column of every retained bin
    const float *col_init;           // cols: -inf where the column owns a bin, NaN where it owns none
    const double *integrated;        // SS_GAIN_REFERENCE: stream s's integrated loudness at integrated[s * integrated_stride]
    uint32_t integrated_stride;      // (doubles)
    uint32_t cols; float gain_db;    // cols: 1 .. 512
};
struct BankSpectrumParams {
    FftBatchParams f;                // the transform's tables, first_bin / n_bins / db_offset (pink = nullptr, out unused)
    const float *hist;               // [stream][kBankSpecN][channels] f32 ring, frame j at slot j & (kBankSpecN - 1)
    uint32_t start;                  // slot of the window's first frame (fed - kBankSpecN, masked), fed the bank-wide frame counter
    const uint64_t *ahead;           // [stream], nullable: frames stream s has had beyond the bank-wide counter (ragged adds) — its
                                     // window starts at slot (start + ahead[s]) masked
    uint32_t n_streams, channels, rows;   // rows per stream: 2 (mid, side) for stereo, otherwise channels
    int32_t *status;                 // [stream][row]
    float *out;                      // rows: [stream][row][n_bins]; columns: [stream][row][cols]
    ChartFold fold;                  // columns (k_meter_bank_spectrum<true>)
};
// frames [frames - take, frames) of every stream's input (stream s at pcm + s * stride) into the ring at slots (fed + f) & mask;
// ahead (nullable): stream s's own counter is fed + ahead[s]
hipError_t launch_bank_history_append(float *hist, const float *pcm, uint64_t stride, uint64_t frames, uint64_t fed,
                                      const uint64_t *ahead, uint32_t n_streams, uint32_t channels, hipStream_t s);
// ragged adds: stream s's newest min(frames_of[s], 16384) frames (its input at pcm + offset_of[s], or pcm + s * stride where
// offset_of is null) behind its own counter fed + ahead[s], and ahead[s] += frames_of[s]; a stream of 0 frames is left alone
hipError_t launch_bank_history_append_ragged(float *hist, const float *pcm, uint64_t stride, const uint64_t *offset_of,
                                             const uint64_t *frames_of, uint64_t fed, uint64_t *ahead, uint32_t n_streams,
                                             uint32_t channels, hipStream_t s);
hipError_t launch_meter_bank_spectrum(const BankSpectrumParams &p, bool columns, hipStream_t s);

// tracked bank spectra (ss_bank_spectrum_track.hip): an exponentially averaged and a peak-hold curve per row, advanced from the rows
// and statuses launch_meter_bank_spectrum(columns = false) has stored, on each stream's own frame counter
struct BankTrackRow { uint64_t last; uint32_t updates; uint32_t pad; };      // a row's clock: fed at its last accepted update; their count
struct BankTrackParams {
    const float *rows;               // [row][n_bins] f32 dB, rows n_bins floats apart (the update only)
    const int32_t *status;           // [row] (the update only)
    uint64_t fed;                    // the bank-wide frame counter
    const uint64_t *ahead;           // [stream], nullable: stream s's own counter is fed + ahead[s]
    uint32_t n_streams, rows_per_stream, n_bins;
    uint32_t bin_stride;             // n_bins rounded up to a multiple of four
    unsigned char *state;            // [row]: P f64 [bin_stride], peak f32 [bin_stride], age u32 [bin_stride] — 16 * bin_stride bytes
    const BankTrackRow *meta_in;     // [row]: the clocks as they stand
    BankTrackRow *meta_out;          // [row]: the update writes EVERY row's clock here (the host swaps the two; read-outs: unused)
    double rate, average_tau_s, decay_db_per_s;
    uint64_t hold_frames;            // (uint64_t)(hold_s * rate + 0.5); ~0: the peak never falls
};
// the columns read-out: launch_meter_bank_spectrum's column tables and gain; avg / hold [row][cols] and updates [row] are nullable
struct BankTrackColumns {
    ChartFold fold;
    float *avg, *hold; uint32_t *updates;
};
hipError_t launch_bank_spectrum_track(const BankTrackParams &p, hipStream_t s);
// the listed streams' rows lose their state (streams == nullptr: streams 0 .. count - 1); meta: the clocks as they stand
hipError_t launch_bank_spectrum_track_reset(BankTrackRow *meta, const uint32_t *streams, uint32_t count, uint32_t rows_per_stream,
                                            hipStream_t s);
// avg / hold: [row][n_bins] f32 dB (either nullable), updates [row] (nullable)
hipError_t launch_bank_spectrum_tracked_rows(const BankTrackParams &p, float *avg, float *hold, uint32_t *updates, hipStream_t s);
hipError_t launch_bank_spectrum_tracked_columns(const BankTrackParams &p, const BankTrackColumns &c, hipStream_t s);

// signal watch of a bank (ss_meter_bank_signal_watch*; ss_bank_signal_watch.hip): the batch signal scan's records of everything a
// stream was given since its watch reset, advanced by one launch per add call.  What sequence q of a stream (0: the frame is
// silent, 1 + c: channel c is clipped) carries from call to call:
struct alignas(16) BankWatchSeq {
    unsigned long long frames;       // frames watched so far (every sequence keeps its own copy: its owning lane reads no other's)
    unsigned long long open;         // frames of the run that holds the newest frame; 0: none
    unsigned long long runs;         // closed runs of at least the minimum
    unsigned long long best, best_at;// the longest closed run and its first frame (the lowest of equals; ~0: none)
    unsigned long long total;        // frames on which the predicate held
    unsigned long long lead;         // the run that held frame 0, once it has closed
    unsigned long long lead_set;     // 0: the predicate has held on every frame so far
    double sum, sum_sq;              // channel q - 1 (sequence 0: unused): over its finite samples, tile by tile behind the state
    unsigned long long clipped, nonfinite, first_nonfinite, last_clip;   // (~0: none)
};                                   // 112 bytes
// (the records are ss_stream_watch / ss_channel_watch: the batch records, then the live fields)
struct BankWatchParams {
    const float *pcm;                // f32 input of this call, any 4-byte alignment: stream s at pcm + offset_of[s], or pcm + s * stride
    uint64_t stride;                 // floats between streams (offset_of == nullptr)
    const uint64_t *offset_of;       // [stream], nullable
    const uint64_t *frames_of;       // [stream], nullable: every stream gets `frames`; a stream of 0 frames is not touched
    uint64_t frames;
    uint32_t n_streams, channels;
    uint32_t tile_frames;            // plan_signal_scan's
    float silence_threshold, clip_level;
    uint32_t silence_min, clip_min;
    BankWatchSeq *state;             // [stream][channels + 1]
    StreamWatch *streams;            // [stream]
    ChannelWatch *channel_watches;   // [stream][channels]
};
// one workgroup per stream walks its frames of this call in tiles and leaves the state and both records behind
hipError_t launch_bank_signal_watch(const BankWatchParams &p, hipStream_t s);
// the listed streams' state and records are empty (streams == nullptr: streams 0 .. count - 1)
hipError_t launch_bank_signal_watch_reset(BankWatchSeq *state, StreamWatch *stream_watches, ChannelWatch *channel_watches,
                                          const uint32_t *streams, uint32_t count, uint32_t channels, hipStream_t s);

// pair watch of a bank (ss_meter_bank_pair_watch*; ss_bank_pair_watch.hip): the batch pair series' entries of everything a stream
// was given since its pair-watch reset, advanced by one launch per add call.  Per (stream, pair) the device holds
//   - the open entry's lane sums, [3][kPairWatchLanes] f64 (s_aa, s_bb, s_ab: a wave's 64 lanes read consecutive doubles), valid
//     where the stream's open_frames > 0, and the frames of the open entry that were skipped so far (one u32);
//   - the ring of the newest window_entries complete entries, entry j at slot j mod window_entries;
//   - the record, an ss_pair_watch.  The record IS the running state: its totals, counts,
//     run fields, entries and open_frames are read at the start of a call and written at its end.
constexpr uint32_t kPairWatchLanes = 256;
constexpr uint32_t kPairWatchWindowMax = SS_BANK_PAIR_WINDOW_MAX;
struct BankPairWatchParams {
    const float *pcm;                // f32 input of this call, any 4-byte alignment: stream s at pcm + offset_of[s], or pcm + s * stride
    uint64_t stride;                 // floats between streams (offset_of == nullptr)
    const uint64_t *offset_of;       // [stream], nullable
    const uint64_t *frames_of;       // [stream], nullable: every stream gets `frames`; a stream of 0 frames is not touched
    uint64_t frames;
    uint32_t n_streams, channels, s100;
    uint32_t window_entries, n_pairs;// 1 .. kPairWatchWindowMax; 1 .. kMaxPairs
    double threshold, power_floor; uint32_t min_run;      // ss_pair_watch_config (the caller has checked)
    double *lanes;                   // [stream][pair][3][kPairWatchLanes]
    uint32_t *open_skipped;          // [stream][pair]
    PairEntry *ring;                 // [stream][window_entries][pair]
    PairWatch *records;              // [stream][pair]
    ChannelPair pairs[kMaxPairs];    // a, b < channels (the caller has checked)
};
// one workgroup per stream walks its frames of this call entry by entry and leaves the state, the ring and the records behind
hipError_t launch_bank_pair_watch(const BankPairWatchParams &p, hipStream_t s);
// the listed streams' records are empty (streams == nullptr: streams 0 .. count - 1); open_frames == 0 and entries == 0 make the
// lane sums and the ring unread
hipError_t launch_bank_pair_watch_reset(PairWatch *records, uint32_t *open_skipped, const uint32_t *streams, uint32_t count,
                                        uint32_t n_pairs, hipStream_t s);

// ---- waveform ---------------------------------------------------------------
struct WaveParams {
    const float *pcm; uint64_t stream_stride; uint64_t n_samples; // interleaved samples per stream
    uint32_t n_streams; uint32_t window;   // number of decimation bins W
    float *out; uint64_t out_stride;       // [stream][W][2] f32 (min, max)
    const uint64_t *samples_of;   // ragged batches: interleaved samples / bins of each stream (nullable)
    const uint32_t *window_of;
    uint32_t mid_of_pairs;        // 1: `pcm` holds n_samples stereo PAIRS and the signal decimated is their mid, (l + r) / 2
                                  // (audio_player.rs:400-419 on the fly: the capture tick's chart, tui.rs:1453-1455)
};
hipError_t launch_waveform(const WaveParams &p, hipStream_t s);

// ---- utilities --------------------------------------------------------------
// raw little-endian PCM -> f32 (format: 1 u8, 2 s16, 3 s24, 4 s32, 5 f32, 6 f64)
hipError_t launch_pcm_to_f32(const void *src, size_t n_samples, int format, float *dst, hipStream_t s);
// render-side reductions (N3)
hipError_t launch_render_spectrum(const float *rows, uint32_t bin_stride, uint32_t n_bins, uint64_t n_rows,
                                  uint32_t rows_per_stream, const uint32_t *col_start, uint32_t cols,
                                  const double *integrated, float gain_db, float *out, hipStream_t s);
hipError_t launch_render_waveform(const float *wave, uint64_t wave_stride, uint32_t n_points, uint32_t n_streams,
                                  uint32_t x_min, uint32_t x_max, uint32_t cols, float *out, hipStream_t s);
hipError_t launch_mid_side(const float *interleaved, size_t frames, float *mid, float *side, hipStream_t s);
// pairs of an interleaved buffer whose mid or side value ((l + r) / 2, (l - r) / 2 in f32) is NaN or infinite — normally none:
// the tick drivers' index for the crate's NaN / infinity rejection.  cls bits: 1 mid NaN, 2 mid inf, 4 side NaN, 8 side inf.
// *count (zeroed by the launcher) counts ALL such pairs; the first `cap` to arrive are listed (in no particular order).
struct NonFinitePair { unsigned long long index; uint32_t cls; uint32_t pad; };
hipError_t launch_nonfinite_pairs(const float *interleaved, size_t pairs, uint32_t *count, NonFinitePair *list, uint32_t cap, hipStream_t s);
// verification utility: out[item * out_stride] += order-independent checksum of words [item * stride_words, + words) (32-bit words)
hipError_t launch_checksum(const void *base, uint64_t words, uint64_t stride_words, uint32_t n_items, uint64_t *out,
                           uint32_t out_stride, hipStream_t s);
// clears up to four device buffers (byte counts: multiples of four; null / zero entries are skipped) in one launch
hipError_t launch_zero4(void *const ptrs[4], const size_t bytes[4], hipStream_t s);
// measurement utility: k_fft4096_ms1's loads and stores with no arithmetic (same grid, occupancy and addresses)
hipError_t launch_fft4096_traffic(const FftBatchParams &p, hipStream_t s);
hipError_t launch_synth(float *pcm, uint32_t n_streams, uint64_t frames, uint32_t channels,
                        uint32_t rate, uint64_t seed, uint32_t first_id, hipStream_t s);

}  // namespace ssk
