// ss_batch.cpp — the batch extension of the C ABI (NOT in the reference): many streams resident in HBM analysed in one
// pass — the data-parallel form of receive_audio_file + analyze_audio_file_samples
// (the reference's src/tui.rs:1207-1241, :1482-1552) over a corpus — plus the render-side reductions (N3) and the
// one-shot calculate_integrated_lufs (src/analyzer.rs:170-182), which runs the batch path on one stream.
#include "ss_host.h"

using namespace ssh;

// ============================================================================
//  batch
// ============================================================================
namespace {

// Per-kernel event timing: a ring of kDepth passes' event sets, so that timed passes queue back to back without a host
// synchronisation between them (bench.py times its kernels INSIDE the timed region); collected when read, or when the ring is full.
struct TimingRing {
    static constexpr uint32_t kDepth = 32;
    bool on = false;
    hipEvent_t ev[kDepth * 2 * SS_KERNEL_COUNT] = {};   // [pass][kernel][edge]
    uint32_t mask[kDepth] = {};                         // which of a pass's events were recorded
    uint32_t head = 0, count = 0;                       // next slot to record into; passes recorded and not yet collected
    double ms[SS_KERNEL_COUNT] = {};
    uint64_t launches[SS_KERNEL_COUNT] = {};
    ~TimingRing() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t create() { hipError_t r = hipSuccess; for (auto &e : ev) if (r == hipSuccess) r = hipEventCreate(&e); return r; }
    // edge 0: the kernel's slot of this pass begins on `stream`, 1: it has ended (timing off: nothing)
    hipError_t mark(int kernel, int edge, hipStream_t stream)
    {
        if (!on) return hipSuccess;
        const int idx = 2 * kernel + edge;
        mask[head] |= 1u << idx;
        return hipEventRecord(ev[(size_t)head * 2 * SS_KERNEL_COUNT + idx], stream);
    }
    void advance() { if (on) { head = (head + 1u) % kDepth; count++; } }      // the pass is queued
    int collect(hipStream_t stream)
    {
        if (!count) return SS_OK;
        HIPCHK(hipStreamSynchronize(stream));
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t slot = (head + kDepth - count + i) % kDepth;
            hipEvent_t *e = ev + (size_t)slot * 2 * SS_KERNEL_COUNT;
            for (int k = 0; k < SS_KERNEL_COUNT; k++) {
                if ((mask[slot] >> (2 * k) & 3u) != 3u) continue;       // this pass did not run kernel k
                float t = 0.f;
                if (hipEventElapsedTime(&t, e[2 * k], e[2 * k + 1]) == hipSuccess) { ms[k] += t; launches[k]++; }
            }
            mask[slot] = 0;
        }
        count = 0;
        return SS_OK;
    }
    void reset() { for (int k = 0; k < SS_KERNEL_COUNT; k++) { ms[k] = 0; launches[k] = 0; } }
};

// opt-in (ss_batch_set_overlap): the spectrum kernel on a second stream beside the time-domain chain
struct Overlap {
    int mode = 0;                     // 0 sequential, 1 the spectrum kernel beside the time-domain chain, 2 beside its tail only
    hipStream_t stream2 = nullptr;    // (from the pool: ss_batch_destroy hands it back)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    ~Overlap() { for (hipEvent_t e : {ev_fork, ev_join}) if (e) (void)hipEventDestroy(e); }
    // what is queued on `then` from here on runs behind everything queued on `first` so far
    static hipError_t order(hipEvent_t ev, hipStream_t first, hipStream_t then) { hipError_t e = hipEventRecord(ev, first); return e == hipSuccess ? hipStreamWaitEvent(then, ev, 0) : e; }
    // fork: stream2 goes on behind everything already queued on the main stream (uploads, the previous pass)
    hipError_t fork(hipStream_t main_stream) { return order(ev_fork, main_stream, stream2); }
    // join: later work on the main stream (downloads, the next pass) sees what stream2 did
    hipError_t join(hipStream_t main_stream) { return order(ev_join, stream2, main_stream); }
};

// columns-only spectrum (SS_BATCH_FFT_COLUMNS): the reduction fused into the spectrum kernel's epilogue
struct Columns {
    bool on = false;
    int gain_mode = SS_GAIN_FIXED;
    float gain_db = 0.0f;
    DevBuf<uint16_t> bin_col;       // chart column of every retained bin (0xFFFF for the row padding)
    DevBuf<uint2> groups;           // the same per group of four bins (FftBatchParams::col_groups)
    DevBuf<float> init;             // FftBatchParams::col_init
    DevBuf<uint2> bins;             // FftBatchParams::col_bins
};

// ragged batches (ss_batch_set_lengths): per-stream frames / windows / sub-blocks / decimation bins
struct Ragged {
    bool on = false;
    std::vector<uint64_t> frames_h;
    std::vector<uint32_t> sub_h;
    uint32_t max_sub = 0;           // sub-blocks of the LONGEST stream (the time-domain geometry follows the lengths, not the slot size)
    DevBuf<uint64_t> frames_d, wave_samples_d;
    DevBuf<uint32_t> windows_d, sub_d, wave_window_d;
};

// per-stream average and peak-hold spectrum (ss_batch_spectrum_stats): all of it allocated at the batch's first reduction, so a
// batch that never asks holds none of it
struct SpecStats {
    bool done = false;                          // a reduction has been queued: there is something to download
    DevBuf<double> sums, part_sums;             // SpecStatsParams' arrays of these names
    DevBuf<float> mean, max, part_max;
    DevBuf<uint32_t> counts, part_counts;
    DevBuf<float> corpus_mean, corpus_max;      // ss_batch_corpus_spectrum: [fft_channels][fft_bin_stride]
    DevBuf<unsigned long long> corpus_counts;   // [fft_channels]
};

// The region list of a follow-up call (ss_batch_loudness_regions, ss_batch_peak_regions, ss_batch_spectrum_regions,
// ss_batch_pair_regions).  Each of the
// four holds its own, stage included: a loudness list, a peak list, a spectrum list and a pair list live side by side.
struct RegionList {
    bool done = false;                          // a list has been queued: there is something to download
    uint32_t n_regions = 0, n_groups = 0;       // of the last call that was queued
    HostStage stage;                            // the caller's list on its way to the device
    DevBuf<ssk::LoudnessRegion> dev;
    // the device list becomes the caller's (checked: check_regions), behind whatever is queued on the batch's stream
    int replace(hipStream_t stream, const ss_loudness_region *regions, uint32_t n)
    {
        HIPCHK(dev.ensure(n));                  // (a buffer that grows is freed first: hipFree waits for whatever still uses it)
        if (n) HIPCHK(stage.send(dev.p, regions, (size_t)n * sizeof(ss_loudness_region), stream));
        return SS_OK;
    }
    void queued(uint32_t n, uint32_t groups) { n_regions = n; n_groups = groups; done = true; }     // ... and its launch is queued
};

// loudness regions (ss_batch_loudness_regions): all of it allocated at the batch's first call and grown by a longer list, so a
// batch that never asks holds none of it
struct Regions {
    RegionList list;
    DevBuf<ssk::RegionResult> results;
    DevBuf<ssk::GroupResult> group_results;
    DevBuf<unsigned long long> group_hist;      // [group][2][1000]
};

// peak series and peak regions (ss_batch_peak_series, ss_batch_peak_regions): all of it allocated at the batch's first call (the
// regions' part grown by a longer list), so a batch that never asks holds none of it
struct Peaks {
    bool series_done = false;                           // queued at least once: there is something to download
    DevBuf<ss_peak_entry> series;                       // [stream][entries_cap][channels]
    RegionList list;                                    // of the last ss_batch_peak_regions
    DevBuf<ssk::RegionPeaks> results;
    DevBuf<float> ch_true, ch_sample;                   // [region][channels]
    DevBuf<unsigned long long> group_acc;               // [group][3] (RegionPeaksParams::group_acc)
    DevBuf<ssk::GroupPeaks> group_results;
};

// spectrum regions (ss_batch_spectrum_regions): all of it allocated at the batch's first call and grown by a longer list, so a
// batch that never asks holds none of it.  The kernels read the list as the host resolved it — `table`: the ssk::SpecRegion
// records, then the groups' member lists — which goes through the list's stage in one upload; the list's own `dev` stays empty.
struct SpectrumRegions {
    RegionList list;
    ssk::SpecStatsPlan plan;                            // of the last list that was queued
    DevBuf<uint32_t> table;                             // 4 words per region, member_start [n_groups + 1], members [grouped regions]
    DevBuf<double> sums, part_sums;                     // SpecRegionsParams::s' arrays of these names
    DevBuf<float> mean, max, part_max;
    DevBuf<uint32_t> counts, part_counts;
    DevBuf<float> group_mean, group_max;                // [group][fft_channels][fft_bin_stride]
    DevBuf<unsigned long long> group_counts;            // [group][fft_channels]
};

// signal scan (ss_batch_signal_scan): all of it allocated at the batch's first call (the lists grown by a larger max_events), so a
// batch that never asks holds none of it
struct SignalScan {
    bool done = false;                                  // queued at least once: there is something to download
    ss_signal_scan_config cfg{};                        // of the last call that was queued
    DevBuf<ssk::SignalTileRuns> tile_runs;              // [stream][tiles_cap][channels + 1]
    DevBuf<ssk::SignalTileChannel> tile_channels;       // [stream][tiles_cap][channels]
    DevBuf<ssk::SignalTileCarry> tile_carry;            // [stream][tiles_cap][channels + 1]
    DevBuf<uint32_t> list_base;                         // [stream][channels + 1]
    DevBuf<ssk::StreamScan> streams;                    // [stream] records (ss_stream_scan)
    DevBuf<ssk::ChannelScan> channels;                  // [stream][channels] records (ss_channel_scan)
    DevBuf<ssk::SignalEvent> events;                    // [stream][2][max_events] records (ss_signal_event)
};

// pair series and pair regions (ss_batch_pair_series, ss_batch_pair_regions): all of it allocated at the batch's first call (the
// series grown by a longer pair list, the regions' part by a longer region list), so a batch that never asks holds none of it
struct Pairs {
    bool series_done = false;                           // queued at least once: there is something to download
    uint32_t n_pairs = 0;                               // of the last series that was queued
    ssk::ChannelPair pairs[ssk::kMaxPairs] = {};
    DevBuf<ssk::PairEntry> series;                      // [stream][entries_cap][n_pairs] records (ss_pair_entry)
    RegionList list;                                    // of the last ss_batch_pair_regions
    uint32_t list_pairs = 0;                            // pairs of the series that list was reduced from
    DevBuf<ssk::RegionPair> results;                    // [region][list_pairs] records (ss_region_pair)
    DevBuf<ssk::GroupPair> group_results;               // [group][list_pairs] records (ss_group_pair)
};

// apply gain (ss_batch_apply_gain): all of it allocated at the batch's first call and grown by a longer point list, so a batch that
// never asks holds none of it.  One table per call goes through the stage in one upload: the records [stream][channels] as an
// untouched batch reads them (the kernel adds to them), then the touched streams, then their segments.
struct Gain {
    bool done = false;                          // queued at least once: there is something to download
    HostStage stage;
    DevBuf<unsigned char> table;
};

// limiter (ss_batch_limit): all of it allocated at the batch's first call and grown only, so a batch that never asks holds none of it.
// One table per call: the stream records [stream], the channel records [stream][channels] and the items go through the stage in one
// upload; the tiles' minima [item][tiles_cap] lie behind them and are the kernels' own.  scratch: the r_q rows of one group of items.
struct Limit {
    bool done = false;                          // queued at least once: there is something to download
    HostStage stage;
    DevBuf<unsigned char> table;
    DevBuf<uint32_t> scratch;
};

// resampler (ss_batch_resample), held by the DESTINATION batch: the taps table of the last plan on the device and the two events
// that order the call between the batches' streams — all of it made at the batch's first call, so a batch that never asks holds
// none of it
struct Resample {
    bool have = false;                          // `taps` holds the table of `plan`
    ss_resample_plan plan{};
    DevBuf<float> taps;                         // [L][T]
    hipEvent_t ev_src = nullptr, ev_done = nullptr;
    ~Resample() { for (hipEvent_t e : {ev_src, ev_done}) if (e) (void)hipEventDestroy(e); }
};

// spectrogram (ss_batch_spectrogram): all of it allocated at the batch's first call and grown by a larger view, so a batch that
// never asks holds none of it
struct Spectrogram {
    bool done = false;                          // a view has been queued: there is something to download
    ss_spectrogram_view view{};                 // of the last call that was queued
    uint32_t map_cols = 0;                      // the f_cols bin_col was built for (0: not yet)
    HostStage stage;                            // bin_col on its way to the device
    DevBuf<uint16_t> bin_col;                   // SpectrogramParams::bin_col (full-row batches)
    DevBuf<float> out;                          // [stream][fft_channel][t_cols][f_cols]
    DevBuf<uint32_t> part;                      // SpectrogramParams::part (plans with runs)
};

}  // namespace

struct ss_batch {
    int device = 0;             // the HIP device this batch lives on
    ss_batch_config cfg{};
    ss_batch_layout lay{};
    hipStream_t stream = nullptr;
    int tp_factor = 0;
    ssk::SpecPlan spec;         // the spectrum kernel, its rows and its grid (ssk::plan_spectrum)
    uint64_t first_start = 0;
    uint32_t wave_window = 0;
    struct {                        // how the time-domain launch cuts the streams (choose_td_geometry): TdParams' fields of these names
        uint32_t nseg = 1, seg_sub = 0, warm_sub = 0, fix_sub = 0;
        uint32_t split_batch = ssk::kTdSplitNone;       // (ragged lengths: one wave per stream / segment)
        bool fixup = false;                             // segments > 0 hand over exactly: the fix-up launch re-runs their first fix_sub
    } td_plan;
    int td_mode = 0;                // ss_batch_set_time_domain_mode
    bool wave_fused = false;     // decimation runs inside the time-domain kernel
    uint32_t wave_halo = 0;
    FftTables *ft = nullptr;
    BinTables *bt = nullptr;
    TdTables *td = nullptr;
    const double *hist_energies = nullptr, *hist_bounds = nullptr;      // the gate's histogram tables (get_hist_tables)
    DevBuf<float> pcm, fft, wave;
    DevBuf<ssk::TdState> state;
    DevBuf<double> sub, weights, integrated, lra, out2;
    DevBuf<double> seg_state;       // [stream][segment][channel][4]: the filter state behind every time segment (exact hand-over)
    DevBuf<uint64_t> hist, corpus;
    DevBuf<uint32_t> counts;
    DevBuf<unsigned char> raw;      // device staging of raw PCM for the asynchronous ingest
    DevBuf<uint64_t> checks;        // ss_batch_checksums: [stream][3]
    // SS_BATCH_LOUDNESS_SERIES: [stream][sub_cap()][2] (momentary, short-term) LUFS and the per-stream maxima
    DevBuf<double> series;
    DevBuf<ssk::LoudnessExtremes> extremes;
    Ragged ragged;
    // render-side reductions (N3); render_spec holds the columns-only rows as well
    DevBuf<float> render_spec, render_wave;
    DevBuf<uint32_t> col_start;
    uint32_t render_cols = 0, render_wave_cols = 0;
    Columns cols;
    SpecStats stats;
    Regions regions;
    Peaks peaks;
    SpectrumRegions spec_regions;
    SignalScan scan;
    Pairs pair;
    Gain gain;
    Limit limit;
    Resample resample;
    Spectrogram spectrogram;
    Overlap ov;
    bool corpus_reduced = false;      // this pass's corpus histograms already hold the all-reduced sums
    int tp_arith = SS_TP_ARITH_F32;   // SS_TP_ARITH_*: the reference's width unless the caller opts into the f16 split
    TimingRing timing;

    // sub-block slots per stream in sub and series (a stream shorter than one sub-block still has a slot)
    uint32_t sub_cap() const { return lay.n_subblocks ? lay.n_subblocks : 1; }
    size_t samples_per_stream() const { return (size_t)cfg.frames_per_stream * cfg.channels; }
    // a stream's own length: what ss_batch_set_lengths gave it, else the slot's (a kernel: the per-stream array, or null for the slot's)
    uint64_t frames_of(uint32_t s) const { return ragged.on ? ragged.frames_h[s] : cfg.frames_per_stream; }
    uint32_t subblocks_of(uint32_t s) const { return ragged.on ? ragged.sub_h[s] : lay.n_subblocks; }
    template <typename T> const T *ragged_ptr(const DevBuf<T> &of_stream) const { return ragged.on ? of_stream.p : nullptr; }
};

namespace ssi {
void *batch_corpus_device(ss_batch *b) { return b ? b->corpus.p : nullptr; }
hipStream_t batch_stream(ss_batch *b) { return b ? b->stream : nullptr; }
int batch_device(const ss_batch *b) { return b ? b->device : 0; }
bool &batch_corpus_reduced(ss_batch *b) { return b->corpus_reduced; }
}  // namespace ssi

namespace {

// What a stream of F frames holds under a batch's config (ss_batch_create, ss_batch_set_lengths, ss_batch_stream_shape):
//  * spectrum windows at the cadence of analyze_audio_file_samples (tui.rs:1482-1526): window [p-N, p) at p = k*hop, skipped
//    when p - N == 0 (saturating_sub) => k from N/hop + 1 to F/hop;
//  * 100 ms sub-blocks of s100 frames (s100 = 0: no time-domain pass);
//  * get_waveform's decimation window and bins over the F x C samples (waveform_shape).
struct StreamShape {
    uint32_t windows = 0, subblocks = 0;
    size_t wave_window = 0, wave_bins = 0;
};
StreamShape stream_shape(const ss_batch_config &c, uint64_t s100, uint64_t F)
{
    StreamShape sh;
    if ((c.flags & SS_BATCH_FFT) && c.hop_frames) {
        const uint64_t hop = c.hop_frames, k_min = c.fft_n / hop + 1, k_max = F / hop;
        sh.windows = k_max >= k_min ? (uint32_t)(k_max - k_min + 1) : 0;
    }
    if (s100) sh.subblocks = (uint32_t)(F / s100);
    if (c.flags & SS_BATCH_WAVEFORM) {
        const double win = c.waveform_window > 0.0 ? c.waveform_window : (double)F / (double)c.sample_rate;
        waveform_shape((size_t)(F * c.channels), win, &sh.wave_window, &sh.wave_bins);
    }
    return sh;
}
StreamShape stream_shape(const ss_batch *b, uint64_t F) { return stream_shape(b->cfg, b->td ? b->td->host.s100 : 0, F); }

// ---- the parameter blocks of a pass's launches --------------------------------------------------------------------

// the spectrum launch of a batch (ss_batch_run, ss_batch_traffic_floor): the plan's and the tables' fields, rows with the pink
// compensation, the batch's input and rows, the ragged window counts, the columns-only reduction
ssk::FftBatchParams batch_fft_params(const ss_batch *b)
{
    const ss_batch_config &c = b->cfg;
    ssk::FftBatchParams p = spectrum_params(b->spec, *b->ft, *b->bt, true);
    p.pcm = b->pcm.p; p.out = b->fft.p;
    p.frames_per_stream = c.frames_per_stream; p.first_start = b->first_start;
    p.n_streams = c.n_streams; p.channels = c.channels; p.n_windows = b->lay.n_windows; p.hop = c.hop_frames;
    p.windows_of = b->ragged_ptr(b->ragged.windows_d);
    if (b->cols.on) {
        p.out_cols = b->render_spec.p; p.bin_col = b->cols.bin_col.p; p.col_groups = b->cols.groups.p; p.col_init = b->cols.init.p; p.col_bins = b->cols.bins.p; p.cols = b->render_cols;
        p.integrated = b->cols.gain_mode == SS_GAIN_REFERENCE ? b->integrated.p : nullptr;
        p.gain_db = b->cols.gain_db;
    }
    return p;
}

// the time-domain launch and its fix-up (a batch with a meter pass: b->td)
ssk::TdParams batch_td_params(const ss_batch *b)
{
    const ss_batch_config &c = b->cfg;
    const uint32_t C = c.channels;
    ssk::TdParams p{};
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * C; p.n_frames = c.frames_per_stream;
    p.n_streams = c.n_streams; p.channels = C; p.k = b->td->dev.p; p.state = b->state.p;
    p.subblocks = b->sub.p; p.sub_cap = b->sub_cap();
    p.sub_stride = (uint64_t)p.sub_cap * C; p.tp_factor = b->tp_factor;
    const auto &plan = b->td_plan;
    p.s100 = b->td->host.s100; p.nseg = plan.nseg; p.seg_sub = plan.seg_sub;
    p.warm_sub = plan.warm_sub; p.fix_sub = plan.fix_sub; p.split_batch = plan.split_batch;
    if (plan.fixup) p.seg_state = b->seg_state.p;       // (sized with the plan: choose_td_geometry)
    p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.tp_f32 = b->tp_arith == SS_TP_ARITH_F32 ? 1u : 0u;
    if (b->wave_fused && !b->ragged.on) { p.wave_out = b->wave.p; p.wave_stride = (uint64_t)2 * b->wave_window; p.wave_window = b->wave_window; p.halo_frames = b->wave_halo; }
    return p;
}

// the gating of every stream's sub-blocks and the loudness series behind it
ssk::FinalizeParams batch_gating_params(const ss_batch *b)
{
    const uint32_t C = b->cfg.channels;
    ssk::FinalizeParams f{};
    f.k = b->td->dev.p; f.subblocks = b->sub.p; f.sub_cap = b->sub_cap();
    f.sub_stride = (uint64_t)f.sub_cap * C;
    f.hist_energies = b->hist_energies; f.hist_bounds = b->hist_bounds; f.weights = b->weights.p; f.hist = b->hist.p;
    f.corpus_hist = b->corpus.p; f.n_streams = b->cfg.n_streams; f.channels = C;
    f.sub_begin = 0; f.sub_end = b->lay.n_subblocks;
    f.sub_end_of = b->ragged_ptr(b->ragged.sub_d);
    f.out_integrated = b->integrated.p; f.out_lra = b->lra.p; f.out_counts = b->counts.p;
    f.state = b->state.p;
    return f;
}

// the standalone decimation (where the time-domain kernel does not carry it)
ssk::WaveParams batch_wave_params(const ss_batch *b)
{
    const ss_batch_config &c = b->cfg;
    ssk::WaveParams p{};
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * c.channels; p.n_samples = c.frames_per_stream * c.channels;
    p.n_streams = c.n_streams; p.window = b->wave_window; p.out = b->wave.p; p.out_stride = (uint64_t)2 * b->wave_window;
    p.samples_of = b->ragged_ptr(b->ragged.wave_samples_d); p.window_of = b->ragged_ptr(b->ragged.wave_window_d);
    return p;
}

// how ss_batch_spectrum_stats cuts this batch's rows (fixed with the shape)
ssk::SpecStatsPlan batch_stats_plan(const ss_batch *b)
{
    return ssk::plan_spectrum_stats(b->cfg.n_streams * b->lay.fft_channels, b->lay.fft_bin_stride, b->lay.n_windows);
}

// the reduction of the rows a pass left (ss_batch_spectrum_stats and what reads its results): the rows, the ragged window counts,
// the plan, the batch's result arrays
ssk::SpecStatsParams batch_stats_params(const ss_batch *b)
{
    const ss_batch_layout &L = b->lay;
    const SpecStats &st = b->stats;
    ssk::SpecStatsParams p{};
    p.rows = b->fft.p; p.bin_stride = L.fft_bin_stride; p.n_bins = L.n_bins;
    p.n_streams = b->cfg.n_streams; p.fft_ch = L.fft_channels; p.n_windows = L.n_windows;
    p.windows_of = b->ragged_ptr(b->ragged.windows_d);
    p.plan = batch_stats_plan(b);
    p.sums = st.sums.p; p.mean = st.mean.p; p.max = st.max.p; p.counts = st.counts.p;
    p.part_sums = st.part_sums.p; p.part_max = st.part_max.p; p.part_counts = st.part_counts.p;
    return p;
}

// ---- the steps of a pass ------------------------------------------------------------------------------------------

// meter state, histograms, corpus histograms and block counts start from zero: one launch (they were four fills)
hipError_t zero_meter(ss_batch *b)
{
    void *const ptrs[4] = {b->state.p, b->hist.p, b->corpus.p, b->counts.p};
    const size_t bytes[4] = {b->state.n * sizeof(ssk::TdState), b->hist.n * sizeof(uint64_t), b->corpus.n * sizeof(uint64_t),
                             b->counts.n * sizeof(uint32_t)};
    return ssk::launch_zero4(ptrs, bytes, b->stream);
}

// the spectrum step, wherever the pass puts it; forked: on stream2, behind what the main stream holds so far
int spectrum_step(ss_batch *b, bool forked)
{
    if (forked) HIPCHK(b->ov.fork(b->stream));
    HIPCHK(b->timing.mark(SS_KERNEL_FFT, 0, b->stream));
    if ((b->cfg.flags & SS_BATCH_FFT) && b->lay.n_windows)
        HIPCHK(ssk::launch_spectrum(b->spec, batch_fft_params(b), forked ? b->ov.stream2 : b->stream));
    HIPCHK(b->timing.mark(SS_KERNEL_FFT, 1, b->stream));
    return SS_OK;
}

// ---- plans made when the shape is known ---------------------------------------------------------------------------

// How the time-domain kernel walks a stream.
//  * whole-stream workgroups (kTdSplitStreams): a stream is ONE segment, its tiles dealt to the four waves of a workgroup, the filter state
//    and the lanes' energy shares handed from tile to tile through LDS — the whole recurrence, nothing truncated.  Needs enough
//    streams to fill the chip with one workgroup each (n_streams x 4 waves against the W0 the chip holds); stereo and eight
//    channels, equal lengths.
//  * segments (the rest): a stream is cut into nseg runs of whole sub-blocks, one wave each; a segment > 0 starts its filter
//    kTdWarmSub sub-blocks (0.1 s) early from a zero state and drops that run-in (what the missing history would add to the
//    output has decayed to 1e-9 of a DC step by then, ss_time_domain.hip).  A segment costs its run-in; pick the segment
//    length that maximises   useful fraction  seg / (seg + warm)  x  fill of the last round  waves / (ceil(waves / W0) W0)
//    (ranks the measured config-5 sweep seg = 2..13 in the right order; measured within noise for config 3).
// mode (ss_batch_set_time_domain_mode): 0 the better score of the two, 1 segments, 2 whole-stream workgroups where the shape allows.
// The plan's hand-over states (seg_state) are sized here, so a pass allocates nothing: nothing may be running on the batch.
int choose_td_geometry(ss_batch *b)
{
    if (!b->td) return SS_OK;
    const ss_batch_config *cfg = &b->cfg;
    const uint32_t C = cfg->channels;
    const uint32_t nsub = b->ragged.max_sub;             // (equal lengths: of every stream, ss_batch_create)
    const double W0 = 256.0 * ssk::td_resident_waves_per_cu(C, b->td->host.s100, b->wave_fused ? b->wave_halo : 0);
    // what a segment boundary costs, in sub-blocks of full work: the run-in (mode 1), or the fix-up's re-run of kTdFixSub sub-blocks
    // at about 0.8 of a full tile each (filter and energies are most of a tile) — config 5's sweep seg = 2 ... 10 with the fix-up:
    // 2.39 / 2.21 / 2.13 / 2.53 / 2.65 / 3.60 ms, best at 4
    const double boundary_cost = b->td_mode == 1 ? (double)kTdWarmSub : 0.8 * (double)kTdFixSub;
    auto score_of = [&](uint32_t seg, uint32_t nseg) {
        const double waves = (double)cfg->n_streams * nseg;
        const double useful = nseg > 1 ? (double)seg / ((double)seg + boundary_cost) : 1.0;
        return useful * waves / (std::ceil(waves / W0) * W0);
    };
    // shortest segment: with the exact hand-over the state a segment leaves is only as good as the segment is long (it started from
    // zero): kTdFixSub sub-blocks at least, so that what it hands on has converged like the fix-up's own re-run
    const uint32_t min_seg = b->td_mode == 1 ? kTdWarmSub : kTdFixSub;
    // Time segments stand on the filter FORGETTING: a segment starts from zero, and what it hands on (fix-up) or what it ran in
    // from (mode 1) is right once the zero-input response of the true state has died — radius^n over min_seg sub-blocks,
    // exp(-48) = 1.6e-21 at every ordinary rate (the 38 Hz high-pass pair: n and 1 - radius scale with the rate alike).  The
    // crate accepts rates from 16 Hz (a sub-block is 2 frames there; between ~100 Hz and ~3.4 kHz the design is not even
    // stable): where radius^n has not fallen below 1e-18 a stream is ONE segment (tools/fuzz_handle.py: 0.1 - 1 LU off at 16 Hz).
    bool forgets = false;
    {
        const double r = sst::kweight_pole_radius((double)cfg->sample_rate);
        const double n = (double)min_seg * (double)b->td->host.s100;
        forgets = r < 1.0 && n * std::log(r) < std::log(b->td_mode == 1 ? 1e-9 : 1e-18);       // (mode 1 is the approximate one: 4e-11 after its 0.1 s)
    }
    uint32_t best_seg = 0;
    double best = nsub ? score_of(nsub, 1) : 0.0;                         // one segment: no run-in
    for (uint32_t want = 2; forgets && want <= nsub; want++) {          // balanced segments: seg = ceil(nsub / want)
        const uint32_t seg = (nsub + want - 1) / want;
        if (seg < min_seg) break;
        const double sc = score_of(seg, (nsub + seg - 1) / seg);
        if (sc > best * 1.0000001) { best = sc; best_seg = seg; }
    }
#ifdef SS_TUNING
    if (const char *e = std::getenv("SS_TD_SEG_SUB")) best_seg = (uint32_t)std::atoi(e);
#endif
    const bool split_ok = (C == 2 || C == 8) && nsub > 0;
    const double wsplit = 4.0 * cfg->n_streams;
    const double split_score = split_ok ? wsplit / (std::ceil(wsplit / W0) * W0) : 0.0;
    // (measured at the bench shape: the coupled waves of a workgroup run 16 % behind independent segment waves — the chain makes a
    // workgroup as slow as its slowest wave, tile by tile — so the automatic choice wants a clear win in fill)
    auto &plan = b->td_plan;
    plan = {};
    uint32_t split = ssk::kTdSplitNone;
    if (split_ok && (b->td_mode == 2 || (b->td_mode == 0 && 0.8 * split_score > best))) split = ssk::kTdSplitStreams;
    else if (best_seg >= min_seg && best_seg < nsub) { plan.seg_sub = best_seg; plan.nseg = (nsub + best_seg - 1) / best_seg; }
    // A handful of streams (one file): even the shortest segments leave most of the chip idle, and a pass takes as long as ONE
    // wave needs for its segment's tiles, one after the other.  There a segment's tiles are dealt to the eight waves of a
    // workgroup instead (the whole-stream form, per segment): if eight waves per shortest segment still fit the chip at once.
    const uint32_t nseg_min = (nsub + min_seg - 1) / min_seg;
    if (forgets && split_ok && b->td_mode == 0 && split == ssk::kTdSplitNone && nsub > min_seg && 8.0 * cfg->n_streams * nseg_min <= W0) {
        split = ssk::kTdSplitSegments; plan.seg_sub = min_seg; plan.nseg = nseg_min;
    }
    if (!b->ragged.on) plan.split_batch = split;          // (ragged lengths: one wave per stream / segment, kTdSplitNone)
    // How segments > 0 start.  The exact hand-over: no run-in, their first kTdFixSub sub-blocks re-run from the true state by a
    // second launch (launch_time_domain_fixup).  Mode 1: the 0.1 s run-in from a zero state of rounds 1-4.  Segments of eight
    // waves (the pass is a latency chain, and a second launch is a fifth of it): every segment runs the FILTER over the kTdFixSub
    // sub-blocks in front of it, from zero, inside the one launch — the state it starts its own frames with is what the second
    // launch would have started from (a zero-state run over 0.2 s: 1.6e-21 of the true state's response left), the run-in tiles
    // cost the filter passes only, no second launch.
    if (plan.nseg > 1) {
        if (split == ssk::kTdSplitSegments) plan.warm_sub = kTdFixSub;
        else if (b->td_mode == 1) plan.warm_sub = kTdWarmSub;
        else { plan.fixup = true; plan.fix_sub = plan.seg_sub < kTdFixSub ? plan.seg_sub : kTdFixSub; }
    }
    if (plan.fixup) HIPCHK(b->seg_state.ensure((size_t)cfg->n_streams * plan.nseg * C * 4));
    return SS_OK;
}

// the columns-only spectrum's tables: the shared column tables (ssh::column_tables), and the columns packed per group of four bins
int upload_column_tables(ss_batch *b)
{
    const ss_batch_layout &L = b->lay;
    const ColumnTables t = column_tables(*b->bt, b->cfg.spectrum_columns, L.fft_bin_stride);
    const std::vector<uint16_t> &bc = t.bin_col;
    HIPCHK(b->cols.bin_col.upload(bc));
    std::vector<uint2> cg(L.fft_bin_stride / 4), cbins(L.fft_bin_stride / 4);
    for (uint32_t g = 0; g < cg.size(); g++) {
        uint32_t o[4];
        bool general = false;
        for (uint32_t e = 0; e < 4; e++) {
            const bool pad = bc[4 * g + e] == 0xFFFF;
            o[e] = pad ? 2048u : 4u * bc[4 * g + e];
            general = general || pad;
        }
        uint32_t n = 1;
        while (n < 4 && o[n] == o[0]) n++;
        for (uint32_t e = n; e < 4; e++) general = general || o[e] != o[3];
        cg[g] = make_uint2(o[0] | (o[3] << 16), general ? 0u : n);
        cbins[g] = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
    }
    HIPCHK(b->cols.bins.upload(cbins));
    HIPCHK(b->cols.init.upload(t.col_init));
    HIPCHK(b->cols.groups.upload(cg));
    return SS_OK;
}

// the decimation is fused into the time-domain pass when that pass runs and a bin (plus its shared edge sample)
// fits the per-wave halo; otherwise the standalone kernel handles it
void choose_wave_fusion(ss_batch *b)
{
    const uint32_t C = b->cfg.channels;
    const uint64_t W = b->wave_window, len = b->cfg.frames_per_stream * C;
    const double spp = (double)len / (double)W;
    if (b->td && W > 0 && spp >= 16.0 && spp <= 1000.0 && len < (1ull << 31)) {
        // (+ 3: the general decimation path reads the aligned 16-byte piece a bin starts in, up to three samples in front of it)
        const uint32_t need = ((uint32_t)std::ceil(spp) + 5 + C - 1) / C;
        uint32_t halo = need < 24 ? 24 : need;
        halo = (halo + 3u) & ~3u;
        if (halo <= 512) { b->wave_fused = true; b->wave_halo = halo; }
    }
}

// ---- moving data ----------------------------------------------------------------------------------------------------

// The one upload: n samples of `format` at `pcm` become the floats at offset `at` of the batch's input, queued on the batch's
// stream.  f32 is copied straight in; anything else is copied to `raw` (device staging of n samples and kPcmReadSlack bytes
// that stays untouched until the conversion has run) and converted from there.  wait: return when the input is there.
int upload_range(ss_batch *b, size_t at, size_t n, const void *pcm, int format, unsigned char *raw, bool wait)
{
    float *dst = b->pcm.p + at;
    if (format == SS_PCM_F32) raw = reinterpret_cast<unsigned char *>(dst);
    HIPCHK(hipMemcpyAsync(raw, pcm, n * ss_pcm_sample_bytes(format), hipMemcpyHostToDevice, b->stream));
    if (format != SS_PCM_F32) HIPCHK(ssk::launch_pcm_to_f32(raw, n, format, dst, b->stream));
    if (wait) HIPCHK(hipStreamSynchronize(b->stream));
    return SS_OK;
}

// The uploads that do not wait stage in one raw area per batch, sized for the whole batch at the format's bytes per sample: the
// sample at float offset `at` stages at the same offset in samples (ranges of different streams do not overlap); growing it
// waits for whatever still reads the old one.
int upload_queued(ss_batch *b, size_t at, size_t n, const void *pcm, int format)
{
    const size_t sb = ss_pcm_sample_bytes(format);
    const size_t bytes = b->samples_per_stream() * b->cfg.n_streams * sb + kPcmReadSlack;
    if (format != SS_PCM_F32 && b->raw.n < bytes) {
        HIPCHK(hipStreamSynchronize(b->stream));
        HIPCHK(b->raw.alloc(bytes));
    }
    return upload_range(b, at, n, pcm, format, format != SS_PCM_F32 ? b->raw.p + at * sb : nullptr, false);
}

// The one download: count elements from the device to the host (or to `kind`'s side) on the batch's stream, behind everything
// queued there, and there when this returns.
template <typename T>
int fetch(ss_batch *b, T *dst, const T *src, size_t count, hipMemcpyKind kind = hipMemcpyDeviceToHost)
{
    HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), kind, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return SS_OK;
}

// ---- follow-up calls: behind a pass, on a list of regions; they hand back one record per region, group or stream -----------------
// The download of n records and its status ladder: no destination for n > 0 records, then the mode, then the capacity; nothing to
// copy means synchronise.  (The caller has checked b.)
template <class Rec>
int fetch_records(ss_batch *b, bool mode_ok, Rec *out, uint32_t cap, uint32_t n, const Rec *src)
{
    if (!out && n) return SS_ERR_INVALID_ARG;
    if (!mode_ok) return SS_ERR_INVALID_MODE;
    if (cap < n) return SS_ERR_CAPACITY;
    if (!n) return ss_batch_sync(b);
    return fetch(b, out, src, n);
}

// Every check of a region list, before anything is queued or allocated: a refused call leaves the previous list, its counts and its
// results as they were.  bound_of_stream(s): whole sub-blocks for loudness, entries (the partial tail included) for peaks.
template <class Bound>
int check_regions(const ss_batch *b, const ss_loudness_region *regions, uint32_t n, uint32_t n_groups, Bound bound_of_stream, uint32_t *longest)
{
    if (!regions && n) return SS_ERR_INVALID_ARG;
    *longest = 0;
    for (uint32_t i = 0; i < n; i++) {
        const ss_loudness_region &r = regions[i];
        if (r.stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
        if ((uint64_t)r.first_subblock + r.n_subblocks > bound_of_stream(r.stream)) return SS_ERR_INVALID_ARG;
        if (r.group != SS_REGION_NO_GROUP && r.group >= n_groups) return SS_ERR_INVALID_ARG;
        if (r.n_subblocks > *longest) *longest = r.n_subblocks;
    }
    return SS_OK;
}

}  // namespace

extern "C" {

int ss_batch_create(const ss_batch_config *cfg, ss_batch **out)
{
    // ---- checks
    if (!cfg || !out) return SS_ERR_INVALID_ARG;
    *out = nullptr;
    if (require_device()) return SS_ERR_DEVICE;
    if (cfg->n_streams == 0 || cfg->frames_per_stream == 0) return SS_ERR_INVALID_ARG;
    if ((cfg->flags & SS_BATCH_ALL) == 0) return SS_ERR_INVALID_ARG;
    const bool columns_only = (cfg->flags & SS_BATCH_FFT_COLUMNS) != 0;
    if (columns_only && (!(cfg->flags & SS_BATCH_FFT) || cfg->spectrum_columns == 0 || cfg->spectrum_columns > 512)) return SS_ERR_INVALID_ARG;
    if ((cfg->flags & SS_BATCH_LOUDNESS_SERIES) && !(cfg->flags & SS_BATCH_LUFS)) return SS_ERR_INVALID_ARG;      // the series reads the gating pass
    const uint32_t C = cfg->channels;
    const uint64_t F = cfg->frames_per_stream;
    const bool meter = (cfg->flags & (SS_BATCH_LUFS | SS_BATCH_TRUE_PEAK)) != 0;
    if (C == 0 || C > 64) return SS_ERR_NOMEM;
    if (meter) {
        int rc = meter_args_ok(C, cfg->sample_rate);
        if (rc) return rc;
    }
    if (cfg->true_peak_factor != 0 && cfg->true_peak_factor != 2 && cfg->true_peak_factor != 4) return SS_ERR_INVALID_ARG;
    {   // sizes that cannot be a buffer: refused before any product of them is formed (a wrapped product would allocate a small
        // buffer and index far beyond it).  2^40 samples = 4 TB of f32, fourteen times the HBM of the card.
        unsigned long long samples = 0;
        if (F > (1ull << 40) || __builtin_mul_overflow((unsigned long long)cfg->n_streams, (unsigned long long)F, &samples) ||
            __builtin_mul_overflow(samples, (unsigned long long)C, &samples) || samples > (1ull << 40))
            return SS_ERR_NOMEM;
    }
    // ---- the handle, its stream and its input: destroyed (streams and events included) on every early return
    std::unique_ptr<ss_batch, decltype(&ss_batch_destroy)> b(new ss_batch(), &ss_batch_destroy);
    b->device = current_device();
    b->cfg = *cfg;
    HIPCHK(stream_acquire(&b->stream));
    ss_batch_layout &L = b->lay;
    L.input_bytes = (uint64_t)cfg->n_streams * F * C * sizeof(float);
    HIPCHK(b->pcm.alloc((size_t)cfg->n_streams * F * C));

    // ---- tables (the spectrum's own checks stay in front of its tables: the status of a refused config is what it was)
    if (meter) {
        b->tp_factor = (cfg->flags & SS_BATCH_TRUE_PEAK)
                           ? (cfg->true_peak_factor ? cfg->true_peak_factor : sst::true_peak_factor_for_rate(cfg->sample_rate))
                           : 0;
        int rc = get_td_tables(cfg->sample_rate, b->tp_factor, C, &b->td);
        if (!rc) rc = get_hist_tables(&b->hist_energies, &b->hist_bounds);
        if (rc) return rc;
    }
    if (cfg->flags & SS_BATCH_FFT) {
        const size_t n = cfg->fft_n;
        if (n < 2) return SS_ERR_TOO_FEW_SAMPLES;
        if (!is_pow2(n)) return SS_ERR_NOT_POW2;
        if (n > 32768) return SS_ERR_UNSUPPORTED;
        if (20000.0f > (float)cfg->sample_rate / 2.0f) return SS_ERR_FREQ_LIMIT;
        if (cfg->hop_frames == 0) return SS_ERR_INVALID_ARG;
        int rc = get_fft_tables(n, &b->ft);
        if (rc) return rc;
        rc = get_bin_tables(cfg->sample_rate, n, &b->bt);
        if (rc) return rc;
    }

    // ---- shape: what a stream of F frames holds, and how the kernels walk it
    const StreamShape sh = stream_shape(b.get(), F);
    if (b->ft) {
        const uint64_t n = cfg->fft_n, hop = cfg->hop_frames;
        L.n_windows = sh.windows;
        b->first_start = (n / hop + 1) * hop - n;         // window 0 ends at (N/hop + 1) * hop (stream_shape)
        b->spec = ssk::plan_spectrum((uint32_t)n, C, (uint32_t)hop, cfg->n_streams, L.n_windows);
        L.fft_channels = b->spec.fft_ch;
        L.n_bins = (uint32_t)b->bt->count;
        L.first_bin = (uint32_t)b->bt->first;
        // Rows start 16-byte aligned (16-byte stores).  Padding them to whole 128-byte lines lifts a pure streaming-store
        // kernel with this row pattern from 3.7 to 4.4 TB/s (tools/ubench_fftio.hip) but does nothing for the real kernel
        // (A/B in one process: 3.14 vs 3.12 ms), so the rows stay compact.
        L.fft_bin_stride = (L.n_bins + 3u) & ~3u;
    }
    if (b->td) L.n_subblocks = b->ragged.max_sub = sh.subblocks;

    // ---- buffers
    if (b->ft) {
        const uint64_t rows = (uint64_t)cfg->n_streams * L.n_windows * L.fft_channels;
        if (columns_only) {
            // the fused reduction lives in the epilogue of k_fft4096_ms1
            if (b->spec.kernel != ssk::SpecKernel::ms1) return SS_ERR_UNSUPPORTED;
            int rc = upload_column_tables(b.get());
            if (rc) return rc;
            b->render_cols = cfg->spectrum_columns;
            HIPCHK(b->render_spec.alloc(rows * b->render_cols));
            b->cols.on = true;
            b->cols.gain_mode = (cfg->flags & SS_BATCH_LUFS) ? SS_GAIN_REFERENCE : SS_GAIN_FIXED;
            L.fft_bytes = rows * b->render_cols * sizeof(float);
        } else {
            L.fft_bytes = rows * L.fft_bin_stride * sizeof(float);
            HIPCHK(b->fft.alloc((size_t)(L.fft_bytes / sizeof(float))));
        }
    }
    if (b->td) {
        HIPCHK(b->state.alloc(cfg->n_streams));
        HIPCHK(b->sub.alloc((size_t)cfg->n_streams * b->sub_cap() * C));
        HIPCHK(b->hist.alloc((size_t)cfg->n_streams * 2 * sst::kHistBins));
        HIPCHK(b->corpus.alloc(2 * sst::kHistBins));
        HIPCHK(b->integrated.alloc(cfg->n_streams));
        HIPCHK(b->lra.alloc(cfg->n_streams));
        HIPCHK(b->counts.alloc((size_t)cfg->n_streams * 2));
        HIPCHK(b->out2.alloc(2));
        std::vector<double> w(C);
        sst::channel_weights(C, w.data());
        HIPCHK(b->weights.upload(w));
        if (cfg->flags & SS_BATCH_LOUDNESS_SERIES) {
            HIPCHK(b->series.alloc((size_t)cfg->n_streams * b->sub_cap() * 2));
            HIPCHK(b->extremes.alloc(cfg->n_streams));
        }
    }
    if (cfg->flags & SS_BATCH_WAVEFORM) {
        if (sh.wave_window > 0xFFFFFFFFull) return SS_ERR_UNSUPPORTED;
        b->wave_window = (uint32_t)sh.wave_window;
        L.n_wave_points = (uint32_t)(2 * sh.wave_bins);
        HIPCHK(b->wave.alloc((size_t)cfg->n_streams * (b->wave_window ? 2 * (size_t)b->wave_window : 2)));
    }

    // ---- plans
    if (cfg->flags & SS_BATCH_WAVEFORM) choose_wave_fusion(b.get());
    int rc = choose_td_geometry(b.get());
    if (rc) return rc;
    HIPCHK(b->timing.create());
    *out = b.release();
    return SS_OK;
}

// synchronise both streams, then release: the members free their events and buffers
void ss_batch_destroy(ss_batch *b)
{
    SS_ON_DEVICE(b);
    if (!b) return;
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->ov.stream2) { (void)hipStreamSynchronize(b->ov.stream2); stream_release(b->ov.stream2); }
    if (b->stream) stream_release(b->stream);
    delete b;
}

int ss_batch_layout_get(const ss_batch *b, ss_batch_layout *out)
{
    SS_ON_DEVICE(b);
    if (!b || !out) return SS_ERR_INVALID_ARG;
    *out = b->lay;
    return SS_OK;
}

// ---- uploads: each entry point says where the range is, which staging a conversion uses and whether it waits ----------

int ss_batch_upload(ss_batch *b, uint32_t first, uint32_t count, const float *pcm)
{
    SS_ON_DEVICE(b);
    if (!b || !pcm) return SS_ERR_INVALID_ARG;
    if ((uint64_t)first + count > b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const size_t per = b->samples_per_stream();
    return upload_range(b, (size_t)first * per, (size_t)count * per, pcm, SS_PCM_F32, nullptr, true);
}

int ss_batch_upload_pcm(ss_batch *b, uint32_t first, uint32_t count, const void *pcm, int format)
{
    SS_ON_DEVICE(b);
    const size_t sb = ss_pcm_sample_bytes(format);
    if (!b || !pcm || !sb) return SS_ERR_INVALID_ARG;
    if ((uint64_t)first + count > b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const size_t per = b->samples_per_stream(), n = per * count;
    // The staging is this call's own, freed behind its wait.  The batch-wide raw area would serve, but every batch that ever
    // took this path would then hold a second copy of its input for good.
    DevBuf<unsigned char> raw;
    if (format != SS_PCM_F32) HIPCHK(raw.alloc(n * sb + kPcmReadSlack));
    return upload_range(b, (size_t)first * per, n, pcm, format, raw.p, true);
}

// ---- ragged batches: streams of different lengths in one batch ------------------------------------------------
// The batch is created for the longest stream (frames_per_stream = the slot size); every stream then gets its own
// window count, sub-block count and decimation geometry by the very rules ss_batch_create applies to the whole
// batch.  Slots are uploaded as before (the tail of a short stream's slot is never read).
// A refused call leaves the batch as it was: every check comes before the first assignment.
int ss_batch_set_lengths(ss_batch *b, const uint64_t *frames, uint32_t count)
{
    SS_ON_DEVICE(b);
    if (!b || !frames || count != b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const ss_batch_config &c = b->cfg;
    for (uint32_t i = 0; i < count; i++) if (frames[i] > c.frames_per_stream) return SS_ERR_INVALID_ARG;
    std::vector<uint64_t> frames_h(frames, frames + count), wave_samples(count, 0);
    std::vector<uint32_t> windows(count, 0), sub_h(count, 0), wave_window(count, 0);
    uint32_t max_sub = 0;
    for (uint32_t i = 0; i < count; i++) {
        const StreamShape sh = stream_shape(b, frames[i]);
        if (sh.wave_window > b->wave_window) return SS_ERR_INVALID_ARG;      // cannot happen for F <= frames_per_stream
        windows[i] = sh.windows; sub_h[i] = sh.subblocks;
        if (sh.subblocks > max_sub) max_sub = sh.subblocks;
        if (c.flags & SS_BATCH_WAVEFORM) {
            wave_window[i] = (uint32_t)sh.wave_window; wave_samples[i] = frames[i] * c.channels;
        }
    }
    Ragged &r = b->ragged;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(r.frames_d.upload(frames_h));
    HIPCHK(r.windows_d.upload(windows));
    HIPCHK(r.sub_d.upload(sub_h));
    HIPCHK(r.wave_window_d.upload(wave_window));
    HIPCHK(r.wave_samples_d.upload(wave_samples));
    r.frames_h.swap(frames_h); r.sub_h.swap(sub_h);
    r.on = true;
    // the time-domain geometry follows the lengths actually set (the longest stream), not the slot size the batch was created with:
    // a batch that is kept and re-used — the one-shot loudness call keeps one — then cuts the same input the same way whatever
    // was analysed before it (the low bits of a reading do not depend on the process' history)
    r.max_sub = max_sub;
    return choose_td_geometry(b);
}

int ss_batch_stream_shape(const ss_batch *b, uint32_t stream, ss_stream_shape *out)
{
    SS_ON_DEVICE(b);
    if (!b || !out || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const uint64_t F = b->frames_of(stream);
    const StreamShape sh = stream_shape(b, F);
    out->frames = F; out->n_windows = sh.windows;
    out->n_subblocks = sh.subblocks; out->n_wave_points = (uint32_t)(2 * sh.wave_bins);
    out->reserved = 0;
    return SS_OK;
}

// ---- pipelined ingest: page-locked host memory + uploads that do not wait -------------------------------------
// A batch owns its stream, so two batches are a double buffer: while one runs, the other's upload is in flight
// on the copy engine.  That only holds for page-locked host memory (pageable copies are staged synchronously).
int ss_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return SS_ERR_INVALID_ARG;
    if (require_device()) return SS_ERR_DEVICE;
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return SS_OK;
}

int ss_host_unregister(void *ptr)
{
    if (!ptr) return SS_ERR_INVALID_ARG;
    HIPCHK(hipHostUnregister(ptr));
    return SS_OK;
}

// like ss_batch_upload_pcm, but returns as soon as the copy and the conversion are queued on the batch's stream:
// `pcm` must stay valid (and should be page-locked) until the next ss_batch_sync / ss_batch_results on this batch
int ss_batch_upload_pcm_async(ss_batch *b, uint32_t first, uint32_t count, const void *pcm, int format)
{
    SS_ON_DEVICE(b);
    if (!b || !pcm || !ss_pcm_sample_bytes(format)) return SS_ERR_INVALID_ARG;
    if ((uint64_t)first + count > b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const size_t per = b->samples_per_stream();
    return upload_queued(b, (size_t)first * per, per * count, pcm, format);
}

// the first n_samples interleaved samples of one stream's slot, raw PCM of any supported format (ragged batches:
// a stream shorter than the slot).  Queued on the batch's stream like ss_batch_upload_pcm_async.
int ss_batch_upload_samples(ss_batch *b, uint32_t stream, const void *pcm, size_t n_samples, int format)
{
    SS_ON_DEVICE(b);
    if (!b || (!pcm && n_samples) || !ss_pcm_sample_bytes(format) || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const size_t per = b->samples_per_stream();
    if (n_samples > per) return SS_ERR_INVALID_ARG;
    return n_samples ? upload_queued(b, (size_t)stream * per, n_samples, pcm, format) : SS_OK;
}

int ss_batch_download_input(ss_batch *b, uint32_t stream, float *pcm, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !pcm || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const size_t per = b->samples_per_stream();
    if (cap < per) return SS_ERR_CAPACITY;
    return fetch(b, pcm, b->pcm.p + (size_t)stream * per, per);
}

void *ss_batch_input_device_ptr(ss_batch *b) { return b ? b->pcm.p : nullptr; }

int ss_batch_synthesize(ss_batch *b, uint64_t seed, uint32_t first_stream_id)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    HIPCHK(ssk::launch_synth(b->pcm.p, b->cfg.n_streams, b->cfg.frames_per_stream, b->cfg.channels,
                             b->cfg.sample_rate, seed, first_stream_id, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return SS_OK;
}

// One pass over every stream, queued on the batch's stream(s); nothing is waited for and nothing allocated.
int ss_batch_run(ss_batch *b)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    TimingRing &t = b->timing;
    int rc = (t.count >= TimingRing::kDepth || !t.on) ? t.collect(b->stream) : SS_OK;     // (a full ring: collect first)
    if (rc) return rc;
    b->corpus_reduced = false;

    // Where the spectrum kernel goes.
    //  * first, on the main stream: the sequential pass.  Per-kernel event timing is meaningless while two kernels share the
    //    chip, so timing passes stay sequential.
    //  * first, forked (overlap mode 1): on stream2 after everything already queued on the main stream (uploads, the previous
    //    pass); the time-domain chain stays on the main stream, join at the end.
    //  * behind the time-domain kernel, forked (mode 2, tail overlap): the time-domain kernel runs first and alone; the spectrum
    //    kernel starts behind it on stream2 while the short latency-bound tail of the chain (gating / histograms per stream, a
    //    standalone decimation) runs on the main stream beside it.
    //  * last, on the main stream: a columns-only spectrum with the reference's per-file gain — the gain is -13 - integrated of
    //    each stream, so the whole time-domain chain (kernel + gating / histograms) runs first.
    enum class At { first, behind_td, last };
    const bool gain_from_meter = b->cols.on && b->cols.gain_mode == SS_GAIN_REFERENCE;
    const int mode = (t.on || gain_from_meter) ? 0 : b->ov.mode;
    const At at = gain_from_meter ? At::last : mode == 2 ? At::behind_td : At::first;
    auto spectrum_if = [&](At here) { return here == at ? spectrum_step(b, mode != 0) : SS_OK; };

    if ((rc = spectrum_if(At::first))) return rc;

    HIPCHK(t.mark(SS_KERNEL_TIME_DOMAIN, 0, b->stream));
    const ssk::TdParams tdp = b->td ? batch_td_params(b) : ssk::TdParams{};
    if (b->td) {
        HIPCHK(zero_meter(b));
        HIPCHK(t.mark(SS_KERNEL_TIME_DOMAIN, 0, b->stream));   // time the kernel, not the memsets
        HIPCHK(ssk::launch_time_domain(tdp, b->stream));
    }
    // the tail starts HERE: the hand-over's second launch (filter and energies of every segment's first 0.2 s: one wave per
    // segment, a chain of ten short tiles each — latency, not throughput, and no matrix-core work) runs beside the spectrum
    // kernel like the gating behind it.  (No time-domain work at all: the spectrum kernel is the pass.)
    if ((rc = spectrum_if(At::behind_td))) return rc;
    if (b->td && b->td_plan.fixup) HIPCHK(ssk::launch_time_domain_fixup(tdp, b->stream));
    HIPCHK(t.mark(SS_KERNEL_TIME_DOMAIN, 1, b->stream));

    HIPCHK(t.mark(SS_KERNEL_FINALIZE, 0, b->stream));
    if (b->td) {
        const ssk::FinalizeParams f = batch_gating_params(b);
        HIPCHK(ssk::launch_finalize(f, b->stream));
        // the series behind the gating pass, on the same stream: behind the hand-over's fix-up launch like it (exact segment
        // heads), inside the FINALIZE timing slot
        if (b->series.p) HIPCHK(ssk::launch_loudness_series(f, b->series.p, b->sub_cap(), b->extremes.p, b->stream));
    }
    HIPCHK(t.mark(SS_KERNEL_FINALIZE, 1, b->stream));

    HIPCHK(t.mark(SS_KERNEL_WAVEFORM, 0, b->stream));
    if ((b->cfg.flags & SS_BATCH_WAVEFORM) && b->wave_window && (!b->wave_fused || b->ragged.on))
        HIPCHK(ssk::launch_waveform(batch_wave_params(b), b->stream));
    HIPCHK(t.mark(SS_KERNEL_WAVEFORM, 1, b->stream));

    if ((rc = spectrum_if(At::last))) return rc;
    if (mode) HIPCHK(b->ov.join(b->stream));
    t.advance();
    return SS_OK;
}

// measurement utility: the spectrum kernel's loads and stores alone (see the header)
int ss_batch_traffic_floor(ss_batch *b, uint32_t reps, double *ms_per_launch)
{
    SS_ON_DEVICE(b);
    if (!b || !ms_per_launch || reps == 0) return SS_ERR_INVALID_ARG;
    if (!(b->cfg.flags & SS_BATCH_FFT) || b->spec.kernel != ssk::SpecKernel::ms1 || !b->lay.n_windows || b->ragged.on) return SS_ERR_UNSUPPORTED;
    if (!b->fft.p) return SS_ERR_INVALID_MODE;          // columns-only batches have no spectrum rows to store into
    const ssk::FftBatchParams p = batch_fft_params(b);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHK(hipEventCreate(&e0));
    hipError_t err = hipEventCreate(&e1);
    if (err == hipSuccess) err = ssk::launch_fft4096_traffic(p, b->stream);            // warm
    if (err == hipSuccess) err = hipEventRecord(e0, b->stream);
    for (uint32_t r = 0; r < reps && err == hipSuccess; r++) err = ssk::launch_fft4096_traffic(p, b->stream);
    if (err == hipSuccess) err = hipEventRecord(e1, b->stream);
    if (err == hipSuccess) err = hipEventSynchronize(e1);
    float ms = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    HIPCHK(err);
    *ms_per_launch = (double)ms / reps;
    return SS_OK;
}

int ss_batch_sync(ss_batch *b)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(b->stream));
    return b->timing.collect(b->stream);
}

int ss_batch_results(ss_batch *b, ss_stream_result *out, uint32_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !out) return SS_ERR_INVALID_ARG;
    const uint32_t n = b->cfg.n_streams;
    if (cap < n) return SS_ERR_CAPACITY;
    std::memset(out, 0, sizeof(ss_stream_result) * n);
    if (!b->state.p) return SS_OK;
    std::vector<double> integ(n), lra(n);
    std::vector<uint32_t> cnt(2 * (size_t)n);
    std::vector<ssk::TdState> st(n);
    HIPCHK(hipMemcpyAsync(integ.data(), b->integrated.p, n * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(lra.data(), b->lra.p, n * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(cnt.data(), b->counts.p, 2 * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(st.data(), b->state.p, n * sizeof(ssk::TdState), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (uint32_t i = 0; i < n; i++) {
        out[i].integrated_lufs = integ[i];
        out[i].loudness_range = lra[i];
        for (uint32_t c = 0; c < 2 && c < b->cfg.channels; c++) {
            const float sp = st[i].sample_peak[c], tp = st[i].true_peak[c];
            out[i].sample_peak[c] = sp;
            out[i].true_peak[c] = tp > sp ? tp : sp;
        }
        out[i].n_gating_blocks = cnt[2 * i];
        out[i].n_st_blocks = cnt[2 * i + 1];
    }
    return SS_OK;
}

// every channel's peaks of one stream: EbuR128::true_peak(c) = max(true, sample) and EbuR128::sample_peak(c)
int ss_batch_peaks(ss_batch *b, uint32_t stream, double *true_pk, double *sample_pk, uint32_t cap_channels)
{
    SS_ON_DEVICE(b);
    if (!b || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    if (!b->state.p) return SS_ERR_INVALID_MODE;                 // the batch runs no meter pass
    const uint32_t C = b->cfg.channels;
    if (cap_channels < C) return SS_ERR_CAPACITY;
    float pk[2 * ssk::kMaxChannels];
    const ssk::TdState *st = b->state.p + stream;
    HIPCHK(hipMemcpyAsync(pk, st->sample_peak, C * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipMemcpyAsync(pk + ssk::kMaxChannels, st->true_peak, C * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (uint32_t c = 0; c < C; c++) peaks_of(pk, c, sample_pk ? sample_pk + c : nullptr, true_pk ? true_pk + c : nullptr);
    return SS_OK;
}

int ss_batch_geometry_get(const ss_batch *b, ss_batch_geometry *out)
{
    if (!b || !out) return SS_ERR_INVALID_ARG;
    std::memset(out, 0, sizeof *out);
    const ss_batch_layout &L = b->lay;
    if ((b->cfg.flags & SS_BATCH_FFT) && L.n_windows) {
        out->fft_windows_per_block = b->spec.windows_per_block;
        out->fft_blocks = b->spec.blocks;
    }
    if (b->td) {
        out->td_segments = b->td_plan.nseg;
        out->td_segment_subblocks = b->td_plan.seg_sub;
        out->td_warm_subblocks = b->td_plan.warm_sub;
        out->td_split = b->td_plan.split_batch;
        out->td_fixup_subblocks = b->td_plan.fix_sub;
        out->td_true_peak_factor = (uint32_t)b->tp_factor;
    }
    out->waveform_fused = (b->wave_fused && !b->ragged.on) ? 1u : 0u;
    out->overlap = (uint32_t)b->ov.mode;
    return SS_OK;
}

int ss_batch_geometry_get_sized(const ss_batch *b, void *out, size_t out_bytes)
{
    if (!b || !out) return SS_ERR_INVALID_ARG;
    ss_batch_geometry g;
    const int rc = ss_batch_geometry_get(b, &g);
    if (rc) return rc;
    std::memcpy(out, &g, out_bytes < sizeof g ? out_bytes : sizeof g);
    return SS_OK;
}

int ss_batch_set_overlap(ss_batch *b, int enable)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    Overlap &ov = b->ov;
    if (enable && !ov.stream2) {
        HIPCHK(stream_acquire(&ov.stream2));
        HIPCHK(hipEventCreateWithFlags(&ov.ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ov.ev_join, hipEventDisableTiming));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    ov.mode = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    return SS_OK;
}

int ss_batch_checksums(ss_batch *b, uint64_t *out, uint32_t cap_streams)
{
    SS_ON_DEVICE(b);
    if (!b || !out) return SS_ERR_INVALID_ARG;
    const uint32_t ns = b->cfg.n_streams;
    if (cap_streams < ns) return SS_ERR_CAPACITY;
    HIPCHK(b->checks.ensure((size_t)3 * ns));
    HIPCHK(hipMemsetAsync(b->checks.p, 0, (size_t)3 * ns * sizeof(uint64_t), b->stream));
    const ss_batch_layout &L = b->lay;
    // 32-bit words per stream of: the spectrum rows, the decimation bins, the sub-block energies
    const struct { const void *p; uint64_t words; } parts[3] = {{b->fft.p, (uint64_t)L.n_windows * L.fft_channels * L.fft_bin_stride},
        {b->wave.p, (uint64_t)2 * b->wave_window}, {b->sub.p, (uint64_t)2 * L.n_subblocks * b->cfg.channels}};
    for (int k = 0; k < 3; k++)
        if (parts[k].p && parts[k].words) HIPCHK(ssk::launch_checksum(parts[k].p, parts[k].words, parts[k].words, ns, b->checks.p + k, 3, b->stream));
    return fetch(b, out, b->checks.p, (size_t)3 * ns);
}

int ss_batch_set_true_peak_arith(ss_batch *b, int arith)
{
    if (!b || (arith != SS_TP_ARITH_F16X3 && arith != SS_TP_ARITH_F32)) return SS_ERR_INVALID_ARG;
    b->tp_arith = arith;
    return SS_OK;
}

int ss_batch_get_true_peak_arith(const ss_batch *b) { return b ? b->tp_arith : SS_ERR_INVALID_ARG; }

int ss_batch_set_time_domain_mode(ss_batch *b, int mode)
{
    SS_ON_DEVICE(b);
    if (!b || mode < 0 || mode > 2) return SS_ERR_INVALID_ARG;      // SS_TD_AUTO / SS_TD_RUN_IN / SS_TD_WHOLE_STREAMS
    HIPCHK(hipStreamSynchronize(b->stream));
    b->td_mode = mode;
    return choose_td_geometry(b);
}

int ss_batch_download_fft(ss_batch *b, uint32_t stream, float *out, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !out || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    if (b->cols.on) return SS_ERR_INVALID_MODE;          // the rows were never stored: ss_batch_download_spectrum_columns
    const size_t rows = (size_t)b->lay.n_windows * b->lay.fft_channels;
    const size_t per = rows * b->lay.n_bins;
    if (cap < per) return SS_ERR_CAPACITY;
    if (!per) return SS_OK;
    // device rows are padded to fft_bin_stride floats; hand back the compact [window][channel][bin] array
    HIPCHK(hipMemcpy2DAsync(out, (size_t)b->lay.n_bins * sizeof(float),
                            b->fft.p + (size_t)stream * rows * b->lay.fft_bin_stride,
                            (size_t)b->lay.fft_bin_stride * sizeof(float), (size_t)b->lay.n_bins * sizeof(float), rows,
                            hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return SS_OK;
}

int ss_batch_bin_tables(const ss_batch *b, double *chart_x, double *freq, double *pink_db)
{
    SS_ON_DEVICE(b);
    if (!b || !b->bt) return SS_ERR_INVALID_ARG;
    const size_t n = b->bt->count;
    if (chart_x) std::memcpy(chart_x, b->bt->chart_x.data(), n * sizeof(double));
    if (freq) std::memcpy(freq, b->bt->freq.data(), n * sizeof(double));
    if (pink_db) std::memcpy(pink_db, b->bt->pink.data(), n * sizeof(double));
    return SS_OK;
}

int ss_batch_download_waveform(ss_batch *b, uint32_t stream, float *out, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !out || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const size_t pts = b->lay.n_wave_points;
    if (cap < pts) return SS_ERR_CAPACITY;
    if (!pts) return SS_OK;
    return fetch(b, out, b->wave.p + (size_t)stream * 2 * b->wave_window, pts);
}

int ss_batch_download_subblocks(ss_batch *b, uint32_t stream, double *out, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !out || stream >= b->cfg.n_streams || !b->sub.p) return SS_ERR_INVALID_ARG;
    const size_t per = (size_t)b->lay.n_subblocks * b->cfg.channels;
    if (cap < per) return SS_ERR_CAPACITY;
    if (!per) return SS_OK;
    return fetch(b, out, b->sub.p + (size_t)stream * per, per);
}

int ss_batch_download_loudness_series(ss_batch *b, uint32_t stream, double *momentary, double *shortterm, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    if (!b->series.p) return SS_ERR_INVALID_MODE;                // the batch was made without SS_BATCH_LOUDNESS_SERIES
    const size_t n = b->subblocks_of(stream);
    if (cap < n) return SS_ERR_CAPACITY;
    if (!n || (!momentary && !shortterm)) return SS_OK;
    std::vector<double> ms(2 * n);
    int rc = fetch(b, ms.data(), b->series.p + (size_t)stream * b->sub_cap() * 2, 2 * n);
    if (rc) return rc;
    for (size_t j = 0; j < n; j++) {
        if (momentary) momentary[j] = ms[2 * j];
        if (shortterm) shortterm[j] = ms[2 * j + 1];
    }
    return SS_OK;
}

int ss_batch_loudness_extremes(ss_batch *b, ss_loudness_extremes *out, uint32_t cap_streams)
{
    SS_ON_DEVICE(b);
    return !b ? SS_ERR_INVALID_ARG : fetch_records(b, b->extremes.p != nullptr, out, cap_streams, b->cfg.n_streams, b->extremes.p);      // (n_streams > 0)
}

int ss_batch_histograms(ss_batch *b, uint64_t *out2000)
{
    SS_ON_DEVICE(b);
    if (!b || !out2000 || !b->corpus.p) return SS_ERR_INVALID_ARG;
    return fetch(b, out2000, b->corpus.p, 2 * sst::kHistBins);
}

int ss_batch_histograms_device(ss_batch *b, void *dst)
{
    SS_ON_DEVICE(b);
    if (!b || !dst || !b->corpus.p) return SS_ERR_INVALID_ARG;
    return fetch(b, static_cast<uint64_t *>(dst), b->corpus.p, 2 * sst::kHistBins, hipMemcpyDeviceToDevice);
}

// The corpus gate without leaving the device: [sum over the ranks] + loudness_global / loudness_range of the corpus
// histograms, queued on the batch's stream behind ss_batch_run.  Nothing is copied or waited for, so a loop of passes
// needs no host synchronisation per pass; ss_batch_corpus_gate_read fetches the pair.
int ss_batch_corpus_gate_enqueue(ss_batch *b, ss_comm *comm)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!b->corpus.p) return SS_ERR_INVALID_MODE;
    if (comm) {
        int rc = ss_batch_allreduce_histograms(b, comm, nullptr);
        if (rc) return rc;
    }
    HIPCHK(ssk::launch_hist_eval(b->corpus.p, b->hist_energies, b->hist_bounds, b->out2.p, b->stream));
    return SS_OK;
}

int ss_batch_corpus_gate_read(ss_batch *b, double *integrated, double *lra)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!b->corpus.p) return SS_ERR_INVALID_MODE;
    double r[2];
    int rc = fetch(b, r, b->out2.p, 2);
    if (rc) return rc;
    if (integrated) *integrated = r[0];
    if (lra) *lra = r[1];
    return SS_OK;
}

double ss_corpus_integrated_lufs(const uint64_t *h) { return h ? sst::gated_loudness(h) : NAN; }
double ss_corpus_loudness_range(const uint64_t *h) { return h ? sst::loudness_range(h) : NAN; }

// ---- render-side reductions ---------------------------------
int ss_batch_render_spectrum(ss_batch *b, uint32_t cols, int gain_mode, float gain_db)
{
    SS_ON_DEVICE(b);
    if (!b || cols == 0 || cols > 65536 || (gain_mode != SS_GAIN_FIXED && gain_mode != SS_GAIN_REFERENCE))
        return SS_ERR_INVALID_ARG;
    const ss_batch_layout &L = b->lay;
    if (!(b->cfg.flags & SS_BATCH_FFT) || !L.n_windows || !L.n_bins || b->cols.on) return SS_ERR_INVALID_MODE;   // (columns-only: no rows to reduce)
    if (gain_mode == SS_GAIN_REFERENCE && !(b->cfg.flags & SS_BATCH_LUFS)) return SS_ERR_INVALID_MODE;
    const std::vector<uint32_t> start = column_starts(*b->bt, cols);
    const uint64_t rows = (uint64_t)b->cfg.n_streams * L.n_windows * L.fft_channels;
    HIPCHK(b->col_start.ensure(cols + 1));
    HIPCHK(hipMemcpyAsync(b->col_start.p, start.data(), (cols + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));           // `start` is a local
    HIPCHK(b->render_spec.ensure(rows * cols));
    b->render_cols = cols;
    HIPCHK(ssk::launch_render_spectrum(b->fft.p, L.fft_bin_stride, L.n_bins, rows, L.n_windows * L.fft_channels,
                                       b->col_start.p, cols,
                                       gain_mode == SS_GAIN_REFERENCE ? b->integrated.p : nullptr, gain_db,
                                       b->render_spec.p, b->stream));
    return SS_OK;
}

int ss_batch_set_columns_gain(ss_batch *b, int gain_mode, float gain_db)
{
    if (!b || !b->cols.on || (gain_mode != SS_GAIN_FIXED && gain_mode != SS_GAIN_REFERENCE)) return SS_ERR_INVALID_ARG;
    if (gain_mode == SS_GAIN_REFERENCE && !(b->cfg.flags & SS_BATCH_LUFS)) return SS_ERR_INVALID_MODE;
    b->cols.gain_mode = gain_mode;
    b->cols.gain_db = gain_db;
    return SS_OK;
}

int ss_batch_download_spectrum_columns(ss_batch *b, uint32_t stream, float *out, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !out || stream >= b->cfg.n_streams || !b->render_cols) return SS_ERR_INVALID_ARG;
    const size_t per = (size_t)b->lay.n_windows * b->lay.fft_channels * b->render_cols;
    if (cap < per) return SS_ERR_CAPACITY;
    return fetch(b, out, b->render_spec.p + (size_t)stream * per, per);
}

// ---- per-stream average and peak-hold spectrum ------------------------------------------------------------------
// a batch whose passes leave rows to reduce (columns-only batches store none)
static bool has_spectrum_rows(const ss_batch *b) { return (b->cfg.flags & SS_BATCH_FFT) && !b->cols.on; }

int ss_batch_spectrum_stats(ss_batch *b)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!has_spectrum_rows(b)) return SS_ERR_INVALID_MODE;
    SpecStats &st = b->stats;
    const size_t per_stream = (size_t)b->lay.fft_channels * b->lay.fft_bin_stride, all = per_stream * b->cfg.n_streams;
    const ssk::SpecStatsPlan plan = batch_stats_plan(b);
    const size_t parts = plan.chunks > 1 ? all * plan.chunks : 0;
    // (the shape of a batch is fixed at create, so only the first call allocates)
    HIPCHK(st.sums.ensure(all)); HIPCHK(st.mean.ensure(all)); HIPCHK(st.max.ensure(all)); HIPCHK(st.counts.ensure(all));
    HIPCHK(st.part_sums.ensure(parts)); HIPCHK(st.part_max.ensure(parts)); HIPCHK(st.part_counts.ensure(parts));
    HIPCHK(st.corpus_mean.ensure(per_stream)); HIPCHK(st.corpus_max.ensure(per_stream)); HIPCHK(st.corpus_counts.ensure(b->lay.fft_channels));
    HIPCHK(ssk::launch_spectrum_stats(batch_stats_params(b), b->stream));
    st.done = true;
    return SS_OK;
}

int ss_batch_spectrum_stats_plan(const ss_batch *b, uint32_t *chunks, uint32_t *chunk_windows)
{
    if (!b) return SS_ERR_INVALID_ARG;
    if (!has_spectrum_rows(b)) return SS_ERR_INVALID_MODE;
    const ssk::SpecStatsPlan plan = batch_stats_plan(b);
    if (chunks) *chunks = plan.chunks;
    if (chunk_windows) *chunk_windows = plan.chunk_windows;
    return SS_OK;
}

// the compact [rows][n_bins] copies of two [rows][fft_bin_stride] device arrays (either host pointer may be null), queued on the
// batch's stream; rows: fft_channels per stream, region or group
static int fetch_stats_rows(ss_batch *b, float *mean_db, float *max_db, const float *mean_d, const float *max_d, size_t rows)
{
    const ss_batch_layout &L = b->lay;
    const size_t row = (size_t)L.n_bins * sizeof(float), pitch = (size_t)L.fft_bin_stride * sizeof(float);
    if (!row) return SS_OK;
    if (mean_db) HIPCHK(hipMemcpy2DAsync(mean_db, row, mean_d, pitch, row, rows, hipMemcpyDeviceToHost, b->stream));
    if (max_db) HIPCHK(hipMemcpy2DAsync(max_db, row, max_d, pitch, row, rows, hipMemcpyDeviceToHost, b->stream));
    return SS_OK;
}

int ss_batch_download_spectrum_stats(ss_batch *b, uint32_t stream, float *mean_db, float *max_db, size_t cap_floats,
                                     uint32_t *windows_counted, uint32_t cap_channels)
{
    SS_ON_DEVICE(b);
    if (!b || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    if (!has_spectrum_rows(b) || !b->stats.done) return SS_ERR_INVALID_MODE;
    const ss_batch_layout &L = b->lay;
    if (cap_floats < (size_t)L.fft_channels * L.n_bins || (windows_counted && cap_channels < L.fft_channels)) return SS_ERR_CAPACITY;
    const size_t at = (size_t)stream * L.fft_channels * L.fft_bin_stride;
    int rc = fetch_stats_rows(b, mean_db, max_db, b->stats.mean.p + at, b->stats.max.p + at, L.fft_channels);
    if (rc) return rc;
    // the count of a channel is bin 0's: one u32 of every [fft_bin_stride] row
    if (windows_counted && L.fft_bin_stride)
        HIPCHK(hipMemcpy2DAsync(windows_counted, sizeof(uint32_t), b->stats.counts.p + at, (size_t)L.fft_bin_stride * sizeof(uint32_t),
                                sizeof(uint32_t), L.fft_channels, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return SS_OK;
}

int ss_batch_corpus_spectrum(ss_batch *b, float *mean_db, float *max_db, size_t cap_floats, uint64_t *windows_counted, uint32_t cap_channels)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!has_spectrum_rows(b) || !b->stats.done) return SS_ERR_INVALID_MODE;
    const ss_batch_layout &L = b->lay;
    if (cap_floats < (size_t)L.fft_channels * L.n_bins || (windows_counted && cap_channels < L.fft_channels)) return SS_ERR_CAPACITY;
    SpecStats &st = b->stats;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the pooled counts are copied out as they are");
    HIPCHK(ssk::launch_spectrum_stats_corpus(batch_stats_params(b), st.corpus_mean.p, st.corpus_max.p, st.corpus_counts.p, b->stream));
    int rc = fetch_stats_rows(b, mean_db, max_db, st.corpus_mean.p, st.corpus_max.p, L.fft_channels);
    if (rc) return rc;
    if (windows_counted && L.fft_bin_stride)
        HIPCHK(hipMemcpyAsync(windows_counted, st.corpus_counts.p, L.fft_channels * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return SS_OK;
}

// ---- spectrogram: time x frequency chart tiles ---------------------------------------------------------------------
static_assert(sizeof(ss_spectrogram_view) == 24, "view layout");

// every check of a view, before anything is queued or allocated
static int check_spectrogram_view(const ss_batch *b, const ss_spectrogram_view *v)
{
    if (!b || !v) return SS_ERR_INVALID_ARG;
    if (v->t_cols == 0 || v->t_cols > ssk::kSpectrogramMaxTCols || v->f_cols == 0 || v->f_cols > ssk::kSpectrogramMaxFCols) return SS_ERR_INVALID_ARG;
    if (v->w_max <= v->w_min) return SS_ERR_INVALID_ARG;
    if (b->cols.on) {           // the pass has reduced frequency and applied its gain: the view's gain is not read
        if (v->f_cols != b->cfg.spectrum_columns) return SS_ERR_INVALID_ARG;
    } else if (v->gain_mode != SS_GAIN_FIXED && v->gain_mode != SS_GAIN_REFERENCE) return SS_ERR_INVALID_ARG;
    if (!(b->cfg.flags & SS_BATCH_FFT)) return SS_ERR_INVALID_MODE;
    if (!b->cols.on && v->gain_mode == SS_GAIN_REFERENCE && !(b->cfg.flags & SS_BATCH_LUFS)) return SS_ERR_INVALID_MODE;
    return SS_OK;
}

// how ss_batch_spectrogram cuts a (checked) view of this batch
static ssk::SpectrogramPlan batch_spectrogram_plan(const ss_batch *b, const ss_spectrogram_view &v)
{
    // the most windows a time column holds inside the slot: ceil(span / t_cols) of the view, never more than the slot has behind w_min
    const uint64_t span = (uint64_t)v.w_max - v.w_min;
    const uint64_t widest = (span + v.t_cols - 1) / v.t_cols, held = b->lay.n_windows > v.w_min ? b->lay.n_windows - v.w_min : 0;
    return ssk::plan_spectrogram((uint64_t)b->cfg.n_streams * b->lay.fft_channels * v.t_cols, (uint32_t)(widest < held ? widest : held));
}

int ss_batch_spectrogram(ss_batch *b, const ss_spectrogram_view *v)
{
    SS_ON_DEVICE(b);
    int rc = check_spectrogram_view(b, v);
    if (rc) return rc;
    const ss_batch_layout &L = b->lay;
    Spectrogram &sg = b->spectrogram;
    ssk::SpectrogramParams p{};
    p.plan = batch_spectrogram_plan(b, *v);
    const size_t cells = (size_t)b->cfg.n_streams * L.fft_channels * v->t_cols * v->f_cols;
    HIPCHK(sg.out.ensure(cells));               // (a buffer that grows is freed first: hipFree waits for whatever still uses it)
    HIPCHK(sg.part.ensure(p.plan.runs > 1 ? cells * p.plan.runs : 0));
    if (!b->cols.on && sg.map_cols != v->f_cols) {
        // the column of every bin (ssh::column_tables); staged, so that the call waits for nothing
        const std::vector<uint16_t> bc = column_tables(*b->bt, v->f_cols, L.fft_bin_stride).bin_col;
        HIPCHK(sg.bin_col.ensure(bc.size()));
        if (!bc.empty()) HIPCHK(sg.stage.send(sg.bin_col.p, bc.data(), bc.size() * sizeof(uint16_t), b->stream));
        sg.map_cols = v->f_cols;
    }
    p.columns_form = b->cols.on ? 1u : 0u;
    p.rows = b->fft.p; p.cols = b->cols.on ? b->render_spec.p : nullptr; p.bin_stride = L.fft_bin_stride;
    p.n_streams = b->cfg.n_streams; p.fft_ch = L.fft_channels; p.n_windows = L.n_windows;
    p.windows_of = b->ragged_ptr(b->ragged.windows_d);
    p.bin_col = sg.bin_col.p;
    p.t_cols = v->t_cols; p.f_cols = v->f_cols; p.w_min = v->w_min; p.w_max = v->w_max;
    p.integrated = !b->cols.on && v->gain_mode == SS_GAIN_REFERENCE ? b->integrated.p : nullptr;
    p.gain_db = v->gain_db;
    p.out = sg.out.p; p.part = sg.part.p;
    HIPCHK(ssk::launch_spectrogram(p, b->stream));
    sg.view = *v;
    sg.done = true;
    return SS_OK;
}

int ss_batch_spectrogram_plan(const ss_batch *b, const ss_spectrogram_view *v, uint32_t *runs, uint32_t *run_windows)
{
    int rc = check_spectrogram_view(b, v);
    if (rc) return rc;
    const ssk::SpectrogramPlan plan = batch_spectrogram_plan(b, *v);
    if (runs) *runs = plan.runs;
    if (run_windows) *run_windows = plan.run_windows;
    return SS_OK;
}

int ss_batch_download_spectrogram(ss_batch *b, uint32_t first_stream, uint32_t count, float *out, size_t cap_floats)
{
    SS_ON_DEVICE(b);
    if (!b || (uint64_t)first_stream + count > b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const Spectrogram &sg = b->spectrogram;
    if (!(b->cfg.flags & SS_BATCH_FFT) || !sg.done) return SS_ERR_INVALID_MODE;
    const size_t per = (size_t)b->lay.fft_channels * sg.view.t_cols * sg.view.f_cols;
    if (!out && count) return SS_ERR_INVALID_ARG;
    if (cap_floats < per * count) return SS_ERR_CAPACITY;
    if (!count) return ss_batch_sync(b);
    return fetch(b, out, sg.out.p + (size_t)first_stream * per, per * count);
}

void ss_spectrogram_column_windows(const ss_spectrogram_view *v, uint32_t t, uint32_t *first, uint32_t *end)
{
    uint32_t a = 0, e = 0;
    if (v && v->t_cols && v->t_cols <= ssk::kSpectrogramMaxTCols && v->w_max > v->w_min && t < v->t_cols) {
        a = ssk::spectrogram_column_first(v->w_min, v->w_max - v->w_min, v->t_cols, t);
        e = ssk::spectrogram_column_first(v->w_min, v->w_max - v->w_min, v->t_cols, t + 1);
    }
    if (first) *first = a;
    if (end) *end = e;
}

// ---- loudness regions: gated loudness of time ranges and groups ----------------------------------------------------
int ss_batch_loudness_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!(b->cfg.flags & SS_BATCH_LUFS)) return SS_ERR_INVALID_MODE;
    uint32_t longest = 0;
    int rc = check_regions(b, regions, n_regions, n_groups, [b](uint32_t s) { return b->subblocks_of(s); }, &longest);
    if (rc) return rc;
    Regions &rg = b->regions;
    HIPCHK(rg.results.ensure(n_regions)); HIPCHK(rg.group_results.ensure(n_groups)); HIPCHK(rg.group_hist.ensure((size_t)n_groups * 2 * sst::kHistBins));
    if ((rc = rg.list.replace(b->stream, regions, n_regions))) return rc;
    ssk::RegionGateParams p{};
    p.k = b->td->dev.p; p.subblocks = b->sub.p; p.sub_cap = b->sub_cap(); p.sub_stride = (uint64_t)p.sub_cap * b->cfg.channels;
    p.hist_energies = b->hist_energies; p.hist_bounds = b->hist_bounds; p.weights = b->weights.p; p.state = b->state.p;
    p.channels = b->cfg.channels;
    p.regions = rg.list.dev.p; p.results = rg.results.p; p.n_regions = n_regions; p.n_groups = n_groups; p.longest = longest;
    p.group_results = rg.group_results.p; p.group_hist = rg.group_hist.p;
    HIPCHK(ssk::launch_region_gate(p, b->stream));
    rg.list.queued(n_regions, n_groups);
    return SS_OK;
}

static bool has_loudness_regions(const ss_batch *b) { return (b->cfg.flags & SS_BATCH_LUFS) && b->regions.list.done; }

int ss_batch_download_region_results(ss_batch *b, ss_region_result *out, uint32_t cap_regions)
{
    SS_ON_DEVICE(b);
    return !b ? SS_ERR_INVALID_ARG : fetch_records(b, has_loudness_regions(b), out, cap_regions, b->regions.list.n_regions, b->regions.results.p);
}

int ss_batch_download_group_results(ss_batch *b, ss_group_result *out, uint32_t cap_groups)
{
    SS_ON_DEVICE(b);
    return !b ? SS_ERR_INVALID_ARG : fetch_records(b, has_loudness_regions(b), out, cap_groups, b->regions.list.n_groups, b->regions.group_results.p);
}

int ss_batch_group_histograms(ss_batch *b, uint32_t group, uint64_t *out2000)
{
    SS_ON_DEVICE(b);
    if (!b || !out2000) return SS_ERR_INVALID_ARG;
    if (!has_loudness_regions(b)) return SS_ERR_INVALID_MODE;
    if (group >= b->regions.list.n_groups) return SS_ERR_INVALID_ARG;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the histograms are copied out as they are");
    return fetch(b, out2000, reinterpret_cast<const uint64_t *>(b->regions.group_hist.p) + (size_t)group * 2 * sst::kHistBins, 2 * sst::kHistBins);
}

// ---- peak series and peak regions: true and sample peak per 100 ms entry, and their maxima over ranges and groups -----------
// the series' time grid and tiling: the batch's rate and slot size alone (no pass, no tables)
static uint32_t peak_s100(const ss_batch *b) { return (b->cfg.sample_rate + 5u) / 10u; }
static ssk::PeakSeriesPlan batch_peak_plan(const ss_batch *b) { return ssk::plan_peak_series(b->cfg.channels, peak_s100(b), b->cfg.frames_per_stream); }
// E_s: entries of a stream of the batch, the tail's partial entry included
static uint64_t peak_entries_of(const ss_batch *b, uint32_t stream)
{
    const uint64_t S = peak_s100(b);
    return S ? (b->frames_of(stream) + S - 1) / S : 0;
}

int ss_batch_peak_series_plan(const ss_batch *b, uint32_t *tile_frames, uint32_t *entries_cap)
{
    if (!b) return SS_ERR_INVALID_ARG;
    const ssk::PeakSeriesPlan plan = batch_peak_plan(b);
    if (tile_frames) *tile_frames = plan.tile_frames;
    if (entries_cap) *entries_cap = plan.entries_cap;
    return SS_OK;
}

int ss_batch_peak_series(ss_batch *b)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const ss_batch_config &c = b->cfg;
    const ssk::PeakSeriesPlan plan = batch_peak_plan(b);
    if (!peak_s100(b) || (uint64_t)plan.entries_cap * peak_s100(b) < c.frames_per_stream) return SS_ERR_UNSUPPORTED;     // (2^32 entries)
    ssk::PeakSeriesParams p{};
    p.factor = c.true_peak_factor ? (int)c.true_peak_factor : sst::true_peak_factor_for_rate(c.sample_rate);
    if (p.factor) {
        uint32_t len = 0;
        static_assert(sizeof p.taps / sizeof p.taps[0] == 36, "three branches of 12 taps, or one of 24");
        int rc = ss_inspect_true_peak(p.factor, p.taps, 36, &len);
        if (rc) return rc;
    }
    // (the shape of a batch is fixed at create, so only the first call allocates)
    HIPCHK(b->peaks.series.ensure((size_t)c.n_streams * plan.entries_cap * c.channels));
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * c.channels; p.n_frames = c.frames_per_stream;
    p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.series = b->peaks.series.p;
    p.n_streams = c.n_streams; p.channels = c.channels; p.s100 = peak_s100(b);
    p.tile_frames = plan.tile_frames; p.entries_cap = plan.entries_cap;
    HIPCHK(ssk::launch_peak_series(p, b->stream));
    b->peaks.series_done = true;
    return SS_OK;
}

int ss_batch_download_peak_series(ss_batch *b, uint32_t stream, ss_peak_entry *out, size_t cap_entries, uint32_t *n_entries)
{
    SS_ON_DEVICE(b);
    if (!b || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    if (!b->peaks.series_done) return SS_ERR_INVALID_MODE;
    const uint64_t n = peak_entries_of(b, stream);
    if (!out && n) return SS_ERR_INVALID_ARG;
    if (cap_entries < n) return SS_ERR_CAPACITY;
    if (n_entries) *n_entries = (uint32_t)n;
    if (!n) return ss_batch_sync(b);
    const size_t C = b->cfg.channels;
    return fetch(b, out, b->peaks.series.p + (size_t)stream * batch_peak_plan(b).entries_cap * C, (size_t)n * C);
}

int ss_batch_peak_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups, double ceiling)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    Peaks &pk = b->peaks;
    if (!pk.series_done) return SS_ERR_INVALID_MODE;
    if (!(ceiling >= 0.0)) return SS_ERR_INVALID_ARG;        // (NaN fails the comparison)
    uint32_t longest = 0;
    int rc = check_regions(b, regions, n_regions, n_groups, [b](uint32_t s) { return peak_entries_of(b, s); }, &longest);
    if (rc) return rc;
    const size_t C = b->cfg.channels;
    HIPCHK(pk.results.ensure(n_regions)); HIPCHK(pk.ch_true.ensure((size_t)n_regions * C)); HIPCHK(pk.ch_sample.ensure((size_t)n_regions * C));
    HIPCHK(pk.group_acc.ensure((size_t)n_groups * 3)); HIPCHK(pk.group_results.ensure(n_groups));
    if ((rc = pk.list.replace(b->stream, regions, n_regions))) return rc;
    ssk::RegionPeaksParams p{};
    p.series = pk.series.p; p.entries_cap = batch_peak_plan(b).entries_cap; p.channels = b->cfg.channels; p.s100 = peak_s100(b);
    p.ceiling = ceiling;
    p.regions = pk.list.dev.p; p.results = pk.results.p; p.ch_true = pk.ch_true.p; p.ch_sample = pk.ch_sample.p;
    p.n_regions = n_regions; p.n_groups = n_groups; p.group_acc = pk.group_acc.p; p.group_results = pk.group_results.p;
    HIPCHK(ssk::launch_region_peaks(p, b->stream));
    pk.list.queued(n_regions, n_groups);
    return SS_OK;
}

int ss_batch_download_region_peaks(ss_batch *b, ss_region_peaks *out, uint32_t cap_regions)
{
    SS_ON_DEVICE(b);
    return !b ? SS_ERR_INVALID_ARG : fetch_records(b, b->peaks.list.done, out, cap_regions, b->peaks.list.n_regions, b->peaks.results.p);
}

int ss_batch_download_group_peaks(ss_batch *b, ss_group_peaks *out, uint32_t cap_groups)
{
    SS_ON_DEVICE(b);
    return !b ? SS_ERR_INVALID_ARG : fetch_records(b, b->peaks.list.done, out, cap_groups, b->peaks.list.n_groups, b->peaks.group_results.p);
}

int ss_batch_download_region_channel_peaks(ss_batch *b, float *true_pk, float *sample_pk, size_t cap_floats)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!b->peaks.list.done) return SS_ERR_INVALID_MODE;
    const size_t n = (size_t)b->peaks.list.n_regions * b->cfg.channels;
    if (cap_floats < n) return SS_ERR_CAPACITY;
    if (n && true_pk) HIPCHK(hipMemcpyAsync(true_pk, b->peaks.ch_true.p, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    if (n && sample_pk) HIPCHK(hipMemcpyAsync(sample_pk, b->peaks.ch_sample.p, n * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    return ss_batch_sync(b);
}

// ---- spectrum regions: average and peak-hold spectrum of time ranges and groups -----------------------------------------------------
static_assert(sizeof(ssk::SpecRegion) == 16, "resolved region layout");

// The windows [first, end) that lie wholly inside the sub-blocks [a, a + n) of S frames, before the cut at a stream's window count:
// window w covers the frames [first_start + w hop, first_start + w hop + fft_n), first_start where stream_shape puts window 0.
// (a, n < 2^32, S < 2^29, fft_n + hop < 2^33: everything fits 64 bits.)
struct WindowRange { uint64_t first, end; };
static WindowRange region_windows(uint64_t S, uint64_t fft_n, uint64_t hop, uint64_t a, uint64_t n)
{
    if (!fft_n || !hop) return {0, 0};
    const uint64_t f0 = a * S, f1 = (a + n) * S, first_start = (fft_n / hop + 1) * hop - fft_n;
    const uint64_t lo = f0 <= first_start ? 0 : (f0 - first_start + hop - 1) / hop;
    const uint64_t hi = f1 >= first_start + fft_n ? (f1 - fft_n - first_start) / hop + 1 : 0;
    return {lo, lo > hi ? lo : hi};
}

void ss_region_windows(uint32_t sample_rate, uint32_t fft_n, uint32_t hop_frames, uint32_t first_subblock, uint32_t n_subblocks,
                       uint32_t *first, uint32_t *end)
{
    const WindowRange r = region_windows(((uint64_t)sample_rate + 5u) / 10u, fft_n, hop_frames, first_subblock, n_subblocks);
    if (first) *first = (uint32_t)std::min<uint64_t>(r.first, 0xFFFFFFFFull);
    if (end) *end = (uint32_t)std::min<uint64_t>(r.end, 0xFFFFFFFFull);
}

int ss_batch_spectrum_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    if (!has_spectrum_rows(b)) return SS_ERR_INVALID_MODE;
    uint32_t longest_sub = 0;
    int rc = check_regions(b, regions, n_regions, n_groups, [b](uint32_t s) { return peak_entries_of(b, s); }, &longest_sub);
    if (rc) return rc;
    const ss_batch_layout &L = b->lay;
    // every region as the kernels read it: its windows, cut to its stream's own count; the longest one makes the plan
    std::vector<uint32_t> own(b->cfg.n_streams, L.n_windows);
    if (b->ragged.on)
        for (uint32_t s = 0; s < b->cfg.n_streams; s++) own[s] = std::min(stream_shape(b, b->frames_of(s)).windows, L.n_windows);
    std::vector<ssk::SpecRegion> resolved(n_regions);
    uint32_t longest = 0, grouped = 0;
    for (uint32_t i = 0; i < n_regions; i++) {
        const ss_loudness_region &r = regions[i];
        const WindowRange w = region_windows(peak_s100(b), b->cfg.fft_n, b->cfg.hop_frames, r.first_subblock, r.n_subblocks);
        const uint32_t nw = own[r.stream];
        resolved[i] = {r.stream, (uint32_t)std::min<uint64_t>(w.first, nw), (uint32_t)std::min<uint64_t>(w.end, nw), r.group};
        longest = std::max(longest, resolved[i].w_end - resolved[i].w_first);
        grouped += r.group != SS_REGION_NO_GROUP;
    }
    SpectrumRegions &sr = b->spec_regions;
    ssk::SpecStatsPlan plan;
    if (!ssk::spectrum_regions_fit(n_regions, n_groups, L.fft_channels, L.fft_bin_stride, longest, &plan)) return SS_ERR_UNSUPPORTED;
    const size_t per = (size_t)L.fft_channels * L.fft_bin_stride, all = per * n_regions, parts = plan.chunks > 1 ? all * plan.chunks : 0;
    HIPCHK(sr.sums.ensure(all)); HIPCHK(sr.mean.ensure(all)); HIPCHK(sr.max.ensure(all)); HIPCHK(sr.counts.ensure(all));
    HIPCHK(sr.part_sums.ensure(parts)); HIPCHK(sr.part_max.ensure(parts)); HIPCHK(sr.part_counts.ensure(parts));
    HIPCHK(sr.group_mean.ensure(per * n_groups)); HIPCHK(sr.group_max.ensure(per * n_groups));
    HIPCHK(sr.group_counts.ensure((size_t)L.fft_channels * n_groups));
    // the table, built in the stage: the records, then member_start (a counting sort's prefix sums) and every group's members in
    // region index order
    const size_t start_at = (size_t)4 * n_regions, members_at = start_at + n_groups + 1, words = members_at + grouped;
    HIPCHK(sr.table.ensure(words));
    HIPCHK(sr.list.stage.take(words * sizeof(uint32_t)));
    uint32_t *t = reinterpret_cast<uint32_t *>(sr.list.stage.buf.p);
    if (n_regions) std::memcpy(t, resolved.data(), (size_t)n_regions * sizeof(ssk::SpecRegion));
    std::vector<uint32_t> next((size_t)n_groups + 1, 0u);           // a group's next free place among the members
    for (const ssk::SpecRegion &r : resolved) if (r.group != SS_REGION_NO_GROUP) next[r.group + 1]++;
    for (uint32_t g = 0; g < n_groups; g++) next[g + 1] += next[g];
    std::memcpy(t + start_at, next.data(), next.size() * sizeof(uint32_t));
    for (uint32_t i = 0; i < n_regions; i++) if (resolved[i].group != SS_REGION_NO_GROUP) t[members_at + next[resolved[i].group]++] = i;
    HIPCHK(sr.list.stage.queue(sr.table.p, words * sizeof(uint32_t), b->stream));
    ssk::SpecRegionsParams q{};
    q.s = batch_stats_params(b);
    q.s.n_streams = n_regions; q.s.windows_of = nullptr; q.s.plan = plan;
    q.s.sums = sr.sums.p; q.s.mean = sr.mean.p; q.s.max = sr.max.p; q.s.counts = sr.counts.p;
    q.s.part_sums = sr.part_sums.p; q.s.part_max = sr.part_max.p; q.s.part_counts = sr.part_counts.p;
    q.regions = reinterpret_cast<const ssk::SpecRegion *>(sr.table.p);
    q.n_groups = n_groups; q.member_start = sr.table.p + start_at; q.members = sr.table.p + members_at;
    q.group_mean = sr.group_mean.p; q.group_max = sr.group_max.p; q.group_counts = sr.group_counts.p;
    HIPCHK(ssk::launch_spectrum_regions(q, b->stream));
    sr.plan = plan;
    sr.list.queued(n_regions, n_groups);
    return SS_OK;
}

static bool has_spectrum_regions(const ss_batch *b) { return has_spectrum_rows(b) && b->spec_regions.list.done; }

int ss_batch_spectrum_regions_plan(const ss_batch *b, uint32_t *chunks, uint32_t *chunk_windows)
{
    if (!b) return SS_ERR_INVALID_ARG;
    if (!has_spectrum_regions(b)) return SS_ERR_INVALID_MODE;
    if (chunks) *chunks = b->spec_regions.plan.chunks;
    if (chunk_windows) *chunk_windows = b->spec_regions.plan.chunk_windows;
    return SS_OK;
}

// the status ladder of the two downloads, `listed` the regions or groups of the last list: the mode, the range, the capacities
static int check_spectra_range(const ss_batch *b, uint32_t listed, uint32_t first, uint32_t count, bool floats, size_t cap_floats,
                               bool counts, size_t cap_counts)
{
    if (!has_spectrum_regions(b)) return SS_ERR_INVALID_MODE;
    if ((uint64_t)first + count > listed) return SS_ERR_INVALID_ARG;
    const size_t rows = (size_t)count * b->lay.fft_channels;
    if ((floats && cap_floats < rows * b->lay.n_bins) || (counts && cap_counts < rows)) return SS_ERR_CAPACITY;
    return SS_OK;
}

int ss_batch_download_region_spectra(ss_batch *b, uint32_t first_region, uint32_t count, float *mean_db, float *max_db, size_t cap_floats,
                                     uint32_t *windows_counted, size_t cap_counts)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const SpectrumRegions &sr = b->spec_regions;
    int rc = check_spectra_range(b, sr.list.n_regions, first_region, count, mean_db || max_db, cap_floats, windows_counted != nullptr, cap_counts);
    if (rc) return rc;
    const ss_batch_layout &L = b->lay;
    const size_t rows = (size_t)count * L.fft_channels, at = (size_t)first_region * L.fft_channels * L.fft_bin_stride;
    if (rows && (rc = fetch_stats_rows(b, mean_db, max_db, sr.mean.p + at, sr.max.p + at, rows))) return rc;
    // the count of a (region, channel) is bin 0's: one u32 of every [fft_bin_stride] row
    if (rows && windows_counted && L.fft_bin_stride)
        HIPCHK(hipMemcpy2DAsync(windows_counted, sizeof(uint32_t), sr.counts.p + at, (size_t)L.fft_bin_stride * sizeof(uint32_t),
                                sizeof(uint32_t), rows, hipMemcpyDeviceToHost, b->stream));
    return ss_batch_sync(b);
}

int ss_batch_download_group_spectra(ss_batch *b, uint32_t first_group, uint32_t count, float *mean_db, float *max_db, size_t cap_floats,
                                    uint64_t *windows_counted, size_t cap_counts)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const SpectrumRegions &sr = b->spec_regions;
    int rc = check_spectra_range(b, sr.list.n_groups, first_group, count, mean_db || max_db, cap_floats, windows_counted != nullptr, cap_counts);
    if (rc) return rc;
    const ss_batch_layout &L = b->lay;
    const size_t rows = (size_t)count * L.fft_channels, at = (size_t)first_group * L.fft_channels * L.fft_bin_stride;
    if (rows && (rc = fetch_stats_rows(b, mean_db, max_db, sr.group_mean.p + at, sr.group_max.p + at, rows))) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the pooled counts are copied out as they are");
    if (rows && windows_counted && L.fft_bin_stride)
        HIPCHK(hipMemcpyAsync(windows_counted, sr.group_counts.p + (size_t)first_group * L.fft_channels, rows * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, b->stream));
    return ss_batch_sync(b);
}

// ---- signal scan: silence, clip runs, DC and non-finite samples of every stream, and the lists of the runs --------------------
static_assert(sizeof(ss_signal_scan_config) == 24, "scan config layout");

// the scan's tiling: the batch's channel count and slot size alone (no pass, no tables)
static ssk::SignalScanPlan batch_scan_plan(const ss_batch *b) { return ssk::plan_signal_scan(b->cfg.channels, b->cfg.frames_per_stream); }

int ss_batch_signal_scan_plan(const ss_batch *b, uint32_t *tile_frames, uint32_t *tiles_cap)
{
    if (!b) return SS_ERR_INVALID_ARG;
    const ssk::SignalScanPlan plan = batch_scan_plan(b);
    if (tile_frames) *tile_frames = plan.tile_frames;
    if (tiles_cap) *tiles_cap = plan.tiles_cap;
    return SS_OK;
}

int ss_batch_signal_scan(ss_batch *b, const ss_signal_scan_config *cfg)
{
    SS_ON_DEVICE(b);
    if (!b || !cfg) return SS_ERR_INVALID_ARG;
    if (!(cfg->silence_threshold >= 0.f) || !(cfg->clip_level > 0.f)) return SS_ERR_INVALID_ARG;        // (NaN fails the comparison)
    if (!cfg->silence_min_frames || !cfg->clip_min_samples || cfg->max_events > 65536u || cfg->reserved) return SS_ERR_INVALID_ARG;
    const ss_batch_config &c = b->cfg;
    const ssk::SignalScanPlan plan = batch_scan_plan(b);
    const size_t tiles = (size_t)c.n_streams * plan.tiles_cap, Q = (size_t)c.channels + 1;
    if ((uint64_t)plan.tiles_cap * plan.tile_frames < c.frames_per_stream || tiles > 0x7FFFFFFFull) return SS_ERR_UNSUPPORTED;      // (2^31 tiles)
    SignalScan &sc = b->scan;
    // (the shape of a batch is fixed at create, so only the first call allocates; the lists grow with max_events)
    HIPCHK(sc.tile_runs.ensure(tiles * Q)); HIPCHK(sc.tile_channels.ensure(tiles * c.channels)); HIPCHK(sc.tile_carry.ensure(tiles * Q));
    HIPCHK(sc.list_base.ensure(c.n_streams * Q)); HIPCHK(sc.streams.ensure(c.n_streams)); HIPCHK(sc.channels.ensure((size_t)c.n_streams * c.channels));
    HIPCHK(sc.events.ensure((size_t)c.n_streams * 2 * cfg->max_events));
    ssk::SignalScanParams p{};
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * c.channels; p.n_frames = c.frames_per_stream;
    p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.n_streams = c.n_streams; p.channels = c.channels; p.tile_frames = plan.tile_frames; p.tiles_cap = plan.tiles_cap;
    p.silence_threshold = cfg->silence_threshold; p.clip_level = cfg->clip_level;
    p.silence_min = cfg->silence_min_frames; p.clip_min = cfg->clip_min_samples; p.max_events = cfg->max_events;
    p.tile_runs = sc.tile_runs.p; p.tile_channels = sc.tile_channels.p; p.tile_carry = sc.tile_carry.p; p.list_base = sc.list_base.p;
    p.streams = sc.streams.p; p.channel_scans = sc.channels.p; p.events = sc.events.p;
    HIPCHK(ssk::launch_signal_scan(p, b->stream));
    sc.cfg = *cfg;
    sc.done = true;
    return SS_OK;
}

int ss_batch_download_stream_scans(ss_batch *b, ss_stream_scan *out, uint32_t cap_streams)
{
    SS_ON_DEVICE(b);
    return !b ? SS_ERR_INVALID_ARG : fetch_records(b, b->scan.done, out, cap_streams, b->cfg.n_streams, b->scan.streams.p);
}

int ss_batch_download_channel_scans(ss_batch *b, ss_channel_scan *out, size_t cap_records)
{
    SS_ON_DEVICE(b);
    if (!b || !out) return SS_ERR_INVALID_ARG;
    if (!b->scan.done) return SS_ERR_INVALID_MODE;
    const size_t n = (size_t)b->cfg.n_streams * b->cfg.channels;
    if (cap_records < n) return SS_ERR_CAPACITY;
    return fetch(b, out, b->scan.channels.p, n);
}

int ss_batch_download_signal_events(ss_batch *b, uint32_t stream, int kind, ss_signal_event *out, size_t cap_events, uint32_t *n_events)
{
    SS_ON_DEVICE(b);
    if (!b || stream >= b->cfg.n_streams || (kind != SS_SIGNAL_SILENCE && kind != SS_SIGNAL_CLIP)) return SS_ERR_INVALID_ARG;
    const SignalScan &sc = b->scan;
    if (!sc.done) return SS_ERR_INVALID_MODE;
    // how many there are is the stream's own record: the count, cut at the lists' slots
    ssk::StreamScan rec;
    int rc = fetch(b, &rec, sc.streams.p + stream, 1);
    if (rc) return rc;
    const uint64_t count = kind == SS_SIGNAL_CLIP ? rec.clip_runs : rec.silence_runs;
    const uint32_t n = count < sc.cfg.max_events ? (uint32_t)count : sc.cfg.max_events;
    if (!out && n) return SS_ERR_INVALID_ARG;
    if (cap_events < n) return SS_ERR_CAPACITY;
    if (n_events) *n_events = n;
    if (!n) return SS_OK;
    const ssk::SignalEvent *src = sc.events.p + ((size_t)stream * 2 + (kind == SS_SIGNAL_CLIP ? 1 : 0)) * sc.cfg.max_events;
    return fetch(b, out, src, n);
}

// ---- pair series and pair regions: sums of x_a^2, x_b^2 and x_a x_b per 100 ms entry, and over ranges and groups ------------------
static_assert(sizeof(ss_pair_region_config) == 24, "pair region config layout");

// the pair list a call means: the caller's, or the one pair (0, 1); checked against the batch's channels
static int pair_list_of(const ss_batch *b, const ss_channel_pair *pairs, uint32_t n_pairs, ssk::ChannelPair (&list)[ssk::kMaxPairs], uint32_t *n)
{
    const uint32_t C = b->cfg.channels;
    if (n_pairs > ssk::kMaxPairs || (!pairs && n_pairs)) return SS_ERR_INVALID_ARG;
    if (!pairs || !n_pairs) {                                   // the default pair needs two channels
        if (C < 2u) return SS_ERR_INVALID_ARG;
        list[0].a = 0u; list[0].b = 1u;
        *n = 1u;
        return SS_OK;
    }
    for (uint32_t k = 0; k < n_pairs; k++) {
        if (pairs[k].a >= C || pairs[k].b >= C) return SS_ERR_INVALID_ARG;
        list[k] = pairs[k];
    }
    *n = n_pairs;
    return SS_OK;
}

int ss_batch_pair_series_plan(const ss_batch *b, uint32_t *tile_frames, uint32_t *entries_cap, uint32_t *n_pairs)
{
    if (!b) return SS_ERR_INVALID_ARG;
    const ssk::ChannelPair dflt = {0u, 1u};                      // before the first call: the default list's plan
    const bool called = b->pair.series_done;
    const ssk::PairSeriesPlan plan = ssk::plan_pair_series(b->cfg.channels, peak_s100(b), b->cfg.frames_per_stream, called ? b->pair.pairs : &dflt, called ? b->pair.n_pairs : 1u);
    if (tile_frames) *tile_frames = plan.sweep_frames;
    if (entries_cap) *entries_cap = plan.entries_cap;
    if (n_pairs) *n_pairs = called ? b->pair.n_pairs : 1u;
    return SS_OK;
}

int ss_batch_pair_series(ss_batch *b, const ss_channel_pair *pairs, uint32_t n_pairs)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const ss_batch_config &c = b->cfg;
    ssk::PairSeriesParams p{};
    int rc = pair_list_of(b, pairs, n_pairs, p.pairs, &p.n_pairs);
    if (rc) return rc;
    const ssk::PairSeriesPlan plan = ssk::plan_pair_series(c.channels, peak_s100(b), c.frames_per_stream, p.pairs, p.n_pairs);
    if (!peak_s100(b) || (uint64_t)plan.entries_cap * peak_s100(b) < c.frames_per_stream) return SS_ERR_UNSUPPORTED;     // (2^32 entries)
    Pairs &pr = b->pair;
    // (a longer pair list grows the series: the buffer is freed first, and hipFree waits for whatever still uses it)
    HIPCHK(pr.series.ensure((size_t)c.n_streams * plan.entries_cap * p.n_pairs));
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * c.channels; p.n_frames = c.frames_per_stream;
    p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.series = pr.series.p;
    p.n_streams = c.n_streams; p.channels = c.channels; p.s100 = peak_s100(b);
    p.entries_cap = plan.entries_cap; p.stereo = plan.stereo ? 1u : 0u;
    HIPCHK(ssk::launch_pair_series(p, b->stream));
    pr.n_pairs = p.n_pairs;
    for (uint32_t k = 0; k < p.n_pairs; k++) pr.pairs[k] = p.pairs[k];
    pr.series_done = true;
    return SS_OK;
}

int ss_batch_download_pair_series(ss_batch *b, uint32_t stream, ss_pair_entry *out, size_t cap_entries, uint32_t *n_entries)
{
    SS_ON_DEVICE(b);
    if (!b || stream >= b->cfg.n_streams) return SS_ERR_INVALID_ARG;
    const Pairs &pr = b->pair;
    if (!pr.series_done) return SS_ERR_INVALID_MODE;
    const uint64_t n = peak_entries_of(b, stream);
    if (!out && n) return SS_ERR_INVALID_ARG;
    if (cap_entries < n) return SS_ERR_CAPACITY;
    if (n_entries) *n_entries = (uint32_t)n;
    if (!n) return ss_batch_sync(b);
    const size_t cap = ssk::plan_peak_series(b->cfg.channels, peak_s100(b), b->cfg.frames_per_stream).entries_cap;
    return fetch(b, out, pr.series.p + (size_t)stream * cap * pr.n_pairs, (size_t)n * pr.n_pairs);
}

int ss_batch_pair_regions(ss_batch *b, const ss_loudness_region *regions, uint32_t n_regions, uint32_t n_groups, const ss_pair_region_config *cfg)
{
    SS_ON_DEVICE(b);
    if (!b || !cfg) return SS_ERR_INVALID_ARG;
    Pairs &pr = b->pair;
    if (!pr.series_done) return SS_ERR_INVALID_MODE;
    if (!(cfg->threshold > -1.0 && cfg->threshold < 1.0) || !(cfg->power_floor >= 0.0)) return SS_ERR_INVALID_ARG;       // (NaN fails the comparisons)
    if (!cfg->min_run || cfg->reserved) return SS_ERR_INVALID_ARG;
    uint32_t longest = 0;
    int rc = check_regions(b, regions, n_regions, n_groups, [b](uint32_t s) { return peak_entries_of(b, s); }, &longest);
    if (rc) return rc;
    const size_t NP = pr.n_pairs;
    if (n_regions * NP > 0x7FFFFFFFull || n_groups * NP > 0x7FFFFFFFull) return SS_ERR_UNSUPPORTED;
    HIPCHK(pr.results.ensure(n_regions * NP)); HIPCHK(pr.group_results.ensure(n_groups * NP));
    if ((rc = pr.list.replace(b->stream, regions, n_regions))) return rc;
    ssk::RegionPairsParams p{};
    p.series = pr.series.p; p.n_pairs = pr.n_pairs;
    p.entries_cap = ssk::plan_peak_series(b->cfg.channels, peak_s100(b), b->cfg.frames_per_stream).entries_cap;
    p.threshold = cfg->threshold; p.power_floor = cfg->power_floor; p.min_run = cfg->min_run;
    p.regions = pr.list.dev.p; p.results = pr.results.p; p.n_regions = n_regions; p.n_groups = n_groups; p.group_results = pr.group_results.p;
    HIPCHK(ssk::launch_region_pairs(p, b->stream));
    pr.list.queued(n_regions, n_groups);
    pr.list_pairs = pr.n_pairs;
    return SS_OK;
}

int ss_batch_download_region_pairs(ss_batch *b, ss_region_pair *out, size_t cap_records)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const Pairs &pr = b->pair;
    return fetch_records(b, pr.list.done, out, cap_records > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap_records, pr.list.n_regions * pr.list_pairs, pr.results.p);
}

int ss_batch_download_group_pairs(ss_batch *b, ss_group_pair *out, size_t cap_records)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const Pairs &pr = b->pair;
    return fetch_records(b, pr.list.done, out, cap_records > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap_records, pr.list.n_groups * pr.list_pairs, pr.group_results.p);
}

// ---- batch gain and PCM export: the gain law and the gain curve (host arithmetic), the sweep, the delivery formats ------------------
static_assert(sizeof(ss_normalise_target) == 32 && sizeof(ss_gain_point) == 16 && offsetof(ss_gain_point, stream) == 8 && offsetof(ss_gain_point, gain) == 12 &&
              sizeof(ss_gain_config) == 16 && offsetof(ss_gain_config, clip_level) == 8 && sizeof(ss_pcm_dither) == 16, "gain call layouts");

int ss_normalisation_gain(const ss_normalise_target *t, double loudness_lufs, double peak_linear, double *gain_db, float *gain, uint32_t *limited_by)
{
    if (!t || std::isnan(t->target_lufs) || std::isnan(t->max_true_peak_dbtp) || std::isnan(t->max_gain_db) || std::isnan(t->min_gain_db) ||
        std::isnan(peak_linear) || t->min_gain_db > t->max_gain_db)
        return SS_ERR_INVALID_ARG;
    double g = 0.0;
    float lin = 1.0f;
    uint32_t why = 0;
    if (!std::isfinite(loudness_lufs)) {
        why = SS_GAIN_UNMEASURED;
    } else {
        g = t->target_lufs - loudness_lufs;
        double headroom = 0.0;
        if (std::isfinite(t->max_true_peak_dbtp) && std::isfinite(peak_linear) && peak_linear > 0.0) {
            headroom = t->max_true_peak_dbtp - 20.0 * std::log10(peak_linear);
            if (g > headroom) { g = headroom; why |= SS_GAIN_LIMITED_PEAK; }
        }
        if (g > t->max_gain_db) { g = t->max_gain_db; why |= SS_GAIN_LIMITED_MAX; }
        if (g < t->min_gain_db) { g = t->min_gain_db; why |= SS_GAIN_LIMITED_MIN; }
        const double exact = std::pow(10.0, g / 20.0);
        lin = (float)exact;
        // the ceiling bound the result: the rounding of the gain must not carry it above
        if ((why & SS_GAIN_LIMITED_PEAK) && g == headroom && (double)lin > exact) lin = std::nextafterf(lin, -INFINITY);
    }
    if (gain_db) *gain_db = g;
    if (gain) *gain = lin;
    if (limited_by) *limited_by = why;
    return SS_OK;
}

double ss_gain_envelope(const ss_gain_point *pts, uint32_t n, uint64_t frame)
{
    if (!pts || !n) return 1.0;
    if (frame <= pts[0].frame) return (double)pts[0].gain;
    if (frame >= pts[n - 1].frame) return (double)pts[n - 1].gain;
    uint32_t lo = 0, hi = n - 1;                                // pts[lo].frame <= frame < pts[hi].frame
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (pts[mid].frame <= frame) lo = mid; else hi = mid;
    }
    const double g0 = (double)pts[lo].gain, g1 = (double)pts[lo + 1].gain;
    const double d = (g1 - g0) / (double)(pts[lo + 1].frame - pts[lo].frame);
    {
#pragma clang fp contract(off)                                  // the product is rounded on its own
        const double step = (double)(frame - pts[lo].frame) * d;
        return g0 + step;
    }
}

// One stream's points as the segments k_apply_gain reads (ssk::GainSegment): what ss_gain_envelope gives, frame for frame.
//  * [0, f_0]: the constant g_0 (a lone point: the whole stream);
//  * point k to point k + 1: the ramp from f_k — from f_0 + 1 for k = 0, frame f_0 being the first segment's — which is empty where
//    f_1 = f_0 + 1; a ramp between equal gains has d = +0 and every value of it is g_k + 0 (which makes +0 of a gain of -0), a constant;
//  * from the last point on: the constant g_last.
static void gain_segments(const ss_gain_point *pts, uint32_t n, std::vector<ssk::GainSegment> *out)
{
    out->push_back({0ull, ssk::kGainConst, (double)pts[0].gain, 0.0});
    for (uint32_t k = 0; k + 1 < n; k++) {
        const uint64_t start = k ? pts[k].frame : pts[0].frame + 1;
        if (start >= pts[k + 1].frame) continue;
        const double g0 = (double)pts[k].gain, g1 = (double)pts[k + 1].gain;
        const double d = (g1 - g0) / (double)(pts[k + 1].frame - pts[k].frame);
        if (d == 0.0) out->push_back({start, ssk::kGainConst, g0 + 0.0, 0.0});
        else out->push_back({start, pts[k].frame, g0, d});
    }
    if (n > 1) out->push_back({pts[n - 1].frame, ssk::kGainConst, (double)pts[n - 1].gain, 0.0});
}

int ss_batch_apply_gain_plan(const ss_batch *b, uint32_t *tile_frames)
{
    if (!b) return SS_ERR_INVALID_ARG;
    if (tile_frames) *tile_frames = ssk::kGainTileFrames;
    return SS_OK;
}

int ss_batch_apply_gain(ss_batch *b, const ss_gain_point *points, uint32_t n_points, const ss_gain_config *cfg)
{
    SS_ON_DEVICE(b);
    if (!b || !cfg || (!points && n_points)) return SS_ERR_INVALID_ARG;
    const ss_batch_config &c = b->cfg;
    const uint32_t C = c.channels;
    if (!(cfg->clip_level > 0.0f) || cfg->reserved) return SS_ERR_INVALID_ARG;          // (NaN fails the comparison)
    if (C < 64u && (cfg->channel_mask >> C)) return SS_ERR_INVALID_ARG;
    // the streams' runs of points: grouped by stream, frames strictly ascending
    std::vector<ssk::GainStream> touched;
    std::vector<ssk::GainSegment> segments;
    {
        std::vector<bool> seen(c.n_streams, false);
        for (uint32_t i = 0; i < n_points;) {
            const uint32_t s = points[i].stream;
            if (s >= c.n_streams || seen[s]) return SS_ERR_INVALID_ARG;
            seen[s] = true;
            uint32_t j = i;
            for (; j < n_points && points[j].stream == s; j++) {
                if (!std::isfinite(points[j].gain) || points[j].frame >= (1ull << 52)) return SS_ERR_INVALID_ARG;
                if (j > i && points[j].frame <= points[j - 1].frame) return SS_ERR_INVALID_ARG;
            }
            const uint32_t at = (uint32_t)segments.size();
            gain_segments(points + i, j - i, &segments);
            touched.push_back({s, at, (uint32_t)segments.size() - at, 0u});
            i = j;
        }
    }
    const uint64_t tiles_cap = (c.frames_per_stream + ssk::kGainTileFrames - 1) / ssk::kGainTileFrames;
    const uint64_t records = (uint64_t)c.n_streams * C;
    if (touched.size() * tiles_cap > 0x7FFFFFFFull || records > 0xFFFFFFFFull) return SS_ERR_UNSUPPORTED;
    // the table: records | touched | segments
    const size_t touched_at = (size_t)records * sizeof(ssk::GainChannel), seg_at = touched_at + touched.size() * sizeof(ssk::GainStream);
    const size_t bytes = seg_at + segments.size() * sizeof(ssk::GainSegment);
    Gain &gn = b->gain;
    HIPCHK(gn.table.ensure(bytes));             // (a buffer that grows is freed first: hipFree waits for whatever still uses it)
    HIPCHK(gn.stage.take(bytes));
    unsigned char *h = gn.stage.buf.p;
    {
        ssk::GainChannel *rec = reinterpret_cast<ssk::GainChannel *>(h);
        for (uint64_t i = 0; i < records; i++) rec[i] = {0.f, 0u, 0ull, ~0ull, 0ull};
        for (const ssk::GainStream &t : touched)
            for (uint32_t ch = 0; ch < C; ch++) rec[(size_t)t.stream * C + ch].touched = 1u;
        if (!touched.empty()) std::memcpy(h + touched_at, touched.data(), touched.size() * sizeof(ssk::GainStream));
        if (!segments.empty()) std::memcpy(h + seg_at, segments.data(), segments.size() * sizeof(ssk::GainSegment));
    }
    HIPCHK(gn.stage.queue(gn.table.p, bytes, b->stream));
    ssk::ApplyGainParams p{};
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * C; p.n_frames = c.frames_per_stream;
    p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.stats = reinterpret_cast<ssk::GainChannel *>(gn.table.p);
    p.touched = reinterpret_cast<const ssk::GainStream *>(gn.table.p + touched_at);
    p.segments = reinterpret_cast<const ssk::GainSegment *>(gn.table.p + seg_at);
    p.channel_mask = cfg->channel_mask ? cfg->channel_mask : (C < 64u ? (1ull << C) - 1ull : ~0ull);
    p.n_touched = (uint32_t)touched.size(); p.channels = C; p.tiles_cap = (uint32_t)tiles_cap;
    uint32_t clip_bits;
    std::memcpy(&clip_bits, &cfg->clip_level, sizeof clip_bits);
    p.clip_bits = std::isinf(cfg->clip_level) ? 0x7F800001u : clip_bits;
    p.stereo = C == 2u && p.channel_mask == 3ull ? 1u : 0u;
    HIPCHK(ssk::launch_apply_gain(p, b->stream));
    gn.done = true;
    return SS_OK;
}

int ss_batch_download_gain_stats(ss_batch *b, ss_gain_channel *out, size_t cap_records)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const Gain &gn = b->gain;
    return fetch_records(b, gn.done, out, cap_records > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap_records, b->cfg.n_streams * b->cfg.channels,
                         reinterpret_cast<const ssk::GainChannel *>(gn.table.p));
}

// ---- batch limiter: the gain curve (host arithmetic), the plan, the two launches per group of items ---------------------------------
static_assert(offsetof(ss_limit_item, gain) == 4 && offsetof(ss_limit_config, ceiling) == 8 && offsetof(ss_limit_config, clip_level) == 12 &&
              offsetof(ss_limit_config, lookahead) == 16 && offsetof(ss_limit_config, detector) == 24 && offsetof(ss_limit_config, scratch_bytes) == 32 &&
              offsetof(ss_limit_stream, min_sum) == 16 && offsetof(ss_limit_stream, touched) == 24, "limiter call layouts");
constexpr uint64_t kLimitScratchDefault = 256ull << 20;

// what ss_limit_curve and ss_batch_limit both ask of the gain and of the curve's part of a config
static bool limit_curve_args_ok(float gain, const ss_limit_config *cfg)
{
    return cfg && std::isfinite(gain) && cfg->ceiling > 0.0f && std::isfinite(cfg->ceiling) &&          // (NaN fails the comparison)
           cfg->lookahead <= SS_LIMIT_LOOKAHEAD_MAX && cfg->hold <= SS_LIMIT_HOLD_MAX;
}

int ss_limit_curve(const float *level, uint64_t n, float gain, const ss_limit_config *cfg, uint32_t advance, uint32_t *r_q, uint64_t *sum, double *curve)
{
    if (!limit_curve_args_ok(gain, cfg) || (!level && n) || advance > 23u) return SS_ERR_INVALID_ARG;
    if (!n) return SS_OK;
    const uint64_t L = cfg->lookahead, H = cfg->hold, A = advance, one = ssk::kLimitOne;
    // step 2
    std::vector<uint32_t> rq(n);
    const double ag = std::fabs((double)gain), ceiling = (double)cfg->ceiling;
    for (uint64_t i = 0; i < n; i++) {
        const double v = (double)level[i] * ag;
        rq[i] = std::isfinite(v) && v > ceiling ? (uint32_t)std::floor(ceiling / v * (double)one) : (uint32_t)one;
    }
    // step 3: w[i] is w_q of frame k = i - L, the minimum of r_q over [k - H, k + L + A] cut to [0, n) — never empty for these k.
    // The window's ends only move forward, so a queue of candidates with ascending values holds its minimum in front.
    std::vector<uint32_t> w(n + L);
    {
        std::vector<uint64_t> queue(n);
        uint64_t head = 0, tail = 0, next = 0;
        for (uint64_t i = 0; i < n + L; i++) {
            const uint64_t hi = i + A < n - 1 ? i + A : n - 1, lo = i > L + H ? i - L - H : 0;
            for (; next <= hi; next++) {
                while (tail > head && rq[queue[tail - 1]] >= rq[next]) tail--;
                queue[tail++] = next;
            }
            while (queue[head] < lo) head++;
            w[i] = rq[queue[head]];
        }
    }
    // step 4: S[m] = w[m .. m + L] summed, a sum that slides
    const uint64_t full = (L + 1) * one;
    uint64_t s = 0;
    for (uint64_t i = 0; i <= L; i++) s += w[i];
    for (uint64_t m = 0; m < n; m++) {
        if (r_q) r_q[m] = rq[m];
        if (sum) sum[m] = s;
        if (curve) curve[m] = (double)s / (double)full;
        if (m + 1 < n) s = s + w[m + L + 1] - w[m];
    }
    return SS_OK;
}

// every check of a limiter config against the batch, and the detector it means: factor 4, 2 or 0
static int check_limit_config(const ss_batch *b, const ss_limit_config *cfg, int *factor)
{
    if (!cfg || !(cfg->ceiling > 0.0f) || !std::isfinite(cfg->ceiling) || !(cfg->clip_level > 0.0f) || cfg->reserved) return SS_ERR_INVALID_ARG;
    if (cfg->lookahead > SS_LIMIT_LOOKAHEAD_MAX || cfg->hold > SS_LIMIT_HOLD_MAX || cfg->detector > (uint32_t)SS_LIMIT_TRUE_PEAK) return SS_ERR_INVALID_ARG;
    const ss_batch_config &c = b->cfg;
    if (c.channels < 64u && (cfg->channel_mask >> c.channels)) return SS_ERR_INVALID_ARG;
    *factor = cfg->detector == SS_LIMIT_TRUE_PEAK ? (c.true_peak_factor ? (int)c.true_peak_factor : sst::true_peak_factor_for_rate(c.sample_rate)) : 0;
    return SS_OK;
}

static ssk::LimitPlan batch_limit_plan(const ss_batch *b, const ss_limit_config *cfg, uint32_t n_items)
{
    return ssk::plan_limit(b->cfg.frames_per_stream, n_items, cfg->scratch_bytes ? cfg->scratch_bytes : kLimitScratchDefault);
}

int ss_batch_limit_plan(const ss_batch *b, const ss_limit_config *cfg, uint32_t n_items, uint32_t *tile_frames, uint32_t *group_streams, uint64_t *scratch_bytes)
{
    if (!b) return SS_ERR_INVALID_ARG;
    int factor = 0;
    int rc = check_limit_config(b, cfg, &factor);
    if (rc) return rc;
    const ssk::LimitPlan plan = batch_limit_plan(b, cfg, n_items);
    if (n_items && !plan.group_streams) return SS_ERR_CAPACITY;
    if (tile_frames) *tile_frames = plan.tile_frames;
    if (group_streams) *group_streams = plan.group_streams;
    if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
    return SS_OK;
}

int ss_batch_limit(ss_batch *b, const ss_limit_item *items, uint32_t n_items, const ss_limit_config *cfg)
{
    SS_ON_DEVICE(b);
    if (!b || (!items && n_items)) return SS_ERR_INVALID_ARG;
    ssk::LimitParams p{};
    int rc = check_limit_config(b, cfg, &p.factor);
    if (rc) return rc;
    const ss_batch_config &c = b->cfg;
    const uint32_t C = c.channels;
    {
        std::vector<bool> seen(c.n_streams, false);
        for (uint32_t i = 0; i < n_items; i++) {
            if (items[i].stream >= c.n_streams || seen[items[i].stream] || !std::isfinite(items[i].gain)) return SS_ERR_INVALID_ARG;
            seen[items[i].stream] = true;
        }
    }
    const ssk::LimitPlan plan = batch_limit_plan(b, cfg, n_items);
    if (n_items && !plan.group_streams) return SS_ERR_CAPACITY;
    const uint64_t records = (uint64_t)c.n_streams * C;
    if ((uint64_t)n_items * plan.tiles_cap > 0x7FFFFFFFull || records > 0xFFFFFFFFull) return SS_ERR_UNSUPPORTED;
    if (p.factor) {
        uint32_t len = 0;
        rc = ss_inspect_true_peak(p.factor, p.taps, 36, &len);
        if (rc) return rc;
        p.advance = len - 1u;
    }
    // the table: stream records | channel records | items | the tiles' minima (not uploaded)
    const size_t ch_at = (size_t)c.n_streams * sizeof(ssk::LimitStream), items_at = ch_at + (size_t)records * sizeof(ssk::GainChannel);
    const size_t bytes = items_at + (size_t)n_items * sizeof(ssk::LimitItem), min_at = (bytes + 15) & ~(size_t)15;
    Limit &lm = b->limit;
    HIPCHK(lm.table.ensure(min_at + (size_t)n_items * plan.tiles_cap * sizeof(uint32_t)));       // (a buffer that grows is freed first: hipFree waits for whatever still uses it)
    HIPCHK(lm.scratch.ensure((size_t)(plan.scratch_bytes / sizeof(uint32_t))));
    HIPCHK(lm.stage.take(bytes));
    unsigned char *h = lm.stage.buf.p;
    {
        ssk::LimitStream *ls = reinterpret_cast<ssk::LimitStream *>(h);
        ssk::GainChannel *rec = reinterpret_cast<ssk::GainChannel *>(h + ch_at);
        const uint64_t full = ((uint64_t)cfg->lookahead + 1u) * ssk::kLimitOne;
        for (uint32_t s = 0; s < c.n_streams; s++) ls[s] = {0ull, ~0ull, full, 0u, 0u};
        for (uint64_t i = 0; i < records; i++) rec[i] = {0.f, 0u, 0ull, ~0ull, 0ull};
        for (uint32_t i = 0; i < n_items; i++) {
            ls[items[i].stream].touched = 1u;
            for (uint32_t ch = 0; ch < C; ch++) rec[(size_t)items[i].stream * C + ch].touched = 1u;
        }
        if (n_items) std::memcpy(h + items_at, items, (size_t)n_items * sizeof(ssk::LimitItem));
    }
    HIPCHK(lm.stage.queue(lm.table.p, bytes, b->stream));
    p.pcm = b->pcm.p; p.stream_stride = c.frames_per_stream * C; p.n_frames = c.frames_per_stream;
    p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.streams = reinterpret_cast<ssk::LimitStream *>(lm.table.p);
    p.stats = reinterpret_cast<ssk::GainChannel *>(lm.table.p + ch_at);
    p.items = reinterpret_cast<const ssk::LimitItem *>(lm.table.p + items_at);
    p.tile_min = reinterpret_cast<uint32_t *>(lm.table.p + min_at);
    p.scratch = lm.scratch.p;
    p.channel_mask = cfg->channel_mask ? cfg->channel_mask : (C < 64u ? (1ull << C) - 1ull : ~0ull);
    p.channels = C; p.tiles_cap = plan.tiles_cap;
    uint32_t clip_bits;
    std::memcpy(&clip_bits, &cfg->clip_level, sizeof clip_bits);
    p.clip_bits = std::isinf(cfg->clip_level) ? 0x7F800001u : clip_bits;
    p.stereo = C == 2u && p.channel_mask == 3ull ? 1u : 0u;
    p.lookahead = cfg->lookahead; p.hold = cfg->hold; p.ceiling = cfg->ceiling;
    for (uint32_t first = 0; first < n_items; first += plan.group_streams) {
        p.item_first = first; p.n_group = n_items - first < plan.group_streams ? n_items - first : plan.group_streams;
        HIPCHK(ssk::launch_limit(p, b->stream));
    }
    lm.done = true;
    return SS_OK;
}

int ss_batch_download_limit_stats(ss_batch *b, ss_limit_stream *streams, size_t cap_streams, ss_gain_channel *channels, size_t cap_records)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    const Limit &lm = b->limit;
    if (!lm.done) return SS_ERR_INVALID_MODE;
    const uint32_t n = b->cfg.n_streams, records = n * b->cfg.channels;
    if ((streams && cap_streams < n) || (channels && cap_records < records)) return SS_ERR_CAPACITY;
    if (streams) HIPCHK(hipMemcpyAsync(streams, lm.table.p, (size_t)n * sizeof(ss_limit_stream), hipMemcpyDeviceToHost, b->stream));
    if (channels) HIPCHK(hipMemcpyAsync(channels, lm.table.p + (size_t)n * sizeof(ss_limit_stream), (size_t)records * sizeof(ss_gain_channel), hipMemcpyDeviceToHost, b->stream));
    return ss_batch_sync(b);
}

// ---- batch resampler: one corpus converted by L / M into another; the host arithmetic is ss_resample_host.cpp's ---------------------------
// what both entry points ask of a plan: it is the one ss_resample_plan_make makes from the plan's own rates, A and passband
static bool resample_plan_ok(const ss_resample_plan *p)
{
    ss_resample_plan q;
    if (!p || p->reserved || ss_resample_plan_make(p->in_rate, p->out_rate, p->attenuation_db, p->passband, &q) != SS_OK) return false;
    return q.up == p->up && q.down == p->down && q.taps == p->taps && q.beta == p->beta && q.cutoff == p->cutoff;
}

static ssk::ResamplePlan batch_resample_plan(const ss_batch *src, const ss_resample_plan *p)
{
    uint32_t form = ssk::kResampleAuto;
#ifdef SS_TUNING
    if (const char *e = std::getenv("SS_RESAMPLE_FORM")) form = (uint32_t)std::atoi(e);     // 1 register taps, 2 LDS taps, 3 direct
#endif
    return ssk::plan_resample(p->up, p->down, p->taps, src->cfg.channels, form);
}

int ss_batch_resample_plan(const ss_batch *src, const ss_resample_plan *p, uint32_t *tile_out_frames, uint32_t *tile_in_frames)
{
    if (!src || !resample_plan_ok(p) || src->cfg.sample_rate != p->in_rate) return SS_ERR_INVALID_ARG;
    const ssk::ResamplePlan plan = batch_resample_plan(src, p);
    if (tile_out_frames) *tile_out_frames = plan.tile_periods * p->up;
    if (tile_in_frames) *tile_in_frames = plan.tile_periods * p->down;
    return SS_OK;
}

int ss_batch_resample(ss_batch *src, ss_batch *dst, const ss_resample_plan *p)
{
    SS_ON_DEVICE(dst);
    if (!src || !dst || src == dst || !resample_plan_ok(p)) return SS_ERR_INVALID_ARG;
    const ss_batch_config &sc = src->cfg, &dc = dst->cfg;
    if (src->device != dst->device || sc.channels != dc.channels || sc.n_streams != dc.n_streams || sc.sample_rate != p->in_rate ||
        dc.sample_rate != p->out_rate)
        return SS_ERR_INVALID_ARG;
    std::vector<uint64_t> lengths(sc.n_streams);
    uint64_t longest = 0;
    for (uint32_t s = 0; s < sc.n_streams; s++) {
        lengths[s] = ss_resample_length(p, src->frames_of(s));
        if (lengths[s] > longest) longest = lengths[s];
    }
    if (longest > dc.frames_per_stream) return SS_ERR_CAPACITY;
    const ssk::ResamplePlan plan = batch_resample_plan(src, p);
    const uint64_t tile_out = (uint64_t)plan.tile_periods * p->up, tiles_cap = (longest + tile_out - 1) / tile_out;
    if (tiles_cap * sc.n_streams > 0x7FFFFFFFull) return SS_ERR_UNSUPPORTED;
    Resample &rs = dst->resample;
    if (!rs.ev_src) HIPCHK(hipEventCreateWithFlags(&rs.ev_src, hipEventDisableTiming));
    if (!rs.ev_done) HIPCHK(hipEventCreateWithFlags(&rs.ev_done, hipEventDisableTiming));
    if (!rs.have || std::memcmp(&rs.plan, p, sizeof *p) != 0) {                 // another plan than the table's: its first call copies the table up
        std::vector<float> table((size_t)p->up * p->taps);
        const int rc = ss_resample_taps(p, table.data(), table.size());
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(dst->stream));                              // (an earlier call's kernel may still read the old table)
        rs.have = false;
        HIPCHK(rs.taps.upload(table));
        rs.plan = *p; rs.have = true;
    }
    // ---- the first change of dst: a failure above has left it as it was
    const int rc = ss_batch_set_lengths(dst, lengths.data(), dc.n_streams);
    if (rc) return rc;
    if (!tiles_cap) return SS_OK;                               // (every stream is empty)
    ssk::ResampleParams k{};
    k.src = src->pcm.p; k.dst = dst->pcm.p; k.taps = rs.taps.p;
    k.src_stride = sc.frames_per_stream * sc.channels; k.dst_stride = dc.frames_per_stream * dc.channels;
    k.n_frames = sc.frames_per_stream; k.frames_of = src->ragged_ptr(src->ragged.frames_d);
    k.n_streams = sc.n_streams; k.channels = sc.channels; k.up = p->up; k.down = p->down; k.n_taps = p->taps;
    k.tiles_cap = (uint32_t)tiles_cap; k.plan = plan;
    // dst's stream reads src behind what src's stream holds; src's stream goes on behind the read
    HIPCHK(Overlap::order(rs.ev_src, src->stream, dst->stream));
    HIPCHK(ssk::launch_resample(k, dst->stream));
    HIPCHK(Overlap::order(rs.ev_done, dst->stream, src->stream));
    return SS_OK;
}

int ss_batch_download_pcm(ss_batch *b, uint32_t first, uint32_t count, void *pcm, size_t cap_bytes, int format, const ss_pcm_dither *dither)
{
    SS_ON_DEVICE(b);
    const size_t sb = ss_pcm_sample_bytes(format);
    if (!b || !sb) return SS_ERR_INVALID_ARG;
    if (dither && (dither->kind > (uint32_t)SS_DITHER_TPDF || dither->reserved)) return SS_ERR_INVALID_ARG;
    if ((uint64_t)first + count > b->cfg.n_streams || (!pcm && count)) return SS_ERR_INVALID_ARG;
    const size_t per = b->samples_per_stream(), n = per * count;
    if (cap_bytes < n * sb) return SS_ERR_CAPACITY;
    if (!n) return ss_batch_sync(b);
    // The staging is this call's own, freed behind its wait (ss_batch_upload_pcm's rule); a lane stores four samples as whole words.
    DevBuf<unsigned char> raw;
    HIPCHK(raw.alloc(((n + 3) & ~(size_t)3) * sb));
    ssk::PcmOutParams p{};
    p.pcm = b->pcm.p; p.per_stream = per; p.n_frames = b->cfg.frames_per_stream; p.frames_of = b->ragged_ptr(b->ragged.frames_d);
    p.n_samples = n; p.out = raw.p; p.first = first; p.channels = b->cfg.channels; p.format = format;
    p.tpdf = dither && dither->kind == SS_DITHER_TPDF ? 1u : 0u; p.seed = dither ? dither->seed : 0ull;
    HIPCHK(ssk::launch_f32_to_pcm(p, b->stream));
    return fetch(b, static_cast<unsigned char *>(pcm), static_cast<const unsigned char *>(raw.p), n * sb);
}

int ss_batch_render_waveform(ss_batch *b, uint32_t cols, uint32_t x_min, uint32_t x_max)
{
    SS_ON_DEVICE(b);
    if (!b || cols == 0 || cols > 65536 || x_max <= x_min) return SS_ERR_INVALID_ARG;
    if (!(b->cfg.flags & SS_BATCH_WAVEFORM) || !b->wave_window) return SS_ERR_INVALID_MODE;
    HIPCHK(b->render_wave.ensure((size_t)b->cfg.n_streams * cols * 2));
    b->render_wave_cols = cols;
    HIPCHK(ssk::launch_render_waveform(b->wave.p, (uint64_t)2 * b->wave_window, b->lay.n_wave_points / 2,
                                       b->cfg.n_streams, x_min, x_max, cols, b->render_wave.p, b->stream));
    return SS_OK;
}

int ss_batch_download_waveform_columns(ss_batch *b, uint32_t stream, float *out, size_t cap)
{
    SS_ON_DEVICE(b);
    if (!b || !out || stream >= b->cfg.n_streams || !b->render_wave_cols) return SS_ERR_INVALID_ARG;
    const size_t per = (size_t)2 * b->render_wave_cols;
    if (cap < per) return SS_ERR_CAPACITY;
    return fetch(b, out, b->render_wave.p + (size_t)stream * per, per);
}

// the waveform chart's x bounds in Player mode (tui.rs:664-681), f64 like the reference
void ss_waveform_view(double playhead_ms, double waveform_window_s, size_t chart_points, double *x_min, double *x_max)
{
    const double half_window = waveform_window_s * 500.0;
    const double max_x = (double)chart_points / 2.0;
    double lo = playhead_ms - half_window;
    lo = std::fmin(lo, max_x - waveform_window_s * 1000.0);
    lo = std::fmax(lo, 0.0);
    double hi = playhead_ms + half_window;
    hi = std::fmin(hi, max_x);
    hi = std::fmax(hi, waveform_window_s * 1000.0);
    if (x_min) *x_min = lo;
    if (x_max) *x_max = hi;
}

int ss_batch_timing_enable(ss_batch *b, int enable)
{
    SS_ON_DEVICE(b);
    if (!b) return SS_ERR_INVALID_ARG;
    int rc = b->timing.collect(b->stream);
    if (rc) return rc;
    b->timing.on = enable != 0;
    b->timing.reset();
    return SS_OK;
}

int ss_batch_timing_read(ss_batch *b, int kernel, double *total_ms, uint64_t *launches)
{
    SS_ON_DEVICE(b);
    if (!b || kernel < 0 || kernel >= SS_KERNEL_COUNT) return SS_ERR_INVALID_ARG;
    int rc = b->timing.collect(b->stream);
    if (rc) return rc;
    if (total_ms) *total_ms = b->timing.ms[kernel];
    if (launches) *launches = b->timing.launches[kernel];
    return SS_OK;
}

// the spectrum kernel a batch of this shape launches (names as rocprofv3 prints them, without template arguments)
const char *ss_batch_kernel_name(const ss_batch *b, int kernel)
{
    if (!b || kernel != SS_KERNEL_FFT) return ss_kernel_name(kernel);
    return ssk::spectrum_kernel_name(b->spec.kernel);
}

const char *ss_kernel_name(int kernel)
{
    switch (kernel) {
        case SS_KERNEL_FFT: return "k_fft4096_ms1";
        case SS_KERNEL_TIME_DOMAIN: return "k_time_domain";
        case SS_KERNEL_FINALIZE: return "k_finalize";
        case SS_KERNEL_WAVEFORM: return "k_waveform";
        default: return "?";
    }
}

}  // extern "C"

// ============================================================================
//  the one-shot loudness of a whole buffer
// ============================================================================
namespace {
// the one loudness-only batch the process keeps for calculate_integrated_lufs / receive_audio_file (see integrated_oneshot)
struct OneshotSlot { ss_batch *b = nullptr; uint32_t rate = 0, channels = 0; uint64_t cap = 0; int device = -1; };
std::mutex oneshot_mu;
OneshotSlot oneshot_slot;

// a one-stream, loudness-only batch of `frames` frames
ss_batch_config oneshot_config(uint32_t rate, uint32_t channels, uint64_t frames)
{
    ss_batch_config cfg{};          // (no spectrum: fft_n and hop_frames stay 0)
    cfg.sample_rate = rate; cfg.channels = channels; cfg.n_streams = 1; cfg.flags = SS_BATCH_LUFS; cfg.frames_per_stream = frames;
    return cfg;
}
}  // namespace

int ssh::integrated_oneshot(uint32_t rate, uint32_t channels, const float *samples, size_t n,
                            bool on_device, double *out)
{
    int rc = meter_args_ok(channels, rate);           // EbuR128::new(...) else return None
    if (rc) return rc;
    // every chunk of samples.chunks(2*sr) must hold whole frames, else add_frames fails -> None
    const size_t chunk = (size_t)rate * 2;
    if (n > 0) {
        if (chunk % channels) { if (n >= chunk || n % channels) return SS_ERR_NOMEM; }
        else if (n % channels) return SS_ERR_NOMEM;
    }
    if (n == 0) { *out = -INFINITY; return SS_OK; }    // no blocks: loudness_global() = -inf
    if (!samples) return SS_ERR_INVALID_ARG;
    // A one-stream, loudness-only batch pass.  Building and tearing down a batch is fourteen device allocations and as many
    // hipFree calls (20-50 us each: most of what opening a file cost), so ONE batch is kept per process for inputs of up to
    // 64 MB — created with a quarter of headroom and re-used through the ragged-length path (ss_batch_set_lengths) for every
    // later call of the same (device, rate, channel count) that fits; the pass runs under a lock.  Longer inputs take a
    // batch of their own as before.
    const uint64_t frames = n / channels;
    constexpr size_t kCacheMaxFloats = (size_t)16 << 20;
    OneshotSlot &slot = oneshot_slot;
    std::unique_lock<std::mutex> lk(oneshot_mu, std::defer_lock);
    ss_batch *b = nullptr;
    const bool cached = n <= kCacheMaxFloats;
    if (cached) {
        lk.lock();
        const int dev = current_device();
        if (!(slot.b && slot.device == dev && slot.rate == rate && slot.channels == channels && slot.cap >= frames)) {
            if (slot.b) { ss_batch_destroy(slot.b); slot = OneshotSlot{}; }
            const ss_batch_config cfg = oneshot_config(rate, channels, frames + frames / 4 + rate);
            rc = ss_batch_create(&cfg, &slot.b);
            if (rc) { slot = OneshotSlot{}; return rc; }
            slot.rate = rate; slot.channels = channels; slot.cap = cfg.frames_per_stream; slot.device = dev;
        }
        b = slot.b;
        rc = ss_batch_set_lengths(b, &frames, 1);
        if (rc) return rc;
    } else {
        const ss_batch_config cfg = oneshot_config(rate, channels, frames);
        rc = ss_batch_create(&cfg, &b);
        if (rc) return rc;
    }
    if (!hip_ok(hipMemcpyAsync(b->pcm.p, samples, n * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b->stream),
                "hipMemcpyAsync(one-shot input)")) rc = SS_ERR_DEVICE;
    if (!rc) rc = ss_batch_run(b);
    if (!rc) rc = ss_batch_sync(b);
    ss_stream_result r{};
    if (!rc) rc = ss_batch_results(b, &r, 1);
    if (!cached) ss_batch_destroy(b);
    if (rc) return rc;
    *out = r.integrated_lufs;
    return SS_OK;
}

extern "C" {

int ss_release_caches(void)
{
    std::lock_guard<std::mutex> lk(oneshot_mu);
    if (oneshot_slot.b) { ss_batch_destroy(oneshot_slot.b); oneshot_slot = OneshotSlot{}; }
    return SS_OK;
}

// Analyzer::calculate_integrated_lufs (analyzer.rs:170-182): fresh meter at the
// handle's sample rate, whole buffer fed in 2*sr-sample chunks, loudness_global.
int ss_calculate_integrated_lufs(ss_analyzer *h, uint32_t channels, const float *samples, size_t n, double *out)
{
    SS_ON_DEVICE(h);
    if (!h || !out) return SS_ERR_INVALID_ARG;
    return integrated_oneshot(h->rate, channels, samples, n, false, out);
}

}  // extern "C"
