// ss_meter_bank.cpp — meter banks (include/soundscope_hip.h, "Meter banks"): N live meters of one shape advanced together.  Host
// logic only: argument checks in the handle's order, the per-stream meters (one MeterStore, as a handle holds one of one stream), the
// staging of the input and the launches — k_time_domain's streaming forms over all streams, k_meter_bank_gate,
// k_meter_bank_readings, k_meter_bank_reset (ss_loudness.hip).  No CPU compute path.
#include "ss_host.h"

using namespace ssh;

struct ss_meter_bank {
    int device = 0;
    hipStream_t stream = nullptr;
    ssh::MeterStore meter;                 // n streams
    ssh::DevBuf<uint32_t> list;            // ss_meter_bank_reset's stream indices
    ssh::DevBuf<float> in;                 // the f32 input of a host call
    ssh::DevBuf<unsigned char> raw;        // ss_meter_bank_add_pcm's bytes
    ssh::DevBuf<ssk::MeterReading> readings;
    std::vector<uint64_t> fed;             // frames since each stream's reset (the device's TdState::frames_fed, mirrored)
    // page-locked staging: a host call's input is copied there and returns behind its launches; the readings come back through
    // page-locked memory as well
    ssh::HostStage stage;
    ssh::PinBuf<ssk::MeterReading> pin_read;
    ssh::DevBuf<unsigned char> rag;        // a ragged add's staging: the per-stream arrays, then (host forms) the packed input
    // spectra (ss_meter_bank_spectrum_enable): the newest 16384 input frames of every stream.  Stream s's frame counter is
    // spec_fed + spec_ahead[s]: what the uniform adds gave everyone, kept here, plus what ragged adds gave that stream, kept on the
    // device (allocated by the first ragged add) — a spectrum call uploads nothing and a uniform add stays as it was
    bool spec_on = false;
    uint64_t spec_fed = 0;
    ssh::DevBuf<uint64_t> spec_ahead;      // [n]
    BinTables *bt = nullptr;
    FftTables *ft = nullptr;
    ssh::DevBuf<float> spec_hist;          // [n][16384][C]
    ssh::DevBuf<float> spec_out;           // rows or columns of the last spectrum call
    ssh::DevBuf<int32_t> spec_status;      // [n][rows]
    ssh::DevBuf<double> spec_pink;         // n_bins f64
    ssh::DevBuf<uint16_t> spec_bin_col;    // n_bins: chart column of each bin for spec_cols
    ssh::DevBuf<float> spec_col_init;      // spec_cols
    uint32_t spec_cols = 0;
    ssh::PinBuf<unsigned char> spec_pin;   // page-locked results: floats, then the statuses
    // tracked spectra (ss_meter_bank_spectrum_track_enable): per row an averaged and a peak-hold curve, advanced behind the
    // transform's row launch.  A row's clock is kept twice; an update reads trk_meta[trk_cur] and writes the other (ssk::BankTrackParams)
    bool trk_on = false;
    ss_spectrum_ballistics trk_cfg{};
    ssh::DevBuf<unsigned char> trk_state;  // [n][rows]: 16 bytes per bin at a stride of n_bins rounded up to four
    ssh::DevBuf<ssk::BankTrackRow> trk_meta;   // [2][n][rows]
    uint32_t trk_cur = 0;
    ssh::DevBuf<float> trk_rows;           // [n][rows][n_bins]: the row launch of an update
    ssh::DevBuf<int32_t> trk_status;       // [n][rows]
    ssh::DevBuf<unsigned char> trk_out;    // a read-out: the curves asked for, then the update counts
    // signal watch (ss_meter_bank_signal_watch_enable): the batch signal scan's records of what every stream was given, advanced by
    // one launch per add (ssk::BankWatchParams).  The records stand behind each other so that a read is one copy
    bool watch_on = false;
    ss_signal_scan_config watch_cfg{};
    ssh::DevBuf<ssk::BankWatchSeq> watch_state;    // [n][channels + 1]
    ssh::DevBuf<unsigned char> watch_rec;  // [n] ssk::StreamWatch, then [n][channels] ssk::ChannelWatch
    ssh::PinBuf<unsigned char> watch_pin;
    // pair watch (ss_meter_bank_pair_watch_enable): the batch pair series' entries of what every stream was given, advanced by one
    // launch per add (ssk::BankPairWatchParams).  pair_fed mirrors the frames each stream has had since its pair-watch reset — the
    // device's entries and open_frames follow from it — so that the ring's read knows which slots hold entries without a copy
    bool pair_on = false;
    ss_pair_watch_config pair_cfg{};
    uint32_t pair_n = 0;                   // pairs
    ssk::ChannelPair pair_list[ssk::kMaxPairs] = {};
    ssh::DevBuf<double> pair_lanes;        // [n][pairs][3][256]
    ssh::DevBuf<uint32_t> pair_open_skipped;   // [n][pairs]
    ssh::DevBuf<ssk::PairEntry> pair_ring; // [n][window_entries][pairs]
    ssh::DevBuf<ssk::PairWatch> pair_rec;  // [n][pairs]
    ssh::PinBuf<unsigned char> pair_pin;   // the records, or one stream's ring
    std::vector<uint64_t> pair_fed;        // [n]
};

namespace {

// the stream has been waited for: the staging buffer is free
hipError_t bank_sync(ss_meter_bank *m)
{
    hipError_t e = hipStreamSynchronize(m->stream);
    if (e == hipSuccess) m->stage.idle();
    return e;
}

// stage host bytes on the device through the page-locked copy
int upload(ss_meter_bank *m, void *dst, const void *src, size_t bytes)
{
    HIPCHK(m->stage.send(dst, src, bytes, m->stream));
    return SS_OK;
}

// the f32 input of a call whose `samples` samples stand on the device at `bytes`: raw PCM is converted into m->in (the caller has
// sized it), f32 (format 0) is used where it landed
int device_input(ss_meter_bank *m, const unsigned char *bytes, uint64_t samples, int format, const float **in)
{
    *in = reinterpret_cast<const float *>(bytes);
    if (!format) return SS_OK;
    HIPCHK(ssk::launch_pcm_to_f32(bytes, samples, format, m->in.p, m->stream));
    *in = m->in.p;
    return SS_OK;
}

// ---- the plan of an add ------------------------------------------------------------------------------------------------------------
// A call is cut into pieces of at most 32 sub-blocks, so that the 96-slot sub-block ring always holds the thirty sub-blocks a
// short-term block reads (ss_add_samples' rule).  A uniform call has no arrays: nothing but its input is uploaded.  A ragged call
// stages, in ONE page-locked copy, arrays of n u64 each, then (host forms) the streams' input, tightly packed.
//   [0] frames of the whole call (the history ring), [1] where each stream's input starts (floats; samples for raw PCM),
//   then per piece: what each stream takes in it (the gating launch), and — only where the piece has streams on both sides of the
//   form switch — that array once more with the long streams zeroed and once with the short ones zeroed.
struct BankPlan {
    // take, lo, hi: array indices (lo == hi == take: one group); all: what every stream takes (uniform; ragged: 0, see `take`)
    struct Piece { size_t take, lo, hi; uint64_t max_short, max_long, all; bool gate; };
    std::vector<uint64_t> arrays;          // n entries each; empty: a uniform call
    std::vector<Piece> pieces;
    uint64_t longest = 0;                  // frames of the longest stream (uniform: of every stream; 0: nothing to do)
    uint64_t total = 0;                    // samples of packed input, every stream's start a multiple of four
};

// frames: every stream's count, with the checks every ragged form shares (null: a uniform call of `each` frames)
int bank_plan(const ss_meter_bank *m, const uint64_t *frames, uint64_t each, bool pack, BankPlan *pl)
{
    const MeterStore &ms = m->meter;
    const uint32_t n = ms.n, C = ms.channels;
    uint64_t total = 0, longest = each;
    for (uint32_t s = 0; frames && s < n; s++) {                         // ss_batch_create's rule: more than 2^40 samples is no buffer
        if (frames[s] > (1ull << 40) || frames[s] * C > (1ull << 40) || (total += (frames[s] * C + 3u) & ~3ull) > (1ull << 40)) return SS_ERR_NOMEM;
        if (frames[s] > longest) longest = frames[s];
    }
    pl->longest = longest;
    if (!longest) return SS_OK;
    const uint64_t S = ms.s100, piece_frames = MeterStore::piece_frames_for(S);
    auto shared = [&](uint64_t take) { return ssk::td_ring_call_shared(C, (uint32_t)S, take); };      // the launch's own form switch
    const size_t n_pieces = (size_t)((longest + piece_frames - 1) / piece_frames);
    if (frames) {
        pl->arrays.assign((2 + n_pieces) * (size_t)n, 0);
        pl->total = pack ? total : 0;
        uint64_t at = 0;
        for (uint32_t s = 0; s < n; s++) {
            pl->arrays[s] = frames[s];
            pl->arrays[n + s] = at;
            if (pack) at += (frames[s] * C + 3u) & ~3ull;
        }
    }
    for (size_t k = 0; k < n_pieces; k++) {
        BankPlan::Piece pc{(2 + k) * (size_t)n, 0, 0, 0, 0, 0, false};
        for (uint32_t s = 0; s < n; s++) {
            const uint64_t f = frames ? frames[s] : each;
            const uint64_t done = k * piece_frames < f ? k * piece_frames : f, left = f - done;
            const uint64_t take = left < piece_frames ? left : piece_frames;
            if (frames) pl->arrays[pc.take + s] = take; else pc.all = take;
            if (shared(take)) { if (take > pc.max_long) pc.max_long = take; }
            else if (take > pc.max_short) pc.max_short = take;
            const uint64_t fed = m->fed[s] + done;
            pc.gate = pc.gate || (fed + take) / S > fed / S;
        }
        pc.lo = pc.hi = pc.take;
        if (pc.max_short && pc.max_long) {                               // both forms in one piece: two launches, each with its own lengths
            pc.lo = pl->arrays.size(); pc.hi = pc.lo + n;
            pl->arrays.resize(pl->arrays.size() + 2 * (size_t)n, 0);
            for (uint32_t s = 0; s < n; s++) {
                const uint64_t take = pl->arrays[pc.take + s];
                pl->arrays[(shared(take) ? pc.hi : pc.lo) + s] = take;
            }
        }
        pl->pieces.push_back(pc);
    }
    return SS_OK;
}

// ---- signal watch ------------------------------------------------------------------------------------------------------------------
// both records begin with the batch scan's
static_assert(offsetof(ss_stream_watch, silent_frames) == offsetof(ss_stream_scan, silent_frames) &&
              offsetof(ss_stream_watch, longest_silence_at) == offsetof(ss_stream_scan, longest_silence_at) &&
              offsetof(ss_stream_watch, clip_runs) == offsetof(ss_stream_scan, clip_runs) && offsetof(ss_stream_watch, frames) == sizeof(ss_stream_scan),
              "ss_stream_watch begins with ss_stream_scan");
static_assert(offsetof(ss_channel_watch, sum) == offsetof(ss_channel_scan, sum) && offsetof(ss_channel_watch, first_nonfinite) == offsetof(ss_channel_scan, first_nonfinite) &&
              offsetof(ss_channel_watch, longest_clip_at) == offsetof(ss_channel_scan, longest_clip_at) &&
              offsetof(ss_channel_watch, clip_runs) == offsetof(ss_channel_scan, clip_runs) && offsetof(ss_channel_watch, trailing_clip) == sizeof(ss_channel_scan),
              "ss_channel_watch begins with ss_channel_scan");

ssk::StreamWatch *watch_streams(const ss_meter_bank *m) { return reinterpret_cast<ssk::StreamWatch *>(m->watch_rec.p); }
ssk::ChannelWatch *watch_channels(const ss_meter_bank *m) { return reinterpret_cast<ssk::ChannelWatch *>(watch_streams(m) + m->meter.n); }
size_t watch_rec_bytes(const ss_meter_bank *m)
{
    return (size_t)m->meter.n * (sizeof(ssk::StreamWatch) + (size_t)m->meter.channels * sizeof(ssk::ChannelWatch));
}

// the watch's launch behind the staging of an add: every stream by its own frames of the WHOLE call (frames_of null: `frames` each)
int watch_advance(ss_meter_bank *m, const float *pcm, const uint64_t *offset_of, uint64_t stride, const uint64_t *frames_of, uint64_t frames)
{
    ssk::BankWatchParams p{};
    p.pcm = pcm; p.stride = stride; p.offset_of = offset_of; p.frames_of = frames_of; p.frames = frames;
    p.n_streams = m->meter.n; p.channels = m->meter.channels;
    p.tile_frames = ssk::plan_signal_scan(m->meter.channels, 0).tile_frames;
    p.silence_threshold = m->watch_cfg.silence_threshold; p.clip_level = m->watch_cfg.clip_level;
    p.silence_min = m->watch_cfg.silence_min_frames; p.clip_min = m->watch_cfg.clip_min_samples;
    p.state = m->watch_state.p; p.streams = watch_streams(m); p.channel_watches = watch_channels(m);
    HIPCHK(ssk::launch_bank_signal_watch(p, m->stream));
    return SS_OK;
}

// ---- pair watch --------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(ss_pair_watch_config) == 24, "pair watch config layout");

// the pair watch's launch behind the staging of an add, with watch_advance's arguments
int pair_watch_advance(ss_meter_bank *m, const float *pcm, const uint64_t *offset_of, uint64_t stride, const uint64_t *frames_of, uint64_t frames)
{
    ssk::BankPairWatchParams p{};
    p.pcm = pcm; p.stride = stride; p.offset_of = offset_of; p.frames_of = frames_of; p.frames = frames;
    p.n_streams = m->meter.n; p.channels = m->meter.channels; p.s100 = (uint32_t)m->meter.s100;
    p.window_entries = m->pair_cfg.window_entries; p.n_pairs = m->pair_n;
    p.threshold = m->pair_cfg.threshold; p.power_floor = m->pair_cfg.power_floor; p.min_run = m->pair_cfg.min_run;
    p.lanes = m->pair_lanes.p; p.open_skipped = m->pair_open_skipped.p; p.ring = m->pair_ring.p; p.records = m->pair_rec.p;
    for (uint32_t k = 0; k < m->pair_n; k++) p.pairs[k] = m->pair_list[k];
    HIPCHK(ssk::launch_bank_pair_watch(p, m->stream));
    return SS_OK;
}

// the pair watch off: nothing on the stream still uses its state afterwards
int pair_watch_drop(ss_meter_bank *m)
{
    if (!m->pair_on) return SS_OK;
    HIPCHK(bank_sync(m));
    m->pair_on = false;
    m->pair_lanes.release(); m->pair_open_skipped.release(); m->pair_ring.release(); m->pair_rec.release(); m->pair_pin.release();
    m->pair_fed.clear();
    return SS_OK;
}

// the launches of an add behind its staging.  Stream s's input stands at pcm + offset_of[s] (offset_of null: pcm + s * stride); `arr`:
// a ragged plan's arrays on the device (null: a uniform call)
int advance(ss_meter_bank *m, const BankPlan &pl, const uint64_t *arr, const float *pcm, const uint64_t *offset_of, uint64_t stride)
{
    const MeterStore &ms = m->meter;
    const uint32_t n = ms.n, C = ms.channels;
    if (m->spec_on && !arr) {
        HIPCHK(ssk::launch_bank_history_append(m->spec_hist.p, pcm, stride, pl.longest, m->spec_fed, m->spec_ahead.p, n, C, m->stream));
        m->spec_fed += pl.longest;
    } else if (m->spec_on) {
        if (!m->spec_ahead.p) {
            HIPCHK(m->spec_ahead.alloc(n));
            HIPCHK(hipMemsetAsync(m->spec_ahead.p, 0, n * sizeof(uint64_t), m->stream));
        }
        HIPCHK(ssk::launch_bank_history_append_ragged(m->spec_hist.p, pcm, stride, offset_of, arr, m->spec_fed, m->spec_ahead.p, n, C, m->stream));
    }
    if (m->watch_on) {                                                   // one launch for the whole call, not one per piece
        int rc = watch_advance(m, pcm, offset_of, stride, arr, pl.longest);
        if (rc) return rc;
    }
    if (m->pair_on) {
        int rc = pair_watch_advance(m, pcm, offset_of, stride, arr, pl.longest);
        if (rc) return rc;
        for (uint32_t s = 0; s < n; s++) m->pair_fed[s] += arr ? pl.arrays[s] : pl.longest;
    }
    const uint64_t piece_frames = MeterStore::piece_frames_for(ms.s100);
    const ssk::MeterBankParams q = ms.bank_params();
    for (size_t k = 0; k < pl.pieces.size(); k++) {
        const BankPlan::Piece &pc = pl.pieces[k];
        // a stream runs the form a handle runs for a call of its length: one wave up to a tile, the eight-wave workgroup beyond (a
        // ragged piece with streams of both kinds: one launch each; a uniform piece: one launch, its form chosen by its length)
        for (int g = 0; g < 2; g++) {
            const uint64_t longest = g ? pc.max_long : pc.max_short;
            if (!longest) continue;
            ssk::TdParams p = ms.td_params(pcm + k * piece_frames * C, stride, longest);
            p.frames_of = arr ? arr + (g ? pc.hi : pc.lo) : nullptr;
            p.offset_of = offset_of;
            p.tp_f32 = 1u;                                               // SS_TP_ARITH_F32, the handle's default
            HIPCHK(ssk::launch_time_domain(p, m->stream));
        }
        // the gating launch only when some stream completes a sub-block (each stream's range is derived on the device)
        if (pc.gate) HIPCHK(ssk::launch_meter_bank_gate(q, pc.all, arr ? arr + pc.take : nullptr, m->stream));
    }
    for (uint32_t s = 0; s < n; s++) m->fed[s] += arr ? pl.arrays[s] : pl.longest;
    return SS_OK;
}

// every stream advanced by `frames` frames of device-resident f32 input (stream s at pcm + s * stride)
int advance_uniform(ss_meter_bank *m, const float *pcm, uint64_t frames, uint64_t stride)
{
    BankPlan pl;
    int rc = bank_plan(m, nullptr, frames, false, &pl);
    return rc ? rc : advance(m, pl, nullptr, pcm, nullptr, stride);
}

// host forms: arrays and packed input (sb bytes per sample; format 0: f32, used where it lands) through one page-locked copy
int add_ragged_host(ss_meter_bank *m, const void *const *pcm, const uint64_t *frames, int format, size_t sb)
{
    if (!frames) return SS_ERR_INVALID_ARG;
    const uint32_t n = m->meter.n, C = m->meter.channels;
    for (uint32_t s = 0; s < n; s++) if (frames[s] && (!pcm || !pcm[s])) return SS_ERR_INVALID_ARG;
    BankPlan pl;
    int rc = bank_plan(m, frames, 0, true, &pl);
    if (rc || !pl.longest) return rc;
    const size_t head = (pl.arrays.size() * sizeof(uint64_t) + 15u) & ~(size_t)15u, body = (size_t)pl.total * sb;
    HIPCHK(m->rag.ensure(head + body + kPcmReadSlack));
    if (format) HIPCHK(m->in.ensure(pl.total));
    HIPCHK(m->stage.take(head + body));
    char *pin = reinterpret_cast<char *>(m->stage.buf.p);
    std::memcpy(pin, pl.arrays.data(), pl.arrays.size() * sizeof(uint64_t));
    for (uint32_t s = 0; s < n; s++) {
        const size_t bytes = (size_t)frames[s] * C * sb, padded = (size_t)((frames[s] * C + 3u) & ~3ull) * sb;
        char *dst = pin + head + (size_t)pl.arrays[n + s] * sb;
        if (bytes) std::memcpy(dst, pcm[s], bytes);
        std::memset(dst + bytes, 0, padded - bytes);
    }
    HIPCHK(m->stage.queue(m->rag.p, head + body, m->stream));
    const uint64_t *arr = reinterpret_cast<const uint64_t *>(m->rag.p);
    const float *in = nullptr;
    rc = device_input(m, m->rag.p + head, pl.total, format, &in);
    if (rc) return rc;
    return advance(m, pl, arr, in, arr + n, 0);
}

// the stream list of a reset: every index checked, then the list on the device at *dev (streams null — every stream: nothing to
// check or send, *dev null)
int stream_list(ss_meter_bank *m, const uint32_t *streams, uint32_t count, const uint32_t **dev)
{
    *dev = nullptr;
    if (!streams) return SS_OK;
    for (uint32_t i = 0; i < count; i++) if (streams[i] >= m->meter.n) return SS_ERR_INVALID_ARG;
    HIPCHK(m->list.ensure(count));
    *dev = m->list.p;
    return upload(m, m->list.p, streams, count * sizeof(uint32_t));
}

// streams null: every stream
int bank_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    const uint32_t *dev;
    int rc = stream_list(m, streams, count, &dev);
    if (rc) return rc;
    if (!streams) count = m->meter.n;
    HIPCHK(ssk::launch_meter_bank_reset(m->meter.bank_params(), dev, count, m->stream));
    for (uint32_t i = 0; i < count; i++) m->fed[streams ? streams[i] : i] = 0;
    return SS_OK;
}

int null_bank() { return require_device() ? SS_ERR_DEVICE : SS_ERR_INVALID_ARG; }

uint32_t spec_rows(const ss_meter_bank *m) { return m->meter.channels == 2 ? 2u : m->meter.channels; }

// the transform's launch parameters for the windows as they stand (rows; the caller adds what columns need)
ssk::BankSpectrumParams spectrum_params(const ss_meter_bank *m, float *out, int32_t *status)
{
    ssk::BankSpectrumParams q{};
    q.f = one_window_fft(ssk::plan_spectrum(SS_BANK_SPECTRUM_N, m->meter.channels, kOneWindowHop, 1, 1), *m->ft, *m->bt);
    q.hist = m->spec_hist.p;
    q.start = (uint32_t)((m->spec_fed - SS_BANK_SPECTRUM_N) & (SS_BANK_SPECTRUM_N - 1));
    q.ahead = m->spec_ahead.p;
    q.n_streams = m->meter.n; q.channels = m->meter.channels; q.rows = spec_rows(m);
    q.status = status; q.out = out;
    return q;
}

// the chart-column tables of `cols` columns on the device (kept until another count is asked for)
int column_tables(ss_meter_bank *m, uint32_t cols)
{
    if (cols == m->spec_cols) return SS_OK;
    const ColumnTables t = ssh::column_tables(*m->bt, cols, m->bt->count);
    HIPCHK(m->spec_bin_col.upload(t.bin_col));
    HIPCHK(m->spec_col_init.upload(t.col_init));
    m->spec_cols = cols;
    return SS_OK;
}

// The column fold of a launch: the tables of `cols` columns, the pink compensation and the gain — SS_GAIN_REFERENCE: every stream's
// integrated loudness after the last add, the readings read() returns, left on the device by a launch of their own.
int column_fold(ss_meter_bank *m, uint32_t cols, int gain_mode, float gain_db, ssk::ChartFold *q)
{
    int rc = column_tables(m, cols);
    if (rc) return rc;
    q->pink = m->spec_pink.p; q->bin_col = m->spec_bin_col.p; q->col_init = m->spec_col_init.p;
    q->cols = cols; q->gain_db = gain_db;
    if (gain_mode != SS_GAIN_REFERENCE) return SS_OK;
    HIPCHK(ssk::launch_meter_bank_readings(m->meter.bank_params(), m->readings.p, m->stream));
    static_assert(sizeof(ssk::MeterReading) % sizeof(double) == 0, "readings as doubles");
    q->integrated = &m->readings.p[0].integrated;
    q->integrated_stride = sizeof(ssk::MeterReading) / sizeof(double);
    return SS_OK;
}

// the spectrum launch of every (stream, row), one copy of its results (`per_row` floats each) and statuses into page-locked memory,
// and from there to the caller
int spectrum_run(ss_meter_bank *m, bool columns, uint32_t cols, int gain_mode, float gain_db, uint32_t per_row, float *vals, int32_t *status)
{
    const uint32_t R = spec_rows(m);
    const size_t rows = (size_t)m->meter.n * R, fbytes = rows * per_row * sizeof(float), sbytes = rows * sizeof(int32_t);
    HIPCHK(m->spec_out.ensure(rows * per_row));
    if (fbytes + sbytes > m->spec_pin.n) {
        HIPCHK(bank_sync(m));
        HIPCHK(m->spec_pin.ensure(fbytes + sbytes));
    }
    ssk::BankSpectrumParams q = spectrum_params(m, m->spec_out.p, m->spec_status.p);
    int rc = columns ? column_fold(m, cols, gain_mode, gain_db, &q.fold) : SS_OK;
    if (rc) return rc;
    HIPCHK(ssk::launch_meter_bank_spectrum(q, columns, m->stream));
    unsigned char *pin = m->spec_pin.p;
    HIPCHK(hipMemcpyAsync(pin, m->spec_out.p, fbytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(pin + fbytes, m->spec_status.p, sbytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    std::memcpy(vals, pin, fbytes);
    std::memcpy(status, pin + fbytes, sbytes);
    return SS_OK;
}

// ---- tracked spectra ---------------------------------------------------------------------------------------------------------------
static_assert(sizeof(ss_spectrum_ballistics) == 24, "ss_spectrum_ballistics layout");

size_t track_rows_of(const ss_meter_bank *m) { return (size_t)m->meter.n * spec_rows(m); }

// the tracked state is dropped: nothing on the stream still uses it afterwards
int track_drop(ss_meter_bank *m)
{
    if (!m->trk_on) return SS_OK;
    HIPCHK(bank_sync(m));
    m->trk_on = false;
    m->trk_state.release(); m->trk_meta.release(); m->trk_rows.release(); m->trk_status.release(); m->trk_out.release();
    return SS_OK;
}

ssk::BankTrackParams track_params(const ss_meter_bank *m)
{
    const size_t rows = track_rows_of(m);
    const double rate = (double)m->meter.rate, frames = m->trk_cfg.hold_s * rate + 0.5;
    ssk::BankTrackParams p{};
    p.rows = m->trk_rows.p; p.status = m->trk_status.p;
    p.fed = m->spec_fed; p.ahead = m->spec_ahead.p;
    p.n_streams = m->meter.n; p.rows_per_stream = spec_rows(m);
    p.n_bins = (uint32_t)m->bt->count; p.bin_stride = (p.n_bins + 3u) & ~3u;
    p.state = m->trk_state.p;
    p.meta_in = m->trk_meta.p + m->trk_cur * rows;
    p.meta_out = m->trk_meta.p + (m->trk_cur ^ 1u) * rows;
    p.rate = rate; p.average_tau_s = m->trk_cfg.average_tau_s; p.decay_db_per_s = m->trk_cfg.decay_db_per_s;
    p.hold_frames = frames < 18446744073709551615.0 ? (uint64_t)frames : ~0ull;      // (+inf, or beyond u64: never falls)
    return p;
}

// Where a read-out's results stand in trk_out, in floats: the averaged curve at 0 and the peak-hold curve at `hold_at`, `plane` floats
// each, then the update counts of the `rows` rows at `counts_at`.
struct TrackOut {
    size_t plane, hold_at, counts_at, rows;
    size_t bytes() const { return counts_at * sizeof(float) + rows * sizeof(uint32_t); }
};

// a read-out's results behind its launch: trk_out into page-locked memory in one copy, waited for, and from there what the caller
// asked for (a null pointer: not that one)
int track_fetch(ss_meter_bank *m, const TrackOut &o, float *avg, float *hold, uint32_t *updates)
{
    HIPCHK(hipMemcpyAsync(m->spec_pin.p, m->trk_out.p, o.bytes(), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    const float *h = reinterpret_cast<const float *>(m->spec_pin.p);
    if (avg) std::memcpy(avg, h, o.plane * sizeof(float));
    if (hold) std::memcpy(hold, h + o.hold_at, o.plane * sizeof(float));
    if (updates) std::memcpy(updates, h + o.counts_at, o.rows * sizeof(uint32_t));
    return SS_OK;
}

// room for a read-out of `bytes` on the device and in page-locked memory
int track_room(ss_meter_bank *m, size_t bytes)
{
    if (bytes > m->trk_out.n || bytes > m->spec_pin.n) HIPCHK(bank_sync(m));
    HIPCHK(m->trk_out.ensure(bytes));
    HIPCHK(m->spec_pin.ensure(bytes));
    return SS_OK;
}

}  // namespace

extern "C" {

int ss_meter_bank_create(uint32_t n_streams, uint32_t channels, uint32_t rate, int32_t true_peak_factor, ss_meter_bank **out)
{
    if (!out) return SS_ERR_INVALID_ARG;
    *out = nullptr;
    if (require_device()) return SS_ERR_DEVICE;
    int rc = meter_args_ok(channels, rate);
    if (rc) return rc;
    if (n_streams == 0 || (true_peak_factor != 0 && true_peak_factor != 2 && true_peak_factor != 4)) return SS_ERR_INVALID_ARG;
    std::unique_ptr<ss_meter_bank, decltype(&ss_meter_bank_destroy)> m(new ss_meter_bank(), &ss_meter_bank_destroy);
    m->device = current_device();
    rc = m->meter.build(n_streams, channels, rate, true_peak_factor);
    if (rc) return rc;
    HIPCHK(stream_acquire(&m->stream));
    const size_t N = n_streams;
    HIPCHK(m->readings.alloc(N));
    HIPCHK(m->pin_read.alloc(N));
    m->fed.assign(N, 0);
    rc = bank_reset(m.get(), nullptr, n_streams);
    if (rc) return rc;
    HIPCHK(bank_sync(m.get()));
    *out = m.release();
    return SS_OK;
}

void ss_meter_bank_destroy(ss_meter_bank *m)
{
    SS_ON_DEVICE(m);
    if (!m) return;
    if (m->stream) { (void)hipStreamSynchronize(m->stream); stream_release(m->stream); }
    delete m;
}

int ss_meter_bank_add(ss_meter_bank *m, const float *pcm, uint64_t frames)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (frames == 0) return SS_OK;
    if (!pcm) return SS_ERR_INVALID_ARG;
    const uint64_t per = frames * m->meter.channels, total = per * m->meter.n;
    HIPCHK(m->in.ensure(total));
    int rc = upload(m, m->in.p, pcm, total * sizeof(float));
    if (rc) return rc;
    return advance_uniform(m, m->in.p, frames, per);
}

int ss_meter_bank_add_device(ss_meter_bank *m, const float *pcm_device, uint64_t frames, uint64_t stream_stride_floats)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (frames == 0) return SS_OK;
    if (!pcm_device || stream_stride_floats < frames * m->meter.channels) return SS_ERR_INVALID_ARG;
    return advance_uniform(m, pcm_device, frames, stream_stride_floats);
}

int ss_meter_bank_add_pcm(ss_meter_bank *m, const void *pcm, uint64_t frames, int format)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    const size_t sb = ss_pcm_sample_bytes(format);
    if (!sb) return SS_ERR_INVALID_ARG;
    if (frames == 0) return SS_OK;
    if (!pcm) return SS_ERR_INVALID_ARG;
    const uint64_t per = frames * m->meter.channels, total = per * m->meter.n;
    HIPCHK(m->raw.ensure(total * sb + kPcmReadSlack));
    HIPCHK(m->in.ensure(total));
    int rc = upload(m, m->raw.p, pcm, total * sb);
    if (rc) return rc;
    const float *in = nullptr;
    rc = device_input(m, m->raw.p, total, format, &in);
    return rc ? rc : advance_uniform(m, in, frames, per);
}

int ss_meter_bank_add_ragged(ss_meter_bank *m, const float *const *pcm, const uint64_t *frames)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    return add_ragged_host(m, reinterpret_cast<const void *const *>(pcm), frames, 0, sizeof(float));
}

int ss_meter_bank_add_ragged_pcm(ss_meter_bank *m, const void *const *pcm, const uint64_t *frames, int format)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    const size_t sb = ss_pcm_sample_bytes(format);
    if (!sb) return SS_ERR_INVALID_ARG;
    return add_ragged_host(m, pcm, frames, format, sb);
}

int ss_meter_bank_add_ragged_device(ss_meter_bank *m, const float *pcm_device, const uint64_t *frames, uint64_t stream_stride_floats)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!frames) return SS_ERR_INVALID_ARG;
    BankPlan pl;
    int rc = bank_plan(m, frames, 0, false, &pl);
    if (rc || !pl.longest) return rc;
    if (!pcm_device || stream_stride_floats < pl.longest * m->meter.channels) return SS_ERR_INVALID_ARG;
    const size_t bytes = pl.arrays.size() * sizeof(uint64_t);
    HIPCHK(m->rag.ensure(bytes));
    rc = upload(m, m->rag.p, pl.arrays.data(), bytes);
    if (rc) return rc;
    return advance(m, pl, reinterpret_cast<const uint64_t *>(m->rag.p), pcm_device, nullptr, stream_stride_floats);
}

int ss_meter_bank_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    return bank_reset(m, streams, count);
}

int ss_meter_bank_read(ss_meter_bank *m, ss_meter_reading *out, uint32_t cap_streams)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!out) return SS_ERR_INVALID_ARG;
    if (cap_streams < m->meter.n) return SS_ERR_CAPACITY;
    HIPCHK(ssk::launch_meter_bank_readings(m->meter.bank_params(), m->readings.p, m->stream));
    HIPCHK(hipMemcpyAsync(m->pin_read.p, m->readings.p, m->meter.n * sizeof(ssk::MeterReading), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    std::memcpy(out, m->pin_read.p, m->meter.n * sizeof(ss_meter_reading));
    return SS_OK;
}

int ss_meter_bank_peaks(ss_meter_bank *m, uint32_t stream, double *true_pk, double *sample_pk, uint32_t cap_channels)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (stream >= m->meter.n) return SS_ERR_INVALID_ARG;
    if ((true_pk || sample_pk) && cap_channels < m->meter.channels) return SS_ERR_CAPACITY;
    float pk[2 * ssk::kMaxChannels];
    HIPCHK(hipMemcpyAsync(pk, &m->meter.state.p[stream].sample_peak[0], sizeof pk, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    for (uint32_t c = 0; c < m->meter.channels; c++)
        peaks_of(pk, c, sample_pk ? sample_pk + c : nullptr, true_pk ? true_pk + c : nullptr);
    return SS_OK;
}

int ss_meter_bank_histograms(ss_meter_bank *m, uint32_t stream, uint64_t *out2000)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (stream >= m->meter.n || !out2000) return SS_ERR_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(out2000, m->meter.hist.p + (size_t)stream * 2 * sst::kHistBins, 2 * sst::kHistBins * sizeof(uint64_t),
                          hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    return SS_OK;
}

int ss_meter_bank_spectrum_enable(ss_meter_bank *m, int enable)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    int rc = track_drop(m);                                                        // the tracked curves belong to the history they followed
    if (rc) return rc;
    if (!enable) {
        HIPCHK(bank_sync(m));
        m->spec_on = false;
        m->spec_hist.release(); m->spec_out.release(); m->spec_status.release();
        return SS_OK;
    }
    if (20000.0f > (float)m->meter.rate / 2.0f) return SS_ERR_FREQ_LIMIT;         // get_fft's FrequencyLimit check, before any allocation
    rc = get_fft_tables(SS_BANK_SPECTRUM_N, &m->ft);
    if (rc) return rc;
    rc = get_bin_tables(m->meter.rate, SS_BANK_SPECTRUM_N, &m->bt);
    if (rc) return rc;
    if (!m->spec_pink.p) HIPCHK(m->spec_pink.upload(m->bt->pink));
    const size_t floats = (size_t)m->meter.n * SS_BANK_SPECTRUM_N * m->meter.channels;
    HIPCHK(m->spec_hist.ensure(floats));
    HIPCHK(hipMemsetAsync(m->spec_hist.p, 0, floats * sizeof(float), m->stream));  // (re-enabling starts again from zeros)
    HIPCHK(m->spec_status.ensure((size_t)m->meter.n * spec_rows(m)));
    m->spec_fed = 0;
    if (m->spec_ahead.p) HIPCHK(hipMemsetAsync(m->spec_ahead.p, 0, m->meter.n * sizeof(uint64_t), m->stream));
    m->spec_on = true;
    return SS_OK;
}

int ss_meter_bank_spectrum_layout(const ss_meter_bank *m, uint32_t *rows_per_stream, uint32_t *n_bins, double *chart_x, double *pink,
                                  uint32_t cap_bins)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->spec_on) return SS_ERR_INVALID_MODE;
    const uint32_t nb = (uint32_t)m->bt->count;
    if ((chart_x || pink) && cap_bins < nb) return SS_ERR_CAPACITY;
    if (rows_per_stream) *rows_per_stream = spec_rows(m);
    if (n_bins) *n_bins = nb;
    for (uint32_t i = 0; i < nb; i++) {
        if (chart_x) chart_x[i] = m->bt->chart_x[i];
        if (pink) pink[i] = m->bt->pink[i];
    }
    return SS_OK;
}

int ss_meter_bank_spectrum(ss_meter_bank *m, float *rows, size_t cap_floats, int32_t *status, uint32_t cap_rows)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!rows || !status) return SS_ERR_INVALID_ARG;
    if (!m->spec_on) return SS_ERR_INVALID_MODE;
    const uint32_t nb = (uint32_t)m->bt->count;
    const size_t R = (size_t)m->meter.n * spec_rows(m);
    if (cap_floats < R * nb || cap_rows < R) return SS_ERR_CAPACITY;
    return spectrum_run(m, false, 0, SS_GAIN_FIXED, 0.0f, nb, rows, status);
}

int ss_meter_bank_spectrum_columns(ss_meter_bank *m, uint32_t cols, int gain_mode, float gain_db, float *out, size_t cap_floats,
                                   int32_t *status, uint32_t cap_rows)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!out || !status || cols == 0 || cols > 512 || (gain_mode != SS_GAIN_FIXED && gain_mode != SS_GAIN_REFERENCE))
        return SS_ERR_INVALID_ARG;
    if (!m->spec_on) return SS_ERR_INVALID_MODE;
    const size_t R = (size_t)m->meter.n * spec_rows(m);
    if (cap_floats < R * cols || cap_rows < R) return SS_ERR_CAPACITY;
    return spectrum_run(m, true, cols, gain_mode, gain_db, cols, out, status);
}

int ss_meter_bank_spectrum_track_enable(ss_meter_bank *m, const ss_spectrum_ballistics *cfg)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!cfg) return track_drop(m);
    if (!(cfg->average_tau_s >= 0.0) || std::isinf(cfg->average_tau_s) || !(cfg->hold_s >= 0.0) || !(cfg->decay_db_per_s >= 0.0) ||
        std::isinf(cfg->decay_db_per_s))
        return SS_ERR_INVALID_ARG;
    if (!m->spec_on) return SS_ERR_INVALID_MODE;
    int rc = track_drop(m);                                                        // enabling again starts from empty state
    if (rc) return rc;
    const size_t rows = track_rows_of(m), nb = m->bt->count, stride = (nb + 3u) & ~(size_t)3u;
    HIPCHK(m->trk_state.alloc(rows * stride * 16u));
    HIPCHK(m->trk_meta.alloc(2 * rows));
    HIPCHK(m->trk_rows.alloc(rows * nb));
    HIPCHK(m->trk_status.alloc(rows));
    HIPCHK(hipMemsetAsync(m->trk_meta.p, 0, 2 * rows * sizeof(ssk::BankTrackRow), m->stream));     // updates == 0: a row without state
    m->trk_cfg = *cfg;
    m->trk_cur = 0;
    m->trk_on = true;
    return SS_OK;
}

int ss_meter_bank_spectrum_track(ss_meter_bank *m)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->trk_on) return SS_ERR_INVALID_MODE;
    HIPCHK(ssk::launch_meter_bank_spectrum(spectrum_params(m, m->trk_rows.p, m->trk_status.p), false, m->stream));
    HIPCHK(ssk::launch_bank_spectrum_track(track_params(m), m->stream));
    m->trk_cur ^= 1u;
    return SS_OK;
}

int ss_meter_bank_spectrum_track_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->trk_on) return SS_ERR_INVALID_MODE;
    ssk::BankTrackRow *meta = m->trk_meta.p + m->trk_cur * track_rows_of(m);
    if (streams && !count) return SS_OK;                                           // (an empty list: nothing is staged)
    const uint32_t *dev;
    int rc = stream_list(m, streams, count, &dev);
    if (rc) return rc;
    HIPCHK(ssk::launch_bank_spectrum_track_reset(meta, dev, streams ? count : m->meter.n, spec_rows(m), m->stream));
    return SS_OK;
}

int ss_meter_bank_spectrum_tracked(ss_meter_bank *m, float *avg_rows, float *hold_rows, size_t cap_floats, uint32_t *updates,
                                   uint32_t cap_rows)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->trk_on) return SS_ERR_INVALID_MODE;
    const size_t R = track_rows_of(m), plane = R * m->bt->count;
    if (((avg_rows || hold_rows) && cap_floats < plane) || (updates && cap_rows < R)) return SS_ERR_CAPACITY;
    // the curves asked for, then the counts: one copy
    const size_t hold_at = avg_rows ? plane : 0;
    const TrackOut o{plane, hold_at, hold_at + (hold_rows ? plane : 0), R};
    int rc = track_room(m, o.bytes());
    if (rc) return rc;
    float *base = reinterpret_cast<float *>(m->trk_out.p);
    HIPCHK(ssk::launch_bank_spectrum_tracked_rows(track_params(m), avg_rows ? base : nullptr, hold_rows ? base + o.hold_at : nullptr,
                                                  reinterpret_cast<uint32_t *>(base + o.counts_at), m->stream));
    return track_fetch(m, o, avg_rows, hold_rows, updates);
}

int ss_meter_bank_spectrum_tracked_columns(ss_meter_bank *m, uint32_t cols, int gain_mode, float gain_db, float *avg_cols,
                                           float *hold_cols, size_t cap_floats, uint32_t *updates, uint32_t cap_rows)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (cols == 0 || cols > 512 || (gain_mode != SS_GAIN_FIXED && gain_mode != SS_GAIN_REFERENCE)) return SS_ERR_INVALID_ARG;
    if (!m->trk_on) return SS_ERR_INVALID_MODE;
    const size_t R = track_rows_of(m), plane = R * cols;
    if (((avg_cols || hold_cols) && cap_floats < plane) || (updates && cap_rows < R)) return SS_ERR_CAPACITY;
    const TrackOut o{plane, plane, 2 * plane, R};                                    // both curves (a few KB per stream), then the counts
    int rc = track_room(m, o.bytes());
    if (rc) return rc;
    ssk::BankTrackColumns c{};
    if ((rc = column_fold(m, cols, gain_mode, gain_db, &c.fold))) return rc;
    float *base = reinterpret_cast<float *>(m->trk_out.p);
    c.avg = base; c.hold = base + o.hold_at; c.updates = reinterpret_cast<uint32_t *>(base + o.counts_at);
    HIPCHK(ssk::launch_bank_spectrum_tracked_columns(track_params(m), c, m->stream));
    return track_fetch(m, o, avg_cols, hold_cols, updates);
}

int ss_meter_bank_signal_watch_enable(ss_meter_bank *m, const ss_signal_scan_config *cfg)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!cfg) {
        if (!m->watch_on) return SS_OK;
        HIPCHK(bank_sync(m));                                                       // nothing on the stream still uses the state
        m->watch_on = false;
        m->watch_state.release(); m->watch_rec.release(); m->watch_pin.release();
        return SS_OK;
    }
    // ss_batch_signal_scan's refusals, and no event list yet
    if (!(cfg->silence_threshold >= 0.f) || !(cfg->clip_level > 0.f)) return SS_ERR_INVALID_ARG;        // (NaN fails the comparison)
    if (!cfg->silence_min_frames || !cfg->clip_min_samples || cfg->max_events || cfg->reserved) return SS_ERR_INVALID_ARG;
    const size_t n = m->meter.n, Q = (size_t)m->meter.channels + 1;
    HIPCHK(m->watch_state.ensure(n * Q));                                           // (enabling again keeps the allocations)
    HIPCHK(m->watch_rec.ensure(watch_rec_bytes(m)));
    HIPCHK(m->watch_pin.ensure(watch_rec_bytes(m)));
    HIPCHK(ssk::launch_bank_signal_watch_reset(m->watch_state.p, watch_streams(m), watch_channels(m), nullptr, m->meter.n, m->meter.channels,
                                               m->stream));
    m->watch_cfg = *cfg;
    m->watch_on = true;
    return SS_OK;
}

int ss_meter_bank_signal_watch_plan(const ss_meter_bank *m, uint32_t *tile_frames)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->watch_on) return SS_ERR_INVALID_MODE;
    if (tile_frames) *tile_frames = ssk::plan_signal_scan(m->meter.channels, 0).tile_frames;
    return SS_OK;
}

int ss_meter_bank_signal_watch_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->watch_on) return SS_ERR_INVALID_MODE;
    if (streams && !count) return SS_OK;                                           // (an empty list: nothing is staged)
    const uint32_t *dev;
    int rc = stream_list(m, streams, count, &dev);
    if (rc) return rc;
    HIPCHK(ssk::launch_bank_signal_watch_reset(m->watch_state.p, watch_streams(m), watch_channels(m), dev, streams ? count : m->meter.n,
                                               m->meter.channels, m->stream));
    return SS_OK;
}

int ss_meter_bank_signal_watch(ss_meter_bank *m, ss_stream_watch *streams_out, uint32_t cap_streams, ss_channel_watch *channels_out,
                               size_t cap_records)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->watch_on) return SS_ERR_INVALID_MODE;
    const size_t n = m->meter.n, sbytes = n * sizeof(ssk::StreamWatch), cbytes = n * m->meter.channels * sizeof(ssk::ChannelWatch);
    if ((streams_out && cap_streams < n) || (channels_out && cap_records < n * m->meter.channels)) return SS_ERR_CAPACITY;
    // the add calls left the records as they stand: no launch, one copy of what was asked for
    const size_t from = streams_out ? 0 : sbytes, to = channels_out ? sbytes + cbytes : sbytes;
    if (to > from) HIPCHK(hipMemcpyAsync(m->watch_pin.p + from, m->watch_rec.p + from, to - from, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    if (streams_out) std::memcpy(streams_out, m->watch_pin.p, sbytes);
    if (channels_out) std::memcpy(channels_out, m->watch_pin.p + sbytes, cbytes);
    return SS_OK;
}

int ss_meter_bank_pair_watch_enable(ss_meter_bank *m, const ss_channel_pair *pairs, uint32_t n_pairs, const ss_pair_watch_config *cfg)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!cfg) return pair_watch_drop(m);
    // ss_batch_pair_series' pair-list refusals (ss_batch.cpp's pair_list_of, on the bank's channel count) and ss_batch_pair_regions'
    // config refusals, before anything is allocated or queued
    const uint32_t C = m->meter.channels;
    ssk::ChannelPair list[ssk::kMaxPairs] = {};
    uint32_t np = n_pairs;
    if (n_pairs > ssk::kMaxPairs || (!pairs && n_pairs)) return SS_ERR_INVALID_ARG;
    if (!pairs || !n_pairs) {                                                      // the default pair needs two channels
        if (C < 2u) return SS_ERR_INVALID_ARG;
        list[0].a = 0u; list[0].b = 1u;
        np = 1u;
    }
    for (uint32_t k = 0; pairs && k < n_pairs; k++) {
        if (pairs[k].a >= C || pairs[k].b >= C) return SS_ERR_INVALID_ARG;
        list[k] = pairs[k];
    }
    if (!(cfg->threshold > -1.0 && cfg->threshold < 1.0) || !(cfg->power_floor >= 0.0)) return SS_ERR_INVALID_ARG;        // (NaN fails the comparisons)
    if (!cfg->min_run || !cfg->window_entries || cfg->window_entries > SS_BANK_PAIR_WINDOW_MAX) return SS_ERR_INVALID_ARG;
    const size_t n = m->meter.n, R = cfg->window_entries;
    const bool same = m->pair_on && np == m->pair_n && R == m->pair_cfg.window_entries;
    if (m->pair_on && !same) {                                                     // another shape: the stream may still use the old state
        int rc = pair_watch_drop(m);
        if (rc) return rc;
    }
    HIPCHK(m->pair_lanes.ensure(n * np * 3u * ssk::kPairWatchLanes));              // (enabling again with the same shape keeps the allocations)
    HIPCHK(m->pair_open_skipped.ensure(n * np));
    HIPCHK(m->pair_ring.ensure(n * R * np));
    HIPCHK(m->pair_rec.ensure(n * np));
    const size_t rec_bytes = n * np * sizeof(ssk::PairWatch), ring_bytes = R * np * sizeof(ssk::PairEntry);
    HIPCHK(m->pair_pin.ensure(rec_bytes > ring_bytes ? rec_bytes : ring_bytes));
    HIPCHK(ssk::launch_bank_pair_watch_reset(m->pair_rec.p, m->pair_open_skipped.p, nullptr, m->meter.n, np, m->stream));
    m->pair_cfg = *cfg;
    m->pair_n = np;
    for (uint32_t k = 0; k < np; k++) m->pair_list[k] = list[k];
    m->pair_fed.assign(n, 0);
    m->pair_on = true;
    return SS_OK;
}

int ss_meter_bank_pair_watch_plan(const ss_meter_bank *m, uint32_t *lanes, uint32_t *window_entries, uint32_t *n_pairs)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->pair_on) return SS_ERR_INVALID_MODE;
    if (lanes) *lanes = ssk::kPairWatchLanes;
    if (window_entries) *window_entries = m->pair_cfg.window_entries;
    if (n_pairs) *n_pairs = m->pair_n;
    return SS_OK;
}

int ss_meter_bank_pair_watch_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->pair_on) return SS_ERR_INVALID_MODE;
    if (streams && !count) return SS_OK;                                           // (an empty list: nothing is staged)
    const uint32_t *dev;
    int rc = stream_list(m, streams, count, &dev);
    if (rc) return rc;
    if (!streams) count = m->meter.n;
    HIPCHK(ssk::launch_bank_pair_watch_reset(m->pair_rec.p, m->pair_open_skipped.p, dev, count, m->pair_n, m->stream));
    for (uint32_t i = 0; i < count; i++) m->pair_fed[streams ? streams[i] : i] = 0;
    return SS_OK;
}

int ss_meter_bank_pair_watch(ss_meter_bank *m, ss_pair_watch *out, size_t cap_records)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->pair_on) return SS_ERR_INVALID_MODE;
    if (!out) return SS_ERR_INVALID_ARG;
    const size_t records = (size_t)m->meter.n * m->pair_n, bytes = records * sizeof(ssk::PairWatch);
    if (cap_records < records) return SS_ERR_CAPACITY;
    // the add calls left the records as they stand: no launch, one copy
    HIPCHK(hipMemcpyAsync(m->pair_pin.p, m->pair_rec.p, bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    std::memcpy(out, m->pair_pin.p, bytes);
    return SS_OK;
}

int ss_meter_bank_pair_watch_entries(ss_meter_bank *m, uint32_t stream, ss_pair_entry *out, size_t cap_entries, uint64_t *first_entry,
                                     uint32_t *n_entries)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!m->pair_on) return SS_ERR_INVALID_MODE;
    if (stream >= m->meter.n) return SS_ERR_INVALID_ARG;
    const uint64_t E = m->pair_fed[stream] / m->meter.s100, R = m->pair_cfg.window_entries;
    const uint32_t n = (uint32_t)(E < R ? E : R), NP = m->pair_n;
    if (!out && n) return SS_ERR_INVALID_ARG;
    if (cap_entries < n) return SS_ERR_CAPACITY;
    // slots [0, n) hold the newest n entries (n < R: entries 0 .. n - 1 in place; n == R: entry j at slot j mod R): one copy
    const size_t bytes = (size_t)n * NP * sizeof(ssk::PairEntry);
    if (n) HIPCHK(hipMemcpyAsync(m->pair_pin.p, m->pair_ring.p + (size_t)stream * R * NP, bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(bank_sync(m));
    const uint64_t first = E - n;
    const ssk::PairEntry *ring = reinterpret_cast<const ssk::PairEntry *>(m->pair_pin.p);
    for (uint32_t j = 0; j < n; j++)
        std::memcpy(out + (size_t)j * NP, ring + (size_t)((first + j) % R) * NP, (size_t)NP * sizeof(ssk::PairEntry));
    if (first_entry) *first_entry = first;
    if (n_entries) *n_entries = n;
    return SS_OK;
}

}  // extern "C"
