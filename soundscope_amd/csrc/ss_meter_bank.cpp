// ss_meter_bank.cpp — meter banks (include/soundscope_hip.h, "Meter banks"): N live meters of one shape advanced together.  Host
// logic only: argument checks in the handle's order, the per-stream device state (laid out as ss_analyzer holds its meter), the
// staging of the input and the launches — k_time_domain's streaming forms over all streams, k_meter_bank_gate,
// k_meter_bank_readings, k_meter_bank_reset (ss_loudness.hip).  No CPU compute path.
#include "ss_host.h"

using namespace ssh;

struct ss_meter_bank {
    int device = 0;
    uint32_t n = 0, channels = 0, rate = 0;
    int tp_factor = 0;
    hipStream_t stream = nullptr;
    TdTables *td = nullptr;
    uint64_t s100 = 0, ring_frames = 0;
    bool st_on = false;
    ssh::DevBuf<ssk::TdState> state;
    ssh::DevBuf<uint64_t> hist;            // [n][2][1000]
    ssh::DevBuf<double> sub;               // [n][kSubCap][C]
    ssh::DevBuf<double> ring;              // [n][ring_frames][C]
    ssh::DevBuf<double> weights;
    ssh::DevBuf<uint32_t> counts;          // [n][2]
    ssh::DevBuf<uint32_t> list;            // ss_meter_bank_reset's stream indices
    ssh::DevBuf<float> in;                 // the f32 input of a host call
    ssh::DevBuf<unsigned char> raw;        // ss_meter_bank_add_pcm's bytes
    ssh::DevBuf<ssk::MeterReading> readings;
    std::vector<uint64_t> fed;             // frames since each stream's reset (the device's TdState::frames_fed, mirrored)
    // page-locked staging: a host call's input is copied there and returns behind its launches (the event says when the copy
    // to the device has left the buffer); the readings come back through the same kind of buffer
    void *pin = nullptr;
    size_t pin_bytes = 0;
    hipEvent_t pin_ev = nullptr;
    bool pin_busy = false;
    ssk::MeterReading *pin_read = nullptr;
    static constexpr uint32_t kSubCap = ss_analyzer::kSubCap;
};

static_assert(sizeof(ss_meter_reading) == 72 && sizeof(ssk::MeterReading) == sizeof(ss_meter_reading), "ss_meter_reading layout");
static_assert(offsetof(ss_meter_reading, true_peak) == offsetof(ssk::MeterReading, true_peak) &&
              offsetof(ss_meter_reading, frames) == offsetof(ssk::MeterReading, frames), "ss_meter_reading layout");

namespace {

ssk::MeterBankParams bank_params(const ss_meter_bank *m, const double *he, const double *hb)
{
    ssk::MeterBankParams q{};
    q.k = m->td->dev.p; q.state = m->state.p;
    q.subblocks = m->sub.p; q.sub_stride = (uint64_t)ss_meter_bank::kSubCap * m->channels; q.sub_cap = ss_meter_bank::kSubCap;
    q.ring = m->ring.p; q.ring_stride = m->ring_frames * m->channels; q.ring_frames = m->ring_frames;
    q.weights = m->weights.p; q.hist = m->hist.p; q.counts = m->counts.p;
    q.hist_energies = he; q.hist_bounds = hb;
    q.n_streams = m->n; q.channels = m->channels; q.st_on = m->st_on ? 1u : 0u;
    return q;
}

// a page-locked buffer of at least `bytes` no copy is still reading
int pin_take(ss_meter_bank *m, size_t bytes)
{
    if (m->pin_busy) { HIPCHK(hipEventSynchronize(m->pin_ev)); m->pin_busy = false; }
    if (bytes > m->pin_bytes) {
        if (m->pin) { (void)hipHostFree(m->pin); m->pin = nullptr; m->pin_bytes = 0; }
        HIPCHK(hipHostMalloc(&m->pin, bytes, hipHostMallocDefault));
        m->pin_bytes = bytes;
    }
    return SS_OK;
}

// stage host bytes on the device: page-locked copy, one DMA, an event behind it
int upload(ss_meter_bank *m, void *dst, const void *src, size_t bytes)
{
    int rc = pin_take(m, bytes);
    if (rc) return rc;
    std::memcpy(m->pin, src, bytes);
    HIPCHK(hipMemcpyAsync(dst, m->pin, bytes, hipMemcpyHostToDevice, m->stream));
    HIPCHK(hipEventRecord(m->pin_ev, m->stream));
    m->pin_busy = true;
    return SS_OK;
}

// every stream advanced by `frames` frames of device-resident f32 input (stream s at pcm + s * stride): pieces of at most 32
// sub-blocks, so that the 96-slot sub-block ring always holds the thirty sub-blocks a short-term block reads (ss_add_samples' rule)
int advance(ss_meter_bank *m, const float *pcm, uint64_t frames, uint64_t stride)
{
    const double *he, *hb;
    int rc = get_hist_tables(&he, &hb);
    if (rc) return rc;
    const uint32_t C = m->channels;
    const uint64_t S = m->s100, piece_frames = 32 * S;
    const ssk::MeterBankParams q = bank_params(m, he, hb);
    for (uint64_t done = 0; done < frames;) {
        const uint64_t take = frames - done < piece_frames ? frames - done : piece_frames;
        ssk::TdParams p{};
        p.pcm = pcm + done * C; p.stream_stride = stride; p.n_frames = take; p.n_streams = m->n; p.channels = C;
        p.k = m->td->dev.p; p.state = m->state.p;
        p.subblocks = q.subblocks; p.sub_stride = q.sub_stride; p.sub_cap = q.sub_cap;
        p.ring = q.ring; p.ring_frames = q.ring_frames; p.ring_stride = q.ring_stride;
        p.tp_factor = m->tp_factor; p.s100 = (uint32_t)S; p.nseg = 1; p.seg_sub = 0; p.warm_sub = 0;
        p.tp_f32 = 1u;                                                   // SS_TP_ARITH_F32, the handle's default
        HIPCHK(ssk::launch_time_domain(p, m->stream));
        // the gating launch only when some stream completes a sub-block (each stream's range is derived on the device)
        bool any = false;
        for (uint32_t s = 0; s < m->n; s++) {
            any = any || (m->fed[s] + take) / S > m->fed[s] / S;
            m->fed[s] += take;
        }
        if (any) HIPCHK(ssk::launch_meter_bank_gate(q, take, m->stream));
        done += take;
    }
    return SS_OK;
}

int bank_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    const double *he, *hb;
    int rc = get_hist_tables(&he, &hb);
    if (rc) return rc;
    const uint32_t *dev = nullptr;
    if (streams) {
        HIPCHK(m->list.ensure(count));
        rc = upload(m, m->list.p, streams, count * sizeof(uint32_t));
        if (rc) return rc;
        dev = m->list.p;
    }
    HIPCHK(ssk::launch_meter_bank_reset(bank_params(m, he, hb), dev, count, m->stream));
    for (uint32_t i = 0; i < count; i++) m->fed[streams ? streams[i] : i] = 0;
    return SS_OK;
}

int null_bank() { return require_device() ? SS_ERR_DEVICE : SS_ERR_INVALID_ARG; }

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
    m->n = n_streams; m->channels = channels; m->rate = rate;
    m->tp_factor = true_peak_factor ? true_peak_factor : sst::true_peak_factor_for_rate(rate);
    rc = get_td_tables(rate, m->tp_factor, channels, &m->td);
    if (rc) return rc;
    // the handle's geometry (handle_make_meter): 3 s of filtered samples rounded up to a whole sub-block
    m->s100 = (rate + 5) / 10;
    m->ring_frames = (uint64_t)rate * 3000 / 1000;
    if (m->ring_frames % m->s100) m->ring_frames += m->s100 - m->ring_frames % m->s100;
    if (m->ring_frames * channels >= (1ull << 31)) return SS_ERR_UNSUPPORTED;       // (32-bit ring positions in the kernels)
    m->st_on = 30 * m->s100 <= m->ring_frames;                  // ss_get_shortterm_lufs' own condition
    HIPCHK(stream_acquire(&m->stream));
    HIPCHK(hipEventCreateWithFlags(&m->pin_ev, hipEventDisableTiming));
    const size_t N = n_streams;
    HIPCHK(m->state.alloc(N));
    HIPCHK(m->hist.alloc(N * 2 * sst::kHistBins));
    HIPCHK(m->sub.alloc(N * ss_meter_bank::kSubCap * channels));
    HIPCHK(m->ring.alloc(N * m->ring_frames * channels));
    HIPCHK(m->counts.alloc(N * 2));
    HIPCHK(m->readings.alloc(N));
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&m->pin_read), N * sizeof(ssk::MeterReading), hipHostMallocDefault));
    std::vector<double> w(channels);
    sst::channel_weights(channels, w.data());
    HIPCHK(m->weights.upload(w));
    m->fed.assign(N, 0);
    rc = bank_reset(m.get(), nullptr, n_streams);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(m->stream));
    *out = m.release();
    return SS_OK;
}

void ss_meter_bank_destroy(ss_meter_bank *m)
{
    SS_ON_DEVICE(m);
    if (!m) return;
    if (m->stream) { (void)hipStreamSynchronize(m->stream); stream_release(m->stream); }
    if (m->pin_ev) (void)hipEventDestroy(m->pin_ev);
    if (m->pin) (void)hipHostFree(m->pin);
    if (m->pin_read) (void)hipHostFree(m->pin_read);
    delete m;
}

int ss_meter_bank_add(ss_meter_bank *m, const float *pcm, uint64_t frames)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (frames == 0) return SS_OK;
    if (!pcm) return SS_ERR_INVALID_ARG;
    const uint64_t per = frames * m->channels, total = per * m->n;
    HIPCHK(m->in.ensure(total));
    int rc = upload(m, m->in.p, pcm, total * sizeof(float));
    if (rc) return rc;
    return advance(m, m->in.p, frames, per);
}

int ss_meter_bank_add_device(ss_meter_bank *m, const float *pcm_device, uint64_t frames, uint64_t stream_stride_floats)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (frames == 0) return SS_OK;
    if (!pcm_device || stream_stride_floats < frames * m->channels) return SS_ERR_INVALID_ARG;
    return advance(m, pcm_device, frames, stream_stride_floats);
}

int ss_meter_bank_add_pcm(ss_meter_bank *m, const void *pcm, uint64_t frames, int format)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    const size_t sb = ss_pcm_sample_bytes(format);
    if (!sb) return SS_ERR_INVALID_ARG;
    if (frames == 0) return SS_OK;
    if (!pcm) return SS_ERR_INVALID_ARG;
    const uint64_t per = frames * m->channels, total = per * m->n;
    HIPCHK(m->raw.ensure(total * sb + 8));                       // (+8: the converter's wide reads of 24-bit samples)
    HIPCHK(m->in.ensure(total));
    int rc = upload(m, m->raw.p, pcm, total * sb);
    if (rc) return rc;
    HIPCHK(ssk::launch_pcm_to_f32(m->raw.p, total, format, m->in.p, m->stream));
    return advance(m, m->in.p, frames, per);
}

int ss_meter_bank_reset(ss_meter_bank *m, const uint32_t *streams, uint32_t count)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!streams) return bank_reset(m, nullptr, m->n);
    for (uint32_t i = 0; i < count; i++) if (streams[i] >= m->n) return SS_ERR_INVALID_ARG;
    return bank_reset(m, streams, count);
}

int ss_meter_bank_read(ss_meter_bank *m, ss_meter_reading *out, uint32_t cap_streams)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (!out) return SS_ERR_INVALID_ARG;
    if (cap_streams < m->n) return SS_ERR_CAPACITY;
    const double *he, *hb;
    int rc = get_hist_tables(&he, &hb);
    if (rc) return rc;
    HIPCHK(ssk::launch_meter_bank_readings(bank_params(m, he, hb), m->readings.p, m->stream));
    HIPCHK(hipMemcpyAsync(m->pin_read, m->readings.p, m->n * sizeof(ssk::MeterReading), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->pin_busy = false;
    std::memcpy(out, m->pin_read, m->n * sizeof(ss_meter_reading));
    return SS_OK;
}

int ss_meter_bank_peaks(ss_meter_bank *m, uint32_t stream, double *true_pk, double *sample_pk, uint32_t cap_channels)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (stream >= m->n) return SS_ERR_INVALID_ARG;
    if ((true_pk || sample_pk) && cap_channels < m->channels) return SS_ERR_CAPACITY;
    static_assert(offsetof(ssk::TdState, true_peak) == offsetof(ssk::TdState, sample_peak) + sizeof(float) * ssk::kMaxChannels,
                  "sample_peak and true_peak are read as one block");
    float pk[2 * ssk::kMaxChannels];
    HIPCHK(hipMemcpyAsync(pk, &m->state.p[stream].sample_peak[0], sizeof pk, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->pin_busy = false;
    for (uint32_t c = 0; c < m->channels; c++) {
        const float sp = pk[c], tp = pk[ssk::kMaxChannels + c];
        if (sample_pk) sample_pk[c] = (double)sp;
        if (true_pk) true_pk[c] = (double)(tp > sp ? tp : sp);       // true_peak(): max(true, sample)
    }
    return SS_OK;
}

int ss_meter_bank_histograms(ss_meter_bank *m, uint32_t stream, uint64_t *out2000)
{
    SS_ON_DEVICE(m);
    if (!m) return null_bank();
    if (stream >= m->n || !out2000) return SS_ERR_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(out2000, m->hist.p + (size_t)stream * 2 * sst::kHistBins, 2 * sst::kHistBins * sizeof(uint64_t),
                          hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    m->pin_busy = false;
    return SS_OK;
}

}  // extern "C"
