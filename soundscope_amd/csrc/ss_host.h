// ss_host.h — what the host-side translation units of the library share (never installed): the HIP error channel, the RAII
// owners of memory (DevBuf: device, PinBuf: page-locked host, HostStage: a page-locked buffer a copy may still be reading), the
// per-device caches of constant tables, per-thread scratch, the live meter and the handle type.
//   ss_host.cpp         caches, device selection, status strings, table inspection, the live meter (MeterStore)
//   ss_analyzer.cpp     the Analyzer mirror (one entry point per Rust method, analyzer.rs:29-183)
//   ss_ingest.cpp       RIFF/WAVE header walk and PCM conversion
//   ss_batch.cpp        the batch extension (BASELINE configs 3-5) and the render-side reductions (N3)
//   ss_session.cpp      the tick drivers (N1)
//   ss_meter_bank.cpp   meter banks: many live meters advanced together
//   ss_comm.cpp         the all-reduce of the corpus histograms (RCCL opened at run time; does not include this header)
//   ss_tables.cpp       the host-side design of the constant tables (includes ss_tables.h only)
//   ss_resample_host.cpp  the resampler's plan rule, table and reference chain (includes the public header only)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ss_internal.h"
#include "ss_kernels.h"        // (and with it the public header, include/soundscope_hip.h)
#include "ss_tables.h"

namespace ssh {

// text of the last HIP error on this thread (ss_last_device_error)
SS_HIDDEN std::string &last_error();
SS_HIDDEN bool hip_ok(hipError_t e, const char *what);
#define HIPCHK(expr)                                        \
    do {                                                    \
        if (!ssh::hip_ok((expr), #expr)) return SS_ERR_DEVICE; \
    } while (0)

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { swap(o); return *this; }     // (o frees what this held)
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr; n = 0;
    }
    hipError_t alloc(size_t count)
    {
        release();
        if (!count) return hipSuccess;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t ensure(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
    hipError_t upload(const std::vector<T> &h)
    {
        hipError_t e = h.size() == n ? hipSuccess : alloc(h.size());      // (same size: the allocation is kept — a free and a malloc are 30-250 us)
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

// Page-locked host memory, owned like DevBuf owns device memory.  dev: the same memory as the device sees it (kernels write
// results straight into it).  A regrow frees first; the caller has made sure that nothing on the device still uses the buffer.
template <typename T>
struct PinBuf {
    T *p = nullptr, *dev = nullptr;
    size_t n = 0;
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    PinBuf(PinBuf &&o) noexcept { swap(o); }
    PinBuf &operator=(PinBuf &&o) noexcept { swap(o); return *this; }     // (o frees what this held)
    ~PinBuf() { release(); }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr; n = 0;
    }
    hipError_t alloc(size_t count)
    {
        release();
        if (!count) return hipSuccess;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), p, 0);
        if (e == hipSuccess) n = count; else release();
        return e;
    }
    hipError_t ensure(size_t count) { return count <= n ? hipSuccess : alloc(count); }
    void swap(PinBuf &o) { std::swap(p, o.p); std::swap(dev, o.dev); std::swap(n, o.n); }
};

// A page-locked buffer that host input is copied into on its way to the device, and an event that says when that copy has left
// it: the call returns behind its launches, and the next user of the buffer waits for the event only if nobody has waited for the
// stream in between.
struct HostStage {
    PinBuf<unsigned char> buf;
    hipEvent_t ev = nullptr;             // created at first use
    bool busy = false;
    ~HostStage() { if (ev) (void)hipEventDestroy(ev); }
    // `bytes` of page-locked memory at buf.p that no copy is still reading (a busy buffer is waited for, a small one regrown)
    hipError_t take(size_t bytes)
    {
        hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e == hipSuccess && busy && (e = hipEventSynchronize(ev)) == hipSuccess) busy = false;
        return e == hipSuccess ? buf.ensure(bytes) : e;
    }
    // the copy out of the buffer has just been enqueued on `stream`
    hipError_t sent(hipStream_t stream)
    {
        hipError_t e = hipEventRecord(ev, stream);
        if (e == hipSuccess) busy = true;
        return e;
    }
    void idle() { busy = false; }        // the owner has synchronised the stream
    // the first `bytes` of the buffer, filled behind a take, on their way to `dst` on the device: one DMA, the event behind it
    hipError_t queue(void *dst, size_t bytes, hipStream_t stream)
    {
        hipError_t e = hipMemcpyAsync(dst, buf.p, bytes, hipMemcpyHostToDevice, stream);
        return e == hipSuccess ? sent(stream) : e;
    }
    // the staged upload in one call: `bytes` at `src` through the buffer to `dst`; `src` is free again when this returns
    hipError_t send(void *dst, const void *src, size_t bytes, hipStream_t stream)
    {
        hipError_t e = take(bytes);
        if (e != hipSuccess) return e;
        std::memcpy(buf.p, src, bytes);
        return queue(dst, bytes, stream);
    }
};

// what ssk::launch_pcm_to_f32's wide reads of 24-bit samples may touch behind the last sample: every raw PCM buffer on the device is
// allocated this many bytes longer than its samples
constexpr size_t kPcmReadSlack = 8;

// EbuR128::sample_peak(c) and EbuR128::true_peak(c) = max(true, sample) of channel c, from a host copy of a state's peaks
// (`block`: TdState::sample_peak | TdState::true_peak, read as one block of 2 * kMaxChannels floats: adjacent, ss_kernels.h)
inline void peaks_of(const float *block, uint32_t c, double *sample_pk, double *true_pk)
{
    const float sp = block[c], tp = block[ssk::kMaxChannels + c];
    if (sample_pk) *sample_pk = (double)sp;
    if (true_pk) *true_pk = (double)(tp > sp ? tp : sp);
}

// ---- per-process caches of device-resident constant tables ------------------
struct FftTables {
    size_t n = 0;
    std::vector<float> window_host;
    DevBuf<float> window, half_window;
    DevBuf<float2> tw_n, tw_256;
    const float2 *core_tw4096 = nullptr, *core_tw256 = nullptr;   // n == 16384: tables of the 4096-point core
};

struct BinTables {
    size_t first = 0, count = 0;
    std::vector<double> freq, pink, chart_x;
    DevBuf<float> pink_dev;
    DevBuf<float> offpink4096_dev;      // db_offset(4096) + pink, for the N = 4096 kernels
    DevBuf<float> off4096_dev;          // db_offset(4096) alone (ss_get_fft adds the pink compensation in f64 on the host, analyzer.rs:82)
};

struct TdTables {
    ssk::TdConst host;
    DevBuf<ssk::TdConst> dev;
};

// One context per HIP device: device pointers are only valid on the device that allocated them, and
// hipSetDevice is per thread, so the caches are looked up by the device current at the call.
struct Ctx {
    std::mutex mu;
    std::map<size_t, std::unique_ptr<FftTables>> fft;
    std::map<std::pair<uint32_t, size_t>, std::unique_ptr<BinTables>> bins;
    std::map<std::pair<uint32_t, uint32_t>, std::unique_ptr<TdTables>> td;   // (rate, factor | channels << 8)
    DevBuf<double> hist_energies, hist_bounds;
    // idle streams of handles and batches that were destroyed (stream_acquire / stream_release)
    std::vector<hipStream_t> idle_streams;
};

// the table cache of the calling thread's current device
SS_HIDDEN Ctx &ctx();
// Streams of handles, sessions and batches come from a per-device pool: hipStreamCreateWithFlags costs 1.7-18 ms and
// hipStreamDestroy 1.5 ms on this stack (rocprofv3 --hip-trace over six session opens: 52 of their 70 ms, tools/probe_open_hipapi.sh)
// — a file open made two of each.  stream_release takes an IDLE stream (the caller has synchronised it).
SS_HIDDEN hipError_t stream_acquire(hipStream_t *out);
SS_HIDDEN void stream_release(hipStream_t s);
SS_HIDDEN int current_device();

// Scratch of the handle-less entry points (ss_get_waveform, ss_mid_side, ss_pcm_decode): one set per calling
// thread and device, so concurrent callers never serialise on a shared buffer.
struct Scratch {
    DevBuf<float> in, out;
    DevBuf<unsigned char> raw;
    hipStream_t stream = nullptr;
    ~Scratch() { if (stream) (void)hipStreamDestroy(stream); }
};
SS_HIDDEN Scratch &scratch();

// makes `device` current for the scope of one entry point (handles are bound to the device they were created on)
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int device)
    {
        if (device < 0) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = (hipSetDevice(device) == hipSuccess);
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};
#define SS_ON_DEVICE(obj) DeviceScope device_scope_((obj) ? (obj)->device : -1)

SS_HIDDEN int probe_devices();
SS_HIDDEN int require_device();
SS_HIDDEN int get_fft_tables(size_t n, FftTables **out);
SS_HIDDEN int get_bin_tables(uint32_t rate, size_t n, BinTables **out);
SS_HIDDEN int get_td_tables(uint32_t rate, int factor, uint32_t channels, TdTables **out);
SS_HIDDEN int get_hist_tables(const double **energies, const double **bounds);
inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
// chart column of a bin: floor(chart_x / 100 * cols), the last column closed on the right (include/soundscope_hip.h)
inline uint32_t spectrum_column_of(double chart_x, uint32_t cols)
{
    double f = std::floor(chart_x / 100.0 * (double)cols);
    if (f < 0) f = 0;
    return f >= (double)cols ? cols - 1 : (uint32_t)f;
}
// The chart's column map of bt's bins (chart_x ascends).  Starts: column c owns the bins [start[c], start[c + 1]), cols <= 65536.
// Tables, cols <= 512: bin_col[stride], the column of bins [0, count) and 0xFFFF behind them; col_init[cols], -inf where the column
// owns a bin and a quiet NaN where it owns none (ss_chart_dev.h).
SS_HIDDEN std::vector<uint32_t> column_starts(const BinTables &bt, uint32_t cols);
struct ColumnTables { std::vector<uint16_t> bin_col; std::vector<float> col_init; };
SS_HIDDEN ColumnTables column_tables(const BinTables &bt, uint32_t cols, size_t stride);

// run-in of a time segment that starts from a zero filter state, in 100 ms sub-blocks.  What the missing history would
// have contributed to the OUTPUT is the tail of the K-weighting impulse response: the slowest pole pair (38 Hz high-pass,
// |p| = 0.99502 at 48 kHz, a near-double pole) decays by e^-23.9 per sub-block, times a polynomial factor ~ (1 + 24 n).
// Measured on adversarial material (DC offset plus a strong 7 Hz component, every segment one sub-block long): sub-block
// energies within 2.7e-10 of a sequential f64 filter with a one-sub-block run-in, 1.6e-10 with two — both at the
// arithmetic noise of the recurrence on such material (tools: tests/test_gpu_bench_shapes.py
// ::test_segmented_run_in_on_dc_offset_material pins the histograms).  One sub-block it is: the run-in is redundant work
// (config 5: 4 instead of 5 sub-blocks per 3-sub-block segment).
constexpr uint32_t kTdWarmSub = 1;
// sub-blocks at the head of a time segment > 0 that the fix-up launch re-runs from the exact incoming state.  Behind them the main
// launch's trajectory (zero state at the segment's start) differs from the true one by A^n s: e^-48 (1 + 48) ~ 7e-20 of the state
// after 0.2 s — on the DC-offset torture material (state 4e4 x the offset) 1e-13 of the filtered signal, under the 2e-11 at which any
// two orders of evaluating this recurrence differ (measured: exact whole-stream path vs one-segment path, profiles/r05_ab_td_handover.txt)
constexpr uint32_t kTdFixSub = 2;

SS_HIDDEN int meter_args_ok(uint32_t channels, uint32_t rate);

// The live loudness meter of n streams, laid out per stream as [stream][...]: a handle holds one (n = 1), a meter bank one of n.
struct SS_HIDDEN MeterStore {
    // sub-block ring slots per stream: calls are cut into pieces of at most 32 sub-blocks, so the ring always holds the thirty
    // sub-blocks a short-term block reads
    static constexpr uint32_t kSubCap = 96;
    TdTables *td = nullptr;
    const double *hist_energies = nullptr, *hist_bounds = nullptr;      // the gate's histogram tables (get_hist_tables)
    int tp_factor = 0;                   // effective
    uint32_t n = 0, channels = 0, rate = 0;
    uint64_t s100 = 0;                   // frames per 100 ms sub-block
    uint64_t ring_frames = 0;            // the filtered-sample ring: 3 s rounded up to a whole sub-block
    bool st_on = false;                  // thirty sub-blocks fit the ring (otherwise the crate has no short-term blocks at this rate)
    DevBuf<ssk::TdState> state;          // [n]
    DevBuf<uint64_t> hist;               // [n][2][1000]
    DevBuf<double> sub, ring, weights;   // [n][kSubCap][C], [n][ring_frames][C], [C]
    DevBuf<uint32_t> counts;             // [n][2]

    static uint64_t ring_frames_for(uint32_t rate);
    // a call is cut into pieces of at most 32 sub-blocks (the 96-slot sub-block ring then always holds a short-term block's thirty)
    static uint64_t piece_frames_for(uint64_t s100) { return 32 * s100; }
    // the effective true-peak factor of a meter (tp_cfg 0: the crate's rule for the rate)
    static int true_peak_factor_for(uint32_t rate, int tp_cfg);
    // EbuR128::new for n streams into a FRESH store: argument checks, tables, geometry, buffers, weights (tp_cfg: the true-peak
    // factor, 0 = the crate's rule for the rate).  Nothing else is touched, so a caller that must keep its meter on failure builds
    // into a local store and moves it in on success.
    int build(uint32_t n_streams, uint32_t channels, uint32_t rate, int tp_cfg);
    // a streaming call of `frames` frames of every stream (stream s at pcm + s * stream_stride) on the meter: one time segment, the
    // sub-block and filtered-sample rings.  The caller sets tp_f32 (and a tick's short-term fields).
    ssk::TdParams td_params(const float *pcm, uint64_t stream_stride, uint64_t frames) const;
    ssk::MeterBankParams bank_params() const;
    // the gating of stream 0's sub-blocks [sub_begin, sub_end) (ssk::launch_finalize_stream: the handle)
    ssk::FinalizeParams stream_gating(uint64_t sub_begin, uint64_t sub_end) const;
};

// The FftBatchParams fields that follow from a spectrum plan and the tables: the tables (the N = 16384 core twiddles included),
// n and windows_per_block, the bins of bt in rows padded to four (16-B aligned), the dB offset and, for the N = 4096 forms, offpink
// and publish_mask.  pink: the rows carry the pink compensation (batches); otherwise raw dBFS (a handle adds it in f64 on the host).
SS_HIDDEN ssk::FftBatchParams spectrum_params(const ssk::SpecPlan &plan, const FftTables &ft, const BinTables &bt, bool pink);
// One window of ft.n points of one stream (ss_get_fft, the ticks, the meter banks: their rows agree bit for bit) is a batch of one
// stream and one window at this hop: plan it with ssk::plan_spectrum(n, channels, kOneWindowHop, 1, 1).
constexpr uint32_t kOneWindowHop = 1024;
// spectrum_params in raw dBFS for that one window; the caller sets pcm, out, channels and the window's start
SS_HIDDEN ssk::FftBatchParams one_window_fft(const ssk::SpecPlan &plan, const FftTables &ft, const BinTables &bt);

}  // namespace ssh

// ============================================================================
//  handle
// ============================================================================
struct ss_analyzer {
    int device = 0;            // the HIP device this handle's buffers live on
    uint32_t rate = 0;         // sticks on a failed configure (meter.rate: the rate the current meter was built for)
    int tp_cfg = 0;            // 0 = crate rule
    int tp_arith = SS_TP_ARITH_F32;   // ss_analyzer_set_true_peak_arith
    int tp_cfg_applied = 0;    // the tp_cfg the current meter was built with
    bool meter_ok = false;
    hipStream_t stream = nullptr;
    ssh::MeterStore meter;               // one stream
    ssh::DevBuf<double> out2, ring_scratch;
    ssh::DevBuf<float> in;
    // get_fft(&self): the handle is const at the boundary; the payload of the last error (ss_get_fft_error_values) and the
    // page-locked mailboxes below are the call's own scratch
    mutable float fft_err_a = 0.0f, fft_err_b = 0.0f;
    uint64_t frames_fed = 0;
    // The reference's render loop asks for the integrated loudness, the loudness range and the true peak on EVERY frame (tui.rs:917,
    // :950, :969; a frame every 8 ms, a tick every 21): a reading is taken from the device once per state of the meter —
    // `change_count` moves with every feed, reset and re-configuration — and handed out from here until the state moves again.
    uint64_t change_count = 1;
    uint64_t eval_stamp = 0, peaks_stamp = 0;               // (both readings are taken together: one wait)
    double eval_cache[2] = {0.0, 0.0};                       // (integrated, range) at eval_stamp
    float peaks_cache[2 * ssk::kMaxChannels] = {};          // sample peaks | true peaks at peaks_stamp
    // Small calls — a tick through the Analyzer API: get_fft x 2, add_samples, get_shortterm_lufs on 16384 samples — move no
    // data with pageable copy commands and read-backs (a pageable 64 KB hipMemcpyAsync blocks the caller and costs more than the
    // kernel behind it): the samples are copied by the host into page-locked memory, from where ONE DMA takes them to HBM (the
    // kernels read their input in small pieces: in place over PCIe that cost them 10-14 us), and results are written by the
    // kernels into page-locked memory (PinBuf::dev).  Two input stages, so that add_samples returns behind its launches; every call
    // that waits for the stream frees both.  All of them are allocated together at first use (pin_ready, ss_analyzer.cpp).
    static constexpr size_t kPinFloats = 32768;
    ssh::HostStage pin_in[2];                                // kPinFloats floats each
    int pin_next = 0;
    hipEvent_t ring_ev = nullptr;                            // a ring reading (short-term / momentary) is there
    bool pin_ok = false;                                     // pin_ready has got all of them
    ssh::PinBuf<float> pin_out;                              // kPinFloats / 2 + 1 dB values
    ssh::PinBuf<double> pin_d;                               // a getter's pair of doubles
    ssh::PinBuf<float> pin_peaks;                            // 2 * kMaxChannels floats: the state's peaks, copied there
    ssh::PinBuf<double> pin_eval;                            // (integrated, range) of the state the readings were last asked for
    ssh::PinBuf<uint32_t> pin_flag;                          // the readings launch stores its number there, last
    uint32_t readings_seq = 0;                               // readings launches so far
    uint64_t prefetch_stamp = 0;                             // change_count the launch in flight is of (0: none)
};

namespace ssh {
// ss_analyzer.cpp: pieces of the handle the batch one-shot and the tick drivers reuse
SS_HIDDEN int handle_reset(ss_analyzer *h);
// enqueue (no wait) the readings the reference's render loop asks for on every frame — integrated loudness and range, every
// channel's peaks — behind whatever has just changed the meter's state: the getters then find them waiting
SS_HIDDEN int prefetch_readings(ss_analyzer *h, bool on_demand = false);      // on_demand: a getter asking (never switched off)
// the same riding a gating launch that is about to be enqueued on h->stream (k_finalize_stream takes the readings behind its
// histogram updates): fills the launch's fields and marks the readings as on their way
SS_HIDDEN int attach_readings(ss_analyzer *h, ssk::FinalizeParams *gating);
// add_frames_f32 on the handle's meter; on_device: `samples` already lives in HBM (nothing is copied or waited for)
// `deferred`: a single-piece device-resident call hands the gating launch (k_finalize_stream) of its new sub-blocks back to the
// caller instead of enqueueing it (n_streams != 0: launch it with ssk::launch_finalize_stream on h->stream before anything else reads the
// histograms) — the tick drivers put the short-term reading in front of it
// `tick`: what a tick wants to ride the launch of a single-piece device-resident call (ssk::launch_time_domain / k_tick): its
// spectrum, and the short-term reading of the window that ends with the call; `fused` tells whether both did — if not, neither
// was launched
struct TickExtras {
    const ssk::FftBatchParams *fft = nullptr;   // nullptr: no spectrum this tick (then nothing is fused)
    double *shortterm_out = nullptr;            // (energy, loudness), device-visible; nullptr: no reading wanted
    bool fused = false;                         // out: the spectrum rode the loudness call's launch (k_tick)
    bool st_fused = false;                      // out: ... and so did the short-term reading (its window parameters were set)
};
SS_HIDDEN int add_samples_impl(ss_analyzer *h, const float *samples, size_t n, bool on_device, ssk::FinalizeParams *deferred = nullptr,
                               TickExtras *tick = nullptr);
SS_HIDDEN int ring_loudness_enqueue(ss_analyzer *h, uint64_t frames, double *out2_dev = nullptr);   // out2_dev: where (energy, loudness) go — default the handle's device pair; the tick drivers pass mapped pinned memory
SS_HIDDEN void waveform_shape(size_t n, double waveform_window, size_t *window_out, size_t *bins_out);
// ss_batch.cpp: Analyzer::calculate_integrated_lufs on a host or device-resident buffer (a one-stream batch pass)
SS_HIDDEN int integrated_oneshot(uint32_t rate, uint32_t channels, const float *samples, size_t n, bool on_device, double *out);
}  // namespace ssh
