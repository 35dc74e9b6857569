// ss_bank_spectrum_track.hip: the averaged and the peak-hold spectrum of every row of a meter bank, kept on the device beside the
// history ring (ss_meter_bank_spectrum_track*) — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference: it draws the
// instantaneous row only.  Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.7.3.
//
// The kernels consume the rows and statuses k_meter_bank_spectrum<false> has just stored (rows[row][n_bins] f32 dB, n_bins floats
// apart: not 16-byte aligned at every rate) and know nothing else of the transform.  A row's state is three planes of bin_stride
// (n_bins rounded up to four) entries — P f64, peak f32, age u32, 16 bytes per bin — so a lane that owns four consecutive bins
// moves 32 + 16 + 16 contiguous bytes and a wave-instruction a whole stretch of one plane.  Nothing is shared between lanes.
//
// A row's clock (last, updates) is read by every wave of the row and written by one of them.  It is kept twice: a launch reads one
// copy and writes the other, for EVERY row (an untouched row is copied through), and the host swaps the two — no wave can see the
// clock another wave of the same launch has advanced.
#include "ss_kernels.h"
#include "ss_chart_dev.h"

// hold_db must equal the same IEEE expression evaluated on the host bit for bit: no fused multiply-add anywhere in this file
#pragma clang fp contract(off)

namespace ssk {

namespace {

constexpr float kLog2Of10Over10 = 0.33219280948873623f;      // 10^(v / 10) = 2^(v log2(10) / 10), as k_spectrum_stats forms it

// the three planes of a row's state, from the row's group of four bins `g` on
struct TrackPlanes { double *P; float *peak; uint32_t *age; };
__device__ __forceinline__ TrackPlanes track_planes(const BankTrackParams &p, uint32_t row, uint32_t bin)
{
    unsigned char *st = p.state + (size_t)row * p.bin_stride * 16u;
    return TrackPlanes{reinterpret_cast<double *>(st) + bin, reinterpret_cast<float *>(st + (size_t)p.bin_stride * 8u) + bin,
                       reinterpret_cast<uint32_t *>(st + (size_t)p.bin_stride * 12u) + bin};
}

// The peak-hold curve: a pure function of (peak, age), shared by the update and both read-outs.
__device__ __forceinline__ float track_hold_db(const BankTrackParams &p, float peak, uint32_t age)
{
    const uint64_t over = age > p.hold_frames ? age - p.hold_frames : 0u;
    return (float)((double)peak - p.decay_db_per_s * ((double)over / p.rate));
}

__device__ __forceinline__ float track_avg_db(double P) { return (float)(10.0 * log10(P)); }

// four floats of a row whose rows lie n_bins apart: one 16-byte access where the address allows it.  Bins behind n_bins read 0.
__device__ __forceinline__ void row_load4(const float *rows, size_t at, uint32_t bin, uint32_t n_bins, float v[4])
{
    if ((at & 3u) == 0 && bin + 4u <= n_bins) {
        const float4 x = *reinterpret_cast<const float4 *>(rows + at);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = bin + e < n_bins ? rows[at + e] : 0.0f;
}

__device__ __forceinline__ void row_store4(float *rows, size_t at, uint32_t bin, uint32_t n_bins, const float v[4])
{
    if ((at & 3u) == 0 && bin + 4u <= n_bins) {
        *reinterpret_cast<float4 *>(rows + at) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (bin + e < n_bins) rows[at + e] = v[e];
}

__device__ __forceinline__ uint64_t track_fed(const BankTrackParams &p, uint32_t row)
{
    return p.fed + (p.ahead ? p.ahead[row / p.rows_per_stream] : 0u);
}

}  // namespace

// One wave per (row, slice of 64 groups of four bins).  The row's decision — skipped (nothing arrived, or the row is refused),
// seeded, or advanced by delta frames with weight alpha — is the same in every lane of the wave.
__global__ __launch_bounds__(256) void k_bank_spectrum_track(BankTrackParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t groups = p.bin_stride / 4u, slices = (groups + 63u) / 64u;
    const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (item >= p.n_streams * p.rows_per_stream * slices) return;
    const uint32_t row = item / slices, slice = item - row * slices;
    const BankTrackRow m = p.meta_in[row];
    const uint64_t fed = track_fed(p, row), delta = fed - m.last;
    const bool seed = m.updates == 0u;
    const bool accepted = p.status[row] == 0 && (seed || delta != 0u);
    if (slice == 0u && lane == 0u) {
        BankTrackRow o = m;
        if (accepted) { o.last = fed; o.updates = m.updates == 0xFFFFFFFFu ? m.updates : m.updates + 1u; }
        p.meta_out[row] = o;
    }
    const uint32_t g = slice * 64u + lane;
    if (!accepted || g >= groups) return;
    const uint32_t bin = 4u * g;
    float v[4];
    row_load4(p.rows, (size_t)row * p.n_bins + bin, bin, p.n_bins, v);
    const TrackPlanes s = track_planes(p, row, bin);
    double P[4];
    float peak[4];
    uint32_t age[4];
    if (seed) {
#pragma unroll
        for (int e = 0; e < 4; e++) { P[e] = (double)exp2f(v[e] * kLog2Of10Over10); peak[e] = v[e]; age[e] = 0u; }
    } else {
        const double2 p0 = reinterpret_cast<const double2 *>(s.P)[0], p1 = reinterpret_cast<const double2 *>(s.P)[1];
        const float4 k = *reinterpret_cast<const float4 *>(s.peak);
        const uint4 a = *reinterpret_cast<const uint4 *>(s.age);
        P[0] = p0.x; P[1] = p0.y; P[2] = p1.x; P[3] = p1.y;
        peak[0] = k.x; peak[1] = k.y; peak[2] = k.z; peak[3] = k.w;
        age[0] = a.x; age[1] = a.y; age[2] = a.z; age[3] = a.w;
        const double alpha = -expm1(-(double)delta / (p.rate * p.average_tau_s));      // tau == 0: -expm1(-inf) == 1
        const uint64_t step = delta < 0xFFFFFFFFull ? delta : 0xFFFFFFFFull;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double pw = (double)exp2f(v[e] * kLog2Of10Over10);
            P[e] = P[e] + alpha * (pw - P[e]);
            const uint64_t sum = (uint64_t)age[e] + step;
            const uint32_t aged = sum < 0xFFFFFFFFull ? (uint32_t)sum : 0xFFFFFFFFu;
            const bool captured = v[e] >= track_hold_db(p, peak[e], aged);
            peak[e] = captured ? v[e] : peak[e];
            age[e] = captured ? 0u : aged;
        }
    }
    reinterpret_cast<double2 *>(s.P)[0] = make_double2(P[0], P[1]);
    reinterpret_cast<double2 *>(s.P)[1] = make_double2(P[2], P[3]);
    *reinterpret_cast<float4 *>(s.peak) = make_float4(peak[0], peak[1], peak[2], peak[3]);
    *reinterpret_cast<uint4 *>(s.age) = make_uint4(age[0], age[1], age[2], age[3]);
}

// ss_meter_bank_spectrum_track_reset: the listed streams' rows (streams == nullptr: streams 0 .. count - 1) have no state
__global__ __launch_bounds__(256) void k_bank_spectrum_track_reset(BankTrackRow *meta, const uint32_t *streams, uint32_t count,
                                                                   uint32_t rows_per_stream)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= count * rows_per_stream) return;
    const uint32_t i = idx / rows_per_stream, r = idx - i * rows_per_stream;
    meta[(size_t)(streams ? streams[i] : i) * rows_per_stream + r] = BankTrackRow{0u, 0u, 0u};
}

// The two curves as rows [row][n_bins] f32 dB (either may be null) and every row's count of accepted updates: one lane per
// (row, group of four bins).  A row without state reads NaN.
__global__ __launch_bounds__(256) void k_bank_spectrum_tracked_rows(BankTrackParams p, float *avg, float *hold, uint32_t *updates)
{
    const uint32_t groups = p.bin_stride / 4u;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= p.n_streams * p.rows_per_stream * groups) return;
    const uint32_t row = idx / groups, g = idx - row * groups, bin = 4u * g;
    const uint32_t n = p.meta_in[row].updates;
    if (g == 0u && updates) updates[row] = n;
    float a[4], h[4];
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] = h[e] = __builtin_nanf("");
    if (n) {
        const TrackPlanes s = track_planes(p, row, bin);
        if (avg) {
            const double2 p0 = reinterpret_cast<const double2 *>(s.P)[0], p1 = reinterpret_cast<const double2 *>(s.P)[1];
            a[0] = track_avg_db(p0.x); a[1] = track_avg_db(p0.y); a[2] = track_avg_db(p1.x); a[3] = track_avg_db(p1.y);
        }
        if (hold) {
            const float4 k = *reinterpret_cast<const float4 *>(s.peak);
            const uint4 ag = *reinterpret_cast<const uint4 *>(s.age);
            h[0] = track_hold_db(p, k.x, ag.x); h[1] = track_hold_db(p, k.y, ag.y);
            h[2] = track_hold_db(p, k.z, ag.z); h[3] = track_hold_db(p, k.w, ag.w);
        }
    }
    const size_t at = (size_t)row * p.n_bins + bin;
    if (avg) row_store4(avg, at, bin, p.n_bins, a);
    if (hold) row_store4(hold, at, bin, p.n_bins, h);
}

// The two curves folded into chart columns by k_meter_bank_spectrum<true>'s rule (ss_chart_dev.h): one workgroup per row, x =
// (float)((double)dB + pink) of every bin into its column with lds_fmax (a maximum has no order: the result is exact), gain and
// clamp once per column at the flush.  A column without a bin and a row without state are NaN.
__global__ __launch_bounds__(256) void k_bank_spectrum_tracked_columns(BankTrackParams p, BankTrackColumns c)
{
    __shared__ float acc_mem[2 * 512];
    lds_f32 *acc = (lds_f32 *)acc_mem;
    const uint32_t row = blockIdx.x;
    const uint32_t n = p.meta_in[row].updates;
    if (threadIdx.x == 0 && c.updates) c.updates[row] = n;
    for (uint32_t k = threadIdx.x; k < c.fold.cols; k += 256u) acc[k] = acc[512u + k] = c.fold.col_init[k];
    __syncthreads();
    if (n) {
        const TrackPlanes s = track_planes(p, row, 0u);
        for (uint32_t i = threadIdx.x; i < p.n_bins; i += 256u) {
            const double pink = c.fold.pink[i];
            const uint32_t col = c.fold.bin_col[i];
            const float a = track_avg_db(s.P[i]), h = track_hold_db(p, s.peak[i], s.age[i]);
            lds_fmax(acc + col, (float)((double)a + pink));
            lds_fmax(acc + 512u + col, (float)((double)h + pink));
        }
    }
    __syncthreads();
    const float gain = chart_gain(c.fold, row / p.rows_per_stream);
    for (uint32_t k = threadIdx.x; k < c.fold.cols; k += 256u) {
        const float ka = acc[k], kh = acc[512u + k];
        const bool none = !n || ka != ka;                              // NaN: the column owns no bin
        const size_t at = (size_t)row * c.fold.cols + k;
        if (c.avg) c.avg[at] = none ? __builtin_nanf("") : chart_clamp(ka + gain);
        if (c.hold) c.hold[at] = none ? __builtin_nanf("") : chart_clamp(kh + gain);
    }
}

namespace {

// rows x bin_stride below 2^31: every kernel here indexes (row, group) in 32 bits
bool track_shape_ok(const BankTrackParams &p)
{
    return (uint64_t)p.n_streams * p.rows_per_stream * p.bin_stride < (1ull << 31) && p.bin_stride % 4u == 0 && p.n_bins <= p.bin_stride;
}

}  // namespace

hipError_t launch_bank_spectrum_track(const BankTrackParams &p, hipStream_t s)
{
    const uint32_t n_rows = p.n_streams * p.rows_per_stream;
    if (!n_rows || !p.n_bins) return hipSuccess;
    if (!track_shape_ok(p)) return hipErrorInvalidValue;
    const uint32_t waves = n_rows * ((p.bin_stride / 4u + 63u) / 64u);
    hipLaunchKernelGGL(k_bank_spectrum_track, dim3((waves + 3u) / 4u), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_bank_spectrum_track_reset(BankTrackRow *meta, const uint32_t *streams, uint32_t count, uint32_t rows_per_stream,
                                            hipStream_t s)
{
    const uint64_t n = (uint64_t)count * rows_per_stream;
    if (!n) return hipSuccess;
    if (n >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_spectrum_track_reset, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, meta, streams, count, rows_per_stream);
    return hipGetLastError();
}

hipError_t launch_bank_spectrum_tracked_rows(const BankTrackParams &p, float *avg, float *hold, uint32_t *updates, hipStream_t s)
{
    const uint32_t n_rows = p.n_streams * p.rows_per_stream;
    if (!n_rows || !p.n_bins) return hipSuccess;
    if (!track_shape_ok(p)) return hipErrorInvalidValue;
    const uint32_t items = n_rows * (p.bin_stride / 4u);
    hipLaunchKernelGGL(k_bank_spectrum_tracked_rows, dim3((items + 255u) / 256u), dim3(256), 0, s, p, avg, hold, updates);
    return hipGetLastError();
}

hipError_t launch_bank_spectrum_tracked_columns(const BankTrackParams &p, const BankTrackColumns &c, hipStream_t s)
{
    const uint32_t n_rows = p.n_streams * p.rows_per_stream;
    if (!n_rows || !p.n_bins) return hipSuccess;
    if (!track_shape_ok(p) || c.fold.cols == 0 || c.fold.cols > 512u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_spectrum_tracked_columns, dim3(n_rows), dim3(256), 0, s, p, c);
    return hipGetLastError();
}

}  // namespace ssk
