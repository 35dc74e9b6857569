// ss_spectrogram.hip: time x frequency chart tiles of a batch pass's spectra (ss_batch_spectrogram) — hand-written gfx950 (CDNA4,
// wave64) kernels.  Not in the reference: it shows one spectrum at a time.  Definition: include/soundscope_hip.h; plan and figures:
// DESIGN.md section 3.6.2.
//
// Rows form.  The kernel knows the row layout only — rows[stream][window][fft_channel][bin_stride] f32 dB — so it serves every
// spectrum kernel's rows.  A (stream, fft_channel) is a PAIR, a (pair, time column) a UNIT; a workgroup owns one run of a unit's
// windows.  A lane owns one group of four consecutive bins at a time and walks the run's windows with kDepth 16-byte loads in
// flight (a wave-instruction reads 1 KB of one row), carrying fmaxf maxima (maxNum: a NaN value is skipped).  The four maxima are
// then folded into the unit's chart columns in LDS — at most 512 slots and a spare one for the row padding, whatever n_bins is —
// as integer maxima of an order-preserving image of the f32 bits (ds_max_u32; no floating-point atomics).  Gain and clamp are
// applied once per cell behind the fold (ss_chart_dev.h, the NaN-keeping clamp).
// A maximum is exact in any order: runs, their join and two calls agree value for value.
#include "ss_kernels.h"
#include "ss_chart_dev.h"

namespace ssk {

namespace {

constexpr uint32_t kSlots = kSpectrogramMaxFCols;     // chart columns a workgroup folds into; slot kSlots takes the row padding
constexpr int kDepth = 8;                             // windows a lane has in flight
constexpr uint32_t kWantWorkgroups = 1024;            // workgroups the sweep wants at least (four per CU, up to 32 KB of loads in flight each)
constexpr uint32_t kMinRunWindows = 16;               // windows a run holds at least: two full rounds of kDepth loads

// order-preserving image of an f32: a < b <=> key(a) < key(b) as u32, for every pair of non-NaN values (-0 below +0).  0 is the
// image of no value (a NaN of all ones, which is never folded): "none yet".
__device__ __forceinline__ uint32_t key_of(float v)
{
    const uint32_t b = __float_as_uint(v);
    return v == v ? (b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u)) : 0u;
}
__device__ __forceinline__ float value_of(uint32_t k)
{
    return k ? __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)) : __builtin_nanf("");
}

// windows of a stream: its own count under ss_batch_set_lengths, never more than the slot holds
__device__ __forceinline__ uint32_t windows_of(const SpectrogramParams &p, uint32_t stream)
{
    const uint32_t nw = p.windows_of ? p.windows_of[stream] : p.n_windows;
    return nw < p.n_windows ? nw : p.n_windows;
}

// the windows [*wa, *wb) run `run` of time column t reads of a stream with nw windows (empty: *wa >= *wb)
__device__ __forceinline__ void run_windows_of(const SpectrogramParams &p, uint32_t t, uint32_t run, uint32_t nw, uint32_t *wa, uint32_t *wb)
{
    const uint32_t span = p.w_max - p.w_min;
    const uint32_t first = spectrogram_column_first(p.w_min, span, p.t_cols, t);
    uint32_t end = spectrogram_column_first(p.w_min, span, p.t_cols, t + 1u);
    end = end < nw ? end : nw;
    const uint64_t a = (uint64_t)first + (uint64_t)run * p.plan.run_windows, b = a + p.plan.run_windows;
    *wa = a < end ? (uint32_t)a : end;
    *wb = b < end ? (uint32_t)b : end;
}

__device__ __forceinline__ void max4(float m[4], const float4 v)
{
    m[0] = fmaxf(m[0], v.x); m[1] = fmaxf(m[1], v.y); m[2] = fmaxf(m[2], v.z); m[3] = fmaxf(m[3], v.w);
}

}  // namespace

// One workgroup per (unit, run).  plan.runs == 1: it stores the unit's cells; otherwise the images of its run's maxima for
// k_spectrogram_join.  LDS: kSlots + 1 words, whatever the rows' length.
__global__ __launch_bounds__(256) void k_spectrogram_rows(SpectrogramParams p)
{
    __shared__ uint32_t slot[kSlots + 1u];
    const uint32_t runs = p.plan.runs;
    const uint32_t unit = blockIdx.x / runs, run = blockIdx.x - unit * runs;
    const uint32_t pair = unit / p.t_cols, t = unit - pair * p.t_cols;
    const uint32_t stream = pair / p.fft_ch, ch = pair - stream * p.fft_ch;
    uint32_t wa, wb;
    run_windows_of(p, t, run, windows_of(p, stream), &wa, &wb);
    for (uint32_t c = threadIdx.x; c <= kSlots; c += 256u) slot[c] = 0u;
    __syncthreads();
    const uint32_t groups = p.bin_stride / 4u;
    const size_t window_stride = (size_t)p.fft_ch * p.bin_stride;
    const float *row0 = p.rows + ((size_t)stream * p.n_windows * p.fft_ch + ch) * p.bin_stride;     // window 0 of the pair
    for (uint32_t g = threadIdx.x; g < groups && wa < wb; g += 256u) {
        const float *src = row0 + 4u * g;
        float m[4];
#pragma unroll
        for (int e = 0; e < 4; e++) m[e] = __builtin_nanf("");
        uint32_t w = wa;
        for (; w + kDepth <= wb; w += kDepth) {
            float4 v[kDepth];
#pragma unroll
            for (int k = 0; k < kDepth; k++) v[k] = *reinterpret_cast<const float4 *>(src + (size_t)(w + k) * window_stride);
#pragma unroll
            for (int k = 0; k < kDepth; k++) max4(m, v[k]);
        }
        if (w < wb) {           // the run's last windows, all in flight together as well (w and wb are the same in every lane)
            const float nan = __builtin_nanf("");
            float4 v[kDepth];
#pragma unroll
            for (int k = 0; k < kDepth - 1; k++) {
                v[k] = make_float4(nan, nan, nan, nan);
                if (w + k < wb) v[k] = *reinterpret_cast<const float4 *>(src + (size_t)(w + k) * window_stride);
            }
#pragma unroll
            for (int k = 0; k < kDepth - 1; k++) max4(m, v[k]);
        }
        // the chart columns of the four bins: they ascend with the bin, so equal ends mean one column
        const uint2 bc = *reinterpret_cast<const uint2 *>(p.bin_col + 4u * g);
        const uint32_t c[4] = {bc.x & 0xFFFFu, bc.x >> 16, bc.y & 0xFFFFu, bc.y >> 16};
        if (c[0] == c[3]) {
            const float mm = fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3]));
            if (mm == mm) atomicMax(&slot[c[0] < kSlots ? c[0] : kSlots], key_of(mm));
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (m[e] == m[e]) atomicMax(&slot[c[e] < kSlots ? c[e] : kSlots], key_of(m[e]));
        }
    }
    __syncthreads();
    if (runs == 1u) {
        const float gain = chart_gain(p.integrated, stream, p.gain_db);
        float *o = p.out + (size_t)unit * p.f_cols;
        for (uint32_t c = threadIdx.x; c < p.f_cols; c += 256u) o[c] = chart_cell_keep_nan(value_of(slot[c]), gain);
    } else {
        uint32_t *o = p.part + ((size_t)unit * runs + run) * p.f_cols;
        for (uint32_t c = threadIdx.x; c < p.f_cols; c += 256u) o[c] = slot[c];
    }
}

// Columns form: the pass has reduced frequency and applied its gain, so a cell is the maximum over its windows of one stored
// column.  One lane per (unit, run, column); consecutive lanes read consecutive columns of a window.
__global__ __launch_bounds__(256) void k_spectrogram_columns(SpectrogramParams p)
{
    const uint32_t runs = p.plan.runs;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t units = (uint64_t)p.n_streams * p.fft_ch * p.t_cols;
    if (idx >= units * runs * p.f_cols) return;
    const uint32_t c = (uint32_t)(idx % p.f_cols);
    const uint64_t ur = idx / p.f_cols;
    const uint32_t unit = (uint32_t)(ur / runs), run = (uint32_t)(ur - (uint64_t)unit * runs);
    const uint32_t pair = unit / p.t_cols, t = unit - pair * p.t_cols;
    const uint32_t stream = pair / p.fft_ch, ch = pair - stream * p.fft_ch;
    uint32_t wa, wb;
    run_windows_of(p, t, run, windows_of(p, stream), &wa, &wb);
    const size_t window_stride = (size_t)p.fft_ch * p.f_cols;
    const float *src = p.cols + ((size_t)stream * p.n_windows * p.fft_ch + ch) * p.f_cols + c;
    float m = __builtin_nanf("");
    uint32_t w = wa;
    for (; w + kDepth <= wb; w += kDepth) {
        float v[kDepth];
#pragma unroll
        for (int k = 0; k < kDepth; k++) v[k] = src[(size_t)(w + k) * window_stride];
#pragma unroll
        for (int k = 0; k < kDepth; k++) m = fmaxf(m, v[k]);
    }
    for (; w < wb; w++) m = fmaxf(m, src[(size_t)w * window_stride]);
    if (runs == 1u) p.out[idx] = m;
    else p.part[idx] = key_of(m);
}

// plans with runs, behind either kernel on the same stream: one lane per cell joins the runs' maxima; the rows form's gain and
// clamp are applied here
__global__ __launch_bounds__(256) void k_spectrogram_join(SpectrogramParams p)
{
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t units = (uint64_t)p.n_streams * p.fft_ch * p.t_cols;
    if (idx >= units * p.f_cols) return;
    const uint32_t unit = (uint32_t)(idx / p.f_cols), c = (uint32_t)(idx - (uint64_t)unit * p.f_cols);
    const uint32_t *src = p.part + (size_t)unit * p.plan.runs * p.f_cols + c;
    uint32_t k = 0u;
#pragma unroll 4
    for (uint32_t r = 0; r < p.plan.runs; r++) { const uint32_t x = src[(size_t)r * p.f_cols]; k = x > k ? x : k; }
    const float v = value_of(k);
    p.out[idx] = p.columns_form ? v : chart_cell_keep_nan(v, chart_gain(p.integrated, unit / p.t_cols / p.fft_ch, p.gain_db));
}

// How the sweep cuts a view: a workgroup per unit, and the windows of a time column in runs where the units alone would leave
// most of the chip idle (one long file, few time columns) — as many runs as bring the grid to kWantWorkgroups, none shorter than
// kMinRunWindows windows.  The bench shape (2048 pairs) is one run whatever the view.
SpectrogramPlan plan_spectrogram(uint64_t units, uint32_t column_windows)
{
    SpectrogramPlan plan;
    const uint64_t want = units ? (kWantWorkgroups + units - 1) / units : 1;
    const uint64_t most = column_windows / kMinRunWindows;
    const uint32_t runs = (uint32_t)(want < most ? want : most);
    plan.run_windows = runs > 1u ? (column_windows + runs - 1u) / runs : (column_windows ? column_windows : 1u);
    plan.runs = column_windows ? (column_windows + plan.run_windows - 1u) / plan.run_windows : 1u;
    return plan;
}

hipError_t launch_spectrogram(const SpectrogramParams &p, hipStream_t s)
{
    const uint64_t units = (uint64_t)p.n_streams * p.fft_ch * p.t_cols;
    if (!units || !p.f_cols) return hipSuccess;
    if (p.f_cols > kSlots || units > 0x7FFFFFFFull || units * p.plan.runs > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (!p.columns_form) {
        if (!p.bin_stride) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_spectrogram_rows, dim3((uint32_t)(units * p.plan.runs)), dim3(256), 0, s, p);
    } else {
        const uint64_t lanes = units * p.plan.runs * p.f_cols;
        if ((lanes + 255) / 256 > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_spectrogram_columns, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, s, p);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.plan.runs <= 1u) return e;
    hipLaunchKernelGGL(k_spectrogram_join, dim3((uint32_t)((units * p.f_cols + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace ssk
