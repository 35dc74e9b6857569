// ss_spectrum_stats.hip: per-stream average and peak-hold spectrum of a batch pass's rows (ss_batch_spectrum_stats), and the same
// pooled over the batch (ss_batch_corpus_spectrum) — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference: it shows
// one spectrum at a time.  Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.6.
//
// The kernels know the row layout only — rows[stream][window][fft_channel][bin_stride] f32 dB — so they serve every spectrum
// kernel's rows.  A (stream, fft_channel) is a PAIR; a lane owns one group of four consecutive bins of a pair and walks the windows
// of its chunk in index order, so a wave-instruction reads 1 KB of one row and nothing is shared between lanes: no LDS, no
// barrier, no atomics.  Every sum has one fixed order (windows inside a chunk, then chunks, then streams, each by index): two
// launches over the same rows agree bit for bit.
//
// ss_spectrum_regions.hip runs the same sweep over time ranges of the streams; what the two share is in ss_spectrum_stats_dev.h.
#include "ss_spectrum_stats_dev.h"

namespace ssk {

namespace {

constexpr uint32_t kStatsWaves = 2048;      // waves the sweep wants at least (eight per CU, 8 KB of loads in flight each)
constexpr uint32_t kStatsMinChunk = 16;     // windows a chunk holds at least: two full rounds of kStatsDepth loads
// windows of a stream: its own count under ss_batch_set_lengths, never more than the slot holds
__device__ __forceinline__ uint32_t stats_windows_of(const SpecStatsParams &p, uint32_t stream)
{
    const uint32_t nw = p.windows_of ? p.windows_of[stream] : p.n_windows;
    return nw < p.n_windows ? nw : p.n_windows;
}

}  // namespace

// One wave per (pair, chunk, slice of 64 bin groups).  plan.chunks == 1: the wave holds the pair's whole sums and stores the
// results; otherwise it stores its chunk's partial sums for k_spectrum_stats_combine — a chunk that starts behind the stream's own
// window count stores nothing, and the combine does not read it.
__global__ __launch_bounds__(256) void k_spectrum_stats(SpecStatsParams p)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t per_pair = p.plan.slices * p.plan.chunks;
    const uint32_t pairs = p.n_streams * p.fft_ch;
    if (item >= (uint64_t)pairs * per_pair) return;
    const uint32_t pair = (uint32_t)(item / per_pair), rest = (uint32_t)(item - (uint64_t)pair * per_pair);
    const uint32_t chunk = rest / p.plan.slices, slice = rest - chunk * p.plan.slices;
    const uint32_t g = slice * 64u + lane;                      // group of four bins
    if (g >= p.bin_stride / 4u) return;
    const uint32_t stream = pair / p.fft_ch, ch = pair - stream * p.fft_ch;
    const uint32_t nw = stats_windows_of(p, stream);
    const uint32_t w_begin = chunk * p.plan.chunk_windows;
    const uint32_t w_end = nw - w_begin < p.plan.chunk_windows ? nw : w_begin + p.plan.chunk_windows;      // (used only where w_begin < nw)
    const bool chunked = p.plan.chunks > 1u;
    if (chunked && w_begin >= nw) return;
    const size_t window_stride = (size_t)p.fft_ch * p.bin_stride;
    const float *src = p.rows + ((size_t)stream * p.n_windows * p.fft_ch + ch) * p.bin_stride + 4u * g;    // window 0's group
    BinStats a;
    stats_clear(a);
    uint32_t w = w_begin;
    if (w_begin < nw) {
        for (; w + kStatsDepth <= w_end; w += kStatsDepth) {
            float4 v[kStatsDepth];
#pragma unroll
            for (int k = 0; k < kStatsDepth; k++) v[k] = *reinterpret_cast<const float4 *>(src + (size_t)(w + k) * window_stride);
#pragma unroll
            for (int k = 0; k < kStatsDepth; k++) stats_add(a, v[k]);
        }
        for (; w < w_end; w++) stats_add(a, *reinterpret_cast<const float4 *>(src + (size_t)w * window_stride));
    }
    if (!chunked) {
        stats_write_results(p, (size_t)pair * p.bin_stride + 4u * g, 4u * g, a);
        return;
    }
    stats_write_parts(p, ((size_t)pair * p.plan.chunks + chunk) * p.bin_stride + 4u * g, a);
}

// chunked plans, behind k_spectrum_stats on the same stream: one lane per (pair, bin group) adds the chunks the stream's own
// window count reaches, in chunk order
__global__ __launch_bounds__(256) void k_spectrum_stats_combine(SpecStatsParams p)
{
    const uint32_t groups = p.bin_stride / 4u;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)p.n_streams * p.fft_ch * groups) return;
    const uint32_t pair = (uint32_t)(idx / groups), g = (uint32_t)(idx - (uint64_t)pair * groups);
    const uint32_t nw = stats_windows_of(p, pair / p.fft_ch);
    const uint32_t chunks = (nw + p.plan.chunk_windows - 1u) / p.plan.chunk_windows;        // (<= plan.chunks: nw <= n_windows)
    BinStats a;
    stats_clear(a);
    const size_t first = (size_t)pair * p.plan.chunks * p.bin_stride + 4u * g;
#pragma unroll 4
    for (uint32_t c = 0; c < chunks; c++) stats_add_parts(a, p, first + (size_t)c * p.bin_stride);
    stats_write_results(p, (size_t)pair * p.bin_stride + 4u * g, 4u * g, a);
}

// The batch pooled: one lane per (fft_channel, bin) adds the streams' power sums and counts in stream order — every counted window
// of every stream weighs the same — and takes the maximum of their maxima.  counts[r]: the pooled count at bin 0.
__global__ __launch_bounds__(256) void k_spectrum_stats_corpus(SpecStatsParams p, float *mean, float *max, unsigned long long *counts)
{
    const uint32_t per_stream = p.fft_ch * p.bin_stride;
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;          // element of a stream's [fft_channel][bin_stride]
    if (idx >= per_stream) return;
    double sum = 0.0;
    float mx = __builtin_nanf("");
    unsigned long long n = 0;
#pragma unroll 8
    for (uint32_t s = 0; s < p.n_streams; s++) {
        const size_t at = (size_t)s * per_stream + idx;
        sum += p.sums[at];
        mx = fmaxf(mx, p.max[at]);
        n += p.counts[at];
    }
    mean[idx] = stats_mean_db(sum, n);
    max[idx] = mx;
    if (idx % p.bin_stride == 0) counts[idx / p.bin_stride] = n;
}

// How the sweep cuts a batch: slices of 64 bin groups per row, and the windows in chunks where (pairs x slices) waves alone would
// leave most of the chip idle (one long file: 2 pairs, tens of thousands of windows) — as many chunks as bring the grid to
// kStatsWaves waves, none shorter than kStatsMinChunk windows.  The bench shape (2048 pairs x 7 slices) is one chunk.
SpecStatsPlan plan_spectrum_stats(uint32_t pairs, uint32_t bin_stride, uint32_t n_windows)
{
    SpecStatsPlan plan;
    plan.slices = (bin_stride / 4u + 63u) / 64u;
    const uint64_t waves = (uint64_t)pairs * plan.slices;
    const uint64_t want = waves ? (kStatsWaves + waves - 1) / waves : 1;
    const uint64_t most = n_windows / kStatsMinChunk;
    const uint32_t chunks = (uint32_t)(want < most ? want : most);
    plan.chunk_windows = chunks > 1u ? (n_windows + chunks - 1u) / chunks : (n_windows ? n_windows : 1u);
    plan.chunks = n_windows ? (n_windows + plan.chunk_windows - 1u) / plan.chunk_windows : 1u;
    return plan;
}

hipError_t launch_spectrum_stats(const SpecStatsParams &p, hipStream_t s)
{
    const uint64_t pairs = (uint64_t)p.n_streams * p.fft_ch, groups = p.bin_stride / 4u;
    if (!pairs || !groups) return hipSuccess;
    const uint64_t waves = pairs * p.plan.slices * p.plan.chunks;
    if ((waves + 3) / 4 > 0x7FFFFFFFull || pairs * groups > (0x7FFFFFFFull << 8)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_spectrum_stats, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.plan.chunks <= 1u) return e;
    hipLaunchKernelGGL(k_spectrum_stats_combine, dim3((uint32_t)((pairs * groups + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_spectrum_stats_corpus(const SpecStatsParams &p, float *mean, float *max, unsigned long long *counts, hipStream_t s)
{
    const uint32_t per_stream = p.fft_ch * p.bin_stride;
    if (!per_stream) return hipSuccess;
    hipLaunchKernelGGL(k_spectrum_stats_corpus, dim3((per_stream + 255u) / 256u), dim3(256), 0, s, p, mean, max, counts);
    return hipGetLastError();
}

}  // namespace ssk
