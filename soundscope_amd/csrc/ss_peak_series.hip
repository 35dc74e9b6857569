// ss_peak_series.hip: the true and sample peak of every 100 ms entry of every stream of a batch, with the frame that attains each
// (ss_batch_peak_series), and their maxima over time ranges and groups of ranges (ss_batch_peak_regions) — hand-written gfx950
// (CDNA4, wave64) kernels.  Not in the reference: its meter keeps one pair of peaks per channel for the whole stream.
// Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.3.2.
//
// k_peak_series: one workgroup per (stream, entry) owns the entry's records of every channel.  It walks the entry in tiles of
// plan.tile_frames frames: the tile's floats and the taps - 1 frames in front of it (zeros in front of the stream's own frame 0)
// are one contiguous run of the corpus, copied into LDS as it lies (16-byte loads on the aligned inside of the run, guarded
// 4-byte loads at its ends: no float outside the run is read, so neither the stream in front nor anything behind the stream's own
// length).  A lane then takes runs of kPeakRun consecutive frames of one channel: it reads the run and its history once into
// registers and forms every branch of every frame as one chain of plain v_fma_f32, oldest tap first.  Value and position travel
// together as (float bits << 32 | ~frame): every captured value is positive, so the integer order is the float order with ties to
// the lowest frame, and zero reads "0 at 0xFFFFFFFF".  The lanes' words meet in LDS (ds_max_u64); global memory sees plain 16-byte
// stores only.  The tile copy and the interpolator (peak_load_tile, peak_frame_max) live in ss_peak_dev.h, which the limiter's
// detector shares.
#include "ss_kernels.h"
#include "ss_peak_dev.h"

namespace ssk {

namespace {

constexpr int kPeakRun = 25;                // frames a lane takes at a time: odd, so the lanes of a wave spread over the LDS banks
constexpr uint32_t kPeakTileFloats = 8192;  // floats of one tile's own frames at most (32 KB of LDS)

__device__ __forceinline__ unsigned long long peak_key(float v, uint32_t frame)
{
    return (unsigned long long)__float_as_uint(v) << 32 | (0xFFFFFFFFu - frame);
}

}  // namespace

// NT: taps of a branch (12 at factor 4, 24 at factor 2, 0: sample peak only); NB: interpolated branches (factor - 1)
template <int NT, int NB>
__global__ __launch_bounds__(kPeakThreads) void k_peak_series(PeakSeriesParams p)
{
    extern __shared__ float4 sh4[];
    __shared__ unsigned long long best[2][kMaxChannels];        // [true, sample][channel]
    float *sh = reinterpret_cast<float *>(sh4);
    constexpr int H = NT ? NT - 1 : 0;
    const uint32_t stream = blockIdx.x / p.entries_cap, entry = blockIdx.x - stream * p.entries_cap;
    const uint32_t C = p.channels, S = p.s100, T = p.tile_frames;
    unsigned long long F = p.frames_of ? p.frames_of[stream] : p.n_frames;
    if (F > p.n_frames) F = p.n_frames;
    const unsigned long long e_begin = (unsigned long long)entry * S;
    if (e_begin >= F) return;                                   // (the whole workgroup: entry >= E_s)
    const unsigned long long e_end = e_begin + S < F ? e_begin + S : F;
    const uint32_t e_frames = (uint32_t)(e_end - e_begin);
    const long long base = (long long)((unsigned long long)stream * p.stream_stride);      // the stream's frame 0, in floats
    if (threadIdx.x < 2u * kMaxChannels) best[threadIdx.x >> 6][threadIdx.x & 63u] = 0ull;
    // the taps live in vector registers (read back from LDS): 36 scalar registers beside the parameters would spill
    __shared__ float tap_s[36];
    if (threadIdx.x < (uint32_t)(NB * NT)) tap_s[threadIdx.x] = p.taps[threadIdx.x];
    __syncthreads();
    float tap[NB ? NB : 1][NT ? NT : 1];
#pragma unroll
    for (int f = 0; f < NB; f++)
#pragma unroll
        for (int d = 0; d < NT; d++) tap[f][d] = tap_s[f * NT + d];

    for (uint32_t t0 = 0; t0 < e_frames; t0 += T) {
        const uint32_t tn = e_frames - t0 < T ? e_frames - t0 : T;
        // floats [g0, g1): frames [e_begin + t0 - H, e_begin + t0 + tn) of the stream; the copy starts at the 16-byte line of g0
        const long long g0 = base + ((long long)(e_begin + t0) - H) * (long long)C, g1 = base + (long long)(e_begin + t0 + tn) * (long long)C;
        const uint32_t shift = (uint32_t)(g0 & 3ll);
        const long long first = g0 - shift;
        const uint32_t n4 = (uint32_t)((g1 - first + 3) >> 2);
        __syncthreads();                                        // the tile before this one has been read (and `best` is cleared)
        peak_load_tile(sh, p.pcm, first, base > g0 ? base : g0, g1, n4);
        __syncthreads();
        const float *x0 = sh + shift;                           // x0[(H + k) * C + c] = frame t0 + k of the tile, channel c
        const uint32_t runs = (tn + kPeakRun - 1) / kPeakRun, items = runs * C;
        for (uint32_t item = threadIdx.x; item < items; item += kPeakThreads) {
            const uint32_t run = item / C, c = item - run * C;
            const uint32_t a = run * kPeakRun;                  // first frame of the run in the tile
            const uint32_t cnt = tn - a < (uint32_t)kPeakRun ? tn - a : (uint32_t)kPeakRun;
            const float *xr = x0 + (size_t)a * C + c;
            float tb = 0.f, sb = 0.f;
            uint32_t tk = 0, sk = 0;
            if (cnt == (uint32_t)kPeakRun) {
                float w[H + kPeakRun];                          // frames a - H .. a + kPeakRun - 1, each read once
#pragma unroll
                for (int i = 0; i < H + kPeakRun; i++) w[i] = xr[(size_t)i * C];
#pragma unroll
                for (int k = 0; k < kPeakRun; k++) {
                    const float ax = fabsf(w[H + k]), v = peak_frame_max<NT, NB>(tap, w + k);
                    if (ax > sb) { sb = ax; sk = (uint32_t)k; }
                    if (v > tb) { tb = v; tk = (uint32_t)k; }       // NaN: never captured
                }
            } else {                                            // the last run of a tile: the window moves through registers
                float w[H + 1];
#pragma unroll
                for (int i = 0; i < H; i++) w[i] = xr[(size_t)i * C];
                for (uint32_t k = 0; k < cnt; k++) {
                    w[H] = xr[(size_t)(H + k) * C];
                    const float ax = fabsf(w[H]), v = peak_frame_max<NT, NB>(tap, w);
                    if (ax > sb) { sb = ax; sk = k; }
                    if (v > tb) { tb = v; tk = k; }
#pragma unroll
                    for (int i = 0; i < H; i++) w[i] = w[i + 1];
                }
            }
            const uint32_t at = t0 + a;                         // the run's first frame in the entry
            if (tb > 0.f) atomicMax(&best[0][c], peak_key(tb, at + tk));
            if (sb > 0.f) atomicMax(&best[1][c], peak_key(sb, at + sk));
        }
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const unsigned long long kt = best[0][threadIdx.x], ks = best[1][threadIdx.x];
        // the record leaves (and k_region_peaks reads it) as one 16-byte word: x, y, z, w are ss_peak_entry's four fields in order
        static_assert(offsetof(ss_peak_entry, sample_peak) == 4 && offsetof(ss_peak_entry, true_peak_frame) == 8 &&
                      offsetof(ss_peak_entry, sample_peak_frame) == 12, "peak entry as a uint4");
        uint4 rec;
        rec.x = (uint32_t)(kt >> 32); rec.y = (uint32_t)(ks >> 32);
        rec.z = 0xFFFFFFFFu - (uint32_t)kt; rec.w = 0xFFFFFFFFu - (uint32_t)ks;
        reinterpret_cast<uint4 *>(p.series)[((size_t)stream * p.entries_cap + entry) * C + threadIdx.x] = rec;
    }
}

// How an entry is cut into tiles: as few tiles as keep a tile's own frames within kPeakTileFloats floats, of equal length.
PeakSeriesPlan plan_peak_series(uint32_t channels, uint32_t s100, uint64_t n_frames)
{
    PeakSeriesPlan plan;
    const uint32_t most = kPeakTileFloats / (channels ? channels : 1u);         // >= 128 frames (64 channels)
    const uint32_t tiles = (s100 + most - 1u) / most;
    plan.tile_frames = tiles ? (s100 + tiles - 1u) / tiles : 1u;
    const uint64_t cap = s100 ? (n_frames + s100 - 1u) / s100 : 0u;
    plan.entries_cap = cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap;
    return plan;
}

hipError_t launch_peak_series(const PeakSeriesParams &p, hipStream_t s)
{
    const uint64_t groups = (uint64_t)p.n_streams * p.entries_cap;
    if (!groups) return hipSuccess;
    if (groups > 0x7FFFFFFFull || !p.channels || p.channels > (uint32_t)kMaxChannels || !p.tile_frames || !p.s100 ||
        (uint64_t)p.tile_frames * p.channels > kPeakTileFloats)
        return hipErrorInvalidValue;
    const int nt = p.factor == 4 ? 12 : p.factor == 2 ? 24 : 0;
    // the tile, its history and the copy's alignment at both ends: in float4
    const size_t floats = (size_t)(p.tile_frames + (nt ? nt - 1 : 0)) * p.channels + 8;
    const size_t lds = (floats + 3) / 4 * sizeof(float4);
    const dim3 grid((uint32_t)groups), block(kPeakThreads);
    if (p.factor == 4) hipLaunchKernelGGL((k_peak_series<12, 3>), grid, block, lds, s, p);
    else if (p.factor == 2) hipLaunchKernelGGL((k_peak_series<24, 1>), grid, block, lds, s, p);
    else if (p.factor == 0) hipLaunchKernelGGL((k_peak_series<0, 0>), grid, block, lds, s, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ============================================================================
//  Peak regions (ss_batch_peak_regions): maxima of the series over runs of one stream's entries, pooled into groups
// ============================================================================
// One workgroup per region (s, a, n): a lane takes entries a + tid, a + tid + 256, ... and walks their channels, so it meets its
// candidates in the order of the tie rule (entry, then frame, then channel) and keeps the first of the largest.  The workgroup
// then agrees on the largest value (ds_max_u32 on the float's bits) and, among the lanes that hold it, on the smallest
// (absolute frame << 6 | channel) (ds_min_u64); per-channel maxima, the count of entries over the ceiling and the first of them
// meet in LDS the same way.  The region's group receives (value bits << 32 | ~region index) with a 64-bit integer maximum and the
// count with an integer add: integers only, so the order in which regions arrive does not show.
__global__ __launch_bounds__(256) void k_region_peaks(RegionPeaksParams p)
{
    __shared__ uint32_t ch_max[2][kMaxChannels];
    __shared__ uint32_t top[2], n_over_s, first_over_s;
    __shared__ unsigned long long where[2];
    const LoudnessRegion rg = p.regions[blockIdx.x];
    const uint32_t tid = threadIdx.x, C = p.channels;
    if (tid < 2u * kMaxChannels) ch_max[tid >> 6][tid & 63u] = 0u;
    if (tid < 2u) { top[tid] = 0u; where[tid] = ~0ull; }
    if (tid == 0u) { n_over_s = 0u; first_over_s = 0xFFFFFFFFu; }
    __syncthreads();
    const uint4 *ser = reinterpret_cast<const uint4 *>(p.series) + (size_t)rg.stream * p.entries_cap * C;
    const uint32_t end = rg.first_subblock + rg.n_subblocks;
    float bv[2] = {0.f, 0.f};
    unsigned long long bw[2] = {~0ull, ~0ull};
    uint32_t over = 0u, first_over = 0xFFFFFFFFu;
    for (uint32_t j = rg.first_subblock + tid; j < end; j += 256u) {
        bool is_over = false;
        const unsigned long long f0 = (unsigned long long)j * p.s100;
        for (uint32_t c = 0; c < C; c++) {
            const uint4 r = ser[(size_t)j * C + c];
            const float v[2] = {__uint_as_float(r.x), __uint_as_float(r.y)};
            const uint32_t at[2] = {r.z, r.w};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (v[k] > 0.f) atomicMax(&ch_max[k][c], __float_as_uint(v[k]));
                const unsigned long long w = (f0 + at[k]) << 6 | c;
                if (v[k] > bv[k] || (v[k] == bv[k] && v[k] > 0.f && w < bw[k])) { bv[k] = v[k]; bw[k] = w; }
            }
            is_over = is_over || (double)v[0] > p.ceiling;
        }
        if (is_over) { over++; if (j < first_over) first_over = j; }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) if (bv[k] > 0.f) atomicMax(&top[k], __float_as_uint(bv[k]));
    if (over) { atomicAdd(&n_over_s, over); atomicMin(&first_over_s, first_over); }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; k++) if (bv[k] > 0.f && __float_as_uint(bv[k]) == top[k]) atomicMin(&where[k], bw[k]);
    __syncthreads();
    if (tid < C) {
        p.ch_true[(size_t)blockIdx.x * C + tid] = __uint_as_float(ch_max[0][tid]);
        p.ch_sample[(size_t)blockIdx.x * C + tid] = __uint_as_float(ch_max[1][tid]);
    }
    if (tid == 0u) {
        RegionPeaks out;
        const bool has_t = top[0] != 0u, has_s = top[1] != 0u;
        out.true_peak = (double)__uint_as_float(top[0]); out.sample_peak = (double)__uint_as_float(top[1]);
        out.true_peak_frame = has_t ? where[0] >> 6 : ~0ull; out.sample_peak_frame = has_s ? where[1] >> 6 : ~0ull;
        out.true_peak_channel = has_t ? (uint32_t)(where[0] & 63ull) : 0xFFFFFFFFu;
        out.sample_peak_channel = has_s ? (uint32_t)(where[1] & 63ull) : 0xFFFFFFFFu;
        out.n_over = n_over_s; out.first_over = first_over_s;
        p.results[blockIdx.x] = out;
        if (rg.group != kRegionNoGroup) {
            unsigned long long *acc = p.group_acc + (size_t)rg.group * 3;
            const unsigned long long inv = 0xFFFFFFFFu - blockIdx.x;
            if (has_t) atomicMax(&acc[0], (unsigned long long)top[0] << 32 | inv);
            if (has_s) atomicMax(&acc[1], (unsigned long long)top[1] << 32 | inv);
            if (n_over_s) atomicAdd(&acc[2], (unsigned long long)n_over_s);
        }
    }
}

// behind the regions: one lane per group turns the group's words into its record
__global__ __launch_bounds__(256) void k_group_peaks(RegionPeaksParams p)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= p.n_groups) return;
    const unsigned long long *acc = p.group_acc + (size_t)g * 3;
    GroupPeaks out;
    out.true_peak = (double)__uint_as_float((uint32_t)(acc[0] >> 32)); out.sample_peak = (double)__uint_as_float((uint32_t)(acc[1] >> 32));
    out.true_peak_region = acc[0] ? 0xFFFFFFFFu - (uint32_t)acc[0] : 0xFFFFFFFFu;
    out.sample_peak_region = acc[1] ? 0xFFFFFFFFu - (uint32_t)acc[1] : 0xFFFFFFFFu;
    out.n_over = acc[2];
    p.group_results[g] = out;
}

hipError_t launch_region_peaks(const RegionPeaksParams &p, hipStream_t s)
{
    if (p.n_regions >> 31 || p.n_groups >> 31 || !p.channels || p.channels > (uint32_t)kMaxChannels) return hipErrorInvalidValue;
    if (p.n_groups) {
        hipError_t e = hipMemsetAsync(p.group_acc, 0, (size_t)p.n_groups * 3 * sizeof(unsigned long long), s);
        if (e != hipSuccess) return e;
    }
    if (p.n_regions) hipLaunchKernelGGL(k_region_peaks, dim3(p.n_regions), dim3(256), 0, s, p);
    if (p.n_groups) hipLaunchKernelGGL(k_group_peaks, dim3((p.n_groups + 255u) / 256u), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace ssk
