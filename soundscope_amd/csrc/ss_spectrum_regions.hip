// ss_spectrum_regions.hip: average and peak-hold spectrum of time ranges of the streams and of groups of them
// (ss_batch_spectrum_regions) — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference.  Definition:
// include/soundscope_hip.h; plan and figures: DESIGN.md section 3.6.3.
//
// The sweep of ss_spectrum_stats.hip over regions: a PAIR is a (region, fft_channel), its windows the range [w_first, w_end) of the
// region's stream that the host resolved the region to, w_end no larger than the stream's own window count.  A lane owns four
// consecutive bins of a pair; no LDS, no barrier, no atomics.  Every sum has one fixed order (windows inside a chunk, then chunks,
// then the member regions of a group, each by index): two calls on the same rows agree bit for bit.
#include "ss_spectrum_stats_dev.h"

namespace ssk {

namespace {

constexpr int kGroupDepth = 8;              // member regions a lane of k_spectrum_region_groups has in flight

// workgroups of k_spectrum_region_groups side by side on the row of a (group, fft_channel): 256 bin groups each
__host__ __device__ inline uint32_t region_group_blocks(uint32_t bin_stride) { return (bin_stride / 4u + 255u) / 256u; }

}  // namespace

// One wave per (region, fft_channel, chunk, slice of 64 bin groups): k_spectrum_stats' loop over the windows [w_first, w_end) of the
// region's stream.  A wave's item is taken from its first lane, so everything but the lane's place in the row is wave-uniform: the
// region record is one scalar fetch, the window count and the row pointer live in scalar registers, and a load's address is that
// pointer plus the lane's byte offset (one vector add per load; 59 VGPRs, eight waves per SIMD like k_spectrum_stats).  Chunk c
// holds the windows from w_first + c * chunk_windows on; plan.chunks == 1: the wave stores the results, a region without a window
// included (NaN, NaN, 0); otherwise the partial sums — a chunk that starts at or behind w_end stores nothing, and the combine does
// not read it.
__global__ __launch_bounds__(256) void k_spectrum_regions(SpecRegionsParams q)
{
    const SpecStatsParams &p = q.s;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = (uint64_t)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t per_pair = p.plan.slices * p.plan.chunks;
    const uint32_t pairs = p.n_streams * p.fft_ch;              // (n_streams: the regions)
    if (item >= (uint64_t)pairs * per_pair) return;
    const uint32_t pair = (uint32_t)(item / per_pair), rest = (uint32_t)(item - (uint64_t)pair * per_pair);
    const uint32_t chunk = rest / p.plan.slices, slice = rest - chunk * p.plan.slices;
    const uint32_t g = slice * 64u + lane;                      // group of four bins
    if (g >= p.bin_stride / 4u) return;
    const uint32_t region = pair / p.fft_ch, ch = pair - region * p.fft_ch;
    const SpecRegion r = q.regions[region];
    const uint64_t first = (uint64_t)r.w_first + (uint64_t)chunk * p.plan.chunk_windows;
    const bool holds = first < r.w_end;
    const bool chunked = p.plan.chunks > 1u;
    if (chunked && !holds) return;
    const uint32_t w_begin = (uint32_t)first;                  // (used only where the chunk holds a window)
    const uint32_t w_end = r.w_end - w_begin < p.plan.chunk_windows ? r.w_end : w_begin + p.plan.chunk_windows;
    const size_t row_bytes = (size_t)p.fft_ch * p.bin_stride * sizeof(float);
    const char *row = reinterpret_cast<const char *>(p.rows + ((size_t)r.stream * p.n_windows * p.fft_ch + ch) * p.bin_stride) + w_begin * row_bytes;
    const uint32_t at_lane = 16u * g;
    BinStats a;
    stats_clear(a);
    if (holds) {
        uint32_t left = w_end - w_begin;
        for (; left >= (uint32_t)kStatsDepth; left -= kStatsDepth, row += kStatsDepth * row_bytes) {
            float4 v[kStatsDepth];
#pragma unroll
            for (int k = 0; k < kStatsDepth; k++) v[k] = *reinterpret_cast<const float4 *>(row + k * row_bytes + at_lane);
#pragma unroll
            for (int k = 0; k < kStatsDepth; k++) stats_add(a, v[k]);
        }
        for (; left; left--, row += row_bytes) stats_add(a, *reinterpret_cast<const float4 *>(row + at_lane));
    }
    if (!chunked) {
        stats_write_results(p, (size_t)pair * p.bin_stride + 4u * g, 4u * g, a);
        return;
    }
    stats_write_parts(p, ((size_t)pair * p.plan.chunks + chunk) * p.bin_stride + 4u * g, a);
}

// chunked plans, behind k_spectrum_regions on the same stream: one lane per (region, fft_channel, bin group) adds the chunks the
// region's own window count reaches, in chunk order
__global__ __launch_bounds__(256) void k_spectrum_regions_combine(SpecRegionsParams q)
{
    const SpecStatsParams &p = q.s;
    const uint32_t groups = p.bin_stride / 4u;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)p.n_streams * p.fft_ch * groups) return;
    const uint32_t pair = (uint32_t)(idx / groups), g = (uint32_t)(idx - (uint64_t)pair * groups);
    const SpecRegion r = q.regions[pair / p.fft_ch];
    const uint32_t nw = r.w_end - r.w_first;
    const uint32_t chunks = nw / p.plan.chunk_windows + (nw % p.plan.chunk_windows ? 1u : 0u);     // (<= plan.chunks: the plan is the longest region's)
    BinStats a;
    stats_clear(a);
    const size_t first = (size_t)pair * p.plan.chunks * p.bin_stride + 4u * g;
#pragma unroll 4
    for (uint32_t c = 0; c < chunks; c++) stats_add_parts(a, p, first + (size_t)c * p.bin_stride);
    stats_write_results(p, (size_t)pair * p.bin_stride + 4u * g, 4u * g, a);
}

// The groups: one lane per (group, fft_channel, bin group) adds its member regions' power sums and counts in region index order
// and takes the maximum of their maxima; counts[group][fft_channel]: the pooled count at bin 0.  The regions' own padding behind
// n_bins reads (0, NaN, 0), so the groups' does too.  A workgroup serves one (group, fft_channel) — region_group_blocks() of them
// side by side on its row — so the member list is read with scalar loads, which the lanes' own loads do not queue behind.
__global__ __launch_bounds__(256) void k_spectrum_region_groups(SpecRegionsParams q)
{
    const SpecStatsParams &p = q.s;
    const uint32_t groups = p.bin_stride / 4u, blocks = region_group_blocks(p.bin_stride);
    const uint32_t gpair = blockIdx.x / blocks, g = (blockIdx.x - gpair * blocks) * 256u + threadIdx.x;
    if (g >= groups) return;
    const uint32_t group = gpair / p.fft_ch, ch = gpair - group * p.fft_ch;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    float mx[4];
    unsigned long long n[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; e++) mx[e] = __builtin_nanf("");
    const auto add = [&](const double2 s0, const double2 s1, const float4 v, const uint4 c) {
        sum[0] += s0.x; sum[1] += s0.y; sum[2] += s1.x; sum[3] += s1.y;
        mx[0] = fmaxf(mx[0], v.x); mx[1] = fmaxf(mx[1], v.y); mx[2] = fmaxf(mx[2], v.z); mx[3] = fmaxf(mx[3], v.w);
        n[0] += c.x; n[1] += c.y; n[2] += c.z; n[3] += c.w;
    };
    // a member's records are found through its index, so a walk one member at a time is a chain of two memory latencies per member
    // (1 ms for a group of 1024): kGroupDepth members' loads are in flight together, and they are added in index order all the same
    const size_t region_stride = (size_t)p.fft_ch * p.bin_stride, lane_at = (size_t)ch * p.bin_stride + 4u * g;
    const uint32_t m_end = q.member_start[group + 1u];
    uint32_t m = q.member_start[group];
    for (; m_end - m >= (uint32_t)kGroupDepth; m += kGroupDepth) {
        double2 s0[kGroupDepth], s1[kGroupDepth];
        float4 v[kGroupDepth];
        uint4 c[kGroupDepth];
        const uint32_t *member = q.members + m;             // (consecutive words: one wide scalar load)
#pragma unroll
        for (int k = 0; k < kGroupDepth; k++) {
            const size_t at = member[k] * region_stride + lane_at;
            s0[k] = reinterpret_cast<const double2 *>(p.sums + at)[0]; s1[k] = reinterpret_cast<const double2 *>(p.sums + at)[1];
            v[k] = *reinterpret_cast<const float4 *>(p.max + at);
            c[k] = *reinterpret_cast<const uint4 *>(p.counts + at);
        }
        __builtin_amdgcn_sched_barrier(0);                  // every load of the batch is issued before the first add waits for one
#pragma unroll
        for (int k = 0; k < kGroupDepth; k++) add(s0[k], s1[k], v[k], c[k]);
    }
    for (; m < m_end; m++) {
        const size_t at = q.members[m] * region_stride + lane_at;
        add(reinterpret_cast<const double2 *>(p.sums + at)[0], reinterpret_cast<const double2 *>(p.sums + at)[1],
            *reinterpret_cast<const float4 *>(p.max + at), *reinterpret_cast<const uint4 *>(p.counts + at));
    }
    const size_t at = (size_t)gpair * p.bin_stride + 4u * g;
    *reinterpret_cast<float4 *>(q.group_mean + at) = make_float4(stats_mean_db(sum[0], n[0]), stats_mean_db(sum[1], n[1]),
                                                                 stats_mean_db(sum[2], n[2]), stats_mean_db(sum[3], n[3]));
    *reinterpret_cast<float4 *>(q.group_max + at) = make_float4(mx[0], mx[1], mx[2], mx[3]);
    if (g == 0u) q.group_counts[gpair] = n[0];
}

// the launch limits of the three kernels: launch_spectrum_stats' own on the regions' grid, and the groups' workgroups
static bool regions_grids_fit(uint64_t pairs, uint64_t gpairs, uint32_t bin_stride, const SpecStatsPlan &plan)
{
    const uint64_t waves = pairs * plan.slices * plan.chunks;                   // (chunks > 1 only where pairs x slices < kStatsWaves)
    return (waves + 3) / 4 <= 0x7FFFFFFFull && pairs * (bin_stride / 4u) <= (0x7FFFFFFFull << 8) && gpairs * region_group_blocks(bin_stride) <= 0x7FFFFFFFull;
}

bool spectrum_regions_fit(uint64_t n_regions, uint64_t n_groups, uint32_t fft_ch, uint32_t bin_stride, uint32_t longest_windows, SpecStatsPlan *plan)
{
    const uint64_t pairs = n_regions * fft_ch, gpairs = n_groups * fft_ch;      // (u32 x u32: no overflow)
    if (pairs > 0xFFFFFFFFull || gpairs > 0xFFFFFFFFull) return false;
    *plan = plan_spectrum_stats((uint32_t)pairs, bin_stride, longest_windows);
    return regions_grids_fit(pairs, gpairs, bin_stride, *plan);
}

hipError_t launch_spectrum_regions(const SpecRegionsParams &q, hipStream_t s)
{
    const SpecStatsParams &p = q.s;
    const uint64_t pairs = (uint64_t)p.n_streams * p.fft_ch, gpairs = (uint64_t)q.n_groups * p.fft_ch, groups = p.bin_stride / 4u;
    if (!groups) return hipSuccess;
    if (!regions_grids_fit(pairs, gpairs, p.bin_stride, p.plan)) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    if (pairs) {
        hipLaunchKernelGGL(k_spectrum_regions, dim3((uint32_t)((pairs * p.plan.slices * p.plan.chunks + 3) / 4)), dim3(256), 0, s, q);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (p.plan.chunks > 1u) {
            hipLaunchKernelGGL(k_spectrum_regions_combine, dim3((uint32_t)((pairs * groups + 255) / 256)), dim3(256), 0, s, q);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    if (gpairs) {
        hipLaunchKernelGGL(k_spectrum_region_groups, dim3((uint32_t)(gpairs * region_group_blocks(p.bin_stride))), dim3(256), 0, s, q);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace ssk
