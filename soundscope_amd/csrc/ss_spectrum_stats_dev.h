// ss_spectrum_stats_dev.h: what the spectrum statistics kernels (ss_spectrum_stats.hip: whole streams) and the spectrum region
// kernels (ss_spectrum_regions.hip: time ranges and groups) share — the sums a lane carries for its four bins, the rule that adds a
// value to them, the mean, and the stores of results and of a chunk's partial sums.  Device code only.
#pragma once
#include "ss_kernels.h"

namespace ssk {

namespace {

constexpr int kStatsDepth = 8;              // windows a lane has in flight
constexpr float kLog2Of10Over10 = 0.33219280948873623f;      // 10^(v / 10) = 2^(v log2(10) / 10)

// what a lane carries for its four bins
struct BinStats {
    double sum[4];          // of the powers 10^(v / 10) of the counted values
    float mx[4];            // their maximum (NaN: none yet — fmaxf is maxNum, the seed disappears with the first value)
    uint32_t n[4];          // how many were counted (a NaN value is skipped)
};

__device__ __forceinline__ void stats_clear(BinStats &a)
{
#pragma unroll
    for (int e = 0; e < 4; e++) { a.sum[e] = 0.0; a.mx[e] = __builtin_nanf(""); a.n[e] = 0u; }
}

__device__ __forceinline__ void stats_add(BinStats &a, const float4 v)
{
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const bool counted = x[e] == x[e];
        a.sum[e] += counted ? (double)exp2f(x[e] * kLog2Of10Over10) : 0.0;
        a.mx[e] = fmaxf(a.mx[e], x[e]);
        a.n[e] += counted ? 1u : 0u;
    }
}

// (float)(10 log10(sum / n)), NaN where nothing was counted
__device__ __forceinline__ float stats_mean_db(double sum, unsigned long long n)
{
    return n ? (float)(10.0 * log10(sum / (double)n)) : __builtin_nanf("");
}

// a pair's results for the four bins from `bin` on, at element `at` of the per-stream arrays; the row padding behind n_bins reads
// as "nothing counted" whatever the rows hold there
__device__ __forceinline__ void stats_write_results(const SpecStatsParams &p, size_t at, uint32_t bin, BinStats a)
{
    float mean[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        if (bin + e >= p.n_bins) { a.sum[e] = 0.0; a.mx[e] = __builtin_nanf(""); a.n[e] = 0u; }
        mean[e] = stats_mean_db(a.sum[e], a.n[e]);
    }
    reinterpret_cast<double2 *>(p.sums + at)[0] = make_double2(a.sum[0], a.sum[1]);
    reinterpret_cast<double2 *>(p.sums + at)[1] = make_double2(a.sum[2], a.sum[3]);
    *reinterpret_cast<float4 *>(p.mean + at) = make_float4(mean[0], mean[1], mean[2], mean[3]);
    *reinterpret_cast<float4 *>(p.max + at) = make_float4(a.mx[0], a.mx[1], a.mx[2], a.mx[3]);
    *reinterpret_cast<uint4 *>(p.counts + at) = make_uint4(a.n[0], a.n[1], a.n[2], a.n[3]);
}

// chunked plans: a chunk's partial sums at element `at` of the part arrays, and their way back into a lane's sums
__device__ __forceinline__ void stats_write_parts(const SpecStatsParams &p, size_t at, const BinStats &a)
{
    reinterpret_cast<double2 *>(p.part_sums + at)[0] = make_double2(a.sum[0], a.sum[1]);
    reinterpret_cast<double2 *>(p.part_sums + at)[1] = make_double2(a.sum[2], a.sum[3]);
    *reinterpret_cast<float4 *>(p.part_max + at) = make_float4(a.mx[0], a.mx[1], a.mx[2], a.mx[3]);
    *reinterpret_cast<uint4 *>(p.part_counts + at) = make_uint4(a.n[0], a.n[1], a.n[2], a.n[3]);
}

__device__ __forceinline__ void stats_add_parts(BinStats &a, const SpecStatsParams &p, size_t at)
{
    const double2 s0 = reinterpret_cast<const double2 *>(p.part_sums + at)[0], s1 = reinterpret_cast<const double2 *>(p.part_sums + at)[1];
    const float4 m = *reinterpret_cast<const float4 *>(p.part_max + at);
    const uint4 n = *reinterpret_cast<const uint4 *>(p.part_counts + at);
    a.sum[0] += s0.x; a.sum[1] += s0.y; a.sum[2] += s1.x; a.sum[3] += s1.y;
    a.mx[0] = fmaxf(a.mx[0], m.x); a.mx[1] = fmaxf(a.mx[1], m.y); a.mx[2] = fmaxf(a.mx[2], m.z); a.mx[3] = fmaxf(a.mx[3], m.w);
    a.n[0] += n.x; a.n[1] += n.y; a.n[2] += n.z; a.n[3] += n.w;
}

}  // namespace

}  // namespace ssk
