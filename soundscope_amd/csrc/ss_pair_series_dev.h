// ss_pair_series_dev.h: what the batch pair kernels (ss_pair_series.hip: one workgroup per (stream, entry)) and the meter banks' pair
// watch (ss_bank_pair_watch.hip: one workgroup per stream walks the frames of an add call) share — a lane's three f64 sums and how a
// frame enters them, the fixed tree in which the lanes of a workgroup meet, the record of an entry, and the ACTIVE / BELOW decision of
// an entry — so that there is one definition of each (include/soundscope_hip.h, "Pair series and pair regions").  The batch kernels
// are pinned to the instructions they had before the helpers moved here (profiles/bank_pair_watch_isa.txt).
#pragma once
#include "ss_kernels.h"

namespace ssk {

namespace {

constexpr uint32_t kPairThreads = 256, kPairWaves = kPairThreads / 64;
constexpr uint32_t kPairDepth = 4;          // loads a lane has in flight

struct PairSums {
    double aa = 0.0, bb = 0.0, ab = 0.0;
    uint32_t skipped = 0;
    // one frame: both samples finite, or skipped (NaN fails the comparison).  Without a branch: a skipped frame adds +0 to every
    // sum, which leaves a sum that started at +0 as it is.
    __device__ __forceinline__ void add(float xa, float xb)
    {
        const float inf = __builtin_inff();
        const bool ok = fabsf(xa) < inf && fabsf(xb) < inf;
        const double a = (double)(ok ? xa : 0.f), b = (double)(ok ? xb : 0.f);
        aa = __builtin_fma(a, a, aa); bb = __builtin_fma(b, b, bb); ab = __builtin_fma(a, b, ab);         // (the products are exact in f64)
        skipped += ok ? 0u : 1u;
    }
};

// The lanes' sums of the whole workgroup into thread 0's `s`: a butterfly across the wave (every lane ends with the wave's sum, the
// same tree in each), then the waves in wave order.  part: kPairWaves * 4 doubles of LDS; ends in a barrier, so it can be used again.
__device__ __forceinline__ void pair_reduce(PairSums &s, double *part)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        s.aa += __shfl_xor(s.aa, d); s.bb += __shfl_xor(s.bb, d); s.ab += __shfl_xor(s.ab, d);
        s.skipped += __shfl_xor(s.skipped, d);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        part[4u * wave] = s.aa; part[4u * wave + 1u] = s.bb; part[4u * wave + 2u] = s.ab;
        reinterpret_cast<uint32_t *>(part + 4u * wave + 3u)[0] = s.skipped;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t w = 1; w < kPairWaves; w++) {
            s.aa += part[4u * w]; s.bb += part[4u * w + 1u]; s.ab += part[4u * w + 2u];
            s.skipped += reinterpret_cast<const uint32_t *>(part + 4u * w + 3u)[0];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void pair_store(PairEntry *dst, const PairSums &s, uint32_t e_frames, bool swap)
{
    double2 lo; lo.x = swap ? s.bb : s.aa; lo.y = swap ? s.aa : s.bb;
    uint4 hi;
    const unsigned long long ab = (unsigned long long)__double_as_longlong(s.ab);
    hi.x = (uint32_t)ab; hi.y = (uint32_t)(ab >> 32); hi.z = e_frames - s.skipped; hi.w = s.skipped;
    reinterpret_cast<double2 *>(dst)[0] = lo;
    reinterpret_cast<uint4 *>(dst)[1] = hi;
}

// An entry is ACTIVE iff s_aa + s_bb > power_floor * frames, and BELOW iff its correlation is under the threshold t (tt = t * t,
// rounded once) — every product one rounded f64 multiplication, no square root, no division.  Declares the two booleans.  A macro:
// as __forceinline__ functions the same statements moved an instruction of k_region_pairs (profiles/bank_pair_watch_isa.txt).
#define SS_PAIR_DECIDE(active, below, aa, bb, ab, frames, power_floor, t, tt)                                                      \
    const bool active = __dadd_rn(aa, bb) > __dmul_rn(power_floor, (double)frames);                                                \
    const double active##_pw = __dmul_rn(aa, bb), active##_qq = __dmul_rn(ab, ab), active##_lim = __dmul_rn(tt, active##_pw);      \
    const bool below = t >= 0.0 ? (ab < 0.0 || active##_qq < active##_lim) : (ab < 0.0 && active##_qq > active##_lim)

}  // namespace

}  // namespace ssk
