// ss_peak_dev.h — the batch's true-peak interpolator on the device: the copy of a run of the corpus into LDS and the maximum over
// the branches of one frame.  Shared by the peak series (ss_peak_series.hip) and the limiter's detector (ss_limiter.hip), so that
// the level a limiter acts on IS the value the series reports for that frame.  Device code only.
#pragma once
#include "ss_kernels.h"

namespace ssk {

namespace {

constexpr uint32_t kPeakThreads = 256;

// the tile's floats from the corpus into LDS: sh[i] = corpus[first + i] for lo <= first + i < hi (the stream's own floats that
// the tile reads), zero elsewhere; `first` may lie in front of lo (history in front of frame 0) and is a multiple of four floats;
// threads: the workgroup's size (the resampler's differs)
__device__ __forceinline__ void peak_load_tile(float *sh, const float *corpus, long long first, long long lo, long long hi, uint32_t n4,
                                               uint32_t threads = kPeakThreads)
{
    for (uint32_t v = threadIdx.x; v < n4; v += threads) {
        const long long g = first + 4ll * v;
        float4 x;
        if (g >= lo && g + 4 <= hi) {
            x = *reinterpret_cast<const float4 *>(corpus + g);
        } else {
            x.x = (g >= lo && g < hi) ? corpus[g] : 0.f;
            x.y = (g + 1 >= lo && g + 1 < hi) ? corpus[g + 1] : 0.f;
            x.z = (g + 2 >= lo && g + 2 < hi) ? corpus[g + 2] : 0.f;
            x.w = (g + 3 >= lo && g + 3 < hi) ? corpus[g + 3] : 0.f;
        }
        *reinterpret_cast<float4 *>(sh + 4u * v) = x;
    }
}

// max over the branches of one frame, the sample itself (branch 0) included: win[0 .. NT - 1] are the frames n - (NT - 1) .. n,
// every interpolated branch one chain of fused multiply-adds from the oldest tap to the newest.  fmaxf is maxNum: a NaN branch
// leaves the others standing, and only a frame whose branches are all NaN reads NaN.
template <int NT, int NB>
__device__ __forceinline__ float peak_frame_max(const float (&tap)[NB ? NB : 1][NT ? NT : 1], const float *win)
{
    constexpr int H = NT ? NT - 1 : 0;
    float v = fabsf(win[H]);
#pragma unroll
    for (int f = 0; f < NB; f++) {
        float y = 0.f;
#pragma unroll
        for (int d = NT - 1; d >= 0; d--) y = __builtin_fmaf(tap[f][d], win[H - d], y);
        v = fmaxf(v, fabsf(y));
    }
    return v;
}

}  // namespace

}  // namespace ssk
