// ss_loudness_dev.h: device-side pieces of the loudness readings that more than one translation unit compiles — the gating
// kernels of ss_loudness.hip and the tick kernel of the time-domain files (ss_td_impl.h) read the same filtered-sample ring.
#pragma once
#include "ss_kernels.h"

namespace ssk {

// ebur128's energy_to_loudness
__device__ __forceinline__ double energy_to_lufs(double e) { return e <= 0.0 ? -INFINITY : 10.0 * log10(e) - 0.691; }

// acc + sum of w_c y^2 over this thread's share of `total` elements of the filtered-sample ring from begin_elem on: elements
// first, first + stride, first + 2 stride, ... of the run, added in that order.  The run is ONE run of ring elements with at most
// one wrap (total <= ring_elems < 2^31), so an element's position is an add and a compare in 32 bits and its channel advances by a
// constant step: no division in the loop (the first version divided two 64-bit numbers per element — most of its 9.8 us inside a
// tick).  Four loads in flight per thread, all requested before the first is used.  A channel of weight 0 is one the crate does
// not filter: its ring stays zero there, whatever the input, and whatever the ring holds is dropped.
__device__ __forceinline__ double ring_sumsq(const double *__restrict__ ring, uint32_t ring_elems, uint32_t C, uint32_t begin_elem,
                                             uint32_t total, uint32_t first, uint32_t stride, const double *__restrict__ weights,
                                             double acc)
{
    const uint32_t cstep = stride % C;
    uint32_t c = first % C, i = first;
    for (; i + 3u * stride < total; i += 4u * stride) {
        double y[4], w[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint32_t e = begin_elem + i + (uint32_t)q * stride;
            if (e >= ring_elems) e -= ring_elems;
            y[q] = ring[e];
            w[q] = weights[c];
            c += cstep; if (c >= C) c -= C;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) acc = w[q] != 0.0 ? fma(w[q] * y[q], y[q], acc) : acc;
    }
    for (; i < total; i += stride) {
        uint32_t e = begin_elem + i;
        if (e >= ring_elems) e -= ring_elems;
        const double y = ring[e], w = weights[c];
        acc = w != 0.0 ? fma(w * y, y, acc) : acc;
        c += cstep; if (c >= C) c -= C;
    }
    return acc;
}

}  // namespace ssk
