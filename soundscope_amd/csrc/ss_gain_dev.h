// ss_gain_dev.h — the sweep that rewrites a tile of the resident corpus in place and keeps what the result holds per channel:
// shared by the batch gain (ss_apply_gain.hip: the envelope of a tile comes from the caller's segments) and the limiter
// (ss_limiter.hip: from the gain curve the workgroup formed in LDS).  Device code only.
// Params: any block with pcm, channels, channel_mask, clip_bits (ApplyGainParams' fields of these names).  Envelope: t_begin (the
// tile's first frame), gain() (the f32 gain of the constant form) and at(off) (the f64 factor of frame t_begin + off).
// Every sample is read and written by the same lane, four loads in flight, so in place is safe.
// Statistics: a lane keeps the maximum of the finite |y| as bits, the counts and the first frame at or over the clip level; the 64
// lanes of a wave meet in a butterfly (__shfl_xor), then lane 0 adds to the stream's record with integer atomics (maximum of the
// bits, additions, a 64-bit minimum): the record does not depend on the order of arrival.
#pragma once
#include "ss_kernels.h"

namespace ssk {

namespace {

constexpr uint32_t kGainThreads = 256, kGainDepth = 4;
typedef float float2v __attribute__((ext_vector_type(2)));

struct GainStat {
    uint32_t peak = 0u, over = 0u, bad = 0u, first = 0xFFFFFFFFu;      // first: frames from the tile's begin
    __device__ __forceinline__ void add(float y, uint32_t off, uint32_t clip_bits)
    {
        const uint32_t a = __float_as_uint(y) & 0x7FFFFFFFu;           // |y|: its bits order as its value does
        if (a < 0x7F800000u) peak = a > peak ? a : peak;
        else bad++;
        if (a >= clip_bits && a <= 0x7F800000u) { over++; first = off < first ? off : first; }       // (no NaN)
    }
    // every lane of the wave calls this together
    __device__ __forceinline__ void publish(GainChannel *rec, unsigned long long tile_begin)
    {
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const uint32_t pk = __shfl_xor(peak, d), fr = __shfl_xor(first, d);
            peak = pk > peak ? pk : peak; first = fr < first ? fr : first;
            over += __shfl_xor(over, d); bad += __shfl_xor(bad, d);
        }
        if ((threadIdx.x & 63u) == 0u) {
            if (peak) atomicMax(reinterpret_cast<uint32_t *>(&rec->sample_peak), peak);      // the bits of a non-negative f32 order as it does
            if (over) { atomicAdd(atomic_u64(&rec->n_over), (unsigned long long)over); atomicMin(atomic_u64(&rec->first_over), tile_begin + first); }
            if (bad) atomicAdd(atomic_u64(&rec->n_nonfinite), (unsigned long long)bad);
        }
    }
};

// y of one sample: the constant form's f32 product, or the f64 product rounded once more
template <bool CONSTANT>
__device__ __forceinline__ float gained(float x, float g, double envelope)
{
    return CONSTANT ? __fmul_rn(x, g) : (float)__dmul_rn((double)x, envelope);
}

// frames [0, t_frames) of a tile at x0 (frame f, channel c: x0[f C + c]), any channel count and mask: 4-byte accesses at the frame's
// stride, channel after channel.  CONSTANT: the tile lies in one constant segment.
template <bool CONSTANT, class Params, class Envelope>
__device__ __forceinline__ void sweep_frames(const Params &p, float *x0, uint32_t t_frames, const Envelope &env, GainChannel *rec)
{
    const uint32_t C = p.channels, tid = threadIdx.x;
    const float g = env.gain();
    for (uint32_t c = 0; c < C; c++) {
        const bool selected = (p.channel_mask >> c) & 1ull;
        GainStat st;
        for (uint32_t f0 = tid; f0 < t_frames; f0 += kGainDepth * kGainThreads) {
            float x[kGainDepth];
#pragma unroll
            for (uint32_t j = 0; j < kGainDepth; j++) {
                const size_t f = f0 + j * kGainThreads < t_frames ? f0 + j * kGainThreads : f0;       // (a frame of the tile either way)
                x[j] = x0[f * C + c];
            }
#pragma unroll
            for (uint32_t j = 0; j < kGainDepth; j++) {
                const uint32_t f = f0 + j * kGainThreads;
                if (f >= t_frames) break;
                float y = x[j];
                if (selected) {
                    y = gained<CONSTANT>(y, g, CONSTANT ? 0.0 : env.at(f));
                    x0[(size_t)f * C + c] = y;
                }
                st.add(y, f, p.clip_bits);
            }
        }
        st.publish(rec + c, env.t_begin);
    }
}

// The same for two channels, both selected: the tile's floats [lo, hi) of the corpus (both even) as vectors of four floats, two
// frames each.  Vectors [v_lo, v_hi) from `first` lie wholly inside; a lone frame in front of the first (lo is 8-byte aligned
// only) or behind the last is two 4-byte accesses of one lane.  CONSTANT: two packed f32 multiplies per vector; otherwise the two
// frames' envelope values and four f64 products.
template <bool CONSTANT, class Params, class Envelope>
__device__ __forceinline__ void sweep_stereo(const Params &p, long long lo, uint32_t t_frames, const Envelope &env, GainChannel *rec)
{
    const uint32_t tid = threadIdx.x, clip = p.clip_bits;
    const long long hi = lo + 2ll * (long long)t_frames;
    const uint32_t shift = (uint32_t)(lo & 3ll);                // 0 or 2: a lone frame in front of the first whole vector
    const long long first = lo - shift;
    const uint32_t v_lo = shift ? 1u : 0u, v_hi = (uint32_t)((hi - first) >> 2);
    const bool tail = ((hi - first) & 3ll) != 0;                // a lone frame behind the last whole vector
    float4 *vec = reinterpret_cast<float4 *>(p.pcm + first);
    const float g = env.gain();
    const float2v gg = {g, g};
    GainStat s0, s1;
    if (tid == 0u && shift) {
        const double e = CONSTANT ? 0.0 : env.at(0u);
        const float y0 = gained<CONSTANT>(p.pcm[lo], g, e), y1 = gained<CONSTANT>(p.pcm[lo + 1], g, e);
        p.pcm[lo] = y0; p.pcm[lo + 1] = y1;
        s0.add(y0, 0u, clip); s1.add(y1, 0u, clip);
    }
    for (uint32_t v0 = v_lo + tid; v0 < v_hi; v0 += kGainDepth * kGainThreads) {
        float4 x[kGainDepth];
#pragma unroll
        for (uint32_t j = 0; j < kGainDepth; j++) x[j] = vec[v0 + j * kGainThreads < v_hi ? v0 + j * kGainThreads : v0];   // (a whole vector either way)
#pragma unroll
        for (uint32_t j = 0; j < kGainDepth; j++) {
            const uint32_t v = v0 + j * kGainThreads;
            if (v >= v_hi) break;
            const uint32_t off = 2u * v - (shift >> 1);         // the vector's first frame, from the tile's begin
            float4 y;
            if (CONSTANT) {
                const float2v a = {x[j].x, x[j].y}, b = {x[j].z, x[j].w};
                const float2v ya = a * gg, yb = b * gg;         // (packed f32 multiplies: round to nearest, nothing to contract)
                y = make_float4(ya.x, ya.y, yb.x, yb.y);
            } else {
                const double ea = env.at(off), eb = env.at(off + 1u);
                y = make_float4(gained<false>(x[j].x, g, ea), gained<false>(x[j].y, g, ea), gained<false>(x[j].z, g, eb), gained<false>(x[j].w, g, eb));
            }
            vec[v] = y;
            s0.add(y.x, off, clip); s1.add(y.y, off, clip);
            s0.add(y.z, off + 1u, clip); s1.add(y.w, off + 1u, clip);
        }
    }
    if (tid == kGainThreads - 1u && tail) {
        const double e = CONSTANT ? 0.0 : env.at(t_frames - 1u);
        const float y0 = gained<CONSTANT>(p.pcm[hi - 2], g, e), y1 = gained<CONSTANT>(p.pcm[hi - 1], g, e);
        p.pcm[hi - 2] = y0; p.pcm[hi - 1] = y1;
        s0.add(y0, t_frames - 1u, clip); s1.add(y1, t_frames - 1u, clip);
    }
    s0.publish(rec, env.t_begin);
    s1.publish(rec + 1, env.t_begin);
}

}  // namespace

}  // namespace ssk
