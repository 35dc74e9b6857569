// ss_apply_gain.hip: the batch acts on its readings — the resident f32 corpus times a gain curve per stream, in place, with what the
// result holds per (stream, channel) (ss_batch_apply_gain), and the corpus converted to a delivery format on its way out
// (ss_batch_download_pcm) — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference.
// Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.3.5.
//
// k_apply_gain: one workgroup per (touched stream, tile of kGainTileFrames frames); streams without a point are not in the grid.
// The host has resolved a stream's points into segments (ss_kernels.h, GainSegment).  A workgroup finds the segments of its tile's
// first and last frame by a binary search on wave-uniform values; where both are one constant segment the tile takes the constant
// form, y = x * g in f32 (the f64 product of two f32 values is exact, so this IS (float)((double)x * g)); any other tile takes the
// f64 form: the envelope of a frame from the tile's one segment (scalar registers), or, where the tile holds several, from the
// segment a lane finds for its frame among them; then two roundings, the f64 multiplication and the conversion.
//   <true>  two channels, both selected: the tile's floats [lo, hi) as 16-byte loads (two frames each) and 16-byte stores, in the
//           constant form two packed f32 multiplies between them, in the f64 form two envelope values and four f64 products; lo
//           and hi are even, and a slot of odd frames makes a stream start 8-byte aligned only, so the aligned inside has at most
//           one lone frame at each end, handled as two 4-byte accesses (k_pair_series<true>'s guard rule: no float outside [lo, hi)
//           is touched).
//   <false> any channel count and mask: 4-byte accesses at the frame's stride, channel after channel (the channels of a frame share
//           its cache lines); an unselected channel is read for the statistics and not written.
// Every sample is read and written by the same lane, four loads in flight, so in place is safe.  Nothing is staged in LDS.
// Statistics: a lane keeps the maximum of the finite |y| as bits, the counts and the first frame at or over the clip level; the 64
// lanes of a wave meet in a butterfly (__shfl_xor), then lane 0 adds to the stream's record with integer atomics (maximum of the
// bits, additions, a 64-bit minimum): the record does not depend on the order of arrival.
// k_f32_to_pcm: a lane converts four consecutive samples and stores them as whole words.
#include "ss_kernels.h"
#include "ss_gain_dev.h"

namespace ssk {

namespace {

// the last segment of [lo, hi) that starts at or before frame n (seg[lo].start <= n)
__device__ __forceinline__ uint32_t seg_find(const GainSegment *seg, uint32_t lo, uint32_t hi, unsigned long long n)
{
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (seg[mid].start <= n) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double seg_value(const GainSegment &s, unsigned long long n)
{
#pragma clang fp contract(off)                                  // (__dmul_rn and __dadd_rn are plain operators to this compiler: it would fuse them)
    const double step = (double)(n - s.base) * s.d;
    return s.base == kGainConst ? s.g : s.g + step;
}

// The envelope over one tile: where the tile lies in ONE segment that segment comes from scalar registers, otherwise a lane finds its
// frame's segment among the tile's s_lo .. s_hi by a search of its own.
struct TileEnvelope {
    const GainSegment *seg;
    uint32_t s_lo, s_hi;
    unsigned long long t_begin;
    GainSegment one;                                            // seg[s_lo]
    __device__ __forceinline__ float gain() const { return (float)one.g; }     // (a constant segment's gain is one of the caller's floats)
    __device__ __forceinline__ double at(uint32_t off) const    // frame t_begin + off
    {
        const unsigned long long n = t_begin + off;
        return s_lo == s_hi ? seg_value(one, n) : seg_value(seg[seg_find(seg, s_lo, s_hi + 1u, n)], n);
    }
};

}  // namespace

template <bool STEREO>
__global__ __launch_bounds__(kGainThreads) void k_apply_gain(ApplyGainParams p)
{
    const uint32_t ti = blockIdx.x / p.tiles_cap, tile = blockIdx.x - ti * p.tiles_cap;
    const GainStream ts = p.touched[ti];
    unsigned long long F = p.frames_of ? p.frames_of[ts.stream] : p.n_frames;
    if (F > p.n_frames) F = p.n_frames;
    const unsigned long long t_begin = (unsigned long long)tile * kGainTileFrames;
    if (t_begin >= F) return;                                   // (the whole workgroup: the tile lies behind the stream's end)
    const unsigned long long t_end = t_begin + kGainTileFrames < F ? t_begin + kGainTileFrames : F;
    const uint32_t t_frames = (uint32_t)(t_end - t_begin);
    TileEnvelope env;
    env.seg = p.segments + ts.seg_first; env.t_begin = t_begin;
    env.s_lo = seg_find(env.seg, 0u, ts.n_seg, t_begin); env.s_hi = seg_find(env.seg, env.s_lo, ts.n_seg, t_end - 1ull);
    env.one = env.seg[env.s_lo];
    const bool constant = env.s_lo == env.s_hi && env.one.base == kGainConst;
    GainChannel *rec = p.stats + (size_t)ts.stream * p.channels;
    const long long at = (long long)((unsigned long long)ts.stream * p.stream_stride) + (long long)t_begin * (long long)p.channels;   // the tile's frame 0, in floats
    if (STEREO) {
        if (constant) sweep_stereo<true>(p, at, t_frames, env, rec);
        else sweep_stereo<false>(p, at, t_frames, env, rec);
    } else {
        if (constant) sweep_frames<true>(p, p.pcm + at, t_frames, env, rec);
        else sweep_frames<false>(p, p.pcm + at, t_frames, env, rec);
    }
}

hipError_t launch_apply_gain(const ApplyGainParams &p, hipStream_t s)
{
    const uint64_t groups = (uint64_t)p.n_touched * p.tiles_cap;
    if (!groups) return hipSuccess;
    if (groups > 0x7FFFFFFFull || !p.channels || p.channels > (uint32_t)kMaxChannels) return hipErrorInvalidValue;
    if (p.channels < 64u && (p.channel_mask >> p.channels)) return hipErrorInvalidValue;
    if (p.stereo && (p.channels != 2u || p.channel_mask != 3ull || (p.stream_stride & 1u))) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups), block(kGainThreads);
    if (p.stereo) hipLaunchKernelGGL(k_apply_gain<true>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_apply_gain<false>, grid, block, 0, s, p);
    return hipGetLastError();
}

// ============================================================================
//  PCM export (ss_batch_download_pcm): the inverse of k_pcm_to_f32
// ============================================================================
namespace {

__device__ __forceinline__ uint32_t mix_u32(uint32_t v)
{
    v ^= v >> 16; v *= 0x7FEB352Du; v ^= v >> 15; v *= 0x846CA68Bu; v ^= v >> 16;
    return v;
}

// the triangular dither of sample i of `stream` (include/soundscope_hip.h): exact, in (-1, 1)
__device__ __forceinline__ float tpdf_of(uint64_t seed, uint32_t stream, uint64_t i)
{
    const uint32_t k = mix_u32(mix_u32(mix_u32((uint32_t)(seed >> 32) ^ stream) ^ (uint32_t)seed) ^ (uint32_t)(i >> 32)) ^ (uint32_t)i;
    const int32_t u1 = (int32_t)(mix_u32(k) >> 8), u2 = (int32_t)(mix_u32(k ^ 0x80000000u) >> 8);
    return (float)(u1 - u2) * (1.0f / 16777216.0f);
}

// rint(x scale [+ d]), halves to even, saturated to [-scale, scale - 1]; NaN -> 0
__device__ __forceinline__ int32_t quantise(float x, float scale, bool dither, float d)
{
#pragma clang fp contract(off)                                  // (the product is exact, so a fused form would agree; this keeps the recipe literal)
    float v = x * scale;
    if (dither) v = v + d;
    if (v != v) return 0;
    const float r = rintf(v);
    const long long top = (long long)scale;
    if (r >= scale) return (int32_t)(top - 1);
    if (r < -scale) return (int32_t)(-top);
    return (int32_t)r;
}

}  // namespace

__global__ __launch_bounds__(256) void k_f32_to_pcm(PcmOutParams p)
{
    const uint64_t groups = (p.n_samples + 3ull) >> 2;
    const uint32_t C = p.channels;
    const int fmt = p.format;
    const float scale = fmt == 1 ? 128.0f : fmt == 2 ? 32768.0f : fmt == 3 ? 8388608.0f : 2147483648.0f;
    const bool integer = fmt >= 1 && fmt <= 4, dither = integer && p.tpdf != 0u;
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < groups; t += (uint64_t)gridDim.x * 256u) {
        const uint64_t i0 = 4ull * t;
        const uint64_t slot = i0 / p.per_stream, j0 = i0 - slot * p.per_stream;
        uint64_t frame = j0 / C;
        uint32_t ch = (uint32_t)(j0 - frame * C), stream = p.first + (uint32_t)slot;
        float x[4];
        int32_t q[4];
        bool fresh = true;                                      // F is not this stream's yet
        uint64_t F = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            x[k] = 0.0f; q[k] = 0;
            if (i0 + k >= p.n_samples) continue;                // (behind the last slot: the staging's padding)
            if (fresh) {
                F = p.frames_of ? p.frames_of[stream] : p.n_frames;
                if (F > p.n_frames) F = p.n_frames;
                fresh = false;
            }
            if (frame < F) {
                const uint64_t i = frame * C + ch;
                x[k] = p.pcm[(uint64_t)stream * p.per_stream + i];
                if (integer) q[k] = quantise(x[k], scale, dither, dither ? tpdf_of(p.seed, stream, i) : 0.0f);
            }
            if (++ch == C) {
                ch = 0u;
                if (++frame == p.n_frames) { frame = 0ull; stream++; fresh = true; }
            }
        }
        switch (fmt) {
            case 1:
                reinterpret_cast<uint32_t *>(p.out)[t] = (uint32_t)(q[0] + 128) | (uint32_t)(q[1] + 128) << 8 | (uint32_t)(q[2] + 128) << 16 | (uint32_t)(q[3] + 128) << 24;
                break;
            case 2:
                reinterpret_cast<uint2 *>(p.out)[t] = make_uint2(((uint32_t)q[0] & 0xFFFFu) | (uint32_t)q[1] << 16, ((uint32_t)q[2] & 0xFFFFu) | (uint32_t)q[3] << 16);
                break;
            case 3: {
                const uint32_t a = (uint32_t)q[0] & 0xFFFFFFu, b = (uint32_t)q[1] & 0xFFFFFFu, c = (uint32_t)q[2] & 0xFFFFFFu, d = (uint32_t)q[3] & 0xFFFFFFu;
                uint32_t *o = reinterpret_cast<uint32_t *>(p.out) + 3ull * t;
                o[0] = a | b << 24; o[1] = b >> 8 | c << 16; o[2] = c >> 16 | d << 8;
                break;
            }
            case 4:
                reinterpret_cast<int4 *>(p.out)[t] = make_int4(q[0], q[1], q[2], q[3]);
                break;
            case 5:
                reinterpret_cast<float4 *>(p.out)[t] = make_float4(x[0], x[1], x[2], x[3]);
                break;
            default: {
                double2 *o = reinterpret_cast<double2 *>(p.out) + 2ull * t;
                o[0] = make_double2((double)x[0], (double)x[1]); o[1] = make_double2((double)x[2], (double)x[3]);
                break;
            }
        }
    }
}

hipError_t launch_f32_to_pcm(const PcmOutParams &p, hipStream_t s)
{
    if (!p.n_samples) return hipSuccess;
    if (!p.per_stream || !p.channels || p.format < 1 || p.format > 6) return hipErrorInvalidValue;
    uint64_t blocks = (((p.n_samples + 3ull) >> 2) + 255ull) / 256ull;
    if (blocks > 65536ull) blocks = 65536ull;
    hipLaunchKernelGGL(k_f32_to_pcm, dim3((uint32_t)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace ssk
