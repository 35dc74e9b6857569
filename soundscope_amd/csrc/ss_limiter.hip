// ss_limiter.hip: the batch's look-ahead peak limiter (ss_batch_limit) — the resident f32 corpus times an item's gain and a gain
// curve that depends on a neighbourhood of frames, in place — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference.
// Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.3.6.
//
// In place is only safe if no workgroup reads frames another one writes, so a group of streams takes two launches, in order on the
// batch's stream: the detector reads the corpus and leaves integers, the second launch reads those integers and rewrites the corpus.
//
// k_limit_detect<NT, NB>: one workgroup per (item of the group, tile of kLimitTileFrames frames).  It walks the tile in pieces of at
// most kLimitStageFloats floats, each staged in LDS with the NT - 1 frames in front of it as k_peak_series stages its tiles (the
// stream's own history, zeros in front of frame 0, nothing at or behind the stream's length).  A lane takes runs of kLimitRun frames
// of one selected channel, forms peak_frame_max of every frame (NT = 0: the sample's magnitude) and meets the other channels in an
// LDS word per frame (ds_max_u32 on the bits of the non-negative value; a value that is not finite stays out).  The words then become r_q, the required gain as an
// integer; the tile's minimum goes to tile_min[item][tile] as one plain store, and the tile's r_q go to the scratch row of the
// item only where that minimum is below 2^30.
//
// k_limit_apply<STEREO>: one workgroup per (item, tile).  It reads the tile_min of the tiles that meet [t0 - L - H, t1 + L + A],
// which is wave-uniform.  All 2^30: the constant form, k_apply_gain's sweep with the item's gain (ss_gain_dev.h) — no scratch
// traffic, no LDS traffic.  Otherwise the curve form: the reach of r_q goes into LDS (2^30 for tiles whose minimum is 2^30 and for
// frames outside the stream), the window minimum is formed in place by doubling steps (r[i] = min(r[i], r[i + s]), s = 1, 2, 4, ...,
// then one step that completes the window's width), and the window sums by a sliding u64 sum per lane over a run of frames; the
// factor g * c[n] of kLimitCurveFrames frames at a time waits in LDS for the sweep's f64 form.  Integer work throughout: any order
// gives the same bits.  The stream's record receives what the tile adds with integer atomics, only where there is something to add.
#include "ss_kernels.h"
#include "ss_gain_dev.h"
#include "ss_peak_dev.h"

namespace ssk {

namespace {

constexpr uint32_t kLimitStageFloats = 4096;        // floats of one staged piece's own frames at most (16 KB of LDS)
constexpr int kLimitRun = 17;                       // frames a lane takes at a time: odd (the LDS banks), and 4096 / 17 = 241 runs fill the 256 lanes
constexpr uint32_t kLimitCurveFrames = 2048;        // frames whose factors wait in LDS at a time (16 KB)
constexpr uint32_t kLimitCurveRun = 9;              // frames of a lane's sliding sum: odd, so the lanes of a wave spread over the LDS banks
constexpr uint32_t kLimitPassDepth = 8;             // words a lane holds between the read and the write of a minimum step
constexpr uint32_t kLimitMaxTiles = 8;              // tiles a reach can meet: (tile + 2 L + H + A) / tile + 2 at the maxima
static_assert(kGainThreads == kPeakThreads, "one workgroup size");
static_assert(kLimitCurveRun * kGainThreads >= kLimitCurveFrames, "the lanes' runs cover a piece");
static_assert((kLimitTileFrames + 2u * SS_LIMIT_LOOKAHEAD_MAX + SS_LIMIT_HOLD_MAX + 23u + kLimitTileFrames - 1u) / kLimitTileFrames + 1u <= kLimitMaxTiles,
              "the tiles of a reach");

// step 1: a channel's value meets the frame's level, the largest FINITE value of the selected channels as bits (0 where there is none)
__device__ __forceinline__ void limit_meet(uint32_t *level, float v)
{
    const uint32_t bits = __float_as_uint(v) & 0x7FFFFFFFu;
    atomicMax(level, bits < 0x7F800000u ? bits : 0u);           // (no branch: the frames of a run stay one block of FMA chains)
}

// step 2: the required gain of a frame from the bits of its level, ag = |g| and the ceiling widened to double
__device__ __forceinline__ uint32_t limit_required(uint32_t level_bits, double ag, double ceiling)
{
    const double v = (double)__uint_as_float(level_bits) * ag;          // exact
    if (!(v > ceiling) || !(v <= 1.7976931348623157e308)) return kLimitOne;     // (NaN fails the first comparison, +inf the second)
    return (uint32_t)floor(ceiling / v * (double)kLimitOne);
}

// r[i] = min(r[i], r[i + s]) for i < n_out, in place: a lane holds kLimitPassDepth results across the barrier that separates the
// reads of a chunk from its writes; a later chunk neither reads what this one writes nor writes what this one has yet to read.
// Every lane of the workgroup calls this together; it ends behind a barrier.
__device__ __forceinline__ void limit_min_pass(uint32_t *r, uint32_t n_out, uint32_t s)
{
    for (uint32_t base = 0; base < n_out; base += kLimitPassDepth * kGainThreads) {
        uint32_t a[kLimitPassDepth];
#pragma unroll
        for (uint32_t k = 0; k < kLimitPassDepth; k++) {
            const uint32_t i = base + k * kGainThreads + threadIdx.x;
            a[k] = kLimitOne;
            if (i < n_out) { const uint32_t u = r[i], v = r[i + s]; a[k] = u < v ? u : v; }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kLimitPassDepth; k++) {
            const uint32_t i = base + k * kGainThreads + threadIdx.x;
            if (i < n_out) r[i] = a[k];
        }
    }
    __syncthreads();
}

// the factors of the sweep's f64 form, from LDS
struct CurveEnvelope {
    const double *e;                                            // e[off]: g * c of frame t_begin + off
    float g;
    unsigned long long t_begin;
    __device__ __forceinline__ float gain() const { return g; }
    __device__ __forceinline__ double at(uint32_t off) const { return e[off]; }
};

}  // namespace

// NT: taps of a branch (12 at factor 4, 24 at factor 2, 0: the sample's magnitude); NB: interpolated branches (factor - 1)
template <int NT, int NB>
__global__ __launch_bounds__(kPeakThreads) void k_limit_detect(LimitParams p)
{
    extern __shared__ float4 sh4[];
    __shared__ uint32_t rq_s[kLimitTileFrames];                 // a frame's level as bits, then its r_q
    __shared__ uint32_t min_s;
    __shared__ float tap_s[36];
    float *sh = reinterpret_cast<float *>(sh4);
    constexpr int H = NT ? NT - 1 : 0;
    const uint32_t slot = blockIdx.x / p.tiles_cap, tile = blockIdx.x - slot * p.tiles_cap;
    const uint32_t item = p.item_first + slot;
    const LimitItem it = p.items[item];
    unsigned long long F = p.frames_of ? p.frames_of[it.stream] : p.n_frames;
    if (F > p.n_frames) F = p.n_frames;
    const unsigned long long t_begin = (unsigned long long)tile * kLimitTileFrames;
    if (t_begin >= F) return;                                   // (the whole workgroup: the tile lies behind the stream's end)
    const uint32_t tn = (uint32_t)(t_begin + kLimitTileFrames < F ? kLimitTileFrames : F - t_begin);
    const uint32_t C = p.channels;
    const long long base = (long long)((unsigned long long)it.stream * p.stream_stride);      // the stream's frame 0, in floats
    for (uint32_t i = threadIdx.x; i < tn; i += kPeakThreads) rq_s[i] = 0u;
    if (threadIdx.x == 0u) min_s = kLimitOne;
    if (threadIdx.x < (uint32_t)(NB * NT)) tap_s[threadIdx.x] = p.taps[threadIdx.x];
    __syncthreads();
    float tap[NB ? NB : 1][NT ? NT : 1];
#pragma unroll
    for (int f = 0; f < NB; f++)
#pragma unroll
        for (int d = 0; d < NT; d++) tap[f][d] = tap_s[f * NT + d];

    const uint32_t most = kLimitStageFloats / C;                // >= 64 frames (64 channels)
    const uint32_t piece = most < kLimitTileFrames ? most : kLimitTileFrames;
    const double ag = fabs((double)it.gain), ceiling = (double)p.ceiling;
    uint32_t lowest = kLimitOne;
    for (uint32_t t0 = 0; t0 < tn; t0 += piece) {
        const uint32_t sn = tn - t0 < piece ? tn - t0 : piece;
        // floats [g0, g1): frames [t_begin + t0 - H, t_begin + t0 + sn) of the stream; the copy starts at the 16-byte line of g0
        const long long g0 = base + ((long long)(t_begin + t0) - H) * (long long)C, g1 = base + (long long)(t_begin + t0 + sn) * (long long)C;
        const uint32_t shift = (uint32_t)(g0 & 3ll);
        const long long first = g0 - shift;
        const uint32_t n4 = (uint32_t)((g1 - first + 3) >> 2);
        __syncthreads();                                        // the piece before this one has been read
        peak_load_tile(sh, p.pcm, first, base > g0 ? base : g0, g1, n4);
        __syncthreads();
        const float *x0 = sh + shift;                           // x0[(H + k) * C + c] = frame t0 + k of the tile, channel c
        const uint32_t runs = (sn + kLimitRun - 1) / kLimitRun, work = runs * C;
        for (uint32_t w_i = threadIdx.x; w_i < work; w_i += kPeakThreads) {
            const uint32_t run = w_i / C, c = w_i - run * C;
            if (!((p.channel_mask >> c) & 1ull)) continue;      // the selected channels are linked; the others are not heard
            const uint32_t a = run * kLimitRun;                  // first frame of the run in the piece
            const uint32_t cnt = sn - a < (uint32_t)kLimitRun ? sn - a : (uint32_t)kLimitRun;
            const float *xr = x0 + (size_t)a * C + c;
            uint32_t *level = rq_s + t0 + a;
            if (cnt == (uint32_t)kLimitRun) {
                float w[H + kLimitRun];                          // frames a - H .. a + kLimitRun - 1, each read once
#pragma unroll
                for (int i = 0; i < H + kLimitRun; i++) w[i] = xr[(size_t)i * C];
#pragma unroll
                for (int k = 0; k < kLimitRun; k++) limit_meet(&level[k], peak_frame_max<NT, NB>(tap, w + k));
            } else {                                            // the last run of a piece: the window moves through registers
                float w[H + 1];
#pragma unroll
                for (int i = 0; i < H; i++) w[i] = xr[(size_t)i * C];
                for (uint32_t k = 0; k < cnt; k++) {
                    w[H] = xr[(size_t)(H + k) * C];
                    limit_meet(&level[k], peak_frame_max<NT, NB>(tap, w));
#pragma unroll
                    for (int i = 0; i < H; i++) w[i] = w[i + 1];
                }
            }
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < sn; i += kPeakThreads) {
            const uint32_t r = limit_required(rq_s[t0 + i], ag, ceiling);
            rq_s[t0 + i] = r;
            lowest = r < lowest ? r : lowest;
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { const uint32_t o = __shfl_xor(lowest, d); lowest = o < lowest ? o : lowest; }
    if ((threadIdx.x & 63u) == 0u && lowest < kLimitOne) atomicMin(&min_s, lowest);
    __syncthreads();
    lowest = min_s;
    if (threadIdx.x == 0u) p.tile_min[(size_t)item * p.tiles_cap + tile] = lowest;
    if (lowest < kLimitOne) {
        uint32_t *row = p.scratch + (size_t)slot * p.n_frames + t_begin;
        for (uint32_t i = threadIdx.x; i < tn; i += kPeakThreads) row[i] = rq_s[i];
    }
}

template <bool STEREO>
__global__ __launch_bounds__(kGainThreads) void k_limit_apply(LimitParams p)
{
    extern __shared__ double dyn[];                             // the curve form's: kLimitCurveFrames factors, then the reach's words
    __shared__ uint32_t tmin_s[kLimitMaxTiles];
    const uint32_t slot = blockIdx.x / p.tiles_cap, tile = blockIdx.x - slot * p.tiles_cap;
    const uint32_t item = p.item_first + slot, tid = threadIdx.x;
    const LimitItem it = p.items[item];
    unsigned long long F = p.frames_of ? p.frames_of[it.stream] : p.n_frames;
    if (F > p.n_frames) F = p.n_frames;
    const unsigned long long t_begin = (unsigned long long)tile * kLimitTileFrames;
    if (t_begin >= F) return;                                   // (the whole workgroup: the tile lies behind the stream's end)
    const uint32_t tn = (uint32_t)(t_begin + kLimitTileFrames < F ? kLimitTileFrames : F - t_begin);
    const uint32_t L = p.lookahead, Hd = p.hold, A = p.advance;
    // the frames whose r_q the tile's curve reads: [t_begin - L - Hd, t_begin + tn + L + A), cut to the stream
    const long long j0 = (long long)t_begin - (long long)L - (long long)Hd;
    const unsigned long long j_lo = j0 > 0 ? (unsigned long long)j0 : 0ull;
    const unsigned long long j_end = t_begin + tn + L + A < F ? t_begin + tn + L + A : F;     // (> j_lo: the tile's own frames)
    const uint32_t tile_lo = (uint32_t)(j_lo / kLimitTileFrames), n_tiles = (uint32_t)((j_end - 1ull) / kLimitTileFrames) - tile_lo + 1u;
    if (tid < n_tiles) tmin_s[tid] = p.tile_min[(size_t)item * p.tiles_cap + tile_lo + tid];
    __syncthreads();
    bool constant = true;
    for (uint32_t k = 0; k < n_tiles; k++) constant = constant && tmin_s[k] == kLimitOne;

    GainChannel *rec = p.stats + (size_t)it.stream * p.channels;
    const long long at = (long long)((unsigned long long)it.stream * p.stream_stride) + (long long)t_begin * (long long)p.channels;   // the tile's frame 0, in floats
    CurveEnvelope env;
    env.e = dyn; env.g = it.gain; env.t_begin = t_begin;
    if (constant) {
        if (STEREO) sweep_stereo<true>(p, at, tn, env, rec);
        else sweep_frames<true>(p, p.pcm + at, tn, env, rec);
        return;
    }

    uint32_t *r = reinterpret_cast<uint32_t *>(dyn + kLimitCurveFrames);
    const uint32_t W = Hd + L + A + 1u, R = tn + 2u * L + Hd + A;        // the window's width; r[i] is frame j0 + i
    const uint32_t *row = p.scratch + (size_t)slot * p.n_frames;
    for (uint32_t i = tid; i < R; i += kGainThreads) {
        const long long j = j0 + (long long)i;
        uint32_t v = kLimitOne;
        if (j >= 0 && (unsigned long long)j < F && tmin_s[(uint32_t)((unsigned long long)j / kLimitTileFrames) - tile_lo] != kLimitOne) v = row[j];
        r[i] = v;
    }
    __syncthreads();
    // step 3: r[i] = min r[i .. i + W - 1], which is w_q of frame t_begin - L + i, for i < tn + L
    uint32_t len = R, width = 1u;
    for (; 2u * width <= W; width *= 2u) { limit_min_pass(r, len - width, width); len -= width; }
    if (W > width) limit_min_pass(r, len - (W - width), W - width);
    // step 4 and 5, kLimitCurveFrames frames at a time: S[n] = r[o .. o + L] summed for frame t_begin + o, then the sweep
    const unsigned long long full = (unsigned long long)(L + 1u) * kLimitOne;
    const double full_d = (double)full, g_d = (double)it.gain;
    uint32_t n_limited = 0u, first_limited = 0xFFFFFFFFu;
    unsigned long long min_sum = full;
    for (uint32_t q0 = 0; q0 < tn; q0 += kLimitCurveFrames) {
        const uint32_t qn = tn - q0 < kLimitCurveFrames ? tn - q0 : kLimitCurveFrames;
        const uint32_t o_lo = tid * kLimitCurveRun, o_hi = o_lo + kLimitCurveRun < qn ? o_lo + kLimitCurveRun : qn;
        if (o_lo < qn) {
            const uint32_t *w = r + q0;
            unsigned long long sum = 0ull;
            for (uint32_t i = o_lo; i <= o_lo + L; i++) sum += w[i];
            for (uint32_t o = o_lo; o < o_hi; o++) {
                if (sum < full) {
                    n_limited++;
                    first_limited = q0 + o < first_limited ? q0 + o : first_limited;
                    min_sum = sum < min_sum ? sum : min_sum;
                }
                {
#pragma clang fp contract(off)                                  // the division and the product are rounded on their own
                    const double c = (double)sum / full_d;
                    dyn[o] = g_d * c;
                }
                if (o + 1u < o_hi) sum += (unsigned long long)w[o + L + 1u] - (unsigned long long)w[o];       // (wraps and comes back: the sum stays >= 0)
            }
        }
        __syncthreads();
        env.t_begin = t_begin + q0;
        if (STEREO) sweep_stereo<false>(p, at + 2ll * (long long)q0, qn, env, rec);
        else sweep_frames<false>(p, p.pcm + at + (long long)q0 * (long long)p.channels, qn, env, rec);
        __syncthreads();                                        // the factors have been read
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint32_t fr = __shfl_xor(first_limited, d);
        const unsigned long long ms = __shfl_xor(min_sum, d);
        first_limited = fr < first_limited ? fr : first_limited; min_sum = ms < min_sum ? ms : min_sum;
        n_limited += __shfl_xor(n_limited, d);
    }
    if ((tid & 63u) == 0u && n_limited) {
        LimitStream *ls = p.streams + it.stream;
        atomicAdd(atomic_u64(&ls->n_limited), (unsigned long long)n_limited);
        atomicMin(atomic_u64(&ls->first_limited), t_begin + first_limited);
        atomicMin(atomic_u64(&ls->min_sum), min_sum);
    }
}

LimitPlan plan_limit(uint64_t n_frames, uint32_t n_items, uint64_t scratch_bytes)
{
    LimitPlan plan{};
    plan.tile_frames = kLimitTileFrames;
    const uint64_t tiles = (n_frames + kLimitTileFrames - 1u) / kLimitTileFrames;
    plan.tiles_cap = tiles > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tiles;
    const uint64_t row = n_frames * sizeof(uint32_t);
    const uint64_t fit = row ? scratch_bytes / row : n_items;
    plan.group_streams = fit < n_items ? (uint32_t)fit : n_items;
    plan.scratch_bytes = row * plan.group_streams;
    return plan;
}

// the detector, then the sweep, of the items [item_first, item_first + n_group): the group's scratch rows are the buffer's first
hipError_t launch_limit(const LimitParams &p, hipStream_t s)
{
    const uint64_t groups = (uint64_t)p.n_group * p.tiles_cap;
    if (!groups) return hipSuccess;
    if (groups > 0x7FFFFFFFull || !p.channels || p.channels > (uint32_t)kMaxChannels) return hipErrorInvalidValue;
    if (p.channels < 64u && (p.channel_mask >> p.channels)) return hipErrorInvalidValue;
    if (p.stereo && (p.channels != 2u || p.channel_mask != 3ull || (p.stream_stride & 1u))) return hipErrorInvalidValue;
    if (p.lookahead > SS_LIMIT_LOOKAHEAD_MAX || p.hold > SS_LIMIT_HOLD_MAX) return hipErrorInvalidValue;
    const int nt = p.factor == 4 ? 12 : p.factor == 2 ? 24 : 0;
    if (p.advance != (uint32_t)(nt ? nt - 1 : 0)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups), block(kGainThreads);
    {
        // a piece, its history and the copy's alignment at both ends: in float4
        const uint32_t most = kLimitStageFloats / p.channels, piece = most < kLimitTileFrames ? most : kLimitTileFrames;
        const size_t floats = (size_t)(piece + (nt ? nt - 1 : 0)) * p.channels + 8;
        const size_t lds = (floats + 3) / 4 * sizeof(float4);
        if (p.factor == 4) hipLaunchKernelGGL((k_limit_detect<12, 3>), grid, block, lds, s, p);
        else if (p.factor == 2) hipLaunchKernelGGL((k_limit_detect<24, 1>), grid, block, lds, s, p);
        else if (p.factor == 0) hipLaunchKernelGGL((k_limit_detect<0, 0>), grid, block, lds, s, p);
        else return hipErrorInvalidValue;
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    // the curve form's LDS: the factors of a piece and the reach at this call's look-ahead and hold
    const size_t lds = kLimitCurveFrames * sizeof(double) + (size_t)(kLimitTileFrames + 2u * p.lookahead + p.hold + p.advance) * sizeof(uint32_t);
    constexpr int lds_max = (int)(kLimitCurveFrames * sizeof(double) + (kLimitTileFrames + 2u * SS_LIMIT_LOOKAHEAD_MAX + SS_LIMIT_HOLD_MAX + 23u) * sizeof(uint32_t));
    static DevicePrep prepared[2];
    const void *fn = p.stereo ? reinterpret_cast<const void *>(k_limit_apply<true>) : reinterpret_cast<const void *>(k_limit_apply<false>);
    const hipError_t pe = prepare_on_device(prepared[p.stereo ? 1 : 0], [fn] {
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    });
    if (pe != hipSuccess) return pe;
    if (p.stereo) hipLaunchKernelGGL(k_limit_apply<true>, grid, block, lds, s, p);
    else hipLaunchKernelGGL(k_limit_apply<false>, grid, block, lds, s, p);
    return hipGetLastError();
}

}  // namespace ssk
