// ss_resample.hip: sample-rate conversion of every stream of a resident corpus by a rational factor L / M into another corpus
// (ss_batch_resample) — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference.
// Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.3.7.
//
// Output n of a stream reads phase p = (n M) % L of the table at input frame base = (n M) / L: acc = fmaf(taps[p][k],
// x[base - T/2 + 1 + k], acc) for k = 0 .. T - 1, one chain per output and channel.  One workgroup per (stream, tile): a tile is
// R * L outputs and starts at a multiple of L, so its first base is the integer tile * R * M and output i of the tile reads phase
// (i M) % L at frame (i M) / L of the tile's input run.  The run — R * M frames and their T - 1 frames of surroundings, zeros outside
// the stream's own [0, F) — is one contiguous piece of the corpus and is copied into LDS as it lies (peak_load_tile: aligned 16-byte
// loads inside, guarded loads at the ends, nothing outside the stream's own frames is read).  Three forms, the same chain in each:
//   k_resample_reg     (mono, stereo) lane = g * L + r owns the output residue r of the periods g, g + G, ...: its phase (r M) % L is fixed, so
//                      its T taps stay in registers and every FMA costs one LDS read (stereo: half of one, an 8-byte read of the
//                      frame).  Consecutive lanes write consecutive frames.
//   k_resample_lds     the table in LDS beside the tile, rows T + 1 floats apart (T is even: at an even stride the lanes of a wave
//                      meet in a few banks), lane = output of the tile: any L and T that fit, two LDS reads per FMA (stereo: one).
//   k_resample_direct  taps and samples from global memory with guarded loads, lane = (output, channel): what fits neither.
#include "ss_kernels.h"
#include "ss_peak_dev.h"

namespace ssk {

namespace {

constexpr uint32_t kResampleTileFloats = 8192;          // floats of a tile's input run the plan aims at (32 KB of LDS)
constexpr uint32_t kResampleRegLdsFloats = 16128;       // the register form's run at most (63 KB: under what a launch takes unasked)
constexpr uint32_t kResampleLdsFloats = 38912;          // table and run of the LDS form at most (152 KB of the CU's 160)
constexpr uint32_t kResampleRegThreads = 512;           // the register form's workgroup at most
constexpr uint32_t kResampleRegTapsMax = 128;           // ... and the taps it holds at most
constexpr uint32_t kResampleThreads = 256;              // the other two forms' workgroup

// frames of a tile's input run: the last output reads up to frame ((R L - 1) M) / L + T - 1 of it
__host__ __device__ inline uint64_t resample_run_frames(uint64_t R, uint64_t L, uint64_t M, uint64_t T) { return (R * L - 1u) * M / L + T; }

struct ResampleTile {
    uint32_t stream, n_out;                 // outputs of this tile (the last tile of a stream: fewer)
    unsigned long long F, n0;               // the stream's own frames; the tile's first output
    long long in0;                          // input frame of the run's first frame (negative in front of the stream)
};

// which (stream, tile) this workgroup has; false: the tile lies behind the stream's output
__device__ __forceinline__ bool resample_tile(const ResampleParams &p, ResampleTile &t)
{
    t.stream = blockIdx.x / p.tiles_cap;
    const uint32_t tile = blockIdx.x - t.stream * p.tiles_cap;
    t.F = p.frames_of ? p.frames_of[t.stream] : p.n_frames;
    if (t.F > p.n_frames) t.F = p.n_frames;
    const unsigned long long f_out = (t.F * p.up + p.down - 1u) / p.down;
    const unsigned long long per = (unsigned long long)p.plan.tile_periods * p.up;
    t.n0 = tile * per;
    if (t.n0 >= f_out) return false;
    t.n_out = (uint32_t)(f_out - t.n0 < per ? f_out - t.n0 : per);
    t.in0 = (long long)((unsigned long long)tile * p.plan.tile_periods * p.down) - (long long)(p.n_taps / 2u - 1u);
    return true;
}

// the tile's input run into LDS; returns x0 with x0[j * C + c] = frame in0 + j of the stream, channel c (zero outside [0, F))
__device__ __forceinline__ const float *resample_load(float *sh, const ResampleParams &p, const ResampleTile &t, uint32_t C)
{
    const long long base = (long long)((unsigned long long)t.stream * p.src_stride);        // the stream's frame 0, in floats
    const long long run = (long long)resample_run_frames(p.plan.tile_periods, p.up, p.down, p.n_taps);
    const long long g0 = base + t.in0 * (long long)C, g1 = g0 + run * (long long)C;
    const long long end = t.in0 + run < (long long)t.F ? t.in0 + run : (long long)t.F;
    const uint32_t shift = (uint32_t)(g0 & 3ll);
    const long long first = g0 - shift;
    peak_load_tile(sh, p.src, first, base > g0 ? base : g0, base + end * (long long)C, (uint32_t)((g1 - first + 3) >> 2), blockDim.x);
    return sh + shift;
}

// one output's chains: tap[k] (registers: TMAX > 0 unrolls to TMAX in groups of four, each behind k < T) times the frames x[k * C + c]
template <int TMAX, int CT, class Taps>
__device__ __forceinline__ void resample_chain(const Taps &tap, const float *x, float *y, uint32_t C, uint32_t T)
{
    if constexpr (CT == 2) {
        float a0 = 0.f, a1 = 0.f;
        if constexpr (TMAX > 0) {
#pragma unroll
            for (int k4 = 0; k4 < TMAX; k4 += 4) {
                if ((uint32_t)k4 < T) {                         // (uniform; no loop exit, so the loop unrolls and tap[] stays in registers)
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        const float2 v = *reinterpret_cast<const float2 *>(x + 2 * (k4 + d));
                        a0 = __builtin_fmaf(tap[k4 + d], v.x, a0); a1 = __builtin_fmaf(tap[k4 + d], v.y, a1);
                    }
                }
            }
        } else {
#pragma unroll 4
            for (uint32_t k = 0; k < T; k++) {
                const float2 v = *reinterpret_cast<const float2 *>(x + 2u * k);
                a0 = __builtin_fmaf(tap[k], v.x, a0); a1 = __builtin_fmaf(tap[k], v.y, a1);
            }
        }
        *reinterpret_cast<float2 *>(y) = make_float2(a0, a1);
    } else {
        for (uint32_t c = 0; c < C; c++) {
            float a = 0.f;
            const float *xc = x + c;
            if constexpr (TMAX > 0) {
#pragma unroll
                for (int k4 = 0; k4 < TMAX; k4 += 4) {
                    if ((uint32_t)k4 < T) {
#pragma unroll
                        for (int d = 0; d < 4; d++) a = __builtin_fmaf(tap[k4 + d], xc[(size_t)(k4 + d) * C], a);
                    }
                }
            } else {
#pragma unroll 4
                for (uint32_t k = 0; k < T; k++) a = __builtin_fmaf(tap[k], xc[(size_t)k * C], a);
            }
            y[c] = a;
        }
    }
}

}  // namespace

// TMAX: the taps a lane can hold (T <= TMAX); CT: channels, 1 or 2 (with the channel count a run-time value the compiler's schedule
// of the unrolled chain takes 249 registers at TMAX = 80 and spills at 128: other channel counts take k_resample_lds)
template <int TMAX, int CT>
__global__ __launch_bounds__(kResampleRegThreads) void k_resample_reg(ResampleParams p)
{
    extern __shared__ float4 sh4[];
    ResampleTile t;
    if (!resample_tile(p, t)) return;                           // (the whole workgroup)
    const uint32_t C = CT ? (uint32_t)CT : p.channels, L = p.up, M = p.down, T = p.n_taps, G = p.plan.groups;
    const uint32_t g = threadIdx.x / L, r = threadIdx.x - g * L;
    const bool active = g < G;
    const uint32_t rm = r * M, ph = rm % L, roff = rm / L;      // the lane's phase, and its frame within a period's input
    float tap[TMAX];
    if (active) {
        const float4 *row = reinterpret_cast<const float4 *>(p.taps + (size_t)ph * T);
#pragma unroll
        for (int k4 = 0; k4 < TMAX; k4 += 4) {
            if ((uint32_t)k4 < T) {
                const float4 v = row[k4 >> 2];
                tap[k4] = v.x; tap[k4 + 1] = v.y; tap[k4 + 2] = v.z; tap[k4 + 3] = v.w;
            }
        }
    }
    const float *x0 = resample_load(reinterpret_cast<float *>(sh4), p, t, C);
    __syncthreads();
    if (!active) return;
    float *out = p.dst + (size_t)t.stream * p.dst_stride + (size_t)t.n0 * C;
    for (uint32_t j = g;; j += G) {
        const uint32_t i = j * L + r;                           // the output, within the tile
        if (i >= t.n_out) break;
        resample_chain<TMAX, CT>(tap, x0 + (size_t)(j * M + roff) * C, out + (size_t)i * C, C, T);
    }
}

// CT: channels at compile time (1, 2; 0: any)
template <int CT>
__global__ __launch_bounds__(kResampleThreads) void k_resample_lds(ResampleParams p)
{
    extern __shared__ float4 sh4[];
    float *sh = reinterpret_cast<float *>(sh4);
    ResampleTile t;
    if (!resample_tile(p, t)) return;
    const uint32_t C = CT ? (uint32_t)CT : p.channels, L = p.up, M = p.down, T = p.n_taps, TS = T + 1u;
    {   // the table, row by row: a lane's (row, column) is divided out once and then stepped by the workgroup's size
        const uint32_t step_ph = kResampleThreads / T, step_k = kResampleThreads - step_ph * T;
        uint32_t ph = threadIdx.x / T, k = threadIdx.x - ph * T;
#pragma unroll 4
        for (uint32_t idx = threadIdx.x; idx < L * T; idx += kResampleThreads) {        // (counted by idx, so that the loads of several rounds are in flight)
            sh[ph * TS + k] = p.taps[idx];
            ph += step_ph; k += step_k;
            if (k >= T) { k -= T; ph++; }
        }
    }
    const float *x0 = resample_load(sh + ((L * TS + 3u) & ~3u), p, t, C);
    __syncthreads();
    float *out = p.dst + (size_t)t.stream * p.dst_stride + (size_t)t.n0 * C;
    for (uint32_t i = threadIdx.x; i < t.n_out; i += kResampleThreads) {
        const uint32_t im = i * M, ph = im % L;
        resample_chain<0, CT>(sh + ph * TS, x0 + (size_t)(im / L) * C, out + (size_t)i * C, C, T);
    }
}

__global__ __launch_bounds__(kResampleThreads) void k_resample_direct(ResampleParams p)
{
    ResampleTile t;
    if (!resample_tile(p, t)) return;
    const uint32_t C = p.channels, L = p.up, M = p.down, T = p.n_taps;
    const float *in = p.src + (size_t)t.stream * p.src_stride;
    float *out = p.dst + (size_t)t.stream * p.dst_stride + (size_t)t.n0 * C;
    const unsigned long long items = (unsigned long long)t.n_out * C;
    for (unsigned long long item = threadIdx.x; item < items; item += kResampleThreads) {
        const uint32_t i = (uint32_t)(item / C), c = (uint32_t)(item - (unsigned long long)i * C);
        const unsigned long long im = (unsigned long long)i * M;
        const float *tap = p.taps + (size_t)(im % L) * T;
        const long long at = t.in0 + (long long)(im / L);
        float a = 0.f;
        for (uint32_t k = 0; k < T; k++) {
            const long long f = at + k;
            const float x = f >= 0 && f < (long long)t.F ? in[(size_t)f * C + c] : 0.f;
            a = __builtin_fmaf(tap[k], x, a);
        }
        out[item] = a;
    }
}

// How a call cuts the streams.  R aims at a run of kResampleTileFloats floats.  The register form (mono and stereo, T <= 128, L <= 512)
// takes the G residue groups that
// leave the fewest lanes of its waves idle (among equals the workgroup nearest 256 lanes: small L would otherwise end in one wave
// beside a 32 KB tile) and a whole number of rounds of them; the LDS form gives up periods until table and run fit.
ResamplePlan plan_resample(uint32_t up, uint32_t down, uint32_t taps, uint32_t channels, uint32_t form)
{
    const uint64_t L = up, M = down, T = taps, C = channels ? channels : 1u;
    auto tile_floats = [&](uint64_t R) { return resample_run_frames(R, L, M, T) * C + 8u; };     // (+ 8: the copy's alignment at both ends)
    auto periods_within = [&](uint64_t floats) -> uint64_t {                                    // the most R whose run fits, 0: none
        if (floats < 8u || (floats - 8u) / C < T + M) return tile_floats(1) <= floats ? 1u : 0u;
        uint64_t R = ((floats - 8u) / C - T) / M;                                               // (a run is at most R M + T frames)
        while (tile_floats(R + 1u) <= floats) R++;
        return R;
    };
    uint64_t most = 0x7FFFFFFFull / (L * M);                    // i * M and R * L * M stay in 31 bits
    if (most > 65536u / L) most = 65536u / L;                   // (a tile of 2^16 outputs at most: steep upsampling has short runs)
    if (!most) most = 1u;
    ResamplePlan plan{};
    plan.threads = kResampleThreads;
    if (form <= kResampleRegTaps && channels <= 2u && T <= kResampleRegTapsMax && L <= kResampleRegThreads) {
        uint64_t R = periods_within(kResampleTileFloats);
        if (!R) R = periods_within(kResampleRegLdsFloats) ? 1u : 0u;
        if (R > most) R = most;
        if (R) {
            uint32_t G = 1, threads = 64;
            double fill = 0.0;
            for (uint64_t cand = 1; cand * L <= kResampleRegThreads && cand <= R; cand++) {
                const uint32_t th = (uint32_t)((cand * L + 63u) / 64u * 64u);
                const double f = (double)(cand * L) / th;
                const bool nearer = (th > 256u ? th - 256u : 256u - th) < (threads > 256u ? threads - 256u : 256u - threads);
                if (f > fill || (f == fill && nearer)) { fill = f; G = (uint32_t)cand; threads = th; }
            }
            R -= R % G;
            plan.form = kResampleRegTaps; plan.tile_periods = (uint32_t)R; plan.groups = G; plan.threads = threads;
            plan.lds_bytes = (uint32_t)(tile_floats(R) * sizeof(float));
            return plan;
        }
    }
    if (form <= kResampleLdsTaps) {
        const uint64_t table = (L * (T + 1u) + 3u) & ~3ull;
        if (table < kResampleLdsFloats) {
            uint64_t R = periods_within(kResampleTileFloats);
            if (!R || table + tile_floats(R) > kResampleLdsFloats) R = periods_within(kResampleLdsFloats - table);
            if (R > most) R = most;
            if (R) {
                plan.form = kResampleLdsTaps; plan.tile_periods = (uint32_t)R;
                plan.lds_bytes = (uint32_t)((table + tile_floats(R)) * sizeof(float));
                return plan;
            }
        }
    }
    uint64_t R = (kResampleTileFloats / C + L - 1u) / L;        // the direct form stages nothing: a few thousand samples per workgroup
    if (R > most) R = most;
    plan.form = kResampleDirect; plan.tile_periods = (uint32_t)(R ? R : 1u);
    return plan;
}

namespace {

template <int CT>
hipError_t launch_resample_lds(const ResampleParams &p, const dim3 &grid, hipStream_t s)
{
    static DevicePrep prepared;
    const void *fn = reinterpret_cast<const void *>(k_resample_lds<CT>);
    const hipError_t pe = prepare_on_device(prepared, [fn] {
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kResampleLdsFloats * sizeof(float)));
    });
    if (pe != hipSuccess) return pe;
    hipLaunchKernelGGL(k_resample_lds<CT>, grid, dim3(kResampleThreads), p.plan.lds_bytes, s, p);
    return hipGetLastError();
}

template <int TMAX>
hipError_t launch_resample_reg(const ResampleParams &p, const dim3 &grid, hipStream_t s)
{
    const dim3 block(p.plan.threads);
    if (p.channels == 1u) hipLaunchKernelGGL((k_resample_reg<TMAX, 1>), grid, block, p.plan.lds_bytes, s, p);
    else if (p.channels == 2u) hipLaunchKernelGGL((k_resample_reg<TMAX, 2>), grid, block, p.plan.lds_bytes, s, p);
    else return hipErrorInvalidValue;                           // (plan_resample gives other channel counts the LDS form)
    return hipGetLastError();
}

}  // namespace

hipError_t launch_resample(const ResampleParams &p, hipStream_t s)
{
    const uint64_t groups = (uint64_t)p.n_streams * p.tiles_cap;
    if (!groups) return hipSuccess;
    if (groups > 0x7FFFFFFFull || !p.channels || p.channels > (uint32_t)kMaxChannels || !p.up || !p.down || p.n_taps < 4u ||
        (p.n_taps & 3u) || (uint64_t)p.up * p.n_taps > SS_RESAMPLE_TAPS_MAX)
        return hipErrorInvalidValue;
    if ((p.channels == 2u && ((p.src_stride | p.dst_stride) & 1u)) || p.src_stride < p.n_frames * p.channels) return hipErrorInvalidValue;
    // the plan is plan_resample's own: the kernels' LDS and index ranges rest on it
    const ResamplePlan q = plan_resample(p.up, p.down, p.n_taps, p.channels, p.plan.form);
    if (q.form != p.plan.form || q.tile_periods != p.plan.tile_periods || q.groups != p.plan.groups || q.threads != p.plan.threads ||
        q.lds_bytes != p.plan.lds_bytes)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups);
    if (q.form == kResampleRegTaps) return p.n_taps <= 80u ? launch_resample_reg<80>(p, grid, s) : launch_resample_reg<(int)kResampleRegTapsMax>(p, grid, s);
    if (q.form == kResampleLdsTaps)
        return p.channels == 1u ? launch_resample_lds<1>(p, grid, s) : p.channels == 2u ? launch_resample_lds<2>(p, grid, s) : launch_resample_lds<0>(p, grid, s);
    hipLaunchKernelGGL(k_resample_direct, grid, dim3(kResampleThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace ssk
