// ss_pair_series.hip: how two channels of a stream relate in the time domain — the f64 sums of x_a^2, x_b^2 and x_a x_b of every
// 100 ms entry of every stream of a batch (ss_batch_pair_series), and their reduction over time ranges and groups of ranges with
// the entries below a correlation threshold and their runs (ss_batch_pair_regions) — hand-written gfx950 (CDNA4, wave64) kernels.
// Not in the reference.  Definition: include/soundscope_hip.h; plan and figures: DESIGN.md section 3.3.4.
//
// k_pair_series: one workgroup per (stream, entry), the peak series' grid.  Nothing is staged: a lane reads its frames from the
// corpus into registers, four loads in flight, widens both samples to f64 and adds the three products (exact in f64) with one
// fused multiply-add each, in ascending frames.  A frame with a NaN or an infinity in either sample adds to no sum and is counted.
// The lanes of a wave then meet in a fixed butterfly (__shfl_xor, distances 32 .. 1: the same tree in every lane), the four waves
// in wave order in LDS.  No atomics; global memory sees two 16-byte stores per record.
//   <true>  two channels, one pair of distinct channels: the entry's floats [lo, hi) are whole frames, so lo and hi are even and the
//           run is 16-byte loads (two frames each) on its aligned inside with at most one lone frame at each end, read as two
//           4-byte loads (peak_load_tile's guard rule: no float outside [lo, hi) is touched).
//   <false> any channel count and pair list: 4-byte loads at the frame's stride, pair after pair (the pairs of a frame share its
//           cache lines).
// k_region_pairs: one lane per (region, pair) walks the region's entries in ascending order — the sums are DEFINED as that
// sequential f64 sum, and the runs are a state machine over the same order.  k_group_pairs: one wave per (group, pair) walks the
// region list 64 regions at a time and adds the records that name the group in ascending region order.
// The lane sums, the workgroup's tree, the entry record and the ACTIVE / BELOW decision live in ss_pair_series_dev.h, shared with
// the meter banks' pair watch (ss_bank_pair_watch.hip).
#include "ss_kernels.h"
#include "ss_pair_series_dev.h"

namespace ssk {

namespace {

constexpr uint32_t kPairNone = 0xFFFFFFFFu;

}  // namespace

template <bool STEREO>
__global__ __launch_bounds__(kPairThreads) void k_pair_series(PairSeriesParams p)
{
    __shared__ double part[kPairWaves * 4];
    const uint32_t stream = blockIdx.x / p.entries_cap, entry = blockIdx.x - stream * p.entries_cap;
    const uint32_t C = p.channels, S = p.s100, tid = threadIdx.x;
    unsigned long long F = p.frames_of ? p.frames_of[stream] : p.n_frames;
    if (F > p.n_frames) F = p.n_frames;
    const unsigned long long e_begin = (unsigned long long)entry * S;
    if (e_begin >= F) return;                                   // (the whole workgroup: entry >= E_s)
    const unsigned long long e_end = e_begin + S < F ? e_begin + S : F;
    const uint32_t e_frames = (uint32_t)(e_end - e_begin);
    const long long base = (long long)((unsigned long long)stream * p.stream_stride);      // the stream's frame 0, in floats
    PairEntry *out = p.series + ((size_t)stream * p.entries_cap + entry) * p.n_pairs;
    if (STEREO) {
        // floats [lo, hi) of the corpus, both even; vectors [v_lo, v_hi) of four floats from `first` lie wholly inside
        const long long lo = base + 2ll * (long long)e_begin, hi = lo + 2ll * (long long)e_frames;
        const uint32_t shift = (uint32_t)(lo & 3ll);            // 0 or 2: a lone frame in front of the first whole vector
        const long long first = lo - shift;
        const uint32_t v_lo = shift ? 1u : 0u, v_hi = (uint32_t)((hi - first) >> 2);
        const bool tail = ((hi - first) & 3ll) != 0;            // a lone frame behind the last whole vector
        const float4 *src = reinterpret_cast<const float4 *>(p.pcm + first);
        PairSums s;
        if (tid == 0u && shift) s.add(p.pcm[lo], p.pcm[lo + 1]);
        for (uint32_t v0 = v_lo + tid; v0 < v_hi; v0 += kPairDepth * kPairThreads) {
            float4 x[kPairDepth];
#pragma unroll
            for (uint32_t j = 0; j < kPairDepth; j++) x[j] = src[v0 + j * kPairThreads < v_hi ? v0 + j * kPairThreads : v0];   // (a whole vector either way)
#pragma unroll
            for (uint32_t j = 0; j < kPairDepth; j++) {
                if (v0 + j * kPairThreads < v_hi) { s.add(x[j].x, x[j].y); s.add(x[j].z, x[j].w); }
            }
        }
        if (tid == kPairThreads - 1u && tail) s.add(p.pcm[hi - 2], p.pcm[hi - 1]);
        pair_reduce(s, part);
        if (tid == 0u) pair_store(out, s, e_frames, p.pairs[0].a != 0u);
    } else {
        const float *x0 = p.pcm + base + (long long)e_begin * (long long)C;     // frame f of the entry, channel c: x0[f C + c]
        for (uint32_t k = 0; k < p.n_pairs; k++) {
            const uint32_t a = p.pairs[k].a, b = p.pairs[k].b;
            PairSums s;
            for (uint32_t f0 = tid; f0 < e_frames; f0 += kPairDepth * kPairThreads) {
                float xa[kPairDepth], xb[kPairDepth];
#pragma unroll
                for (uint32_t j = 0; j < kPairDepth; j++) {
                    const size_t f = f0 + j * kPairThreads < e_frames ? f0 + j * kPairThreads : f0;       // (a frame of the entry either way)
                    xa[j] = x0[f * C + a]; xb[j] = x0[f * C + b];
                }
#pragma unroll
                for (uint32_t j = 0; j < kPairDepth; j++) if (f0 + j * kPairThreads < e_frames) s.add(xa[j], xb[j]);
            }
            pair_reduce(s, part);
            if (tid == 0u) pair_store(out + k, s, e_frames, false);
        }
    }
}

PairSeriesPlan plan_pair_series(uint32_t channels, uint32_t s100, uint64_t n_frames, const ChannelPair *pairs, uint32_t n_pairs)
{
    PairSeriesPlan plan;
    plan.stereo = channels == 2u && n_pairs == 1u && pairs[0].a != pairs[0].b;
    plan.sweep_frames = kPairDepth * kPairThreads * (plan.stereo ? 2u : 1u);
    plan.entries_cap = plan_peak_series(channels, s100, n_frames).entries_cap;
    return plan;
}

hipError_t launch_pair_series(const PairSeriesParams &p, hipStream_t s)
{
    const uint64_t groups = (uint64_t)p.n_streams * p.entries_cap;
    if (!groups) return hipSuccess;
    if (groups > 0x7FFFFFFFull || !p.channels || p.channels > (uint32_t)kMaxChannels || !p.s100 || !p.n_pairs || p.n_pairs > kMaxPairs)
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < p.n_pairs; k++) if (p.pairs[k].a >= p.channels || p.pairs[k].b >= p.channels) return hipErrorInvalidValue;
    if (p.stereo && (p.channels != 2u || p.n_pairs != 1u || p.pairs[0].a == p.pairs[0].b || (p.stream_stride & 1u))) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)groups), block(kPairThreads);
    if (p.stereo) hipLaunchKernelGGL(k_pair_series<true>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_pair_series<false>, grid, block, 0, s, p);
    return hipGetLastError();
}

// ============================================================================
//  Pair regions (ss_batch_pair_regions): the series over runs of one stream's entries, pooled into groups
// ============================================================================
// one lane per (region, pair); the entries' records four at a time (the loads do not wait for the sums)
__global__ __launch_bounds__(64) void k_region_pairs(RegionPairsParams p)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x, NP = p.n_pairs;
    const uint32_t r = i / NP, k = i - r * NP;
    if (r >= p.n_regions) return;
    const LoudnessRegion rg = p.regions[r];
    const uint4 *ser = reinterpret_cast<const uint4 *>(p.series + (size_t)rg.stream * p.entries_cap * NP + k);       // entry j: ser[2 j NP], [2 j NP + 1]
    const uint32_t end = rg.first_subblock + rg.n_subblocks;
    const double t = p.threshold, tt = __dmul_rn(t, t);
    RegionPair out;
    out.s_aa = 0.0; out.s_bb = 0.0; out.s_ab = 0.0; out.frames = 0ull; out.skipped = 0ull;
    out.n_active = 0u; out.n_below = 0u; out.first_below = kPairNone; out.longest_below = 0u; out.longest_below_at = kPairNone; out.below_runs = 0u;
    uint32_t run = 0u;                                          // entries of the open run
    for (uint32_t j0 = rg.first_subblock; j0 < end; j0 += 4u) {
        uint4 lo[4], hi[4];
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            const size_t j = j0 + d < end ? j0 + d : j0;
            lo[d] = ser[2u * j * NP]; hi[d] = ser[2u * j * NP + 1u];
        }
#pragma unroll
        for (uint32_t d = 0; d < 4u; d++) {
            const uint32_t j = j0 + d;
            if (j >= end) break;
            const double aa = __longlong_as_double((long long)((unsigned long long)lo[d].y << 32 | lo[d].x));
            const double bb = __longlong_as_double((long long)((unsigned long long)lo[d].w << 32 | lo[d].z));
            const double ab = __longlong_as_double((long long)((unsigned long long)hi[d].y << 32 | hi[d].x));
            const uint32_t frames = hi[d].z, skipped = hi[d].w;
            out.s_aa = __dadd_rn(out.s_aa, aa); out.s_bb = __dadd_rn(out.s_bb, bb); out.s_ab = __dadd_rn(out.s_ab, ab);
            out.frames += frames; out.skipped += skipped;
            SS_PAIR_DECIDE(active, below, aa, bb, ab, frames, p.power_floor, t, tt);
            if (active) out.n_active++;
            if (active && below) {
                out.n_below++;
                if (out.first_below == kPairNone) out.first_below = j;
                run++;
                if (run > out.longest_below) { out.longest_below = run; out.longest_below_at = j + 1u - run; }
                if (run == p.min_run) out.below_runs++;         // (once per run, when it reaches the minimum)
            } else {
                run = 0u;
            }
        }
    }
    p.results[i] = out;
}

// One wave per (group, pair).  A round takes 64 regions of the list, a lane one: its group word and, where it names the group, its
// record — the loads of a round are in flight together.  The members' sums are then added in lane order, which is region index
// order (every lane holds the same running sums); the counts are integers, so each lane keeps its own and the wave adds them last.
__global__ __launch_bounds__(64) void k_group_pairs(RegionPairsParams p)
{
    const uint32_t NP = p.n_pairs, g = blockIdx.x / NP, k = blockIdx.x - g * NP, lane = threadIdx.x;
    double aa = 0.0, bb = 0.0, ab = 0.0;
    unsigned long long n[5] = {0ull, 0ull, 0ull, 0ull, 0ull};  // frames, skipped, n_active, n_below, below_runs
    for (uint32_t r0 = 0; r0 < p.n_regions; r0 += 64u) {
        const uint32_t r = r0 + lane;
        const bool mine = r < p.n_regions && p.regions[r].group == g;
        double xa = 0.0, xb = 0.0, xab = 0.0;
        if (mine) {
            const RegionPair x = p.results[(size_t)r * NP + k];
            xa = x.s_aa; xb = x.s_bb; xab = x.s_ab;
            n[0] += x.frames; n[1] += x.skipped; n[2] += x.n_active; n[3] += x.n_below; n[4] += x.below_runs;
        }
        for (unsigned long long m = __ballot(mine); m; m &= m - 1ull) {          // (the same word in every lane)
            const int l = __builtin_ctzll(m);
            aa = __dadd_rn(aa, __shfl(xa, l)); bb = __dadd_rn(bb, __shfl(xb, l)); ab = __dadd_rn(ab, __shfl(xab, l));
        }
    }
#pragma unroll
    for (int d = 32; d; d >>= 1)
#pragma unroll
        for (int i = 0; i < 5; i++) n[i] += __shfl_xor(n[i], d);
    if (lane == 0u) {
        GroupPair out;
        out.s_aa = aa; out.s_bb = bb; out.s_ab = ab;
        out.frames = n[0]; out.skipped = n[1]; out.n_active = n[2]; out.n_below = n[3]; out.below_runs = n[4];
        p.group_results[blockIdx.x] = out;
    }
}

hipError_t launch_region_pairs(const RegionPairsParams &p, hipStream_t s)
{
    if (!p.n_pairs || p.n_pairs > kMaxPairs || (uint64_t)p.n_regions * p.n_pairs > 0x7FFFFFFFull || (uint64_t)p.n_groups * p.n_pairs > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const uint32_t nr = p.n_regions * p.n_pairs, ng = p.n_groups * p.n_pairs;
    if (nr) hipLaunchKernelGGL(k_region_pairs, dim3((nr + 63u) / 64u), dim3(64), 0, s, p);
    if (ng) hipLaunchKernelGGL(k_group_pairs, dim3(ng), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace ssk
