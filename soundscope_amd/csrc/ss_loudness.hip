// ss_loudness.hip: gating blocks, histograms, integrated loudness, LRA, ring energies — hand-written gfx950 (CDNA4, wave64) kernels of the soundscope analyzer hot path.
// Reference semantics: /root/reference/src/analyzer.rs (get_fft :55-105, get_waveform :107-137,
// add_samples/getters :139-164, calculate_integrated_lufs :170-182) and src/audio_player.rs:400-419, plus the
// arithmetic of ebur128 0.1.10 / spectrum-analyzer 1.7.0 / microfft 0.6.0 as restated in DESIGN.md.
// Nothing here is translated from the reference: the reference has no GPU code.
#include "ss_kernels.h"
#include "ss_loudness_dev.h"
#include <type_traits>

namespace ssk {
// ============================================================================
//  Gating blocks, histograms, integrated loudness and LRA
//  (ebur128 calc_gating_block / loudness_global / loudness_range, histogram mode)
// ============================================================================
// largest i with bounds[i] <= energy (the caller has checked energy >= bounds[0]) — what ebur128's binary search
// over the bin boundaries returns.  bounds[i] is the energy of -70 + i/10 LUFS, so the index is guessed in closed
// form and then corrected against the table itself (at most a step or two): two dependent loads instead of ten.
__device__ __forceinline__ uint32_t hist_index(const double *__restrict__ bounds, double energy)
{
    const double g = (10.0 * log10(energy) - 0.691 + 70.0) * 10.0;
    int i = g > 0.0 ? (g < (double)(kHistBins - 1) ? (int)g : kHistBins - 1) : 0;
    while (i > 0 && energy < bounds[i]) i--;
    while (i < kHistBins - 1 && energy >= bounds[i + 1]) i++;
    return (uint32_t)i;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// First sub-block of a stream in which a WEIGHTED channel met a non-finite sample (TdState::bad_key), 0xFFFFFFFF if none: one whole
// wave asks, every lane gets the answer.  The crate's filter state is NaN from that sample on, for good: every window that ends
// BEHIND this sub-block has a NaN energy (`sum >= boundary` fails: no histogram entry), whichever segment of a launch computed
// its sub-blocks from whichever starting state; the window that ends WITH it holds what the recurrence itself produced (NaN, or
// +Inf if the sample was an infinity in the sub-block's very last frame).  Channels the crate does not filter (weight 0) never count.
__device__ __forceinline__ uint32_t first_bad_subblock(const TdState *st, uint32_t C, const double *__restrict__ weights, uint32_t lane)
{
    uint32_t key = 0u;
    if (st) for (uint32_t c = lane; c < C; c += 64u) { const uint32_t k = st->bad_key[c]; if (weights[c] != 0.0 && k > key) key = k; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)key, o, 64); key = t > key ? t : key; }
    return ~key;
}

// one wave evaluates gate and LRA on an LDS histogram pair (block, short-term); inlined: `en` / `bd` are LDS copies of the tables
// in the latency-bound callers (every dependent table read is then an LDS access, not a round trip to L2)
__device__ __forceinline__ void eval_hist(const unsigned long long *hb, const unsigned long long *hs,
                          const double *__restrict__ en, const double *__restrict__ bd,
                          double *out_i, double *out_lra)
{
    const int lane = threadIdx.x & 63;
    // ---- integrated: relative gate at -10 LU of the mean of all blocks
    double sum = 0.0; unsigned long long cnt = 0;
    for (int i = lane; i < kHistBins; i += 64) { sum += (double)hb[i] * en[i]; cnt += hb[i]; }
    sum = wave_sum(sum); cnt = wave_sum(cnt);
    double integrated;
    if (cnt == 0) integrated = -INFINITY;
    else {
        const double rel = (sum / (double)cnt) * 0.1;
        uint32_t start;
        if (rel < bd[0]) start = 0;
        else { start = hist_index(bd, rel); if (rel > en[start]) start++; }
        double g = 0.0; unsigned long long c2 = 0;
        for (int i = lane; i < kHistBins; i += 64) if ((uint32_t)i >= start) { g += (double)hb[i] * en[i]; c2 += hb[i]; }
        g = wave_sum(g); c2 = wave_sum(c2);
        integrated = c2 ? 10.0 * log10(g / (double)c2) - 0.691 : -INFINITY;
    }
    // ---- LRA (EBU Tech 3342) on the short-term histogram
    double power = 0.0; unsigned long long size = 0;
    for (int i = lane; i < kHistBins; i += 64) { power += (double)hs[i] * en[i]; size += hs[i]; }
    power = wave_sum(power); size = wave_sum(size);
    double lra = 0.0;
    if (size != 0) {
        const double integ = 0.01 * (power / (double)size);
        uint32_t index;
        if (integ < bd[0]) index = 0;
        else { index = hist_index(bd, integ); if (integ > en[index]) index++; }
        // Percentile bins without a serial walk over the histogram: lane l owns bins [16 l, 16 l + 16), an inclusive scan
        // over the lanes' gated counts tells which lane holds an entry of a given rank, and that lane walks its own 16
        // bins.  (ebur128 walks all bins from the gate: `while acc <= rank { acc += hist[j]; j += 1 }`, entry = bin j - 1,
        // i.e. the first bin at which the cumulative gated count exceeds the rank.)
        const int b0 = lane * 16;
        unsigned long long own = 0;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int i = b0 + ((q + lane) & 15);                    // rotated start: spreads the lanes over the LDS banks
            if (i < kHistBins && (uint32_t)i >= index) own += hs[i];
        }
        unsigned long long incl = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const unsigned long long above = __shfl(incl, 63, 64);
        if (above != 0) {
            const unsigned long long plow = (unsigned long long)((double)(above - 1) * 0.1 + 0.5);
            const unsigned long long phigh = (unsigned long long)((double)(above - 1) * 0.95 + 0.5);
            const unsigned long long excl = incl - own;
            auto energy_of_rank = [&](unsigned long long r) -> double {
                const bool mine = excl <= r && r < incl;             // exactly one lane (ranks are < above)
                double e = 0.0;
                if (mine) {
                    unsigned long long acc = excl;
                    int j = b0 > (int)index ? b0 : (int)index;
                    for (;;) { acc += hs[j]; if (acc > r) break; j++; }
                    e = en[j];
                }
                const int src = __ffsll((long long)__ballot(mine)) - 1;
                return __shfl(e, src, 64);
            };
            const double l_en = energy_of_rank(plow), h_en = energy_of_rank(phigh);
            lra = (10.0 * log10(h_en) - 0.691) - (10.0 * log10(l_en) - 0.691);
        }
    }
    if (lane == 0) { if (out_i) *out_i = integrated; if (out_lra) *out_lra = lra; }
}

// slot of sub-block (j - q) in a ring of `cap` slots, given jm = j % cap and q <= 29 (no division per term)
__device__ __forceinline__ uint32_t ring_back(uint32_t jm, uint32_t q, uint32_t cap)
{
    uint32_t s = jm + cap * 30u - q;          // cap >= 1: the bias keeps it positive for q <= 29 < 30 cap
    return s % cap;
}

// Weighted energy of the N sub-blocks ending with sub-block j (slot jm = j % cap):  sum_c w_c (P[j-N+1][c] + ... + P[j][c]),
// each channel added oldest first.  All loads of a batch are issued before the first addition — written as a loop of
// `cs += P[...]` the thirty terms of a short-term block were thirty dependent round trips to memory (12 us of a tick, and
// the whole of this kernel's time on a long stream).
template <int N, bool DIRECT, int KB = (N < 10 ? N : 10)>
__device__ __forceinline__ double window_energy(const double *__restrict__ P, uint32_t jm, uint32_t cap, uint32_t C,
                                                const double *__restrict__ weights)
{
    constexpr int kBatch = KB;
    static_assert(N % kBatch == 0, "whole batches");
    uint32_t s0 = DIRECT ? jm - (uint32_t)(N - 1) : ring_back(jm, (uint32_t)(N - 1), cap);      // slot of the oldest term
    double sum = 0.0;
    for (uint32_t c = 0; c < C; c++) {
        const double w = weights[c];
        if (w == 0.0) continue;
        double cs = 0.0;
        uint32_t sl = s0;
#pragma unroll
        for (int b = 0; b < N; b += kBatch) {
            double v[kBatch];
#pragma unroll
            for (int q = 0; q < kBatch; q++) {
                v[q] = P[(size_t)sl * C + c];
                sl = DIRECT ? sl + 1u : (sl + 1u == cap ? 0u : sl + 1u);
            }
#pragma unroll
            for (int q = 0; q < kBatch; q++) cs += v[q];
        }
        sum += w * cs;
    }
    return sum;
}

// The same sums for the latency-bound launches (a handful of streams: the kernel's time is its chain of dependent round trips to
// memory, not its work): channels two at a time, every term of both and their weights requested before anything is used — ONE
// round trip per pair of channels where the form above takes one for the weight and N / 10 per channel behind it.  Same additions
// in the same order (a channel whose weight is zero is loaded and dropped, as the `continue` above drops it unread).
template <int N, bool DIRECT>
__device__ __forceinline__ double window_energy_eager(const double *__restrict__ P, uint32_t jm, uint32_t cap, uint32_t C,
                                                      const double *__restrict__ weights)
{
    const uint32_t s0 = DIRECT ? jm - (uint32_t)(N - 1) : ring_back(jm, (uint32_t)(N - 1), cap);
    double sum = 0.0;
    for (uint32_t c = 0; c < C; c += 2) {
        const bool two = c + 1u < C;
        const uint32_t c1 = two ? c + 1u : c;
        const double w0 = weights[c], w1 = weights[c1];
        double v0[N], v1[N];
        uint32_t sl = s0;
#pragma unroll
        for (int q = 0; q < N; q++) {
            v0[q] = P[(size_t)sl * C + c];
            v1[q] = P[(size_t)sl * C + c1];
            sl = DIRECT ? sl + 1u : (sl + 1u == cap ? 0u : sl + 1u);
        }
        double cs0 = 0.0, cs1 = 0.0;
#pragma unroll
        for (int q = 0; q < N; q++) { cs0 += v0[q]; cs1 += v1[q]; }
        if (w0 != 0.0) sum += w0 * cs0;
        if (two && w1 != 0.0) sum += w1 * cs1;
    }
    return sum;
}

// The weighted energy of the N sub-blocks ending with sub-block j, in the form its launch takes: EAGER for the latency-bound
// launches (window_energy_eager), DIRECT where slot == sub-block index (batches; otherwise a ring of `cap` slots)
template <int N, bool EAGER, bool DIRECT>
__device__ __forceinline__ double block_energy(const double *__restrict__ P, uint64_t j, uint32_t cap, uint32_t C,
                                               const double *__restrict__ weights)
{
    const uint32_t jm = DIRECT ? (uint32_t)j : (uint32_t)(j % cap);
    return EAGER ? window_energy_eager<N, DIRECT>(P, jm, cap, C, weights) : window_energy<N, DIRECT>(P, jm, cap, C, weights);
}

// The gating loop, once: the gating and short-term blocks of ONE stream that end with its sub-blocks [sub_begin, sub_end), dealt
// to threads tid, tid + nthr, ... — a gating block ends with every sub-block j >= 3 (j-3..j), a short-term block with j = 29 + 10 m
// (j-29..j).  The blocks are independent: every one at or above the absolute gate is an atomic increment of its bin of hb (gating)
// or hs (short-term) — the LDS pair of a batch's workgroup, or the stream's histograms in memory themselves.  `bd`: the bin
// boundaries (an LDS copy or the table itself: the same bins either way).  Returns this thread's block counts.
struct GateCounts { uint32_t nb, ns; };
template <bool EAGER, bool DIRECT>
__device__ __forceinline__ GateCounts gate_range(const double *__restrict__ P, uint32_t cap, uint32_t C, const double *__restrict__ weights,
                                                 const TdConst &K, const double *__restrict__ bd, double bd0, uint64_t sub_begin,
                                                 uint64_t sub_end, uint64_t bad_from, unsigned long long *hb, unsigned long long *hs,
                                                 uint32_t tid, uint32_t nthr)
{
    // DIRECT: the index is the slot, a 32-bit number (launch_finalize checks).  Counted in 64 bits there, k_finalize<false> spilled
    // 124 bytes of scratch per lane and k_finalize<true> took 256 VGPRs + 60 AGPRs: one wave per SIMD instead of two
    using J = std::conditional_t<DIRECT, uint32_t, uint64_t>;
    const double S = (double)K.s100;
    GateCounts n{0u, 0u};
    for (J j = (J)(sub_begin > 3 ? sub_begin : 3) + tid; j < sub_end; j += nthr) {
        double sum = block_energy<4, EAGER, DIRECT>(P, j, cap, C, weights) / (4.0 * S);
        if (j > bad_from) sum = __builtin_nan("");
        n.nb++;
        if (sum >= bd0) atomicAdd(&hb[hist_index(bd, sum)], 1ull);
    }
    // short-term blocks: dealt densely (thread = m), not as every tenth thread of the loop above
    if (!K.st_off) {
        const uint64_t m_begin = sub_begin > 29 ? (sub_begin - 29 + 9) / 10 : 0;      // first m with 29 + 10 m >= sub_begin
        for (J m = (J)m_begin + tid;; m += nthr) {
            const J j = 29 + 10 * m;
            if (j >= sub_end) break;
            double sum = block_energy<30, EAGER, DIRECT>(P, j, cap, C, weights) / (30.0 * S);
            if (j > bad_from) sum = __builtin_nan("");
            n.ns++;
            if (sum >= bd0) atomicAdd(&hs[hist_index(bd, sum)], 1ull);
        }
    }
    return n;
}

// The two tables the gate reads — bin energies and bin boundaries, 16 KB — into LDS as tab = [energies 1000][bounds 1001]: every
// dependent table read behind it is an LDS access, not a round trip to L2.  also(i): what else the caller brings in with bin i,
// requested in the same trip to memory.
constexpr int kTabDoubles = 2 * kHistBins + 1;
template <class Also>
__device__ __forceinline__ void stage_tables(double *tab, const double *en, const double *bd, int tid, int nthr, Also &&also)
{
    for (int i = tid; i < kHistBins; i += nthr) { also(i); tab[i] = en[i]; tab[kHistBins + i] = bd[i]; }
    if (tid == 0) tab[2 * kHistBins] = bd[kHistBins];
}

// A handle's readings, by one wave whose LDS pair (hb, hs) holds the handle's histograms (the caller's loads, not yet behind a
// barrier): the 2 * kMaxChannels peak floats copied beside the evaluation, (integrated, range) into out2, then `seq` stored into
// *flag behind a system fence — host-visible memory: whoever sees the flag sees out2 and the peaks.
__device__ __forceinline__ void publish_readings(const ReadingsExtra &x, const unsigned long long *hb, const unsigned long long *hs,
                                                 const double *__restrict__ en, const double *__restrict__ bd, double *out2)
{
    static_assert(2 * kMaxChannels == 128, "two floats per lane");
    const int lane = threadIdx.x;
    if (x.peaks_dst) {
        x.peaks_dst[lane] = x.peaks_src[lane];
        x.peaks_dst[64 + lane] = x.peaks_src[64 + lane];
    }
    __syncthreads();
    eval_hist(hb, hs, en, bd, &out2[0], &out2[1]);
    if (x.flag) {
        __threadfence_system();
        __syncthreads();
        if (lane == 0) __hip_atomic_store(x.flag, x.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// One workgroup per stream; the gating blocks of a stream are independent (histogram increments are LDS atomics), so a
// long stream (config 2's 600 s: 6000 sub-blocks) is spread over up to 1024 threads — a thread's iteration is a chain of
// dependent loads, so the kernel's time is its iteration count; wave 0 then evaluates gate and LRA.
// SMALL (a handful of streams: config 2, a file open, calculate_integrated_lufs): the two tables the gate reads come into LDS with
// the histograms, and the sub-block sums are requested eagerly: the kernel's chain of
// dependent trips to L2 / HBM is four long instead of eighteen (config 2: 22.5 -> 20 us, config 5: 31 -> 25 us, profiles/r05_small_batch_finalize.txt).  The big grids keep
// the lean form: 16 KB more LDS traffic per workgroup buys nothing where a thousand workgroups hide each other's latency.
// Batches only: slot == sub-block index, from sub-block 0 on (launch_finalize refuses anything else).
template <bool SMALL>
__global__ __launch_bounds__(SMALL ? 256 : 1024) void k_finalize(FinalizeParams p)
{
    __shared__ unsigned long long hb[kHistBins];
    __shared__ unsigned long long hs[kHistBins];
    __shared__ unsigned int counts[2];
    __shared__ uint32_t bad_from_s;
    __shared__ double tab[SMALL ? kTabDoubles : 1];
    const uint32_t stream = blockIdx.x;
    const int lane = threadIdx.x, nthr = (int)blockDim.x;
    unsigned long long *gh = reinterpret_cast<unsigned long long *>(p.hist) + (size_t)stream * 2 * kHistBins;
    unsigned long long *corpus = reinterpret_cast<unsigned long long *>(p.corpus_hist);
    auto load_hist = [&](int i) { hb[i] = gh[i]; hs[i] = gh[kHistBins + i]; };
    if (SMALL) stage_tables(tab, p.hist_energies, p.hist_bounds, lane, nthr, load_hist);
    else for (int i = lane; i < kHistBins; i += nthr) load_hist(i);
    if (lane < 2) counts[lane] = 0;
    if (lane < 64) {
        const uint32_t bf = first_bad_subblock(p.state ? p.state + stream : nullptr, p.channels, p.weights, (uint32_t)lane);
        if (lane == 0) bad_from_s = bf;
    }
    const double *en = SMALL ? tab : p.hist_energies;
    const double *bd = SMALL ? tab + kHistBins : p.hist_bounds;
    const double bd0 = p.hist_bounds[0];                                                  // (read before the barrier: in flight with the rest)
    const uint64_t sub_end = p.sub_end_of ? p.sub_end_of[stream] : p.sub_end;          // ragged batches
    __syncthreads();

    const GateCounts n = gate_range<SMALL, true>(p.subblocks + (size_t)stream * p.sub_stride, p.sub_cap, p.channels, p.weights, *p.k, bd,
                                                 bd0, 0, sub_end, bad_from_s, hb, hs, (uint32_t)lane, (uint32_t)nthr);
    if (n.nb) atomicAdd(&counts[0], n.nb);
    if (n.ns) atomicAdd(&counts[1], n.ns);
    __syncthreads();
    // corpus contribution = what this call added
    for (int i = lane; i < kHistBins; i += nthr) {
        const unsigned long long db = hb[i] - gh[i], ds = hs[i] - gh[kHistBins + i];
        if (corpus) {
            if (db) atomicAdd(&corpus[i], db);
            if (ds) atomicAdd(&corpus[kHistBins + i], ds);
        }
        gh[i] = hb[i];
        gh[kHistBins + i] = hs[i];
    }
    if (p.out_counts && lane < 2) p.out_counts[stream * 2 + lane] += counts[lane];
    if (lane < 64)          // (wave 0; the histograms in LDS are complete: the barrier above)
        eval_hist(hb, hs, en, bd,
                  p.out_integrated ? &p.out_integrated[stream] : nullptr,
                  p.out_lra ? &p.out_lra[stream] : nullptr);
}

// Streaming form (one handle, a few new sub-blocks per call, no per-call read-out): the same gating rules
// with the histogram updated in place by global atomics instead of a 16 KB round trip through LDS.
__global__ __launch_bounds__(64) void k_finalize_stream(FinalizeParams p)
{
    // one wave, and every step waits for the one before it: the tables the gate reads are staged in
    // LDS first — ONE round trip to L2 instead of one per dependent table read (two per histogram index, eight in eval_hist)
    __shared__ double tab[kTabDoubles];
    const int lane = threadIdx.x;
    stage_tables(tab, p.hist_energies, p.hist_bounds, lane, 64, [](int) {});
    const double *en = tab, *bd = tab + kHistBins;
    const double bd0 = p.hist_bounds[0];
    const uint64_t bad_from = first_bad_subblock(p.state, p.channels, p.weights, (uint32_t)lane);
    __syncthreads();
    unsigned long long *gh = reinterpret_cast<unsigned long long *>(p.hist);
    const GateCounts n = gate_range<true, false>(p.subblocks, p.sub_cap, p.channels, p.weights, *p.k, bd, bd0, p.sub_begin, p.sub_end,
                                                 bad_from, gh, gh + kHistBins, (uint32_t)lane, 64u);
    if (p.out_counts) {
        if (n.nb) atomicAdd(&p.out_counts[0], n.nb);
        if (n.ns) atomicAdd(&p.out_counts[1], n.ns);
    }
    // the handle's readings behind the update (what the reference's render loop asks for on its next frame): the same wave
    // evaluates the histograms it has just touched — no launch of its own inside a tick
    if (p.readings_out) {
        __shared__ unsigned long long hb[kHistBins];
        __shared__ unsigned long long hs[kHistBins];
        __threadfence();                                    // this wave's atomics have landed
        for (int i = lane; i < kHistBins; i += 64) {
            hb[i] = __hip_atomic_load(&gh[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            hs[i] = __hip_atomic_load(&gh[kHistBins + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        publish_readings(p.readings, hb, hs, en, bd, p.readings_out);
    }
}

constexpr uint32_t kFinalizeSmallMax = 64u;      // streams up to which a launch counts as latency-bound (the form with the tables in LDS)
hipError_t launch_finalize(const FinalizeParams &p, hipStream_t s)
{
    if (p.n_streams == 0) return hipSuccess;
    // batches: slot == sub-block index, and the index a 32-bit number (the direct form of gate_range counts in 32 bits)
    if (p.sub_begin != 0 || p.sub_end > p.sub_cap || p.sub_end >> 31) return hipErrorInvalidValue;
    // four waves per stream (even a 100-sub-block stream moves two 8 KB histograms in and out of LDS: 64 / 128 / 256 / 512
    // threads at the bench shape: 0.043 / 0.036 / 0.033 / 0.045 ms), sixteen for a long stream
    const uint32_t threads = p.sub_end > 2048 ? 1024u : 256u;
    // a handful of short streams: the launch is a chain of memory round trips, not work -> the form that shortens the chain
    if (p.n_streams <= kFinalizeSmallMax && threads == 256u) hipLaunchKernelGGL(k_finalize<true>, dim3(p.n_streams), dim3(threads), 0, s, p);
    else hipLaunchKernelGGL(k_finalize<false>, dim3(p.n_streams), dim3(threads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_finalize_stream(const FinalizeParams &p, hipStream_t s)
{
    if (p.n_streams == 0) return hipSuccess;
    hipLaunchKernelGGL(k_finalize_stream, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

// ============================================================================
//  Loudness series (SS_BATCH_LOUDNESS_SERIES): EbuR128::loudness_momentary / loudness_shortterm after every sub-block, and maxima
// ============================================================================
// The crate's partial reading (j < N - 1): its ring starts zeroed, so the window holds sub-blocks 0 ... j only.  The same additions
// as window_energy with the missing leading terms taken as zero (0 + 0 = 0: the first real term lands on an exact zero).
template <int N>
__device__ __forceinline__ double window_energy_head(const double *__restrict__ P, uint32_t j, uint32_t C,
                                                     const double *__restrict__ weights)
{
    double sum = 0.0;
    for (uint32_t c = 0; c < C; c++) {
        const double w = weights[c];
        if (w == 0.0) continue;
        double cs = 0.0;
        for (uint32_t q = 0; q <= j; q++) cs += P[(size_t)q * C + c];
        sum += w * cs;
    }
    return sum;
}

// (value, j) maximum: a NaN never wins, ties go to the lower j; (-inf, 0xFFFFFFFF) is "none yet" and loses to any value
__device__ __forceinline__ void max_at(double &v, uint32_t &at, double v2, uint32_t at2)
{
    if (v2 > v || (v2 == v && at2 < at)) { v = v2; at = at2; }
}

// One workgroup per stream, a thread per sub-block j (long streams loop).  Every full window's energy is formed by the very
// window_energy form and additions k_finalize used for its histograms (the momentary energy at j >= 3 is that gating block's,
// the short-term energy at j = 29 + 10 m that short-term block's), and the first-bad-sub-block rule is k_finalize's.  The
// maxima are a wave / LDS reduction in the same launch.  Batches only: slot == sub-block index.
template <bool SMALL>
__global__ __launch_bounds__(SMALL ? 256 : 1024) void k_loudness_series(FinalizeParams p, double *series, uint64_t series_stride,
                                                                         LoudnessExtremes *extremes)
{
    __shared__ uint32_t bad_from_s;
    __shared__ double red_v[2][16];
    __shared__ uint32_t red_at[2][16];
    const uint32_t stream = blockIdx.x;
    const int tid = threadIdx.x, nthr = (int)blockDim.x;
    if (tid < 64) {
        const uint32_t bf = first_bad_subblock(p.state ? p.state + stream : nullptr, p.channels, p.weights, (uint32_t)tid);
        if (tid == 0) bad_from_s = bf;
    }
    const uint32_t n = (uint32_t)(p.sub_end_of ? p.sub_end_of[stream] : p.sub_end);
    __syncthreads();
    const uint32_t C = p.channels, cap = p.sub_cap;
    const double S = (double)p.k->s100;
    const bool st_on = !p.k->st_off;
    const double *P = p.subblocks + (size_t)stream * p.sub_stride;
    double2 *out = reinterpret_cast<double2 *>(series) + (size_t)stream * series_stride;
    const uint32_t bad_from = bad_from_s;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    double bm = -INFINITY, bs = -INFINITY;
    uint32_t am = kNone, as = kNone;
    for (uint32_t j = (uint32_t)tid; j < n; j += (uint32_t)nthr) {
        double em, es = __builtin_nan("");
        if (j >= 3) em = block_energy<4, SMALL, true>(P, j, cap, C, p.weights);
        else em = window_energy_head<4>(P, j, C, p.weights);
        em /= 4.0 * S;
        if (st_on) {
            if (j >= 29) es = block_energy<30, SMALL, true>(P, j, cap, C, p.weights);
            else es = window_energy_head<30>(P, j, C, p.weights);
            es /= 30.0 * S;
        }
        if (j > bad_from) { em = __builtin_nan(""); es = __builtin_nan(""); }
        const double lm = energy_to_lufs(em), ls = energy_to_lufs(es);
        out[j] = make_double2(lm, ls);
        if (j >= 3) max_at(bm, am, lm, j);
        if (j >= 29) max_at(bs, as, ls, j);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        max_at(bm, am, __shfl_xor(bm, o, 64), (uint32_t)__shfl_xor((int)am, o, 64));
        max_at(bs, as, __shfl_xor(bs, o, 64), (uint32_t)__shfl_xor((int)as, o, 64));
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 0) { red_v[0][wave] = bm; red_at[0][wave] = am; red_v[1][wave] = bs; red_at[1][wave] = as; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < (nthr >> 6); w++) { max_at(bm, am, red_v[0][w], red_at[0][w]); max_at(bs, as, red_v[1][w], red_at[1][w]); }
        extremes[stream] = LoudnessExtremes{bm, bs, am, as};
    }
}

hipError_t launch_loudness_series(const FinalizeParams &p, double *series, uint64_t series_stride, LoudnessExtremes *extremes,
                                  hipStream_t s)
{
    if (p.n_streams == 0) return hipSuccess;
    if (p.sub_begin != 0 || p.sub_end > p.sub_cap || p.sub_end > series_stride || p.sub_end > 0xFFFFFFFFull) return hipErrorInvalidValue;
    // a thread per sub-block, whole waves (a 10 s stream: two waves, not four mostly idle ones); the SMALL form where k_finalize takes it
    const uint64_t nsub = p.sub_end;
    const bool small = p.n_streams <= kFinalizeSmallMax && nsub <= 2048;
    const uint64_t most = small ? 256u : 1024u;
    uint64_t threads = (nsub + 63u) & ~63ull;
    threads = threads < 64u ? 64u : (threads > most ? most : threads);
    if (small) hipLaunchKernelGGL(k_loudness_series<true>, dim3(p.n_streams), dim3((uint32_t)threads), 0, s, p, series, series_stride, extremes);
    else hipLaunchKernelGGL(k_loudness_series<false>, dim3(p.n_streams), dim3((uint32_t)threads), 0, s, p, series, series_stride, extremes);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void k_hist_eval(const unsigned long long *hist2000, const double *en,
                                                  const double *bd, double *out2, ReadingsExtra x)
{
    __shared__ unsigned long long hb[kHistBins];
    __shared__ unsigned long long hs[kHistBins];
    __shared__ double tab[kTabDoubles];                     // the two tables beside the histograms: one round trip for all four
    stage_tables(tab, en, bd, threadIdx.x, 64, [&](int i) { hb[i] = hist2000[i]; hs[i] = hist2000[kHistBins + i]; });
    publish_readings(x, hb, hs, tab, tab + kHistBins, out2);
}

hipError_t launch_hist_eval(const uint64_t *hist2000, const double *energies, const double *bounds,
                            double *out2, hipStream_t s, const ReadingsExtra *peaks)
{
    hipLaunchKernelGGL(k_hist_eval, dim3(1), dim3(64), 0, s,
                       reinterpret_cast<const unsigned long long *>(hist2000), energies, bounds, out2,
                       peaks ? *peaks : ReadingsExtra{nullptr, nullptr, nullptr, 0u});
    return hipGetLastError();
}

// ============================================================================
//  Loudness regions (ss_batch_loudness_regions): the gate of runs of one stream's sub-blocks, pooled into groups
// ============================================================================
// One workgroup per region (s, a, n): the stream's own gating blocks that end with j in [a + 3, a + n) and its short-term blocks
// that end with j = a + 29 + 10 m < a + n (the phase starts with the region), every energy the very block_energy form and division
// k_finalize and k_loudness_series use (a = 0: the same bits), NaN behind the stream's first bad sub-block.  One loop over j feeds
// the gating bin and the momentary maximum and, from a + 29 on, the short-term maximum (every j, as the series has it) and every
// tenth j the short-term bin.  The LDS pair starts from zero; behind the loop its non-zero bins and the block counts (every block
// counts, binned or not: closed forms of n) go to the region's group with u64 atomics — integers only, so the sums do not depend
// on the order — and wave 0 evaluates the pair into the region's result.  Indices are 32-bit: slot == sub-block index < 2^31.
__global__ __launch_bounds__(1024) void k_region_gate(RegionGateParams p)
{
    __shared__ unsigned long long hb[kHistBins];
    __shared__ unsigned long long hs[kHistBins];
    __shared__ uint32_t bad_from_s;
    __shared__ double red_v[2][16];
    __shared__ uint32_t red_at[2][16];
    const LoudnessRegion rg = p.regions[blockIdx.x];
    const int tid = threadIdx.x, nthr = (int)blockDim.x;
    for (int i = tid; i < kHistBins; i += nthr) { hb[i] = 0ull; hs[i] = 0ull; }
    if (tid < 64) {
        const uint32_t bf = first_bad_subblock(p.state + rg.stream, p.channels, p.weights, (uint32_t)tid);
        if (tid == 0) bad_from_s = bf;
    }
    const double *bd = p.hist_bounds;
    const double bd0 = bd[0];
    const uint32_t C = p.channels, cap = p.sub_cap;
    const double S = (double)p.k->s100;
    const bool st_on = !p.k->st_off;
    const double *P = p.subblocks + (size_t)rg.stream * p.sub_stride;
    const uint32_t a = rg.first_subblock, n = rg.n_subblocks, end = a + n;
    __syncthreads();
    const uint32_t bad_from = bad_from_s;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    double bm = -INFINITY, bs = -INFINITY;
    uint32_t am = kNone, as = kNone;
    for (uint32_t j = a + 3u + (uint32_t)tid; j < end; j += (uint32_t)nthr) {
        double em = block_energy<4, false, true>(P, j, cap, C, p.weights) / (4.0 * S);
        if (j > bad_from) em = __builtin_nan("");
        if (em >= bd0) atomicAdd(&hb[hist_index(bd, em)], 1ull);
        max_at(bm, am, energy_to_lufs(em), j);
        if (st_on && j >= a + 29u) {
            double es = block_energy<30, false, true>(P, j, cap, C, p.weights) / (30.0 * S);
            if (j > bad_from) es = __builtin_nan("");
            max_at(bs, as, energy_to_lufs(es), j);
            if ((j - a - 29u) % 10u == 0u && es >= bd0) atomicAdd(&hs[hist_index(bd, es)], 1ull);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        max_at(bm, am, __shfl_xor(bm, o, 64), (uint32_t)__shfl_xor((int)am, o, 64));
        max_at(bs, as, __shfl_xor(bs, o, 64), (uint32_t)__shfl_xor((int)as, o, 64));
    }
    const int wave = tid >> 6;
    if ((tid & 63) == 0) { red_v[0][wave] = bm; red_at[0][wave] = am; red_v[1][wave] = bs; red_at[1][wave] = as; }
    __syncthreads();                                            // (the histograms in LDS are complete as well)
    RegionResult *out = p.results + blockIdx.x;
    const uint32_t nb = n > 3u ? n - 3u : 0u, ns = st_on && n >= 30u ? (n - 30u) / 10u + 1u : 0u;
    GroupResult *grp = rg.group != kRegionNoGroup ? p.group_results + rg.group : nullptr;
    if (tid == 0) {
        for (int w = 1; w < (nthr >> 6); w++) { max_at(bm, am, red_v[0][w], red_at[0][w]); max_at(bs, as, red_v[1][w], red_at[1][w]); }
        out->max_momentary = bm; out->max_shortterm = bs; out->max_momentary_at = am; out->max_shortterm_at = as;
        out->n_gating_blocks = nb; out->n_st_blocks = ns;
        if (grp) {
            if (nb) atomicAdd(atomic_u64(&grp->n_gating_blocks), (unsigned long long)nb);
            if (ns) atomicAdd(atomic_u64(&grp->n_st_blocks), (unsigned long long)ns);
        }
    }
    if (grp) {
        unsigned long long *gh = p.group_hist + (size_t)rg.group * 2 * kHistBins;
        for (int i = tid; i < kHistBins; i += nthr) {
            const unsigned long long db = hb[i], ds = hs[i];
            if (db) atomicAdd(&gh[i], db);
            if (ds) atomicAdd(&gh[kHistBins + i], ds);
        }
    }
    if (tid < 64) eval_hist(hb, hs, p.hist_energies, bd, &out->integrated_lufs, &out->loudness_range);
}

// One wave per group behind the regions, shaped like k_hist_eval: the group's summed pair and the two tables into LDS, eval_hist
// into the group's result (its counts are already there).
__global__ __launch_bounds__(64) void k_group_eval(RegionGateParams p)
{
    __shared__ unsigned long long hb[kHistBins];
    __shared__ unsigned long long hs[kHistBins];
    __shared__ double tab[kTabDoubles];
    const unsigned long long *gh = p.group_hist + (size_t)blockIdx.x * 2 * kHistBins;
    stage_tables(tab, p.hist_energies, p.hist_bounds, threadIdx.x, 64, [&](int i) { hb[i] = gh[i]; hs[i] = gh[kHistBins + i]; });
    __syncthreads();
    GroupResult *out = p.group_results + blockIdx.x;
    eval_hist(hb, hs, tab, tab + kHistBins, &out->integrated_lufs, &out->loudness_range);
}

hipError_t launch_region_gate(const RegionGateParams &p, hipStream_t s)
{
    // slot == sub-block index, a 32-bit number with room for a workgroup's stride behind it; one workgroup per region / group
    if (p.sub_cap >> 31 || p.n_regions >> 31 || p.n_groups >> 31) return hipErrorInvalidValue;
    if (p.n_groups) {
        hipError_t e = hipMemsetAsync(p.group_results, 0, (size_t)p.n_groups * sizeof(GroupResult), s);
        if (e == hipSuccess) e = hipMemsetAsync(p.group_hist, 0, (size_t)p.n_groups * 2 * kHistBins * sizeof(unsigned long long), s);
        if (e != hipSuccess) return e;
    }
    if (p.n_regions) hipLaunchKernelGGL(k_region_gate, dim3(p.n_regions), dim3(region_gate_threads(p.longest)), 0, s, p);
    if (p.n_groups) hipLaunchKernelGGL(k_group_eval, dim3(p.n_groups), dim3(64), 0, s, p);
    return hipGetLastError();
}

// mean square over the last `frames` frames of the filtered ring, channel-weighted
// (calc_gating_block on the ring "as is": loudness_shortterm / loudness_momentary).
// Two stages with a fixed reduction shape (bit-reproducible): kRingBlocks partial sums, then one block — in ONE launch: the
// workgroup that finishes last (a counter behind the partial sums, wrapped back to zero by atomicInc for the next launch)
// reduces the partial sums.  (Through round 3 the second stage was a launch of its own: one more of a tick's launches.)
// The window is ONE run of ring elements with at most one wrap (frames <= ring_frames): ring_sumsq.  256 workgroups: a thread takes
// four or five elements of the three-second window at 48 kHz stereo, all requested before the first is used.
constexpr int kRingBlocks = 256;
__global__ __launch_bounds__(256) void k_ring_energy(const double *ring, uint32_t ring_elems, uint32_t C, uint32_t begin_elem,
                                                     uint32_t total, double frames,
                                                     const double *weights, double *partial, double *out)
{
    __shared__ double red[256];
    __shared__ uint32_t is_last;
    double acc = ring_sumsq(ring, ring_elems, C, begin_elem, total, blockIdx.x * 256u + threadIdx.x, (uint32_t)kRingBlocks * 256u, weights, 0.0);
    // workgroup sum: shuffle tree inside each wave, then the four wave sums in a fixed order
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        __threadfence();                                                   // the partial sum is visible before the count
        is_last = atomicInc(reinterpret_cast<unsigned int *>(partial + kRingBlocks), (unsigned int)kRingBlocks - 1u) == (unsigned int)kRingBlocks - 1u;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    red[threadIdx.x] = __builtin_nontemporal_load(partial + threadIdx.x);
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double e = red[0] / frames;
        out[0] = e;
        out[1] = energy_to_lufs(e);
    }
}

// scratch: kRingBlocks partial sums + the completion counter (zero before the first launch, see ss_analyzer.cpp).
// `out` may be device memory or pinned host memory mapped into the device (the tick drivers: no copy behind the kernel).
hipError_t launch_ring_energy(const double *ring, uint64_t ring_frames, uint32_t channels,
                              uint64_t end_frame, uint64_t frames, const double *weights,
                              double *out, double *scratch, hipStream_t s)
{
    if (frames == 0 || frames > ring_frames || ring_frames * channels >= (1ull << 31)) return hipErrorInvalidValue;
    // ring position of absolute frame f is f % ring_frames; frames before 0 are the zeroed ring
    const uint64_t begin = (end_frame % ring_frames + ring_frames - frames) % ring_frames;
    hipLaunchKernelGGL(k_ring_energy, dim3(kRingBlocks), dim3(256), 0, s, ring, (uint32_t)(ring_frames * channels), channels,
                       (uint32_t)(begin * channels), (uint32_t)(frames * channels), (double)frames, weights, scratch, out);
    return hipGetLastError();
}

// ============================================================================
//  Meter banks: N streaming meters advanced by one launch per stage
// ============================================================================
// Gating of every stream's new sub-blocks behind a bank's time-domain launch: one wave per stream, k_finalize_stream's gate_range
// (the same window form, hence a handle's histograms bit for bit) over the stream's own range, derived from its frame count.
// Streams that completed no sub-block leave at once.  The tables are read where they are (L2): a wave has a few blocks to gate.
// frames_of (ragged adds): what the launch gave each stream; a stream that got nothing leaves before it reads its state.
__global__ __launch_bounds__(64) void k_meter_bank_gate(MeterBankParams p, uint64_t frames_all, const uint64_t *frames_of)
{
    const uint32_t stream = blockIdx.x, lane = threadIdx.x;
    const uint64_t frames = frames_of ? frames_of[stream] : frames_all;
    if (frames == 0) return;
    const TdState *st = p.state + stream;
    const uint64_t S = p.k->s100;
    const uint64_t fed = st->frames_fed;
    const uint64_t sb0 = (fed - frames) / S, sb1 = fed / S;
    if (sb1 == sb0) return;
    const uint64_t bad_from = first_bad_subblock(st, p.channels, p.weights, lane);
    unsigned long long *gh = reinterpret_cast<unsigned long long *>(p.hist) + (size_t)stream * 2 * kHistBins;
    const GateCounts n = gate_range<true, false>(p.subblocks + (size_t)stream * p.sub_stride, p.sub_cap, p.channels, p.weights, *p.k,
                                                 p.hist_bounds, p.hist_bounds[0], sb0, sb1, bad_from, gh, gh + kHistBins, lane, 64u);
    uint32_t *counts = p.counts + 2 * (size_t)stream;
    if (n.nb) atomicAdd(&counts[0], n.nb);
    if (n.ns) atomicAdd(&counts[1], n.ns);
}

hipError_t launch_meter_bank_gate(const MeterBankParams &p, uint64_t frames, const uint64_t *frames_of, hipStream_t s)
{
    if (p.n_streams == 0 || (frames == 0 && !frames_of)) return hipSuccess;
    hipLaunchKernelGGL(k_meter_bank_gate, dim3(p.n_streams), dim3(64), 0, s, p, frames, frames_of);
    return hipGetLastError();
}

// Weighted energy of the N sub-blocks' worth of frames in front of frame F = k S + r of one stream (one wave; every lane gets it):
// the tail of sub-block k - N from offset r (S - r frames of the filtered-sample ring; when r = 0 that sub-block is whole and comes
// from the sub-block ring), the complete sub-blocks k - N + 1 ... k - 1 (sub-block ring) and the current partial sub-block
// (TdState::acc).  What lies in front of frame 0 is zero, as in the crate's zeroed ring.  At most S C ring loads, where summing
// the window itself would take N S C.
template <int N>
__device__ __forceinline__ double bank_window_energy(const MeterBankParams &p, const TdState &st, const double *__restrict__ P,
                                                     const double *__restrict__ R, uint64_t F, uint32_t lane)
{
    const uint32_t C = p.channels, cap = p.sub_cap;
    const uint64_t S = p.k->s100;
    const uint64_t k = F / S;
    const uint32_t r = (uint32_t)(F - k * S);
    double e = 0.0;
    for (uint32_t c = lane; c < C; c += 64u) {
        const double w = p.weights[c];
        if (w != 0.0) e += w * st.acc[c];
    }
    const uint32_t nq = r == 0u ? (uint32_t)N : (uint32_t)(N - 1);     // r = 0: sub-block k - N is whole, from the sub-block ring
    for (uint32_t i = lane; i < nq * C; i += 64u) {
        const uint32_t q = 1u + i / C, c = i - (q - 1u) * C;           // sub-block k - q, channel c
        const double w = p.weights[c];
        if (k >= q && w != 0.0) e += w * P[(size_t)((k - q) % cap) * C + c];
    }
    if (k >= (uint64_t)N && r != 0u) {
        // (S - r <= ring_frames: one run with at most one wrap)
        e = ring_sumsq(R, (uint32_t)(p.ring_frames * C), C, (uint32_t)((((k - N) * S + r) % p.ring_frames) * C), (uint32_t)((S - r) * C),
                       lane, 64u, p.weights, e);
    }
    return wave_sum(e);
}

// One wave per stream: momentary and short-term loudness by the window decomposition above, integrated loudness and range by
// eval_hist on the stream's histograms (a handle's evaluation: the same bits), the peaks of channels 0 and 1, the frame count.
__global__ __launch_bounds__(64) void k_meter_bank_readings(MeterBankParams p, MeterReading *out)
{
    __shared__ unsigned long long hb[kHistBins];
    __shared__ unsigned long long hs[kHistBins];
    __shared__ double ev[2];
    const uint32_t stream = blockIdx.x, lane = threadIdx.x;
    const unsigned long long *gh = reinterpret_cast<const unsigned long long *>(p.hist) + (size_t)stream * 2 * kHistBins;
    for (uint32_t i = lane; i < (uint32_t)kHistBins; i += 64u) { hb[i] = gh[i]; hs[i] = gh[kHistBins + i]; }
    const TdState &st = p.state[stream];
    const uint64_t F = st.frames_fed;
    const double *P = p.subblocks + (size_t)stream * p.sub_stride;
    const double *R = p.ring + (size_t)stream * p.ring_stride;
    const double S = (double)p.k->s100;
    const double em = bank_window_energy<4>(p, st, P, R, F, lane) / (4.0 * S);
    const double es = p.st_on ? bank_window_energy<30>(p, st, P, R, F, lane) / (30.0 * S) : __builtin_nan("");
    __syncthreads();
    eval_hist(hb, hs, p.hist_energies, p.hist_bounds, &ev[0], &ev[1]);
    if (lane == 0) {
        MeterReading m;
        m.momentary = energy_to_lufs(em);
        m.shortterm = p.st_on ? energy_to_lufs(es) : __builtin_nan("");
        m.integrated = ev[0];
        m.loudness_range = ev[1];
        for (uint32_t c = 0; c < 2u; c++) {
            if (c < p.channels) {
                const float sp = st.sample_peak[c], tp = st.true_peak[c];
                m.sample_peak[c] = (double)sp;
                m.true_peak[c] = (double)(tp > sp ? tp : sp);              // true_peak(): max(true, sample)
            } else {
                m.sample_peak[c] = m.true_peak[c] = __builtin_nan("");
            }
        }
        m.frames = F;
        out[stream] = m;
    }
}

hipError_t launch_meter_bank_readings(const MeterBankParams &p, MeterReading *out, hipStream_t s)
{
    if (p.n_streams == 0) return hipSuccess;
    if (p.ring_frames * p.channels >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_meter_bank_readings, dim3(p.n_streams), dim3(64), 0, s, p, out);
    return hipGetLastError();
}

// Clears listed streams' meters: kResetBlocks workgroups per listed stream share its five regions (state, sub-block ring,
// sample ring, histograms, counts), 64-bit stores.
constexpr uint32_t kResetBlocks = 32;
static_assert(sizeof(TdState) % 8 == 0, "TdState is cleared in 64-bit words");
__global__ __launch_bounds__(256) void k_meter_bank_reset(MeterBankParams p, const uint32_t *streams)
{
    const uint32_t item = blockIdx.x / kResetBlocks, part = blockIdx.x - item * kResetBlocks;
    const uint32_t s = streams ? streams[item] : item;
    const uint64_t t0 = (uint64_t)part * 256u + threadIdx.x, stride = (uint64_t)kResetBlocks * 256u;
    auto zero = [&](void *base, uint64_t words) {
        uint64_t *w = static_cast<uint64_t *>(base);
        for (uint64_t i = t0; i < words; i += stride) w[i] = 0ull;
    };
    zero(p.state + s, sizeof(TdState) / 8);
    zero(p.subblocks + (size_t)s * p.sub_stride, (uint64_t)p.sub_cap * p.channels);
    zero(p.ring + (size_t)s * p.ring_stride, p.ring_frames * p.channels);
    zero(p.hist + (size_t)s * 2 * kHistBins, 2 * kHistBins);
    zero(p.counts + 2 * (size_t)s, 1);
}

hipError_t launch_meter_bank_reset(const MeterBankParams &p, const uint32_t *streams, uint32_t count, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    if ((uint64_t)count * kResetBlocks > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_meter_bank_reset, dim3(count * kResetBlocks), dim3(256), 0, s, p, streams);
    return hipGetLastError();
}

}  // namespace ssk
