// ss_bank_pair_watch.hip: the pair watch of a meter bank (ss_meter_bank_pair_watch*) — the f64 sums of x_a^2, x_b^2 and x_a x_b of every
// complete 100 ms entry of every stream, carried across add calls, with the window of the newest entries, the running totals and the
// runs of entries below a correlation threshold — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference.
// Definition: include/soundscope_hip.h (the batch pair series', ss_pair_series.hip, on the concatenation of what a stream was given);
// plan and figures: DESIGN.md section 3.7.5.
//
// k_bank_pair_watch: one workgroup of 256 threads per stream, queued once per add call.  It walks the stream's frames of this call
// entry by entry, pair after pair, as k_pair_series<false> walks an entry: frame i of the entry belongs to lane i mod 256, whichever
// call brought it, and a lane adds its frames in ascending order with four loads in flight.  What makes the cut invisible is the lane
// state: where the call starts inside an entry every lane loads its three sums and goes on adding; where the call ends inside one
// they go back.  Lanes meet — the batch's pair_reduce, the same tree — only when the S-th frame of the entry has arrived; thread 0
// then stores the entry into the ring, adds it to the totals and steps the run state, which stands in LDS (the records of the
// stream's pairs, loaded once and written once per call).  Behind the last frame one lane per pair sums the window over the ring,
// once per call and only where the call completed an entry.  Every load of the input is a 4-byte load of a frame of this call: an
// add_device pointer is any multiple of four bytes and a stride any number of floats, and nothing outside [0, F) frames is read.
// A workgroup whose stream was given nothing returns before any store.
// No atomics on global memory, no floating-point atomics, one writer per global word.
#include "ss_kernels.h"
#include "ss_pair_series_dev.h"

namespace ssk {

namespace {

static_assert(kPairWatchLanes == kPairThreads, "a lane of the state is a thread of the workgroup");
constexpr uint32_t kPairWatchWords = sizeof(PairWatch) / 8u;    // a record as 8-byte words
constexpr unsigned long long kPairNone64 = ~0ull;

__device__ __forceinline__ PairWatch pair_watch_empty()
{
    PairWatch z{};
    z.first_below = kPairNone64; z.longest_below_at = kPairNone64;
    return z;
}

__device__ __forceinline__ double pair_entry_f64(uint32_t lo, uint32_t hi)
{
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}

}  // namespace

__global__ __launch_bounds__(kPairThreads) void k_bank_pair_watch(BankPairWatchParams p)
{
    __shared__ double part[kPairWaves * 4];
    __shared__ unsigned long long rec_words[kMaxPairs * kPairWatchWords];
    __shared__ uint32_t open_skips[kMaxPairs];                  // frames this call skipped in the entry it leaves open
    const uint32_t stream = blockIdx.x, tid = threadIdx.x, C = p.channels, S = p.s100, NP = p.n_pairs, R = p.window_entries;
    const unsigned long long F = p.frames_of ? p.frames_of[stream] : p.frames;
    if (!F) return;                                             // (the whole workgroup: a stream given nothing is not touched)
    const float *in = p.pcm + (p.offset_of ? p.offset_of[stream] : (unsigned long long)stream * p.stride);
    unsigned long long *records = reinterpret_cast<unsigned long long *>(p.records + (size_t)stream * NP);
    PairWatch *rec = reinterpret_cast<PairWatch *>(rec_words);
    for (uint32_t i = tid; i < NP * kPairWatchWords; i += kPairThreads) rec_words[i] = records[i];
    if (tid < kMaxPairs) open_skips[tid] = 0u;
    __syncthreads();
    double *lanes = p.lanes + (size_t)stream * NP * 3u * kPairWatchLanes + tid;   // pair k: lanes[(3 k + {0, 1, 2}) * 256]
    uint32_t *open_skipped = p.open_skipped + (size_t)stream * NP;
    PairEntry *ring = p.ring + (size_t)stream * R * NP;
    const double t = p.threshold, tt = __dmul_rn(t, t);
    const unsigned long long E0 = rec[0].entries;               // (every pair of a stream holds the same entries and open_frames)
    unsigned long long E = E0;
    uint32_t o = rec[0].open_frames, slot = (uint32_t)(E0 % R);
    bool resumed = o != 0u;                                     // the entry the call ends in was open when the call began
    for (unsigned long long pos = 0; pos < F;) {
        // frames [pos, pos + take) of the call are frames [o, o + take) of entry E
        const uint32_t need = S - o, take = F - pos < need ? (uint32_t)(F - pos) : need, i_end = o + take;
        const bool complete = take == need;
        const uint32_t i0 = o + ((tid - o) & (kPairThreads - 1u));     // this lane's first frame of the entry at or behind o
        const float *x0 = in + pos * C;                         // frame i of the entry, channel c: x0[(i - o) C + c]
        for (uint32_t k = 0; k < NP; k++) {
            const uint32_t a = p.pairs[k].a, b = p.pairs[k].b;
            double *mine = lanes + (size_t)k * 3u * kPairWatchLanes;
            PairSums s;
            if (o) { s.aa = mine[0]; s.bb = mine[kPairWatchLanes]; s.ab = mine[2u * kPairWatchLanes]; }
            for (uint32_t f0 = i0; f0 < i_end; f0 += kPairDepth * kPairThreads) {
                float xa[kPairDepth], xb[kPairDepth];
#pragma unroll
                for (uint32_t j = 0; j < kPairDepth; j++) {
                    const size_t f = (f0 + j * kPairThreads < i_end ? f0 + j * kPairThreads : f0) - o;    // (a frame of this call either way)
                    xa[j] = x0[f * C + a]; xb[j] = x0[f * C + b];
                }
#pragma unroll
                for (uint32_t j = 0; j < kPairDepth; j++) if (f0 + j * kPairThreads < i_end) s.add(xa[j], xb[j]);
            }
            if (complete) {
                pair_reduce(s, part);
                if (tid == 0u) {
                    if (o) s.skipped += open_skipped[k];
                    pair_store(ring + (size_t)slot * NP + k, s, S, false);
                    PairWatch &r = rec[k];
                    const uint32_t frames = S - s.skipped;
                    r.total.s_aa = __dadd_rn(r.total.s_aa, s.aa); r.total.s_bb = __dadd_rn(r.total.s_bb, s.bb); r.total.s_ab = __dadd_rn(r.total.s_ab, s.ab);
                    r.total.frames += frames; r.total.skipped += s.skipped;
                    SS_PAIR_DECIDE(active, below, s.aa, s.bb, s.ab, frames, p.power_floor, t, tt);
                    if (active) r.n_active++;
                    if (active && below) {
                        r.n_below++;
                        if (r.first_below == kPairNone64) r.first_below = E;
                        r.trailing_below++;
                        if (r.trailing_below > r.longest_below) { r.longest_below = r.trailing_below; r.longest_below_at = E + 1u - r.trailing_below; }
                        if (r.trailing_below == p.min_run) r.below_runs++;          // (once per run, when it reaches the minimum)
                    } else {
                        r.trailing_below = 0u;
                    }
                }
            } else {                                            // (the call's last frames: the lanes' sums wait for the next call)
                mine[0] = s.aa; mine[kPairWatchLanes] = s.bb; mine[2u * kPairWatchLanes] = s.ab;
                if (s.skipped) atomicAdd(&open_skips[k], s.skipped);
            }
        }
        pos += take;
        if (complete) { E++; o = 0u; slot = slot + 1u == R ? 0u : slot + 1u; resumed = false; }
        else o = i_end;
    }
    __syncthreads();                                            // the run state and the skipped counts in LDS, the ring in memory
    if (tid < NP) {
        PairWatch &r = rec[tid];
        if (o) open_skipped[tid] = (resumed ? open_skipped[tid] : 0u) + open_skips[tid];
        const uint32_t wc = E < R ? (uint32_t)E : R;
        if (E != E0) {
            // the window: the newest wc entries in ascending entry order from +0, ss_batch_pair_regions' rule; four records in flight
            const uint4 *ser = reinterpret_cast<const uint4 *>(ring + tid);      // slot q: ser[2 q NP], [2 q NP + 1]
            const uint32_t first = (uint32_t)((E - wc) % R);
            PairWatchSums w{};
            for (uint32_t j0 = 0; j0 < wc; j0 += 4u) {
                uint4 lo[4], hi[4];
#pragma unroll
                for (uint32_t d = 0; d < 4u; d++) {
                    const size_t q = (first + (j0 + d < wc ? j0 + d : j0)) % R;
                    lo[d] = ser[2u * q * NP]; hi[d] = ser[2u * q * NP + 1u];
                }
#pragma unroll
                for (uint32_t d = 0; d < 4u; d++) {
                    if (j0 + d >= wc) break;
                    w.s_aa = __dadd_rn(w.s_aa, pair_entry_f64(lo[d].x, lo[d].y)); w.s_bb = __dadd_rn(w.s_bb, pair_entry_f64(lo[d].z, lo[d].w));
                    w.s_ab = __dadd_rn(w.s_ab, pair_entry_f64(hi[d].x, hi[d].y));
                    w.frames += hi[d].z; w.skipped += hi[d].w;
                }
            }
            r.window = w;
        }
        r.entries = E; r.open_frames = o; r.window_count = wc;
    }
    __syncthreads();
    for (uint32_t i = tid; i < NP * kPairWatchWords; i += kPairThreads) records[i] = rec_words[i];
}

// ss_meter_bank_pair_watch_enable / _reset: the listed streams (streams == nullptr: streams 0 .. count - 1) have watched nothing —
// empty records, one lane per (stream, pair).  entries == 0 and open_frames == 0 leave the ring and the lane sums unread.
__global__ __launch_bounds__(256) void k_bank_pair_watch_reset(PairWatch *records, uint32_t *open_skipped, const uint32_t *streams, uint32_t count,
                                                               uint32_t n_pairs)
{
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= count * n_pairs) return;
    const uint32_t i = idx / n_pairs, k = idx - i * n_pairs, s = streams ? streams[i] : i;
    records[(size_t)s * n_pairs + k] = pair_watch_empty();
    open_skipped[(size_t)s * n_pairs + k] = 0u;
}

hipError_t launch_bank_pair_watch(const BankPairWatchParams &p, hipStream_t s)
{
    if (!p.n_streams) return hipSuccess;
    if (p.n_streams > 0x7FFFFFFFu || !p.channels || p.channels > (uint32_t)kMaxChannels || !p.s100 || !p.n_pairs || p.n_pairs > kMaxPairs ||
        !p.window_entries || p.window_entries > kPairWatchWindowMax)
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < p.n_pairs; k++) if (p.pairs[k].a >= p.channels || p.pairs[k].b >= p.channels) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_pair_watch, dim3(p.n_streams), dim3(kPairThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_bank_pair_watch_reset(PairWatch *records, uint32_t *open_skipped, const uint32_t *streams, uint32_t count, uint32_t n_pairs,
                                        hipStream_t s)
{
    const uint64_t n = (uint64_t)count * n_pairs;
    if (!n) return hipSuccess;
    if (n >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_pair_watch_reset, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, records, open_skipped, streams, count, n_pairs);
    return hipGetLastError();
}

}  // namespace ssk
