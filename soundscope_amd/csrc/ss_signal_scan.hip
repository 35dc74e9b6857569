// ss_signal_scan.hip: silence, clip runs, DC and non-finite samples of every stream of a batch (ss_batch_signal_scan) — hand-written
// gfx950 (CDNA4, wave64) kernels.  Not in the reference.  Definition: include/soundscope_hip.h; plan and figures: DESIGN.md
// section 3.3.3.
//
// A stream of C channels has C + 1 predicate sequences over its frames: sequence 0 "every channel of the frame is silent",
// sequence 1 + c "the sample of channel c is clipped".  A run is a maximal stretch of frames on which a sequence holds.
//
// k_signal_tiles: one workgroup per (stream, tile of plan.tile_frames frames).  The tile's floats are one contiguous run of the
// corpus, copied into LDS as it lies (the peak series' loading rule: 16-byte loads on the aligned inside of the run, guarded
// 4-byte loads at its ends, no float outside the stream's own frames).  A wave takes 64 frames at a time, a lane one frame: the
// predicates become 64-bit lane masks (__ballot), one word per (sequence, 64 frames), kept in LDS.  The sums are f64: a thread
// takes one channel and every (256 / C)-th frame in ascending order, the threads of a channel meet in a fixed tree in LDS.
// Runs inside a word come from bit operations (one lane per word), words are joined by one lane per sequence.
// k_signal_carry: one wave per stream, one lane per sequence, walks the stream's tiles in ascending order, carries the run open at
// each tile boundary, and writes the records and every (tile, sequence)'s place in the lists.
// k_signal_events: one workgroup per (stream, tile); returns at once where the tile owns no listed run, else rebuilds the masks
// and writes the runs that end in the tile.  Integer arithmetic apart from the sums; no atomics on global memory.
// The tile loader, the mask words, the sums, the word summaries and the join live in ss_signal_scan_dev.h, shared with the meter
// banks' signal watch (ss_bank_signal_watch.hip).
#include "ss_kernels.h"
#include "ss_signal_scan_dev.h"

namespace ssk {

namespace {

struct ScanTile {
    uint32_t stream, tile, tn;                  // tn: the tile's frames (the last tile of a stream may be short)
    unsigned long long F, start;                // the stream's own frames; the tile's first frame
    bool last;                                  // the tile holds the stream's last frame
};

// which tile this workgroup has, false: none (behind the stream's own length)
__device__ __forceinline__ bool scan_tile_of(const SignalScanParams &p, ScanTile &t)
{
    t.stream = blockIdx.x / p.tiles_cap; t.tile = blockIdx.x - t.stream * p.tiles_cap;
    t.F = p.frames_of ? p.frames_of[t.stream] : p.n_frames;
    if (t.F > p.n_frames) t.F = p.n_frames;
    t.start = (unsigned long long)t.tile * p.tile_frames;
    if (t.start >= t.F) return false;
    const unsigned long long left = t.F - t.start;
    t.tn = left < p.tile_frames ? (uint32_t)left : p.tile_frames;
    t.last = left <= p.tile_frames;
    return true;
}

// the tile's floats from the corpus into LDS (scan_load_span's rule; the corpus is 16-byte aligned).  Returns where the tile's frame
// 0 lies in sh.
__device__ __forceinline__ const float *scan_load_tile(float *sh, const SignalScanParams &p, const ScanTile &t)
{
    const long long base = (long long)((unsigned long long)t.stream * p.stream_stride);
    const long long lo = base + (long long)t.start * p.channels, hi = lo + (long long)t.tn * p.channels;
    return scan_load_span(sh, p, lo, hi);
}

}  // namespace

__global__ __launch_bounds__(kScanThreads) void k_signal_tiles(SignalScanParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
    ScanTile t;
    if (!scan_tile_of(p, t)) return;                            // (the whole workgroup)
    const uint32_t C = p.channels, Q = C + 1u, nw = p.tile_frames >> 6, nwt = (t.tn + 63u) >> 6, tid = threadIdx.x;
    float *sh = reinterpret_cast<float *>(scan_lds);
    unsigned char *at = scan_lds + scan_tile_bytes(p.tile_frames, C);
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(at);
    double *sums = reinterpret_cast<double *>(at + kScanMaskBytes);
    uint32_t *counts = reinterpret_cast<uint32_t *>(at + kScanMaskBytes + kScanSumBytes);
    const float *x0 = scan_load_tile(sh, p, t);
    scan_counts_begin(counts);
    __syncthreads();
    scan_masks(x0, p, t.tn, nw, masks);
    scan_sums(x0, p, t.tn, sums, counts);                       // (ends in a barrier: the masks are there too)
    const size_t slot = (size_t)t.stream * p.tiles_cap + t.tile;
    if (tid < C) p.tile_channels[slot * C + tid] = scan_tile_channel(sums, counts, tid);
    // every word to its summary, in place: one lane per (sequence, word); a sequence notes whether it has a word that is not empty
    // and one that is not full
    for (uint32_t i = tid; i < Q * nwt; i += kScanThreads) {
        const uint32_t q = i / nwt, w = i - q * nwt, nb = word_bits(t.tn, w);
        const unsigned long long m = masks[q * nw + w];
        const uint32_t flags = (m ? 1u : 0u) | (m != (nb == 64u ? ~0ull : (1ull << nb) - 1ull) ? 2u : 0u);
        if (flags) atomicOr(&counts[q * 4u + 3u], flags);
        if (m) masks[q * nw + w] = word_summary(m, nb, q ? p.clip_min : p.silence_min);       // (an empty word is its own summary)
    }
    __syncthreads();
    // the words of a sequence joined in ascending order: one lane per sequence
    if (tid < Q) {
        const uint32_t min_len = tid ? p.clip_min : p.silence_min;
        SS_SCAN_JOIN(out, masks, counts, tid, nw, nwt, t.tn, min_len);
        p.tile_runs[slot * Q + tid] = out;
    }
}

// one run of `r` frames that ends: counted, and the longest so far if it is longer than every earlier one
#define SS_SCAN_CLOSE(r, first)                                                     \
    do {                                                                            \
        const uint32_t ok_ = (r) >= (unsigned long long)min_len ? 1u : 0u;          \
        n_runs += ok_; owned += ok_;                                                \
        if ((r) > best) { best = (r); best_at = (first); }                          \
    } while (0)

__global__ __launch_bounds__(64) void k_signal_carry(SignalScanParams p)
{
    const uint32_t stream = blockIdx.x, lane = threadIdx.x, C = p.channels, Q = C + 1u, T = p.tile_frames;
    unsigned long long F = p.frames_of ? p.frames_of[stream] : p.n_frames;
    if (F > p.n_frames) F = p.n_frames;
    const uint32_t nt = (uint32_t)((F + T - 1u) / T);           // <= tiles_cap
    const size_t slot0 = (size_t)stream * p.tiles_cap;
    unsigned long long clip_runs = 0;                           // of the channels in front of this round's (the same in every lane)
    for (uint32_t q0 = 0; q0 < Q; q0 += 64u) {
        const uint32_t q = q0 + lane;
        const bool active = q < Q;
        const uint32_t min_len = q ? p.clip_min : p.silence_min;
        unsigned long long carry = 0, n_runs = 0, best = 0, best_at = kNone64, total = 0, lead = 0, trail = 0, off = 0;
        bool lead_set = false;
        double sum = 0.0, sum_sq = 0.0;
        unsigned long long clipped = 0, nonfinite = 0, first_bad = kNone64;
        for (uint32_t t0 = 0; active && t0 < nt; t0 += 4u) {
            SignalTileRuns R[4];
            SignalTileChannel K[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {                 // four tiles' records in flight
                if (t0 + k < nt) {
                    R[k] = p.tile_runs[(slot0 + t0 + k) * Q + q];
                    if (q) K[k] = p.tile_channels[(slot0 + t0 + k) * C + (q - 1u)];
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t t = t0 + k;
                if (t >= nt) break;
                const unsigned long long start = (unsigned long long)t * T;
                SignalTileCarry cr;
                cr.carry_in = carry; cr.ev_off = off < p.max_events ? (uint32_t)off : p.max_events;
                uint32_t owned = 0;
                if (R[k].all_true) {
                    carry += R[k].head;
                } else {
                    const unsigned long long r = carry + R[k].head;     // the run that ends in this tile's head
                    if (!lead_set) { lead = r; lead_set = true; }
                    if (r) SS_SCAN_CLOSE(r, start - carry);
                    n_runs += R[k].count; owned += R[k].count;
                    if (R[k].longest > best) { best = R[k].longest; best_at = start + R[k].longest_at; }
                    carry = R[k].tail;
                }
                if (t == nt - 1u && carry) {                    // the stream ends: the open run ends with it, in this tile
                    SS_SCAN_CLOSE(carry, F - carry);
                    trail = carry;
                    if (!lead_set) lead = carry;
                }
                total += R[k].total;
                cr.owned = owned;
                p.tile_carry[(slot0 + t) * Q + q] = cr;
                off += owned;
                if (q) {
                    sum += K[k].sum; sum_sq += K[k].sum_sq;
                    clipped += K[k].clipped; nonfinite += K[k].nonfinite;
                    if (first_bad == kNone64 && K[k].first_nonfinite != kNone32) first_bad = start + K[k].first_nonfinite;
                }
            }
        }
        // a channel's runs follow those of the channels in front of it in the clip list
        const unsigned long long mine = active && q ? n_runs : 0ull;
        unsigned long long incl = mine;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const unsigned long long base = clip_runs + incl - mine;
        clip_runs += __shfl(incl, 63);
        if (active) p.list_base[(size_t)stream * Q + q] = q && base < p.max_events ? (uint32_t)base : q ? p.max_events : 0u;
        if (active && q) {
            ChannelScan out;
            out.sum = sum; out.sum_sq = sum_sq; out.nonfinite = nonfinite; out.first_nonfinite = first_bad; out.clipped_samples = clipped;
            out.longest_clip = best; out.longest_clip_at = best_at; out.clip_runs = n_runs;
            p.channel_scans[(size_t)stream * C + (q - 1u)] = out;
        }
        if (q == 0u) {                                          // lane 0 of the first round keeps the stream's record
            StreamScan out;
            out.silent_frames = total; out.leading_silence = lead; out.trailing_silence = trail;
            out.longest_silence = best; out.longest_silence_at = best_at; out.silence_runs = n_runs; out.clip_runs = 0;
            p.streams[stream] = out;
        }
    }
    if (lane == 0u) p.streams[stream].clip_runs = clip_runs;
}
#undef SS_SCAN_CLOSE

__global__ __launch_bounds__(kScanThreads) void k_signal_events(SignalScanParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char scan_lds[];
    ScanTile t;
    if (!scan_tile_of(p, t)) return;
    const uint32_t C = p.channels, Q = C + 1u, nw = p.tile_frames >> 6, nwt = (t.tn + 63u) >> 6, q = threadIdx.x;
    SignalTileCarry cr{};
    uint32_t off = 0;
    bool mine = false;
    if (q < Q) {
        cr = p.tile_carry[((size_t)t.stream * p.tiles_cap + t.tile) * Q + q];
        off = p.list_base[(size_t)t.stream * Q + q] + cr.ev_off;
        mine = cr.owned && off < p.max_events;
    }
    if (!__syncthreads_or(mine)) return;                        // no listed run ends in this tile
    float *sh = reinterpret_cast<float *>(scan_lds);
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(scan_lds + scan_tile_bytes(p.tile_frames, C));
    const float *x0 = scan_load_tile(sh, p, t);
    __syncthreads();
    scan_masks(x0, p, t.tn, nw, masks);
    __syncthreads();
    if (!mine) return;
    // the sequence's runs that end in the tile, in ascending order, each at its place in the list
    const uint32_t min_len = q ? p.clip_min : p.silence_min;
    SignalEvent *list = p.events + ((size_t)t.stream * 2u + (q ? 1u : 0u)) * p.max_events;
    unsigned long long cur = cr.carry_in;                       // frames of the open run so far
    for (uint32_t w = 0; w < nwt && off < p.max_events; w++) {
        const unsigned long long m = masks[q * nw + w];
        const uint32_t nb = word_bits(t.tn, w);
        uint32_t pos = 0;
        while (pos < nb) {
            unsigned long long rest = m >> pos;
            if (!cur) {
                if (!rest) break;
                const uint32_t z = (uint32_t)__builtin_ctzll(rest);
                pos += z; rest >>= z;
            }
            const uint32_t n = ~rest ? (uint32_t)__builtin_ctzll(~rest) : 64u;     // (64: a full word from bit 0)
            cur += n; pos += n;
            if (pos >= nb) break;                               // the run goes on in the next word
            if (cur >= min_len && off < p.max_events) {
                SignalEvent ev;
                ev.first_frame = t.start + 64u * w + pos - cur; ev.frames = cur; ev.channel = q ? q - 1u : kNone32; ev.reserved = 0u;
                list[off++] = ev;
            }
            cur = 0;
        }
    }
    if (t.last && cur >= min_len && cur && off < p.max_events) {
        SignalEvent ev;
        ev.first_frame = t.F - cur; ev.frames = cur; ev.channel = q ? q - 1u : kNone32; ev.reserved = 0u;
        list[off] = ev;
    }
}

// The tile: as many whole 64-frame mask words as keep its floats within kScanTileFloats (>= 128 frames at 64 channels).
SignalScanPlan plan_signal_scan(uint32_t channels, uint64_t n_frames)
{
    SignalScanPlan plan;
    plan.tile_frames = (kScanTileFloats / (channels ? channels : 1u)) & ~63u;
    const uint64_t cap = plan.tile_frames ? (n_frames + plan.tile_frames - 1u) / plan.tile_frames : 0u;
    plan.tiles_cap = cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap;
    return plan;
}

hipError_t launch_signal_scan(const SignalScanParams &p, hipStream_t s)
{
    if (!p.n_streams) return hipSuccess;
    const uint64_t groups = (uint64_t)p.n_streams * p.tiles_cap;
    if (groups > 0x7FFFFFFFull || !p.channels || p.channels > (uint32_t)kMaxChannels || !p.tile_frames || (p.tile_frames & 63u) ||
        (uint64_t)p.tile_frames * p.channels > kScanTileFloats || (uint64_t)(p.channels + 1u) * (p.tile_frames >> 6) > kScanWords)
        return hipErrorInvalidValue;
    const size_t tile = scan_tile_bytes(p.tile_frames, p.channels);
    if (groups) hipLaunchKernelGGL(k_signal_tiles, dim3((uint32_t)groups), dim3(kScanThreads), tile + kScanMaskBytes + kScanSumBytes + kScanCountBytes, s, p);
    hipLaunchKernelGGL(k_signal_carry, dim3(p.n_streams), dim3(64), 0, s, p);
    if (groups && p.max_events) hipLaunchKernelGGL(k_signal_events, dim3((uint32_t)groups), dim3(kScanThreads), tile + kScanMaskBytes, s, p);
    return hipGetLastError();
}

}  // namespace ssk
