// ss_signal_scan_dev.h: what the batch signal scan (ss_signal_scan.hip: every stream of a batch, one workgroup per tile) and the
// meter banks' signal watch (ss_bank_signal_watch.hip: one workgroup per stream walks the frames of an add call) share — the tile's
// geometry in LDS, the tile loader, the predicates as mask words, the sums and counts, a mask word's summary and the join of a
// tile's words into the tile's view of a sequence.  Device code only.  Definition: include/soundscope_hip.h.
//
// The helpers that read launch parameters are templates over the parameter struct: they use its channels, silence_threshold and
// clip_level (SignalScanParams and BankWatchParams both have them).
#pragma once
#include "ss_kernels.h"

namespace ssk {

namespace {

constexpr uint32_t kScanThreads = 256, kScanWaves = kScanThreads / 64;
constexpr uint32_t kScanTileFloats = 8192;  // floats of one tile at most (32 KB of LDS): the peak series' budget
constexpr uint32_t kScanWords = 256;        // mask words of a tile at most: (C + 1) * floor(8192 / 64 C) <= 128 (C + 1) / C
constexpr uint32_t kNone32 = 0xFFFFFFFFu;
constexpr unsigned long long kNone64 = ~0ull;

// dynamic LDS behind the tile's floats, every piece a multiple of 16 bytes
constexpr size_t kScanMaskBytes = kScanWords * sizeof(unsigned long long);
constexpr size_t kScanSumBytes = kScanThreads * 2 * sizeof(double);
constexpr size_t kScanCountBytes = (kMaxChannels + 2) * 4 * sizeof(uint32_t);

__host__ __device__ inline size_t scan_tile_bytes(uint32_t tile_frames, uint32_t channels)
{
    return ((size_t)tile_frames * channels + 8 + 3) / 4 * 16;      // the tile and the copy's alignment at both ends, in float4
}

// four floats of the corpus at g into LDS, those outside [lo, hi) as zeros: the two ends of a tile
__device__ __forceinline__ void scan_load_edge(float *dst, const float *corpus, long long g, long long lo, long long hi)
{
    float4 x;
    x.x = (g >= lo && g < hi) ? corpus[g] : 0.f;
    x.y = (g + 1 >= lo && g + 1 < hi) ? corpus[g + 1] : 0.f;
    x.z = (g + 2 >= lo && g + 2 < hi) ? corpus[g + 2] : 0.f;
    x.w = (g + 3 >= lo && g + 3 < hi) ? corpus[g + 3] : 0.f;
    *reinterpret_cast<float4 *>(dst) = x;
}

// The floats [lo, hi) of the 16-byte-aligned corpus p.pcm into LDS (peak_load_tile's rule): sh[i] = p.pcm[first + i] for lo <= first + i <
// hi, zero elsewhere; `first` is lo rounded down to a multiple of four floats.  16-byte loads on the vectors that lie wholly inside
// [lo, hi), four of them in flight per lane; guarded 4-byte loads at the two ends: no float outside [lo, hi) is read.  Returns where
// p.pcm[lo] lies in sh.
template <class P>
__device__ __forceinline__ const float *scan_load_span(float *sh, const P &p, long long lo, long long hi)
{
    const uint32_t shift = (uint32_t)(lo & 3ll);
    const long long first = lo - shift;
    const uint32_t n4 = (uint32_t)((hi - first + 3) >> 2);
    const uint32_t v_lo = shift ? 1u : 0u, v_hi = (uint32_t)((hi - first) >> 2);     // vectors [v_lo, v_hi) are whole
    const float4 *src = reinterpret_cast<const float4 *>(p.pcm + first);
    for (uint32_t v0 = v_lo + threadIdx.x; v0 < v_hi; v0 += 4u * kScanThreads) {
        float4 x[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) x[j] = src[v0 + j * kScanThreads < v_hi ? v0 + j * kScanThreads : v0];    // (a whole vector either way)
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) if (v0 + j * kScanThreads < v_hi) reinterpret_cast<float4 *>(sh)[v0 + j * kScanThreads] = x[j];
    }
    if (threadIdx.x == 0u && v_lo) scan_load_edge(sh, p.pcm, first, lo, hi);
    if (threadIdx.x == 64u && v_hi >= v_lo && v_hi < n4) scan_load_edge(sh + 4u * v_hi, p.pcm, first + 4ll * v_hi, lo, hi);
    return sh + shift;
}

__device__ __forceinline__ uint32_t word_bits(uint32_t tn, uint32_t w) { return tn - 64u * w < 64u ? tn - 64u * w : 64u; }

// The tile's predicates as mask words: masks[q * nw + w] bit l = sequence q holds on frame 64 w + l (frames behind tn: 0).  A
// wave takes four words at a time (w, w + 4, w + 8, w + 12: four LDS reads in flight), a lane one frame of each, and walks the
// frame's channels: the silence word is the AND of the channels' ballots, a clip word one ballot.
template <class P>
__device__ __forceinline__ void scan_masks(const float *x0, const P &p, uint32_t tn, uint32_t nw, unsigned long long *masks)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, C = p.channels, nwt = (tn + 63u) >> 6;
    for (uint32_t w0 = wave; w0 < nwt; w0 += 4u * kScanWaves) {
        const float *xf[4];
        bool valid[4];
        unsigned long long silent[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            const uint32_t f = 64u * (w0 + j * kScanWaves) + lane;
            valid[j] = f < tn;                                  // (false in every lane of a word behind the tile's last)
            xf[j] = x0 + (size_t)(valid[j] ? f : 0u) * C;
            silent[j] = __ballot(valid[j]);
        }
        for (uint32_t c = 0; c < C; c++) {
            float a[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) a[j] = valid[j] ? fabsf(xf[j][c]) : __builtin_nanf("");     // (a NaN holds neither predicate)
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t w = w0 + j * kScanWaves;
                silent[j] &= __ballot(a[j] <= p.silence_threshold);
                const unsigned long long clip = __ballot(a[j] >= p.clip_level);
                if (lane == 0u && w < nwt) masks[(1u + c) * nw + w] = clip;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
            const uint32_t w = w0 + j * kScanWaves;
            if (lane == 0u && w < nwt) masks[w] = silent[j];
        }
    }
}

// Every channel's sums and counts of the tile.  Thread t takes channel t % C and the frames t / C, t / C + G, ... (G = 256 / C
// whole frames a step: the threads of a step read consecutive floats), adds its share in ascending frames, and the G threads of a
// channel meet in a fixed tree in LDS: sums[c][2] holds the channel's result behind the last step.  counts[1 + c][4] = {clipped,
// non-finite, first non-finite frame (minimum), -} take integer LDS atomics.  The caller synchronises before; the tree ends in a barrier.
template <class P>
__device__ __forceinline__ void scan_sums(const float *x0, const P &p, uint32_t tn, double *sums, uint32_t *counts)
{
    const uint32_t t = threadIdx.x, C = p.channels, G = kScanThreads / C, c = t % C, j0 = t / C;
    const float inf = __builtin_inff();
    double s = 0.0, ss = 0.0;
    uint32_t n_clip = 0, n_bad = 0, first_bad = kNone32;
    if (j0 < G) {
#pragma unroll 4
        for (uint32_t f = j0; f < tn; f += G) {
            const float x = x0[(size_t)f * C + c], a = fabsf(x);
            if (a < inf) {                                      // (NaN: false)
                const double d = (double)x;
                s += d; ss = __builtin_fma(d, d, ss);           // (d * d is exact in f64)
            } else {
                n_bad++;
                if (first_bad == kNone32) first_bad = f;
            }
            n_clip += a >= p.clip_level ? 1u : 0u;
        }
    }
    sums[2u * t] = s; sums[2u * t + 1u] = ss;
    if (n_clip) atomicAdd(&counts[(1u + c) * 4u], n_clip);
    if (n_bad) { atomicAdd(&counts[(1u + c) * 4u + 1u], n_bad); atomicMin(&counts[(1u + c) * 4u + 2u], first_bad); }
    __syncthreads();
    for (uint32_t h = kScanThreads / 2u; h; h >>= 1) {          // thread (j0, c) sits at t = j0 C + c
        if (j0 < h && j0 + h < G) { sums[2u * t] += sums[2u * (t + h * C)]; sums[2u * t + 1u] += sums[2u * (t + h * C) + 1u]; }
        __syncthreads();
    }
}

// counts[q][4] of every sequence q: the three counts of channel q - 1, and the sequence's flags (1: a word is not empty, 2: a
// word is not full)
__device__ __forceinline__ void scan_counts_begin(uint32_t *counts)
{
    if (threadIdx.x <= (uint32_t)kMaxChannels) {
        uint4 z; z.x = 0u; z.y = 0u; z.z = kNone32; z.w = 0u;
        reinterpret_cast<uint4 *>(counts)[threadIdx.x] = z;
    }
}

// One mask word of nb bits as a packed summary: head (the run at bit 0) | tail (the run at bit nb - 1) << 8 | inner runs of at
// least min_len << 16 | the longest inner run << 24 | its first bit << 32 | set bits << 40 | all set << 48
__device__ __forceinline__ unsigned long long word_summary(unsigned long long m, uint32_t nb, uint32_t min_len)
{
    const unsigned long long full = nb == 64u ? ~0ull : (1ull << nb) - 1ull;
    const unsigned long long pop = (unsigned long long)__popcll(m);
    if (m == full) return (unsigned long long)nb | (unsigned long long)nb << 8 | pop << 40 | 1ull << 48;
    const uint32_t head = (uint32_t)__builtin_ctzll(~m);                        // < nb: a bit below nb is clear
    const uint32_t tail = (uint32_t)__builtin_clzll(~(m << (64u - nb)));        // < nb
    unsigned long long mi = m & ~((1ull << head) - 1ull);
    if (tail) mi &= (1ull << (nb - tail)) - 1ull;
    uint32_t cnt = 0, best = 0, best_at = 0;
    while (mi) {                                                                // starts are m & ~(m << 1): the lowest first
        const uint32_t s = (uint32_t)__builtin_ctzll(mi);                       // >= 1: bit 0 belongs to the head or is clear
        const uint32_t len = (uint32_t)__builtin_ctzll(~(mi >> s));             // <= 62
        mi &= ~(((1ull << len) - 1ull) << s);
        cnt += len >= min_len ? 1u : 0u;
        if (len > best) { best = len; best_at = s; }
    }
    return (unsigned long long)head | (unsigned long long)tail << 8 | (unsigned long long)cnt << 16 | (unsigned long long)best << 24 |
           (unsigned long long)best_at << 32 | pop << 40;
}

// one tile's view of channel c behind scan_sums
__device__ __forceinline__ SignalTileChannel scan_tile_channel(const double *sums, const uint32_t *counts, uint32_t c)
{
    SignalTileChannel out;
    out.sum = sums[2u * c]; out.sum_sq = sums[2u * c + 1u];
    out.clipped = counts[(1u + c) * 4u]; out.nonfinite = counts[(1u + c) * 4u + 1u]; out.first_nonfinite = counts[(1u + c) * 4u + 2u];
    out.pad = 0u;
    return out;
}

// The summaries of sequence q's words joined in ascending order into the tile's view of the sequence: one lane per sequence.  The
// words' summaries stand in masks (an empty word is its own summary), the sequence's flags in counts[q][3].  The statements declare
// their locals and the result, a SignalTileRuns `out`, in the caller's scope: use them inside a block of their own.
// A macro, not a function: as a function (by value, by reference, through a pointer: all tried) the same text compiles to other
// machine code in k_signal_tiles — another loop guard, one instruction fewer, pairs of instructions swapped — and the batch kernels
// are pinned to the instructions they had before the helpers moved here (profiles/bank_signal_watch_isa.txt).
#define SS_SCAN_JOIN(out, masks, counts, q, nw, nwt, tn, min_len)                                                                   \
        const uint32_t flags = (counts)[(q) * 4u + 3u];                                                                             \
        const bool join = flags == 3u;                          /* (nothing to join where every word is empty, or every word full) */ \
        uint32_t lead = 0, cur = 0, cur_at = 0, count = 0, best = 0, best_at = 0, total = flags & 2u ? 0u : (tn);                   \
        bool all = flags != 2u;                                 /* every word so far is full (no word at all is not empty: false) */ \
        for (uint32_t w = 0; w < (join ? (nwt) : 0u); w++) {                                                                        \
            const unsigned long long s = (masks)[(q) * (nw) + w];                                                                   \
            const uint32_t nb = word_bits((tn), w), head = (uint32_t)(s & 255u), tail = (uint32_t)(s >> 8 & 255u);                  \
            if (!cur) cur_at = 64u * w;                                                                                             \
            if (s >> 48 & 1u) {                                                                                                     \
                cur += nb;                                                                                                          \
            } else {                                                                                                                \
                const uint32_t r = cur + head;                  /* the run that ends in this word's head */                         \
                if (all) { lead = r; all = false; }             /* ... is the tile's own head */                                    \
                else if (r) { count += r >= (min_len) ? 1u : 0u; if (r > best) { best = r; best_at = cur_at; } }                    \
                const uint32_t wb = (uint32_t)(s >> 24 & 255u);                                                                     \
                count += (uint32_t)(s >> 16 & 255u);                                                                                \
                if (wb > best) { best = wb; best_at = 64u * w + (uint32_t)(s >> 32 & 255u); }                                       \
                cur = tail; cur_at = 64u * w + nb - tail;                                                                           \
            }                                                                                                                       \
            total += (uint32_t)(s >> 40 & 255u);                                                                                    \
        }                                                                                                                           \
        SignalTileRuns out;                                                                                                         \
        (out).head = all ? (tn) : lead; (out).tail = all ? (tn) : cur; (out).all_true = all ? 1u : 0u;                              \
        (out).count = count; (out).longest = best; (out).longest_at = best_at; (out).total = total; (out).pad = 0u

}  // namespace

}  // namespace ssk
