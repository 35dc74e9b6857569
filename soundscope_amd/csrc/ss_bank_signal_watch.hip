// ss_bank_signal_watch.hip: the signal watch of a meter bank (ss_meter_bank_signal_watch*) — silence, clip runs, DC and non-finite
// samples of every stream, carried across add calls — hand-written gfx950 (CDNA4, wave64) kernels.  Not in the reference.
// Definition: include/soundscope_hip.h (the batch scan's, ss_signal_scan.hip, on the concatenation of what a stream was given); plan
// and figures: DESIGN.md section 3.7.4.
//
// k_bank_signal_watch: one workgroup per stream, queued once per add call.  It walks the stream's frames of this call in tiles of
// plan_signal_scan's tile_frames, in ascending order.  A tile is the batch tile kernel's work through the shared helpers
// (ss_signal_scan_dev.h): the floats into LDS, the predicates as mask words, the f64 sums and the counts, the words' summaries, the
// join with one lane per sequence.  The lane that owns sequence q then folds the tile's view into the sequence's state, which it
// holds in registers — as k_signal_carry folds a tile behind its carry — and behind the last tile writes the state back and the
// stream's records, the open run included.  A workgroup whose stream was given nothing returns before any store.
// No atomics on global memory, no floating-point atomics, one writer per global word; tile-local quantities are u32, state is u64.
#include "ss_kernels.h"
#include "ss_signal_scan_dev.h"

namespace ssk {

namespace {

// behind the batch tile kernel's LDS: the last clipped frame + 1 of every channel's tile (0: none), rounded up to 16 bytes
constexpr size_t kWatchLastBytes = ((kMaxChannels + 1) * sizeof(uint32_t) + 15u) / 16u * 16u;

__device__ __forceinline__ BankWatchSeq watch_empty()
{
    BankWatchSeq z{};
    z.best_at = kNone64; z.first_nonfinite = kNone64; z.last_clip = kNone64;
    return z;
}

// the record fields of a sequence as its state stands: the open run counts where it reaches the minimum and takes part in the
// longest (strict >: ties go to the lowest frame)
struct WatchRuns { unsigned long long runs, best, best_at, lead; };
__device__ __forceinline__ WatchRuns watch_runs(const BankWatchSeq &st, uint32_t min_len)
{
    WatchRuns r;
    r.runs = st.runs + (st.open >= (unsigned long long)min_len ? 1u : 0u);          // (min_len >= 1: no open run is not counted)
    const bool open_is_longest = st.open > st.best;
    r.best = open_is_longest ? st.open : st.best;
    r.best_at = open_is_longest ? st.frames - st.open : st.best_at;
    r.lead = st.lead_set ? st.lead : st.open;                                        // (every frame so far: the open run)
    return r;
}

__device__ __forceinline__ void watch_store_stream(StreamWatch *dst, const BankWatchSeq &st, uint32_t min_len, unsigned long long clip_runs)
{
    const WatchRuns r = watch_runs(st, min_len);
    StreamWatch out;
    out.silent_frames = st.total; out.leading_silence = r.lead; out.trailing_silence = st.open;
    out.longest_silence = r.best; out.longest_silence_at = r.best_at; out.silence_runs = r.runs; out.clip_runs = clip_runs;
    out.frames = st.frames;
    *dst = out;
}

__device__ __forceinline__ void watch_store_channel(ChannelWatch *dst, const BankWatchSeq &st, const WatchRuns &r)
{
    ChannelWatch out;
    out.sum = st.sum; out.sum_sq = st.sum_sq; out.nonfinite = st.nonfinite; out.first_nonfinite = st.first_nonfinite;
    out.clipped_samples = st.clipped; out.longest_clip = r.best; out.longest_clip_at = r.best_at; out.clip_runs = r.runs;
    out.trailing_clip = st.open; out.last_clip_frame = st.last_clip;
    *dst = out;
}

}  // namespace

__global__ __launch_bounds__(kScanThreads) void k_bank_signal_watch(BankWatchParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char watch_lds[];
    const uint32_t stream = blockIdx.x, tid = threadIdx.x, C = p.channels, Q = C + 1u, T = p.tile_frames, nw = T >> 6;
    const unsigned long long F = p.frames_of ? p.frames_of[stream] : p.frames;
    if (!F) return;                                             // (the whole workgroup: a stream given nothing is not touched)
    float *sh = reinterpret_cast<float *>(watch_lds);
    unsigned char *at = watch_lds + scan_tile_bytes(T, C);
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(at);
    double *sums = reinterpret_cast<double *>(at + kScanMaskBytes);
    uint32_t *counts = reinterpret_cast<uint32_t *>(at + kScanMaskBytes + kScanSumBytes);
    uint32_t *last = reinterpret_cast<uint32_t *>(at + kScanMaskBytes + kScanSumBytes + kScanCountBytes);
    const float *in = p.pcm + (p.offset_of ? p.offset_of[stream] : (unsigned long long)stream * p.stride);
    const bool owner = tid < Q;                                 // lane q owns sequence q (65 sequences at 64 channels: two waves)
    const uint32_t min_len = tid ? p.clip_min : p.silence_min;
    BankWatchSeq *mine = p.state + (size_t)stream * Q + tid;
    BankWatchSeq st{};
    if (owner) st = *mine;
    for (unsigned long long start = 0; start < F; start += T) {
        const uint32_t tn = F - start < T ? (uint32_t)(F - start) : T, nwt = (tn + 63u) >> 6;
        // The loader's 16-byte rule on the address itself: an add_device pointer is any multiple of four bytes and a stride any number
        // of floats.  The corpus is the tile's first float rounded down to 16 bytes, the tile its floats [lo, lo + tn C), lo < 4.
        const float *first = in + start * C;
        const long long lo = (long long)(reinterpret_cast<uintptr_t>(first) >> 2 & 3u);
        struct { const float *pcm; } corpus = {first - lo};
        const float *x0 = scan_load_span(sh, corpus, lo, lo + (long long)tn * C);
        scan_counts_begin(counts);
        if (tid < Q) last[tid] = 0u;
        __syncthreads();
        scan_masks(x0, p, tn, nw, masks);
        scan_sums(x0, p, tn, sums, counts);                     // (ends in a barrier: the masks are there too)
        // every word to its summary, in place, as k_signal_tiles has it; a clip word also notes the channel's last clipped frame
        for (uint32_t i = tid; i < Q * nwt; i += kScanThreads) {
            const uint32_t q = i / nwt, w = i - q * nwt, nb = word_bits(tn, w);
            const unsigned long long m = masks[q * nw + w];
            const uint32_t flags = (m ? 1u : 0u) | (m != (nb == 64u ? ~0ull : (1ull << nb) - 1ull) ? 2u : 0u);
            if (flags) atomicOr(&counts[q * 4u + 3u], flags);
            if (m && q) atomicMax(&last[q], 64u * w + 64u - (uint32_t)__builtin_clzll(m));
            if (m) masks[q * nw + w] = word_summary(m, nb, q ? p.clip_min : p.silence_min);
        }
        __syncthreads();
        if (owner) {
            SS_SCAN_JOIN(R, masks, counts, tid, nw, nwt, tn, min_len);
            // the tile folded behind the state, as k_signal_carry folds it behind its carry; the tile's frame 0 is frame st.frames
            if (R.all_true) {
                st.open += R.head;
            } else {
                const unsigned long long r = st.open + R.head;  // the run that ends in this tile's head
                if (!st.lead_set) { st.lead = r; st.lead_set = 1u; }
                if (r) {
                    st.runs += r >= (unsigned long long)min_len ? 1u : 0u;
                    if (r > st.best) { st.best = r; st.best_at = st.frames - st.open; }
                }
                st.runs += R.count;
                if (R.longest > st.best) { st.best = R.longest; st.best_at = st.frames + R.longest_at; }
                st.open = R.tail;
            }
            st.total += R.total;
            if (tid) {
                const SignalTileChannel K = scan_tile_channel(sums, counts, tid - 1u);
                st.sum += K.sum; st.sum_sq += K.sum_sq;
                st.clipped += K.clipped; st.nonfinite += K.nonfinite;
                if (st.first_nonfinite == kNone64 && K.first_nonfinite != kNone32) st.first_nonfinite = st.frames + K.first_nonfinite;
                if (last[tid]) st.last_clip = st.frames + last[tid] - 1u;
            }
            st.frames += tn;
        }
        __syncthreads();                                        // the tile, the words and the counts are the next tile's to write
    }
    // the state back, and the records as it stands; lane 0 adds the channels' clip runs up from LDS (the sums' place)
    unsigned long long *clip_runs = reinterpret_cast<unsigned long long *>(sums);
    const WatchRuns r = watch_runs(st, min_len);
    if (owner) {
        *mine = st;
        if (tid) {
            watch_store_channel(p.channel_watches + (size_t)stream * C + (tid - 1u), st, r);
            clip_runs[tid - 1u] = r.runs;
        }
    }
    __syncthreads();
    if (tid == 0u) {
        unsigned long long n = 0;
        for (uint32_t c = 0; c < C; c++) n += clip_runs[c];
        watch_store_stream(p.streams + stream, st, min_len, n);
    }
}

// ss_meter_bank_signal_watch_enable / _reset: the listed streams (streams == nullptr: streams 0 .. count - 1) have watched nothing —
// empty state and empty records, one lane per (stream, sequence)
__global__ __launch_bounds__(256) void k_bank_signal_watch_reset(BankWatchSeq *state, StreamWatch *stream_watches, ChannelWatch *channel_watches,
                                                                 const uint32_t *streams, uint32_t count, uint32_t channels)
{
    const uint32_t Q = channels + 1u, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= count * Q) return;
    const uint32_t i = idx / Q, q = idx - i * Q, s = streams ? streams[i] : i;
    const BankWatchSeq z = watch_empty();
    state[(size_t)s * Q + q] = z;
    if (q) watch_store_channel(channel_watches + (size_t)s * channels + (q - 1u), z, watch_runs(z, 1u));
    else watch_store_stream(stream_watches + s, z, 1u, 0u);
}

hipError_t launch_bank_signal_watch(const BankWatchParams &p, hipStream_t s)
{
    if (!p.n_streams) return hipSuccess;
    if (p.n_streams > 0x7FFFFFFFu || !p.channels || p.channels > (uint32_t)kMaxChannels || !p.tile_frames || (p.tile_frames & 63u) ||
        (uint64_t)p.tile_frames * p.channels > kScanTileFloats || (uint64_t)(p.channels + 1u) * (p.tile_frames >> 6) > kScanWords)
        return hipErrorInvalidValue;
    const size_t lds = scan_tile_bytes(p.tile_frames, p.channels) + kScanMaskBytes + kScanSumBytes + kScanCountBytes + kWatchLastBytes;
    hipLaunchKernelGGL(k_bank_signal_watch, dim3(p.n_streams), dim3(kScanThreads), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_bank_signal_watch_reset(BankWatchSeq *state, StreamWatch *stream_watches, ChannelWatch *channel_watches,
                                          const uint32_t *streams, uint32_t count, uint32_t channels, hipStream_t s)
{
    const uint64_t n = (uint64_t)count * (channels + 1u);
    if (!n) return hipSuccess;
    if (n >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bank_signal_watch_reset, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, s, state, stream_watches, channel_watches,
                       streams, count, channels);
    return hipGetLastError();
}

}  // namespace ssk
