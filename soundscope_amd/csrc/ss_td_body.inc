// ss_td_body.inc: the body of k_time_domain (ss_time_domain.hip), included where a kernel runs it: in k_time_domain itself and
// in the tick kernel k_tick, behind the spectrum's workgroups.  Text, not a function: as an inlined device function the
// 128-register batch instantiation came out with 20 bytes of scratch per lane where the kernel's own body has none.
// Expects in scope: the template parameters FACTOR, RING, CT, WAVE, WPS, SPLIT, LATE (or constants of those names), the kernel
// arguments p, L, tile_len, wave_lds_floats, halo_frames, and `block_id` (the workgroup's index among those that run this body).
    using Cfg = TpCfg<FACTOR>;
    // SPLIT comes in two forms.  Streaming calls (RING: the handle's add_samples, the ticks): ONE call's tiles shared by eight waves,
    // latency is everything, the state is applied BEHIND the scan ((A^L)^(c + 1) per lane, see below).  Batches (!RING): a whole
    // stream walked by the four waves of its workgroup, throughput is everything: the state in front of a tile is waited for in
    // front of the scan (as the one-wave path has it, no per-lane matrices in registers) and the tile's end state is published right
    // behind the scan; tiles are staged through the prefetch registers, the next own tile requested a whole tile ahead.
    constexpr bool kSplitBatch = SPLIT && !RING;
    constexpr bool kSplitCall = SPLIT && RING;
    // how the state crosses a tile boundary inside a workgroup: applied BEHIND the scan (streaming calls; and a handful of streams cut
    // into short segments, split_batch == 2, where the chain of a segment's eight tiles is what the launch takes) or waited for in
    // front of it (whole streams on four waves: no per-lane matrices in registers).  A constant for everything but batch SPLIT.
    constexpr bool late = LATE;                         // (template parameter; streaming calls are always instantiated with it)
    static_assert(!kSplitCall || LATE, "streaming calls hand the state over behind the scan");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    // wave-uniform by construction: tell the compiler, so that everything derived from it (stream, segment, tile
    // geometry, loop bounds) lives in SGPRs and branches on the scalar unit instead of through exec masks
    const uint32_t wave_in_block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nwb = SPLIT ? (uint32_t)(blockDim.x >> 6) : (uint32_t)kTdWavesPerBlock;      // waves of this workgroup (SPLIT: 8 or 4, a power of two)
    const uint32_t gw = SPLIT ? block_id : block_id * kTdWavesPerBlock + wave_in_block;   // global wave = (stream, segment); SPLIT: stream
    // (fix-up launch: one wave per segment > 0 — segment sg's first sub-blocks, from the state segment sg - 1 left)
    const bool fix = p.fixup != 0u;
    const uint32_t wps = fix ? p.nseg - 1u : p.nseg;                       // waves (SPLIT: workgroups) per stream
    if (gw >= p.n_streams * wps) return;                                   // whole wave leaves (no barriers used) — SPLIT: the whole workgroup
    const uint32_t stream = gw / wps, sg = gw - stream * wps + (fix ? 1u : 0u);
    TdShare *const sh = reinterpret_cast<TdShare *>(smem + (size_t)nwb * wave_lds_floats * sizeof(float));

    float *tilebuf = reinterpret_cast<float *>(smem) + (size_t)wave_in_block * wave_lds_floats;
    const TdConst &K = *p.k;
    const uint32_t C = CT ? (uint32_t)CT : p.channels;
    const uint32_t S = p.s100;
    const uint32_t nch = 64u / C;                       // chunks per tile (C <= 64)
    // Lane -> (chunk, channel).  Natural: chunk = lane / C.  Channel counts that divide 16 (compile-time) deal the chunks
    // round-robin to the four DPP rows of the wave instead: row r = lane / 16 holds chunks r, r + 4, r + 8, ..., so the scan
    // steps of distance 4, 8, 16 ... are shifts INSIDE a row (v_mov_dpp row_shr, VALU rate) and only the distances 1 and 2
    // cross rows (ds_bpermute: 22 cycles of the LDS crossbar each, and a dependent latency per step).  The walk through the
    // interleaved tile is bank-conflict free for odd L ((r + 4 q) L C + c covers 64 distinct banks) and 2-way conflicted for
    // L = 30, which td_chunk_frames still prefers where it cuts the sub-block into whole tiles of whole chunks.
    constexpr bool kRowScan = (CT != 0) && (16 % (CT ? CT : 1) == 0);
    const uint32_t lane_q = (lane & 15u) / C;           // position of this lane's chunk inside its row
    const uint32_t chunk = kRowScan ? (lane >> 4) + 4u * lane_q : lane / C;
    const uint32_t ch = kRowScan ? (lane & 15u) - lane_q * C : lane - chunk * C;
    const bool lane_ok = chunk < nch;
    // lane holding chunk c of this lane's channel
    auto lane_of_chunk = [&](uint32_t c) -> uint32_t { return kRowScan ? ((c & 3u) << 4) + (c >> 2) * C + ch : c * C + ch; };
    float *tile = tilebuf + halo_frames * C;            // tile[f*C + c]; tile[-q*C + c] = x[-q]
    unsigned *tpk = reinterpret_cast<unsigned *>(tilebuf + wave_lds_floats - kMaxChannels);   // per-channel peak slots
    TdState &st = p.state[stream];
    // streaming launches over many streams (meter banks' ragged adds): a stream without frames in this launch is not touched — the
    // wave (SPLIT: the workgroup, the length is the stream's) leaves in front of its first read of the stream's state — and the
    // tightly packed input has a base per stream.  RING only: the batch instantiations keep their instructions.
    if constexpr (RING) { if (p.frames_of && p.frames_of[stream] == 0) return; }
    const float *src_base = p.pcm + (size_t)stream * p.stream_stride;
    if constexpr (RING) { if (p.offset_of) src_base = p.pcm + p.offset_of[stream]; }
    const float *const src = src_base;

    // ---- this wave's frame range (relative to the call) and its run-in.
    // Segment boundaries sit on the absolute sub-block grid so every sub-block has one owner.
    // Multi-segment (batch) launches start from a reset meter by contract: segments must not read
    // state another segment of the same launch writes at its end.
    const bool carry_in = (p.nseg == 1);
    const uint64_t fed0 = carry_in ? st.frames_fed : 0;
    uint64_t seg_begin, seg_end;                        // frames of this call, [begin, end)
    const uint64_t n_frames = p.frames_of ? p.frames_of[stream] : p.n_frames;         // ragged batches: this stream's own length
    if (p.nseg == 1) { seg_begin = 0; seg_end = n_frames; }
    else {
        seg_begin = (uint64_t)sg * p.seg_sub * S;
        seg_end = (sg + 1 == p.nseg) ? n_frames : (uint64_t)(sg + 1) * p.seg_sub * S;
        if (fix && seg_end > seg_begin + (uint64_t)p.fix_sub * S) seg_end = seg_begin + (uint64_t)p.fix_sub * S;
        if (seg_begin > n_frames) seg_begin = n_frames;
        if (seg_end > n_frames) seg_end = n_frames;
    }
    // run-in (SS_TD_RUN_IN): sg > 0 implies seg_begin >= warm — unless a ragged stream ends in front of this segment: then the
    // range is empty and there is nothing to run in for (seg_begin was clamped to the stream's length above; stepping back from
    // THERE would start before the stream, for stream 0 before the batch's buffer: tools/fuzz_batch.py seed 117)
    uint64_t warm_frames = (sg == 0 || seg_begin >= seg_end) ? 0 : (uint64_t)p.warm_sub * S;
    if (warm_frames > seg_begin) warm_frames = seg_begin;
    uint64_t pos = seg_begin - warm_frames;             // first frame this wave reads
    uint32_t off = (uint32_t)((fed0 + pos) % S);        // position inside the current sub-block
    uint64_t sb = (fed0 + pos) / S;                     // absolute sub-block index

    // tile geometry: a tile never crosses a sub-block boundary of the absolute grid; a sub-block is
    // cut into equal pieces of at most tile_len frames
    // (toff = off % tile_len is carried along instead of being divided out for every tile)
#define SS_TILE_FRAMES(at, off_in, toff_in, out)                            \
    do {                                                                    \
        uint64_t n_ = 0;                                                    \
        if ((at) < seg_end) {                                               \
            n_ = tile_len - (toff_in);                                      \
            if (n_ > S - (off_in)) n_ = S - (off_in);                       \
            if (n_ > seg_end - (at)) n_ = seg_end - (at);                   \
        }                                                                   \
        (out) = (uint32_t)n_;                                               \
    } while (0)
    uint32_t seg;
    uint32_t toff = off % tile_len;                     // position inside the current piece of the sub-block
    uint32_t slot = (uint32_t)(sb % p.sub_cap);         // where the current sub-block's energies go (ring of sub_cap)
    SS_TILE_FRAMES(pos, off, toff, seg);
    // (the first tile's length and its prefetch stand HERE, in front of the initial state and the true-peak constants: the loads fly
    // earliest, and the temporaries of their addresses are gone before the state is live — behind it the four-waves builds spilled a
    // part of the initial state around this setup.  A wave without a tile requests nothing.)
    // register prefetch of a tile: kTdPrefetch float4 per lane (clamped index keeps it branch-free)
#define SS_PREFETCH(at, frames)                                             \
    do {                                                                    \
        const float *g_ = src + (at) * C;                                   \
        const uint32_t nv_ = ((frames) * C) >> 2;                           \
        if (nv_ != 0 && (reinterpret_cast<uintptr_t>(g_) & 15u) == 0) {     \
            const float4 *g4_ = reinterpret_cast<const float4 *>(g_);       \
            _Pragma("unroll") for (int q_ = 0; q_ < kTdPrefetch; q_++) {    \
                uint32_t i_ = lane + 64u * q_;                              \
                i_ = i_ < nv_ ? i_ : nv_ - 1;                               \
                pf[q_] = g4_[i_];                                           \
            }                                                               \
        }                                                                   \
    } while (0)

    float4 pf[kTdPrefetch];
#pragma unroll
    for (int q = 0; q < kTdPrefetch; q++) pf[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    // the tile `steps` tiles behind (pos, off, toff, seg): scalar arithmetic only
    auto tile_ahead = [&](uint32_t steps, uint64_t &apos, uint32_t &aoff, uint32_t &atoff, uint32_t &aseg) {
        for (uint32_t k = 0; k < steps && aseg != 0u; k++) {
            apos += aseg; aoff += aseg; atoff += aseg;
            const bool sd = aoff == S;
            if (sd) aoff = 0;
            if (sd || atoff >= tile_len) atoff = 0;
            SS_TILE_FRAMES(apos, aoff, atoff, aseg);
        }
    };
    if (kSplitBatch) {                                  // this wave's first tile is tile `wave_in_block`
        uint64_t apos = pos; uint32_t aoff = off, atoff = toff, aseg = seg;
        tile_ahead(wave_in_block, apos, aoff, atoff, aseg);
        if (aseg != 0u) { const uint32_t ah = apos >= halo_frames ? halo_frames : 0u; SS_PREFETCH(apos - ah, aseg + ah); }
    } else {
        SS_PREFETCH(pos, seg);
    }

    // ---- initial state: the stream's carried state (streaming call) or zeros
    double cv[4] = {0.0, 0.0, 0.0, 0.0};               // carry, held by every lane of channel `ch`
    double e_run = 0.0;                                 // this lane's share of the current sub-block's energy
    double e_call = 0.0;                                // SPLIT, a tick: this lane's share of the whole call's energy (short-term reading)
    float sp_run = 0.0f, tp_run = 0.0f;
    if (carry_in && lane_ok) {
#pragma unroll
        for (int q = 0; q < 4; q++) cv[q] = st.v[ch][q];
        if (lane < C) e_run = st.acc[lane];
    }
    if (fix && lane_ok) {                               // the exact state behind segment sg - 1
        const double *sv = p.seg_state + (((size_t)stream * p.nseg + (sg - 1u)) * C + ch) * 4u;
#pragma unroll
        for (int q = 0; q < 4; q++) cv[q] = sv[q];
    }
    bool halo_nf = false;
    if (lane < C) {
        // the frames in front of the first tile: the carried history (streaming call), the input itself (a segment > 0: the
        // interpolator and the decimation bins reach across the boundary), or zeros (the start of a stream)
        for (uint32_t q = 1; q <= halo_frames; q++) {
            float hv = 0.0f;
            if (carry_in) { if (q <= (uint32_t)kTpHistMax) hv = st.tp_hist[lane][q - 1]; }
            else if (pos >= q) hv = src[(pos - q) * C + lane];
            tile[-(int)(q * C) + (int)lane] = hv;
            if (q <= (uint32_t)kTpHistMax) halo_nf = halo_nf || !(fabsf(hv) < INFINITY);
        }
    }
    // (wave-uniform from here on) a non-finite sample — NaN, +-Inf — within the interpolator's reach in front of the current tile
    bool halo_bad = FACTOR != 0 && __ballot(halo_nf) != 0ull;
    tpk[lane] = 0u;
    if (SPLIT) {
        if (wave_in_block == 0) {
            if (lane == 0) { sh->tiles_done = 0u; sh->state_ready = 0u; sh->waves_done = 0u; }
            sh->e_lane[lane] = e_run;                    // (st.acc in the lanes of chunk 0 ... as e_run carries it)
            if (lane_ok && chunk == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++) sh->carry[ch][q] = cv[q];
            }
        }
        __syncthreads();
    }

    // ---- min-max decimation cursor (Analyzer::get_waveform fused into this pass): a bin is produced by
    // the wave whose tile holds the bin's LAST sample; its first samples may sit in the halo.
    const uint64_t wv_len = n_frames * C;
    const double wv_spp = WAVE ? (double)wv_len / (double)p.wave_window : 0.0;
    const uint32_t wv_spp_i = WAVE ? (uint32_t)wv_spp : 0u;
    // first bin whose end lies beyond interleaved index b0 (the bins in front of it ended in earlier tiles)
    auto wave_cursor_at = [&](const uint64_t b0) -> uint32_t {
        if (WAVE >= 2) return (uint32_t)(b0 / wv_spp_i);            // integer samples per bin: bin i ends at (i + 1) spp
        double gq = floor((double)b0 / wv_spp) - 2.0;
        uint32_t g = gq > 0.0 ? (uint32_t)gq : 0u;
        for (;;) {
            const double ed = ceil((double)(g + 1) * wv_spp);
            uint64_t e = (uint64_t)ed;
            if (e > wv_len) e = wv_len;
            if (e > b0 || g >= p.wave_window) break;
            g++;
        }
        return g;
    };
    uint32_t wv_cur = 0;
    if (WAVE && !SPLIT && sg != 0) wv_cur = wave_cursor_at(seg_begin * C);     // (SPLIT: set tile by tile, the waves take turns)

    const bool tp_fixed = (16u % C) == 0u;              // each lane's column always belongs to one channel
    // (the way out for a wave without a tile stands HERE, in front of the true-peak constants: behind them the four-waves builds
    // spilled half the initial state around that setup for the early way out alone)
    // ---- fold this wave's results into the stream state (a lambda: a wave without a single tile — an empty segment of a
    // ragged batch — leaves through it in front of the tile loop, so that the loop itself runs at least once and the compiler
    // keeps no spare copy of the initial state for a zero-trip path)
    auto fold_results = [&](const uint32_t ti) {
    // SPLIT: the carried state (filter, energy shares, history) is the last tile's; its wave writes it, the others only their peaks
    const bool state_owner = !SPLIT || (ti != 0u && ((ti - 1u) & (nwb - 1u)) == wave_in_block) || (ti == 0u && wave_in_block == 0u);
    if (SPLIT && state_owner && ti != 0u) e_run = sh->e_lane[lane];
    // energy of the trailing incomplete sub-block: reduce the lanes' shares (streaming calls carry it over)
    {
        double e = e_run;
        for (uint32_t d = 32; d >= 1; d >>= 1) {
            const double o = __shfl_down(e, d * C, 64);
            if (lane + d * C < 64u) e += o;
        }
        e_run = e;
    }
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        const float o = __shfl_down(sp_run, d * C, 64);
        if (lane + d * C < 64u) sp_run = fmaxf(sp_run, o);
    }
    if (FACTOR != 0 && tp_fixed) {
        uint32_t lane_f = lane;                          // (rebuilt here: see the rare paths of the true-peak product)
        asm volatile("" : "+v"(lane_f));
        atomicMax(&tpk[(lane_f & 15u) % C], __float_as_uint(tp_run));
    }
    {
        uint32_t lane_p = lane;
        asm volatile("" : "+v"(lane_p));
        if (lane_p < C) {
            if (FACTOR != 0) atomicMax(reinterpret_cast<unsigned *>(&st.true_peak[lane_p]), tpk[lane_p]);
            atomicMax(reinterpret_cast<unsigned *>(&st.sample_peak[lane_p]), __float_as_uint(sp_run));
        }
    }
    // (addresses below from opaque copies of the lane's roles: shared with the prologue's reads of the same places they were kept in
    // registers across the whole tile loop — and spilled around it in the builds that have none to spare)
    uint32_t ch_o = ch, lane_o = lane;
    asm volatile("" : "+v"(ch_o), "+v"(lane_o));
    // every segment's end state for the fix-up launch (flushed at the sub-block boundary it ends on like any carry)
    if ((!SPLIT || state_owner) && !fix && p.seg_state && lane_ok && chunk == 0) {
        double *sv = p.seg_state + (((size_t)stream * p.nseg + sg) * C + ch_o) * 4u;
#pragma unroll
        for (int q = 0; q < 4; q++) sv[q] = cv[q];
    }
    if (sg + 1 == p.nseg && state_owner && !fix) {       // the last segment owns the carried filter state
        if (lane_ok && chunk == 0) {             // ... flushed like at the end of every add_frames call (see the sub-block boundary above)
#pragma unroll
            for (int q = 0; q < 4; q++) st.v[ch_o][q] = fabs(cv[q]) < 2.2250738585072014e-308 ? 0.0 : cv[q];
        }
        if (lane_o < C) {
            st.acc[lane_o] = e_run;
            for (int q = 1; q <= kTpHistMax; q++) st.tp_hist[lane_o][q - 1] = tile[-(int)(q * C) + (int)lane_o];
        }
        if (lane_o == 0) st.frames_fed = fed0 + n_frames;
    }
    // ---- a tick's short-term reading (k_tick): the window's energy = what the ring workgroups of this launch summed over the
    // frames in front of this call (ring_window_partial) + this call's own frames, which the waves have in their lanes.  The wave
    // that arrives last adds everything in a fixed order and writes (energy, loudness) where the host reads it.
    if (SPLIT && RING && p.st_out) {
        double ec = 0.0;
        if (lane_ok) { const double wc = p.st_weights[ch]; ec = wc != 0.0 ? e_call * wc : 0.0; }      // (weight 0: the crate does not filter that channel)
        for (int d = 32; d >= 1; d >>= 1) ec += __shfl_down(ec, d, 64);
        uint32_t arrived = 0u;
        if (lane == 0) {
            sh->call_e[wave_in_block] = ec;
            arrived = __hip_atomic_fetch_add(&sh->waves_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        arrived = (uint32_t)__builtin_amdgcn_readfirstlane((int)arrived);
        if (arrived == nwb - 1u) {
            // this workgroup's share (the waves' sums in wave order), then the count: the last of the launch's contributors sums
            // (tick_reading_arrive / tick_reading_finish, ss_time_domain.hip) — no wave waits for another workgroup
            uint32_t last = 0u;
            if (lane == 0) {
                double tot = 0.0;
                for (uint32_t w = 0; w < nwb; w++) tot += sh->call_e[w];
                p.st_scratch[kRingTickBlocks + 1] = tot;
                last = tick_reading_arrive(p) ? 1u : 0u;
            }
            last = (uint32_t)__builtin_amdgcn_readfirstlane((int)last);
            if (last) tick_reading_finish(p, lane);
        }
    }
    };
    if (seg == 0) { fold_results(0u); return; }
    // stereo at factor 4 and the reference's f32 width: packed-f32 VALU form (see the tile loop), fifteen frames of both channels per lane
    // (not in the four-waves register build of whole-stream workgroups — opt-in SS_TD_WHOLE_STREAMS on a grid of more than 768 of them —
    // which has no room for the window beside the tile hand-over's state: that one keeps the matrix-pipe form)
    constexpr bool kTpValu = (FACTOR == 4) && (CT == 2 || CT == 6 || CT == 8) && !(kSplitBatch && WPS == 4);
    // factor 2 (96 ... 191 kHz: ONE branch of 24 taps): the same form with the branch cut in two halves of twelve taps that two
    // NEIGHBOURING lanes run over the same fifteen frames — the second half is the first half's structure twelve frames further back
    // with its own taps, so the taps are per-lane VGPR pairs here — and one DPP add per result joins them
    // (the three-waves register builds only: six tap pairs per lane beside the window are twelve registers the four-waves builds
    // do not have — grids of more than 768 workgroups keep the matrix-pipe form at factor 2)
    constexpr bool kTpValu2 = (FACTOR == 2) && (CT == 2 || CT == 6 || CT == 8) && WPS <= 3;
    // Channel counts that do not divide sixteen (3, 5, 7 ...: the matrix-pipe form walks them channel by channel, 2-3x slower) and
    // factor 2 in the four-waves builds of 2 / 6 / 8 channels: a lane takes fifteen frames of ONE channel and runs the branches with
    // plain v_fma_f32, taps from SGPRs.  Mono, 4 and 16 channels stay on the matrix pipe: measured 12-14 % FASTER there than this
    // form (profiles/r06_ab_tp_plain_fma.txt).  (Not the four-waves build of whole-stream workgroups.)
    constexpr bool kTpPlain = (FACTOR != 0) && !kTpValu && !kTpValu2 && !(kSplitBatch && WPS == 4) && (CT == 0 || CT == 2 || CT == 6 || CT == 8);
    constexpr int kTpValuFrames = 15;
    constexpr uint32_t kTpPairs = CT ? (uint32_t)CT / 2u : 1u;      // channel pairs (c, c + 1) of a frame: the packed operands
    // ---- constant A fragments of the banded-Toeplitz true-peak product, and this lane's column role
    const int mrow = lane & 15, kq = lane >> 4;
    float afrag[Cfg::KSTEPS > 0 ? Cfg::KSTEPS : 1];
    const uint32_t tp_bpg = 16u / (tp_fixed ? C : 1u);  // blocks per 16-column group
    int tp_lane_off = 0;                                // float offset of this lane's window inside group 0
    // (general-count builds that also hold the plain-FMA form rebuild the fragments per tile from an opaque lane id: kept across the
    // tile loop beside that form's window they were what the four-waves build spilled)
    constexpr bool kAfragPerTile = kTpPlain && CT == 0;
    auto build_afrag = [&](uint32_t lane_src, float (&af)[Cfg::KSTEPS > 0 ? Cfg::KSTEPS : 1], int &lane_off) {
        const int mr = (int)(lane_src & 15u), kqq = (int)(lane_src >> 4);
        const int fph = mr / Cfg::BLK, r = mr - fph * Cfg::BLK;
#pragma unroll
        for (int s = 0; s < Cfg::KSTEPS; s++) {
            const int k = 4 * s + kqq;
            const int t = Cfg::HIST - 1 + r - k;
            af[s] = (mr < Cfg::ROWS && t >= 0 && t < Cfg::HIST) ? K.tp[fph][t] : 0.0f;   // row 15 (factor 4) is all zero
        }
        lane_off = ((int)((uint32_t)mr / C) * Cfg::BLK - (Cfg::HIST - 1) + kqq) * (int)C + (int)((uint32_t)mr % C);
    };
    if (FACTOR != 0 && !kAfragPerTile) build_afrag(lane, afrag, tp_lane_off);
    // Planar f16-split form of the same product (factor 4, channel counts that divide 16): after the K-weighting
    // passes of a tile every sample is converted ONCE to an f16 pair, s x = x_hi + x_lo with s a power of two taken
    // from the tile's own sample peak (so accuracy does not depend on level and nothing over- or underflows), and
    // stored IN PLACE over the f32 tile (dead by then; the next tile's halo is copied out first) in 256-byte blocks
    // of FB = 64 / C frames: [hi c = 0 .. C-1][lo c = 0 .. C-1], FB halves each, block k holding converted frames
    // [k FB - 12, (k + 1) FB - 12).  A block occupies exactly the bytes of FB source frames, so the conversion walks
    // the blocks from the top down and never overwrites a sample it still has to read.
    // Column (channel, block of 4 outputs b) then reads its 16-sample window [4 b - 12, 4 b + 4) as aligned 8-byte
    // pieces of the hi and the lo plane, and D = A_hi B_hi + A_hi B_lo + A_lo B_hi runs as three
    // v_mfma_f32_16x16x16_f16 with rows (phase f, output r), A[(f,r)][k] = c_f[12 + r - k]; the dropped lo*lo term and
    // the split remainders are < 2^-21 of the tile's peak.  One group of 16 columns advances every window by exactly one
    // block, so the read addresses of a lane just step by 256 bytes per group.  Unlike the f32 MFMA this runs beside
    // other waves' f64 VALU work (tools/ubench4.hip), and the per-window split that used to cost 18 VALU
    // lane-instructions per sample is about 4.
    // (gfx950's K = 32 form, v_mfma_f32_16x16x32_f16 — two products instead of three — is NOT used: a wave issuing it
    // corrupts v_pk_add_f32 results of OTHER waves on the same SIMD, i.e. of the spectrum kernel when the two kernels
    // share the chip; isolated by tools/ubench_k32_interference.hip, profiles/r03_ubench_k32_interference.txt, DESIGN 8.)
    constexpr bool kTpPlanar = (FACTOR == 4);
    halfx4 a16_lo = {0, 0, 0, 0};                       // lane (mrow, kq): a_lo[4 kq + j], j = 0..3
    halfx4 a16_hi = {0, 0, 0, 0};                       //                  a_hi[4 kq + j]
    if (kTpPlanar) {
        const int fph = mrow >> 2, r = mrow & 3;       // rows 0..11 = (phase, output); rows 12..15 are zero
        auto tap = [&](int k) -> float {               // A[(f, r)][k] = c_f[12 + r - k]
            const int t = 12 + r - k;
            return (mrow < 12 && t >= 0 && t < 12) ? K.tp[fph][t] : 0.0f;
        };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float c = tap(4 * kq + j);
            a16_lo[j] = (_Float16)(c - (float)(_Float16)c);
            a16_hi[j] = (_Float16)c;
        }
    }
    // sample peak (as bits of a non-negative float) of the 12 frames in front of the current tile: the FIR window
    // reaches them, so they take part in the choice of the tile's scale.  A streaming call starts from carried history.
    uint32_t tp_prev_bits = 0;
    if (kTpPlanar) {
        __builtin_amdgcn_wave_barrier();
        float h = 0.0f;
        if (lane < C)
            for (int q = 1; q <= 12; q++) h = fmaxf(h, fabsf(tile[-(int)(q * C) + (int)lane]));
        tp_prev_bits = wave_max_nonneg_bits(h);
    }
    const double a1 = K.a[1], a2 = K.a[2], a3 = K.a[3], a4 = K.a[4];
    // output taps: the instantiations that publish y (RING: handles, ticks, banks) keep the gain b0 in them; batches — the fix-up
    // launch with the main one, so that both halves of a hand-over agree — need y for e += y^2 alone and run them with unit gain,
    // referred to the input (SS_KW_OUT_UNIT, ss_td_impl.h: y / b0 = x + g1 v1 + ... + g4 v4).  A tile's energy is scaled by b0^2
    // where it joins e_run, so everything behind that point — the sub-block close, the trailing partial sub-block, TdState::acc,
    // which a later streaming call continues from — is in y's units
    // (not the four-waves register build of whole-stream workgroups, opt-in: five samples' tap chains in flight cost that build
    // 12-24 more bytes of scratch per lane than the partial sums do — it has no hand-over launch to agree with)
    constexpr bool kUnitGainBuild = !RING && !(kSplitBatch && WPS == 4);
    // (a tile with a non-finite sample among its frames or in the state in front of it runs the gained taps, whatever the build:
    // where an infinity turns into a NaN — in the step behind it, Inf - Inf between b0 v0 and b1 v1 — decides which sub-block's
    // energy is NaN and which +Inf, and the gating reads that as the crate's filter leaves it; x + g1 Inf would stay an infinity
    // one step longer.  Rare and wave-uniform: see pass 2.)
    const double bt0 = K.b[0];
    const double bt1 = kUnitGainBuild ? K.bu[1] : K.b[1], bt2 = kUnitGainBuild ? K.bu[2] : K.b[2];
    const double bt3 = kUnitGainBuild ? K.bu[3] : K.b[3], bt4 = kUnitGainBuild ? K.bu[4] : K.b[4];

    SS_PROF_DECL

    uint32_t ti = 0;                                    // index of the tile within the call (SPLIT: whose turn it is)
    do {
        // the tile behind this one
        const uint64_t npos = pos + seg;
        uint32_t noff = off + seg, ntoff = toff + seg;
        const bool sub_done = (noff == S);
        if (sub_done) noff = 0;
        if (sub_done || ntoff >= tile_len) ntoff = 0;
        uint32_t nseg_frames;
        SS_TILE_FRAMES(npos, noff, ntoff, nseg_frames);
        if (!SPLIT || (ti & (nwb - 1u)) == wave_in_block) {
        SS_TRACE(8);
        // keep the scan matrices in memory (scalar loads at the point of use): hoisting all of them
        // out of the tile loop would cost 224 SGPRs
        const_f64_ptr mpow = (const_f64_ptr)(uintptr_t)((kSplitCall || (kSplitBatch && p.split_batch == 2u)) ? &K.m_pow_split[0][0] : &K.m_pow[0][0]);      // (by chunk length: td_launch_w)
        asm volatile("" : "+s"(mpow));
        const bool warm = pos < seg_begin;              // run-in tile: filter only
        const uint32_t nchunks = (seg + L - 1) / L;

        // ---- stage the tile from the prefetch registers (remainder / unaligned: direct)
        // (batches on whole workgroups: the halo of a tile is the input in front of it — staged and prefetched WITH the tile, as
        // one run of halo + tile frames, wherever a whole halo exists)
        const uint32_t hst = (kSplitBatch && pos >= halo_frames) ? halo_frames : 0u;
        {
            const float *g = src + (pos - hst) * C;
            const uint32_t total = (seg + hst) * C;
            float *const tbase = tile - hst * C;
            uint32_t done = 0;
            if ((reinterpret_cast<uintptr_t>(g) & 15u) == 0) {
                const uint32_t nv = total >> 2;
                float4 *t4 = reinterpret_cast<float4 *>(tbase);
                // no predicate: a lane past the tile's end holds a copy of the last float4 (clamped prefetch index) and writes
                // it where it belongs — the same value to the same place, without exec-mask branches
                const uint32_t last = nv ? nv - 1u : 0u;
                // (a streaming call's waves: no register prefetch; short segments on eight waves, LATE: the wave's FIRST tile comes
                // from the registers — requested in front of the loop — and a second one, where a segment has more than eight
                // tiles, is loaded here: holding a look-ahead across the tile beside the per-lane matrices would spill)
                const bool from_pf = !kSplitCall && (!(kSplitBatch && late) || ti < nwb);
                if (from_pf) {
                    // (whole rounds of 64 float4 through one lane address and immediate offsets, the clamp only for the round the tile
                    // ends in: measured in round 6 — the compiler then splits the 16-byte loads into dwords; not kept)
#pragma unroll
                    for (int q = 0; q < kTdPrefetch; q++) {
                        const uint32_t i = lane + 64u * q;
                        if (nv) t4[i < last ? i : last] = pf[q];           // (nv is wave-uniform)
                    }
                }
                const float4 *g4 = reinterpret_cast<const float4 *>(g);
                uint32_t lane_s = lane;
                asm volatile("" : "+v"(lane_s));
                for (uint32_t i = lane_s + 64u * (from_pf ? kTdPrefetch : 0); i < nv; i += 64u) t4[i] = g4[i];
                done = nv << 2;
            }
            for (uint32_t i = done + lane; i < total; i += 64u) tbase[i] = g[i];
            for (uint32_t i = seg * C + lane; i < seg * C + kTdTailFrames * C; i += 64u) tile[i] = 0.0f;
        }
        // next tile's loads fly while this one is processed
        if (!SPLIT) SS_PREFETCH(npos, nseg_frames);
        if (kSplitBatch && !late) {                     // this wave's NEXT tile lies nwb tiles behind this one
            uint64_t apos = npos; uint32_t aoff = noff, atoff = ntoff, aseg = nseg_frames;
            tile_ahead(nwb - 1u, apos, aoff, atoff, aseg);
            if (aseg != 0u) { const uint32_t ah = apos >= halo_frames ? halo_frames : 0u; SS_PREFETCH(apos - ah, aseg + ah); }
        }
        if (SPLIT && hst == 0u) {
            // the halo of a tile another wave left: the frames in front of it come from the call's input, or — in front of
            // the call — from the carried history (tp_hist[c][k] = frame -1 - k of the call)
            for (uint32_t j = lane; j < halo_frames * C; j += 64u) {
                const uint32_t q = j / C + 1u, c = j - (q - 1u) * C;
                float v = 0.0f;
                if (pos >= q) v = src[(pos - q) * C + c];
                else if (q - (uint32_t)pos <= (uint32_t)kTpHistMax) v = st.tp_hist[c][q - (uint32_t)pos - 1u];
                tile[-(int)(q * C) + (int)c] = v;
            }
        }
        if (SPLIT && kTpPlanar) {                       // sample peak of the twelve frames the first FIR windows reach back to
            __builtin_amdgcn_wave_barrier();
            float h = 0.0f;
            if (lane < C)
                for (int q = 1; q <= 12; q++) h = fmaxf(h, fabsf(tile[-(int)(q * C) + (int)lane]));
            tp_prev_bits = wave_max_nonneg_bits(h);
        }
        if (SPLIT && FACTOR != 0) {                     // (one wave per run of tiles: carried along at the tile's end instead)
            const uint32_t hn = (halo_frames < (uint32_t)kTpHistMax ? halo_frames : (uint32_t)kTpHistMax) * C;
            bool nf = false;
            for (uint32_t j = lane; j < hn; j += 64u) nf = nf || !(fabsf(tile[-(int)(j + 1u)]) < INFINITY);
            halo_bad = __ballot(nf) != 0ull;
        }
        __builtin_amdgcn_wave_barrier();               // LDS is in-order per wave: only ordering is needed
        SS_PROF_MARK(0);

        // ---- min-max decimation of the bins that END inside this tile (analyzer.rs:107-137): bin i =
        // [floor(i*spp), min(ceil((i+1)*spp), len)), the same f64 expressions as the reference; eight lanes
        // per bin, IEEE minNum/maxNum seeded with NaN (f32::min/max ignore NaN; an all-NaN bin stays NaN)
        if (WAVE && !warm) {
            if (SPLIT) wv_cur = wave_cursor_at(pos * C);
            // (the host only fuses when the stream length fits 31 bits, so 32-bit indices are exact)
            const uint32_t t0 = (uint32_t)(pos * C), t1 = (uint32_t)((pos + seg) * C);   // tile's interleaved index range
            const uint32_t wlen = (uint32_t)wv_len;
            // (the bin roles below are rebuilt per tile from opaque copies of the lane id instead of living in registers across the tile
            // loop, which the four-waves build has none to spare of)
            // Exact-integer samples-per-bin that is a multiple of four (96 at 48 kHz stereo, W = duration in ms):
            // floor(i spp) and ceil((i+1) spp) are the integer products themselves, bins are 16-byte aligned in the
            // tile, so eight lanes cover a bin with 16-byte LDS reads: eight bins per iteration.
            if (WAVE >= 2) {
                // Eight lanes per bin, eight bins per iteration.  (Four lanes per bin — sixteen bins per iteration, a 48 kHz stereo tile's
                // twenty bins in two iterations instead of three, 40 VALU instructions fewer per tile — measured in round 6: no faster,
                // +0.8 % if anything; this phase runs at the lowest wave priority, in the shadow of the other waves' f64 passes.)
                constexpr uint32_t LPB = 8u, NR = 24u / LPB, BPI = 64u / LPB;      // lanes per bin, unconditional reads, bins per iteration
                uint32_t lane_d = lane;
                asm volatile("" : "+v"(lane_d));
                const uint32_t lane8 = lane_d & (LPB - 1u), n4 = wv_spp_i >> 2, lbin = lane_d / LPB;
                for (;;) {
                    const uint32_t i = wv_cur + lbin;
                    const uint32_t bs = i * wv_spp_i, be = bs + wv_spp_i;           // be <= len: W spp == len exactly
                    const bool valid = i < p.wave_window && be <= t1;
                    float mn = __builtin_nanf(""), mx = __builtin_nanf("");
                    if (valid) {
                        const float4 *bp4 = reinterpret_cast<const float4 *>(tile + ((int)bs - (int)t0));   // may reach into the halo
                        // NR reads cover spp <= 96 (48 kHz stereo), the next ones spp <= 128; clamped indices repeat an element,
                        // which cannot change a min / max.  All reads are issued before the arithmetic.
                        // (three reads in flight at a time: twelve registers — six at once is what the four-waves build has no room for)
#pragma unroll
                        for (uint32_t gq = 0; gq < NR; gq += 3u) {
                            float4 v[3];
#pragma unroll
                            for (uint32_t it = 0; it < 3u; it++) {
                                uint32_t j = lane8 + LPB * (gq + it);
                                j = j < n4 ? j : n4 - 1;
                                v[it] = bp4[j];
                            }
#if defined(__HIP_DEVICE_COMPILE__)
                            __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
                            for (uint32_t it = 0; it < 3u; it++) {
                                mn = fminf(fminf(mn, v[it].x), fminf(fminf(v[it].y, v[it].z), v[it].w));
                                mx = fmaxf(fmaxf(mx, v[it].x), fmaxf(fmaxf(v[it].y, v[it].z), v[it].w));
                            }
#if defined(__HIP_DEVICE_COMPILE__)
                            __builtin_amdgcn_sched_barrier(0);
#endif
                        }
                        if (n4 > 24u) {                                                // wave-uniform
#pragma unroll
                            for (uint32_t it = NR; it < 32u / LPB; it++) {
                                const uint32_t j = lane8 + LPB * it;
                                const float4 w = bp4[j < n4 ? j : n4 - 1];
                                mn = fminf(fminf(mn, w.x), fminf(fminf(w.y, w.z), w.w));
                                mx = fmaxf(fmaxf(mx, w.x), fmaxf(fmaxf(w.y, w.z), w.w));
                            }
                        }
                        if (WAVE == 3)                                                 // longer bins (192 at 96 kHz stereo)
                            for (uint32_t j = lane8 + 32u; j < n4; j += 8u) {
                                const float4 w = bp4[j];
                                mn = fminf(fminf(mn, w.x), fminf(fminf(w.y, w.z), w.w));
                                mx = fmaxf(fmaxf(mx, w.x), fmaxf(fmaxf(w.y, w.z), w.w));
                            }
                    }
                    // all-reduce over the bin's lanes: xor 1, xor 2 (quad_perm), and — eight lanes — the mirror inside each half row.
                    // DPP on the operand of v_min / v_max itself (IEEE minNum / maxNum: a NaN partner is ignored, an all-NaN bin stays
                    // NaN); written out because the builtin route costs four instructions per step and value.  The s_nop keep the two
                    // wait states a DPP read needs after a VALU write of the same register.
                    asm volatile("s_nop 1\n\t"
                                 "v_min_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                 "v_max_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                 "s_nop 0\n\t"
                                 "v_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                                 "v_max_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
                                 : "+v"(mn), "+v"(mx));
                    if (LPB == 8u)
                        asm volatile("s_nop 1\n\t"
                                     "v_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                                     "v_max_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf"
                                     : "+v"(mn), "+v"(mx));
                    if (valid && lane8 == 0) {
                        float2 *o = reinterpret_cast<float2 *>(p.wave_out + (size_t)stream * p.wave_stride) + i;
                        *o = make_float2(mn, mx);
                    }
                    const uint32_t nvalid = (uint32_t)__popcll(__ballot(valid && lane8 == 0));
                    wv_cur += nvalid;
                    if (nvalid < BPI) break;                  // the next bin ends beyond this tile
                }
            } else {
                // Any samples-per-bin (44.1 kHz material: 88.2): a bin starts and ends anywhere, so it is read as the ALIGNED 16-byte
                // pieces of the tile that overlap it — eight lanes per bin, eight bins per iteration: the pieces that lie wholly inside
                // the bin through clamped indices without predicates (a repeated piece cannot change a min / max), the first and the last
                // overlapping piece by the bin's even and odd lanes with their elements outside [bs, be) replaced by NaN, which minNum /
                // maxNum ignore.  (Until round 6: sixteen lanes per bin reading dwords, four bins per iteration — 900 instructions per
                // 1470-frame tile at 44.1 kHz stereo, a fifth of the kernel.)
                uint32_t lane_d = lane;
                asm volatile("" : "+v"(lane_d));
                const uint32_t lane8 = lane_d & 7u, lbin = lane_d >> 3;
                const float4 *t4 = reinterpret_cast<const float4 *>(tile);
                for (;;) {
                    const uint32_t i = wv_cur + lbin;
                    const uint32_t bs = (uint32_t)((double)i * wv_spp);
                    uint32_t be = (uint32_t)ceil((double)(i + 1) * wv_spp);
                    if (be > wlen) be = wlen;
                    const bool valid = i < p.wave_window && be <= t1 && bs < wlen;
                    float mn = __builtin_nanf(""), mx = __builtin_nanf("");
                    if (valid) {
                        const int r0 = (int)bs - (int)t0, r1 = (int)be - (int)t0;     // the bin, relative to the tile (r0 may lie in the halo)
                        {   // the piece the bin starts in (even lanes) / ends in (odd lanes): element c of piece qe is sample 4 qe + c
                            const int qe = (lane8 & 1u) ? ((r1 + 3) >> 2) - 1 : (r0 >> 2);
                            const float4 ev = t4[qe];
                            const uint32_t lo = (uint32_t)(r0 - 4 * qe), span = (uint32_t)(r1 - r0);   // inside: (c - lo) < span, unsigned
                            const float qn = __builtin_nanf("");
                            const float e0 = (0u - lo) < span ? ev.x : qn, e1 = (1u - lo) < span ? ev.y : qn;
                            const float e2 = (2u - lo) < span ? ev.z : qn, e3 = (3u - lo) < span ? ev.w : qn;
                            mn = fminf(fminf(e0, e1), fminf(e2, e3));
                            mx = fmaxf(fmaxf(e0, e1), fmaxf(e2, e3));
                        }
#if defined(__HIP_DEVICE_COMPILE__)
                        __builtin_amdgcn_sched_barrier(0);
#endif
                        const int qi0 = (r0 + 3) >> 2, nin = (r1 >> 2) - qi0;        // pieces wholly inside: [qi0, qi0 + nin), nin >= 2 (spp >= 16)
                        {
                            // (two reads in flight, not three: the four-waves build of this form has four registers fewer to spare
                            // than the whole-samples-per-bin form above)
                            float4 v[2];
#pragma unroll
                            for (int it = 0; it < 2; it++) {
                                int j = (int)lane8 + 8 * it;
                                j = j < nin ? j : nin - 1;
                                v[it] = t4[qi0 + j];
                            }
#if defined(__HIP_DEVICE_COMPILE__)
                            __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
                            for (int it = 0; it < 2; it++) {
                                mn = fminf(fminf(mn, v[it].x), fminf(fminf(v[it].y, v[it].z), v[it].w));
                                mx = fmaxf(fmaxf(mx, v[it].x), fmaxf(fmaxf(v[it].y, v[it].z), v[it].w));
                            }
                            for (int j = (int)lane8 + 16; j < nin; j += 8) {
                                const float4 w = t4[qi0 + j];
                                mn = fminf(fminf(mn, w.x), fminf(fminf(w.y, w.z), w.w));
                                mx = fmaxf(fmaxf(mx, w.x), fmaxf(fmaxf(w.y, w.z), w.w));
                            }
                        }
                    }
                    asm volatile("s_nop 1\n\t"
                                 "v_min_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                 "v_max_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                 "s_nop 0\n\t"
                                 "v_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                                 "v_max_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
                                 "s_nop 0\n\t"
                                 "v_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
                                 "v_max_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf"
                                 : "+v"(mn), "+v"(mx));
                    if (valid && lane8 == 0) {
                        float2 *o = reinterpret_cast<float2 *>(p.wave_out + (size_t)stream * p.wave_stride) + i;
                        *o = make_float2(mn, mx);
                    }
                    const uint32_t nvalid = (uint32_t)__popcll(__ballot(valid && lane8 == 0));
                    wv_cur += nvalid;
                    if (nvalid < 8u) break;                   // the next bin ends beyond this tile
                }
            }
        }

        SS_PROF_MARK(1);
        const bool active = lane_ok && chunk < nchunks;
        const uint32_t len = active ? ((seg - chunk * L) < L ? (seg - chunk * L) : L) : 0u;
        const float *xs = tile + (size_t)chunk * L * C + ch;
        const uint32_t nb_full = L / kTdBatch;          // whole batches in a full chunk
        // (Stereo reading whole frames as ds_read_b64 + select in the two passes below — mod-64 banks, two deep instead of the
        // four of ds_read_b32's mod-32 banks at this chunk stride — was measured: 1.99 -> 2.13 ms,
        // profiles/r03_ab_ms1_td_variants.txt; the select and the unmergeable reads cost more than the conflicts.  And the
        // conflicts cost little: with both passes walking the tile lane-linear (conflict-free, wrong results, timing only)
        // the kernel went from 1.946 to 1.918 ms, profiles/r03_ab_td_conflict_free_passes.txt.)

        // ---- pass 1: zero-state response of the state recurrence
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        bool tile_nf = false;                           // (wave-uniform) a non-finite sample among this tile's own frames
        {
            // One wave per run of tiles (!SPLIT): the state in front of the tile is in this wave's registers, so chunk 0 runs its
            // first pass FROM it and comes out with its true end state — where every chunk started from zero, chunk 0's lanes then
            // added (A^L) D cv as a matrix product: 28 f64 instructions of the whole wave for two lanes' worth of work.
            const bool from_state = !SPLIT && chunk == 0;
            double v1 = from_state ? cv[0] : 0.0, v2 = from_state ? cv[1] : 0.0, v3 = from_state ? cv[2] : 0.0, v4 = from_state ? cv[3] : 0.0;
            uint32_t i = 0;
            if (len == L) {                             // full chunk: batched, predicate-free, look-ahead form
                const float *xp = xs + 3 * C;           // the batch loop consumes x[i + 3]
                SS_KW_LA_INIT((double)xs[0], (double)xs[C], (double)xs[2 * C])
                for (uint32_t bq = 0; bq < nb_full; bq++, xp += kTdBatch * C) {
                    float xb[kTdBatch];
#pragma unroll
                    for (int u = 0; u < kTdBatch; u++) xb[u] = xp[u * (int)C];   // reaches <= 3 frames past the chunk (slack)
#pragma unroll
                    for (int u = 0; u < kTdBatch; u++) { SS_KW_LA_STEP((double)xb[u]) SS_KW_SHIFT() }
                }
                i = nb_full * kTdBatch;
                if (i < L) {                            // chunk lengths that are no multiple of the batch (L = 49 at 44.1 kHz):
                    const uint32_t rem = L - i;         // one more batch of reads (into the next chunk or the zeroed slack), of
                    float xb[kTdBatch];                 // which the first `rem` (wave-uniform) are consumed
#pragma unroll
                    for (int u = 0; u < kTdBatch; u++) xb[u] = xp[u * (int)C];
#pragma unroll
                    for (int u = 0; u < kTdBatch - 1; u++)
                        if ((uint32_t)u < rem) { SS_KW_LA_STEP((double)xb[u]) SS_KW_SHIFT() }
                    i = L;
                }
            }
            for (; i < len; i++) { SS_KW_STATE((double)xs[i * C]) SS_KW_SHIFT() }
            z[0] = v1; z[1] = v2; z[2] = v3; z[3] = v4;
            // Non-finite input.  A NaN or an infinity among this chunk's samples leaves its zero-state end non-finite (NaN never
            // leaves the recurrence; an infinity turns into one within two steps, Inf - Inf, unless it is the chunk's last sample) —
            // and nothing else can: the run started from zero, f32 input cannot overflow f64.  (Chunk 0 of a one-wave run starts
            // from the carried state: once that is poisoned every later tile of the run reports itself — the same sub-block or a
            // later one, which the maximum below ignores — and keeps to the exact true-peak loop.)  One compare per tile.  Inside a
            // segment the recurrence itself carries the poison on like the crate's Filter::process does; what a segmented launch
            // needs to know is the FIRST such sub-block per channel (TdState::bad_key: the gating kernels), and the true-peak
            // product needs to know that this tile does not go through the matrix pipe (0 x NaN, below).
            tile_nf = __ballot(active && !(fabs(v1) < (double)INFINITY)) != 0ull;
            if (tile_nf) {                              // (rare: everything it needs rebuilt from an opaque copy of the lane id, so that
                uint32_t lane_b = lane;                 //  nothing of it is kept in registers across the tile loop)
                asm volatile("" : "+v"(lane_b));
                const uint32_t ch_b = kRowScan ? (lane_b & 15u) % C : lane_b % C;
                if (!(fabs(v1) < (double)INFINITY))     // (a lane without a chunk ran no step: v1 = 0)
                    atomicMax(&p.state[stream].bad_key[ch_b], ~(uint32_t)(sb < 0xFFFFFFFEull ? sb : 0xFFFFFFFEull));
            }
            state_diff(z);                              // the scan runs in difference coordinates
            // (SPLIT: the state in front of this tile is another wave's to deliver — the scan below runs without it, and what
            // it adds to every chunk's end state, (A^L)^(c + 1) D cv by linearity, is applied when it arrives: the tile-to-tile
            // chain is a read, sixteen FMAs and a write per tile instead of the whole scan)
            if (kSplitBatch && !late) {
                // the state in front of this tile: published by the wave of the tile before it, right behind ITS scan
                while (__hip_atomic_load(&sh->state_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < ti) __builtin_amdgcn_s_sleep(1);
                if (lane_ok) {
#pragma unroll
                    for (int q = 0; q < 4; q++) cv[q] = sh->carry[ch][q];
                }
            }
            if (SPLIT && !late && active && chunk == 0) {
                double cw[4] = {cv[0], cv[1], cv[2], cv[3]};
                state_diff(cw);
                mat4_apply_add(mpow, cw, z);
            }
        }
        SS_PROF_MARK(2);
        double hc[16];                                  // SPLIT: this lane's (A^L)^(chunk + 1), requested in front of the scan
        double zown[4] = {0.0, 0.0, 0.0, 0.0};          // SPLIT: the zero-state end of this lane's own chunk (the scan overwrites z)
        double cwd[4] = {0.0, 0.0, 0.0, 0.0};           // SPLIT: the state in front of the tile, in difference coordinates
        double pz[4] = {0.0, 0.0, 0.0, 0.0};            // SPLIT: the state in front of this lane's chunk, in difference coordinates
        if (late) {
#pragma unroll
            for (int q = 0; q < 4; q++) zown[q] = z[q];
            const double *hp = &K.m_chunk_split[lane_ok ? chunk : 0u][0];
#pragma unroll
            for (int q = 0; q < 16; q++) hc[q] = hp[q];
        }
        // ---- in-wave scan over chunks: z_i += (A^L)^(2^k) z_{i - 2^k}  (the steps commute: powers of one matrix)
        if (kRowScan) {
            // distances 1 and 2: the source chunk sits in another row
#pragma unroll
            for (int kstep = 0; kstep < 2; kstep++) {
                const uint32_t d = 1u << kstep;
                if (d >= nchunks) break;                // wave-uniform
                const int src = (int)lane_of_chunk(chunk >= d ? chunk - d : 0u);
                const double xin[4] = {__shfl(z[0], src, 64), __shfl(z[1], src, 64), __shfl(z[2], src, 64), __shfl(z[3], src, 64)};
                if (active && chunk >= d) mat4_apply_add(mpow + 16 * kstep, xin, z);
            }
            // distances 4, 8, 16, 32: q - 1, q - 2, q - 4, q - 8 inside the row; lanes without a source read zeros (bound_ctrl)
#define SS_DPP_SHR64(v, N)                                                                                              \
    __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x110 + (N), 0xF, 0xF, true),                      \
                     __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x110 + (N), 0xF, 0xF, true))
#define SS_ROW_STEP(N, KSTEP)                                                                                           \
    if ((4u << ((KSTEP) - 2)) < nchunks) {                                                                                 \
        const double xin[4] = {SS_DPP_SHR64(z[0], N), SS_DPP_SHR64(z[1], N), SS_DPP_SHR64(z[2], N), SS_DPP_SHR64(z[3], N)}; \
        mat4_apply_add(mpow + 16 * (KSTEP), xin, z);                                                                    \
    }
            constexpr int CC = CT ? CT : 1;
            if (CC * 1 <= 8) { SS_ROW_STEP(CC * 1 <= 8 ? CC * 1 : 1, 2) }
            if (CC * 2 <= 8) { SS_ROW_STEP(CC * 2 <= 8 ? CC * 2 : 1, 3) }
            if (CC * 4 <= 8) { SS_ROW_STEP(CC * 4 <= 8 ? CC * 4 : 1, 4) }
            if (CC * 8 <= 8) { SS_ROW_STEP(CC * 8 <= 8 ? CC * 8 : 1, 5) }
#undef SS_ROW_STEP
#undef SS_DPP_SHR64
        } else {
            for (int kstep = 0; (1u << kstep) < nchunks; kstep++) {
                const uint32_t d = (1u << kstep) * C;
                const double xin[4] = {__shfl_up(z[0], d, 64), __shfl_up(z[1], d, 64), __shfl_up(z[2], d, 64), __shfl_up(z[3], d, 64)};
                if (active && lane >= d) mat4_apply_add(mpow + 16 * kstep, xin, z);
            }
        }
        if (late) {
            // the state in front of this tile: published by the wave of the tile before it
            while (__hip_atomic_load(&sh->state_ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < ti) __builtin_amdgcn_s_sleep(1);
            SS_TRACE(9);
            if (lane_ok) {
#pragma unroll
                for (int q = 0; q < 4; q++) cv[q] = sh->carry[ch][q];
            }
            double cw[4] = {cv[0], cv[1], cv[2], cv[3]};
            state_diff(cw);
            if (lane_ok && chunk < nchunks) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    z[r] = fma(hc[r * 4 + 0], cw[0], fma(hc[r * 4 + 1], cw[1], fma(hc[r * 4 + 2], cw[2], fma(hc[r * 4 + 3], cw[3], z[r]))));
            }
#pragma unroll
            for (int q = 0; q < 4; q++) cwd[q] = cw[q];
        }
        // z = state after this lane's chunk (valid for full chunks); initial state = previous chunk's
        double v1, v2, v3, v4;
        {
            const int src = (int)lane_of_chunk(chunk ? chunk - 1u : 0u);
            const double p0 = __shfl(z[0], src, 64), p1 = __shfl(z[1], src, 64), p2 = __shfl(z[2], src, 64), p3 = __shfl(z[3], src, 64);
            const bool first = chunk == 0;
            if (late) { pz[0] = first ? cwd[0] : p0; pz[1] = first ? cwd[1] : p1; pz[2] = first ? cwd[2] : p2; pz[3] = first ? cwd[3] : p3; }
            double q1 = p0, q2 = p1, q3 = p2, q4 = p3;
            state_undiff(q1, q2, q3, q4);               // back to (v1 .. v4)
            v1 = first ? cv[0] : q1; v2 = first ? cv[1] : q2; v3 = first ? cv[2] : q3; v4 = first ? cv[3] : q4;
        }
        // SPLIT: the tile's end state stands in the last chunk's lanes right here — a whole chunk's as the scan left it, a
        // partial one's (rem < L samples) as its own zero-state end + A^rem x the state in front of it — and the next tile's wave
        // gets it a whole second pass earlier (flushed like every carry across a gating-block boundary, see tile_carry_out).
        // Not in the tail of a decay: near the sub-normal range the scan's difference coordinates lose digits the plain
        // recurrence keeps (the crate's flush decides on the state's last bits there) — such a tile hands over behind its
        // second pass.
        bool early_state = false;
        if (SPLIT) {
            const uint32_t rem = seg - (nchunks - 1u) * L;                  // samples of the last chunk (wave-uniform)
            double s1 = z[0], s2 = z[1], s3 = z[2], s4 = z[3];
            if (late && rem != L) {
                double sp_[4] = {zown[0], zown[1], zown[2], zown[3]};
                const_f64_ptr mrem = (const_f64_ptr)(uintptr_t)&K.m_step_split[rem < 68u ? rem : 0u][0];
                mat4_apply_add(mrem, pz, sp_);
                s1 = sp_[0]; s2 = sp_[1]; s3 = sp_[2]; s4 = sp_[3];
            }
            state_undiff(s1, s2, s3, s4);
            const double sv[4] = {s1, s2, s3, s4};
            const bool last = lane_ok && chunk == nchunks - 1u;
            bool tiny = false;
#pragma unroll
            for (int q = 0; q < 4; q++) tiny = tiny || (sv[q] != 0.0 && fabs(sv[q]) < 1e-200);
            early_state = (late || rem == L) && __ballot(last && tiny) == 0ull;      // (a batch tile that ends inside a chunk hands over behind its second pass)
            if (early_state) {
                if (last) {
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        sh->carry[ch][q] = (sub_done && sb + 1 >= 4 && fabs(sv[q]) < 2.2250738585072014e-308) ? 0.0 : sv[q];
                }
                __builtin_amdgcn_wave_barrier();
                if (lane == 0) __hip_atomic_store(&sh->state_ready, ti + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        SS_PROF_MARK(3);
        // ---- pass 2: true-state rerun + energy + sample peak
        float sp = 0.0f;                                // this lane's max |x| over its chunk (also steers the true-peak path)
        {
            double e = 0.0;
            uint32_t i = 0;
            // ring position of this lane's chunk: one modulo per tile (wave-uniform), then an add and a compare per sample —
            // (base + i) % ring_frames per sample and lane was a 64-bit division in every step of the second pass: 2.4 of a
            // tile's 3.8 us inside a tick (tools/probe_tick_tiles.py)
            const uint32_t rf32 = (uint32_t)p.ring_frames;
            uint32_t rpos = 0u;
            double *const ring = RING ? p.ring + (size_t)stream * p.ring_stride : nullptr;     // (wave-uniform: a scalar base)
            if (RING) {
                const uint32_t tile_rbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((fed0 + pos) % p.ring_frames));
                rpos = tile_rbase + chunk * L;
                if (rpos >= rf32) rpos -= rf32;
            }
#define SS_RING_PUT(v_) do { if (RING) { ring[(size_t)rpos * C + ch] = (v_); rpos = rpos + 1u == rf32 ? 0u : rpos + 1u; } } while (0)
            // (wave-uniform) unit gain for this tile: the build's form, unless a non-finite value is in reach of its filter — among
            // its own frames (tile_nf; a one-wave run's poisoned state shows there too, chunk 0 runs its first pass from it) or in the
            // state another wave handed over
            bool unit_tile = false;
            if (kUnitGainBuild) {
                bool state_nf = false;
                if (SPLIT) state_nf = __ballot(lane_ok && !(fabs(cv[0]) < (double)INFINITY && fabs(cv[1]) < (double)INFINITY &&
                                                            fabs(cv[2]) < (double)INFINITY && fabs(cv[3]) < (double)INFINITY)) != 0ull;
                unit_tile = !(tile_nf || state_nf);
            }
            // the build's output taps (SS_KW_LA_OUT reads kUnitGain); a unit-gain build's non-finite tile skips the look-ahead loops
            // and takes the plain step-by-step loop below — the form a partial chunk takes anyway — with the gained taps
            constexpr bool kUnitGain = kUnitGainBuild;
            const double b0 = bt0, b1 = bt1, b2 = bt2, b3 = bt3, b4 = bt4;
            if (len == L && (!kUnitGainBuild || unit_tile)) {
                // sample peak over x[0 .. L+2]: the three look-ahead samples are the next chunk's (or the
                // zeroed slack behind the tile), so including them cannot change the channel's maximum
                const float *xp = xs + 3 * C;
                const float xa = xs[0], xb1 = xs[C], xc = xs[2 * C];
                sp = fmaxf(fmaxf(fabsf(xa), fabsf(xb1)), fabsf(xc));
                SS_KW_LA_INIT((double)xa, (double)xb1, (double)xc)
                SS_KW_LA_OUT_INIT()
                double xq0 = (double)xa, xq1 = (double)xb1, xq2 = (double)xc;     // the samples the look-ahead has taken in already
                for (uint32_t bq = 0; bq < nb_full; bq++, xp += kTdBatch * C) {
                    float xb[kTdBatch];
#pragma unroll
                    for (int u = 0; u < kTdBatch; u++) xb[u] = xp[u * (int)C];
#pragma unroll
                    for (int u = 0; u < kTdBatch; u++) {
                        sp = fmaxf(sp, fabsf(xb[u]));
                        SS_KW_LA_STEP((double)xb[u]) SS_KW_LA_OUT(xq0) SS_KW_SHIFT()
                        e = fma(y_, y_, e);
                        SS_RING_PUT(y_);
                        xq0 = xq1; xq1 = xq2; xq2 = (double)xb[u];
                    }
                }
                i = nb_full * kTdBatch;
                if (i < L) {
                    const uint32_t rem = L - i;
                    float xb[kTdBatch];
#pragma unroll
                    for (int u = 0; u < kTdBatch; u++) xb[u] = xp[u * (int)C];
#pragma unroll
                    for (int u = 0; u < kTdBatch - 1; u++)
                        if ((uint32_t)u < rem) {
                            // (x[i + 3] of the last three steps belongs to the next chunk: harmless in a maximum, see above)
                            sp = fmaxf(sp, fabsf(xb[u]));
                            SS_KW_LA_STEP((double)xb[u]) SS_KW_LA_OUT(xq0) SS_KW_SHIFT()
                            e = fma(y_, y_, e);
                            SS_RING_PUT(y_);
                            xq0 = xq1; xq1 = xq2; xq2 = (double)xb[u];
                        }
                    i = L;
                }
            }
            // (the gained taps of a unit-gain build: scalar loads here, for the non-finite tile alone)
            double gb0 = bt0, gb1 = bt1, gb2 = bt2, gb3 = bt3, gb4 = bt4;
            if (kUnitGainBuild && !unit_tile) {
                const_f64_ptr bp = (const_f64_ptr)(uintptr_t)&K.b[0];
                asm volatile("" : "+s"(bp));
                gb0 = bp[0]; gb1 = bp[1]; gb2 = bp[2]; gb3 = bp[3]; gb4 = bp[4];
            }
            for (; i < len; i++) {
                const float xf = xs[i * C];
                sp = fmaxf(sp, fabsf(xf));
                SS_KW_STATE((double)xf)
                double y_;
                if (kUnitGainBuild && unit_tile) y_ = SS_KW_OUT_UNIT((double)xf);
                else y_ = fma(gb0, v0_, fma(gb4, v4, fma(gb3, v3, fma(gb2, v2, gb1 * v1))));
                SS_KW_SHIFT()
                e = fma(y_, y_, e);
                SS_RING_PUT(y_);
            }
#undef SS_RING_PUT
            if (SPLIT) {                                // the lanes' shares travel from tile to tile (same sums, same order)
                while (__hip_atomic_load(&sh->tiles_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < ti) __builtin_amdgcn_s_sleep(1);
                SS_TRACE(10);
                e_run = sh->e_lane[lane];
            }
            if (!warm) {
                if (unit_tile) {                        // (b0^2 by a scalar load at the point of use: one FMA instead of the add)
                    const_f64_ptr eg = (const_f64_ptr)(uintptr_t)&K.bu[0];
                    asm volatile("" : "+s"(eg));
                    e_run = fma(eg[0], e, e_run);
                } else e_run += e;
                sp_run = fmaxf(sp_run, sp);
            }
            if (SPLIT && RING) e_call += e;
        }
        // carry-out: exact state after the last valid sample, to the lanes of the channel (chunk 0's lane consumes it), and the
        // close of a sub-block.  Runs at the end of the tile — or, SPLIT, right behind the second pass, where the next tile's
        // wave is waiting for it.
        auto tile_carry_out = [&]() {
        if (kRowScan && CT <= 2) {
            // the source lanes are wave-uniform: v_readlane per channel instead of eight trips through the LDS crossbar
            const uint32_t lastc = nchunks - 1u;
            const uint32_t l0 = ((lastc & 3u) << 4) + (lastc >> 2) * C;     // lane of (last chunk, channel 0)
            auto rl64 = [](double v, uint32_t src) -> double {
                return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), (int)src), __builtin_amdgcn_readlane(__double2loint(v), (int)src));
            };
            const double vv[4] = {v1, v2, v3, v4};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double a = rl64(vv[q], l0);
                cv[q] = (CT == 2 && ch == 1u) ? rl64(vv[q], l0 + 1u) : a;
            }
        } else {
            const uint32_t src_lane = lane_of_chunk(nchunks - 1);
            cv[0] = __shfl(v1, src_lane, 64); cv[1] = __shfl(v2, src_lane, 64);
            cv[2] = __shfl(v3, src_lane, 64); cv[3] = __shfl(v4, src_lane, 64);
        }
        // ---- sub-block complete: deterministic tree over the lanes' energy shares (fixed shape)
        if (sub_done) {
            if (!warm) {
                double e = e_run;
                for (uint32_t d = 32; d >= 1; d >>= 1) {
                    const double o = __shfl_down(e, d * C, 64);
                    if (lane + d * C < 64u) e += o;
                }
                uint32_t lane_e = lane;
                asm volatile("" : "+v"(lane_e));
                if (lane_e < C) p.subblocks[(size_t)stream * p.sub_stride + (size_t)slot * C + lane_e] = e;
            }
            e_run = 0.0;
            // ebur128 flushes sub-normal filter state to zero at the end of every internal filter call (restated at
            // oracle/ss_oracle.c:570-571).  add_frames cuts its input where a gating block completes: at the fourth
            // 100 ms boundary after a reset and at every boundary after it (needed_frames = 4 s100, then s100).
            if (sb + 1 >= 4) {
#pragma unroll
                for (int q = 0; q < 4; q++) cv[q] = fabs(cv[q]) < 2.2250738585072014e-308 ? 0.0 : cv[q];
            }
        }
        if (SPLIT) {                                    // hand over: energy shares — and the state, unless the scan has published it
            sh->e_lane[lane] = e_run;
            if (!early_state && lane_ok && chunk == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++) sh->carry[ch][q] = cv[q];
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                if (!early_state) __hip_atomic_store(&sh->state_ready, ti + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_store(&sh->tiles_done, ti + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        };
        if (SPLIT || kTpValu || kTpValu2 || (kTpPlain && CT != 0)) tile_carry_out();   // (the true peak below wants the registers the end states stand in)
        SS_PROF_MARK(4);
        // ---- true peak on the matrix pipe (not during the run-in)
        // The crate's own loop (ebur128 0.1.10 interp: acc += x[n - t] c_f[t], t ascending, product and sum rounded separately;
        // `if v > max` ignores a NaN like fmaxf does; restated at oracle/ss_oracle.c:563-582) over frames [first_frame, + nfr), one
        // output sample per lane and step.  Rare by definition (tiles with a non-finite sample in reach, slivers of a tile):
        // rolled loops, the taps through a per-lane pointer the compiler cannot see through — nothing of it hoisted into the
        // tile loop's registers, which the hot path has none to spare of.
        auto tp_exact_range = [&](uint32_t first_frame, uint32_t nfr) {
            uint32_t lane_x = lane;
            asm volatile("" : "+v"(lane_x));
            const float *tapv = &K.tp[0][0] + (lane_x & 0u);
            const uint32_t nx = nfr * C;
            const float *x0 = tile + (size_t)first_frame * C;
#pragma nounroll
            for (uint32_t idx = lane_x; idx < nx; idx += 64u) {
                const float *xq = x0 + idx;
                float m = 0.0f;
#pragma nounroll
                for (int f = 0; f < Cfg::NPH; f++) {
                    float acc = 0.0f;
#pragma nounroll
                    for (int t = 0; t < Cfg::HIST; t++) acc = tp_mul_then_add(acc, xq[-t * (int)C], tapv[f * kTpHistMax + t]);
                    m = fmaxf(m, fabsf(acc));
                }
                atomicMax(&tpk[idx % C], __float_as_uint(m));
            }
        };
        bool halo_done = false;
        const uint32_t tp_now_bits = kTpPlanar ? wave_max_nonneg_bits(sp) : 0u;      // this tile's sample peak, wave-uniform
        if (FACTOR != 0 && !warm) {
            // f32 product (bit-exact fmaf chain) over `nfr` frames starting at float offset `base_f` of the tile
            auto tp_f32_range = [&](uint32_t first_frame, uint32_t nfr) {
                const float *t0 = tile + (size_t)first_frame * C;
                const uint32_t nblk = (nfr + Cfg::BLK - 1) / Cfg::BLK;     // blocks per channel
                const uint32_t ncol = nblk * C;
                const uint32_t ngroups = (ncol + 15) >> 4;
                constexpr int GS = 16 * Cfg::BLK;                          // floats per group (16 columns x BLK outputs)
                const uint32_t nfull = nfr / (tp_bpg * Cfg::BLK);          // groups whose every output lies inside the range
                uint32_t gi = 0;
                if (kAfragPerTile) {
                    uint32_t lane_a = lane;
                    asm volatile("" : "+v"(lane_a));
                    build_afrag(lane_a, afrag, tp_lane_off);
                }
                const float *bp = t0 + tp_lane_off;
                for (; gi + 2 <= nfull; gi += 2, bp += 2 * GS) {
                    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                    float bv0[Cfg::KSTEPS], bv1[Cfg::KSTEPS];
#pragma unroll
                    for (int s = 0; s < Cfg::KSTEPS; s++) { bv0[s] = bp[4 * s * (int)C]; bv1[s] = bp[GS + 4 * s * (int)C]; }
#pragma unroll
                    for (int s = 0; s < Cfg::KSTEPS; s++) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[s], bv0[s], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[s], bv1[s], acc1, 0, 0, 0);
                    }
                    // max |.| of the eight results: v_max3 with |abs| source modifiers, four instructions (through the fmaxf / fabsf
                    // builtins the compiler quiets every operand first: fourteen — 120 VALU instructions per tile, a tenth of the
                    // kernel's).  ONE asm statement naming both accumulators (it cannot move in front of an MFMA), the wait states a
                    // VALU read needs behind an 8-pass MFMA write inside the string (inline asm hides the hazard from the compiler),
                    // the accumulator of the LAST MFMA read last.  (The products are finite here: a tile with a non-finite sample
                    // in reach takes the exact path below.)
                    asm volatile("s_nop 10\n\t"
                                 "v_max3_f32 %0, %0, |%1|, |%2|\n\t"
                                 "v_max3_f32 %0, %0, |%3|, |%4|\n\t"
                                 "v_max3_f32 %0, %0, |%5|, |%6|\n\t"
                                 "v_max3_f32 %0, %0, |%7|, |%8|"
                                 : "+v"(tp_run)
                                 : "v"(acc0[0]), "v"(acc0[1]), "v"(acc0[2]), "v"(acc0[3]), "v"(acc1[0]), "v"(acc1[1]), "v"(acc1[2]), "v"(acc1[3]));
                }
                // (rare paths below rebuild what they need from an opaque copy of the lane id: hoisted out of the tile loop their
                // lane-dependent constants were what the four-waves-per-SIMD build kept in scratch)
                for (; gi < ngroups; gi++, bp += GS) {                     // odd full group and the masked tail
                    uint32_t lane_t = lane;
                    asm volatile("" : "+v"(lane_t));
                    const int kq = (int)(lane_t >> 4), mrow = (int)(lane_t & 15u);
                    const uint32_t bi = gi * tp_bpg + (uint32_t)mrow / C;
                    const bool col_ok = (gi * 16 + (uint32_t)mrow) < ncol;
                    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < Cfg::KSTEPS; s++)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[s], col_ok ? bp[4 * s * (int)C] : 0.0f, acc, 0, 0, 0);
#pragma unroll
                    for (int reg = 0; reg < 4; reg++) {
                        const int row = 4 * kq + reg;
                        const bool ok = col_ok && (bi * Cfg::BLK + (uint32_t)(row % Cfg::BLK)) < nfr;
                        tp_run = fmaxf(tp_run, ok ? fabsf(acc[reg]) : 0.0f);
                    }
                }
            };
            if (tile_nf || halo_bad) {
                // (a non-finite sample in reach: not through the matrix pipe — the crate's own loop, behind the tile's carry-out below)
            } else if (kTpValu && p.tp_f32) {
                // ---- 2 / 6 / 8 channels, factor 4, the reference's f32 width: the interpolator on the packed-f32 VALU.  A banded-Toeplitz
                // product on 16x16x4 tiles spends 51 MACs per sample on the 36 an output needs (15 of 16 rows, 12 of 16 K), holds the
                // SIMD for 3072 clocks per 960-frame stereo tile and lets no other wave's VALU work issue meanwhile; here a lane takes
                // FIFTEEN consecutive frames of BOTH channels of a pair — a frame of interleaved stereo is an aligned register pair
                // (L, R), which is exactly a packed operand — reads its 26-frame window once (ds_read_b64, lane stride 30 dwords:
                // conflict-free) and runs the 3 phases x 12 taps folded about their centre (SS_TP_VALU_FOLD1) as 30 packed
                // instructions per frame with the taps broadcast from SGPR pairs through op_sel: 450 packed (5.2 issue clocks each at
                // four waves per SIMD) + 60 plain per tile, 2500 clocks — the unfolded 540 FMAs measured -9 % kernel time against the
                // matrix pipe (profiles/r06_ab_tp_packed_valu.txt), the fold -5 % more.  The tile's frames are dealt
                // 15 to a lane; the last lane of a tile that is no multiple of 15 takes the tile's LAST fifteen frames (its first ones
                // a second time: a maximum does not mind), and a tile of fewer than fifteen frames takes the crate's loop.
                if (seg < kTpValuFrames) tp_exact_range(0u, seg);
                else {
                    uint32_t lane_v = lane;
                    asm volatile("" : "+v"(lane_v));
                    const_f64_ptr cp = (const_f64_ptr)(uintptr_t)&K.tp_fold[0][0];   // folded tap pairs (f[2 m], f[2 m + 1]): scalar loads
                    asm volatile("" : "+s"(cp));
                    double tf[9];
#pragma unroll
                    for (int m = 0; m < 9; m++) tf[m] = cp[m];
                    // (more channels: a lane takes fifteen frames of ONE pair of adjacent channels, the pairs of a run of frames side
                    // by side in neighbouring lanes — eight channels: lane stride 120 dwords per run, 2 per pair: conflict-free too)
                    const uint32_t nl = (seg + (uint32_t)kTpValuFrames - 1u) / (uint32_t)kTpValuFrames * kTpPairs;
                    float mL = 0.0f, mR = 0.0f;
                    for (uint32_t l0 = 0; l0 < nl; l0 += 64u) {
                        const uint32_t li = l0 + lane_v;
                        if (li < nl) {
                            const uint32_t run = li / kTpPairs, pair = li - run * kTpPairs;
                            uint32_t first = run * (uint32_t)kTpValuFrames;
                            first = first + (uint32_t)kTpValuFrames <= seg ? first : seg - (uint32_t)kTpValuFrames;
                            const v2f_td *wp = reinterpret_cast<const v2f_td *>(tile) + ((int)first - 11) * (int)kTpPairs + (int)pair;
                            // (the window slides through the registers a frame at a time: thirteen frames live, not twenty-six —
                            // the four-waves build has 128 registers and the next tile's prefetch is in 32 of them)
                            v2f_td W[kTpValuFrames + 11];                             // frames first - 11 .. first + 14
#pragma unroll
                            for (int j = 0; j < 13; j++) W[j] = wp[j * (int)kTpPairs];
#pragma unroll
                            for (int j = 0; j < kTpValuFrames; j++) {                 // (L, R) at frame first + j
#if defined(__HIP_DEVICE_COMPILE__)
                                __builtin_amdgcn_sched_barrier(0);
#endif
                                {
                                    v2f_td sv, yv, dv;
                                    SS_TP_VALU_FOLD1(sv, yv, dv, W, j, tf);
                                    SS_TP_VALU_FOLD1_MAX(mL, mR, sv, yv, dv);
                                }
#if defined(__HIP_DEVICE_COMPILE__)
                                __builtin_amdgcn_sched_barrier(0);
#endif
                                if (j + 13 < kTpValuFrames + 11) W[j + 13] = wp[(j + 13) * (int)kTpPairs];    // (for frame j + 2)
                            }
                            if (CT != 2) {                                           // (a lane's pair changes from round to round)
                                atomicMax(&tpk[2u * pair], __float_as_uint(mL));
                                atomicMax(&tpk[2u * pair + 1u], __float_as_uint(mR));
                                mL = 0.0f; mR = 0.0f;
                            }
                        }
                    }
                    // stereo: a lane's two maxima fold into the ONE running value the other forms keep (lane -> channel lane & 1): each
                    // pair of neighbours shares both (v_max with a DPP operand, the two wait states a DPP read needs behind a VALU write)
                    if (CT == 2) {
                        asm volatile("s_nop 1\n\t"
                                     "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                     "v_max_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
                                     : "+v"(mL), "+v"(mR));
                        tp_run = fmaxf(tp_run, (lane_v & 1u) ? mR : mL);
                    }
                }
            } else if (kTpValu2) {
                if (seg < kTpValuFrames) tp_exact_range(0u, seg);
                else {
                    uint32_t lane_v = lane;
                    asm volatile("" : "+v"(lane_v));
                    const uint32_t hsel = lane_v & 1u;                     // which half of the branch this lane runs: taps 12 hsel .. + 11
                    v2f_td tv[6];                                          // (c[12 h + 2 m], c[12 h + 2 m + 1])
                    {
                        const v2f_td *tp2 = reinterpret_cast<const v2f_td *>(&K.tp[0][0]) + 6u * hsel;
#pragma unroll
                        for (int m = 0; m < 6; m++) tv[m] = tp2[m];
                    }
                    const uint32_t nl = (seg + (uint32_t)kTpValuFrames - 1u) / (uint32_t)kTpValuFrames * kTpPairs * 2u;
                    float mL = 0.0f, mR = 0.0f;
                    for (uint32_t l0 = 0; l0 < nl; l0 += 64u) {
                        const uint32_t li = l0 + lane_v;
                        if (li < nl) {                                     // (nl is even: a lane and its neighbour are in or out together)
                            const uint32_t unit = li >> 1, run = unit / kTpPairs, pair = unit - run * kTpPairs;
                            uint32_t first = run * (uint32_t)kTpValuFrames;
                            first = first + (uint32_t)kTpValuFrames <= seg ? first : seg - (uint32_t)kTpValuFrames;
                            // this half's window: x[n - 12 h - k], k = 0 .. 11 — the first half's, twelve frames further back
                            const v2f_td *wp = reinterpret_cast<const v2f_td *>(tile) + ((int)first - 11 - 12 * (int)hsel) * (int)kTpPairs + (int)pair;
                            v2f_td W[kTpValuFrames + 11];
#pragma unroll
                            for (int j = 0; j < 14; j++) W[j] = wp[j * (int)kTpPairs];
#pragma unroll
                            for (int g = 0; g < kTpValuFrames / 3; g++) {
#if defined(__HIP_DEVICE_COMPILE__)
                                __builtin_amdgcn_sched_barrier(0);
#endif
                                {
                                    v2f_td a[3];
                                    SS_TP_VALU_PHASE3V(a[0], a[1], a[2], W, g, tv);
                                    // the other half's sums from the neighbouring lane (both lanes end up with the whole output), then
                                    // the maxima (two wait states in front of a DPP read of a VALU result)
                                    asm("s_nop 1\n\t"
                                        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                        "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                        "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                        "v_add_f32_dpp %3, %3, %3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                        "v_add_f32_dpp %4, %4, %4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                        "v_add_f32_dpp %5, %5, %5 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                                        "v_max3_f32 %6, %6, |%0|, |%2|\n\tv_max3_f32 %7, %7, |%1|, |%3|\n\t"
                                        "v_max_f32_e64 %6, %6, |%4|\n\tv_max_f32_e64 %7, %7, |%5|"
                                        : "+v"(a[0].x), "+v"(a[0].y), "+v"(a[1].x), "+v"(a[1].y), "+v"(a[2].x), "+v"(a[2].y), "+v"(mL), "+v"(mR));
                                }
#if defined(__HIP_DEVICE_COMPILE__)
                                __builtin_amdgcn_sched_barrier(0);
#endif
                                if (g + 1 < kTpValuFrames / 3) {
#pragma unroll
                                    for (int j = 14 + 3 * g; j < 17 + 3 * g; j++) W[j] = wp[j * (int)kTpPairs];
                                }
                            }
                            if (CT != 2) {
                                atomicMax(&tpk[2u * pair], __float_as_uint(mL));
                                atomicMax(&tpk[2u * pair + 1u], __float_as_uint(mR));
                                mL = 0.0f; mR = 0.0f;
                            }
                        }
                    }
                    if (CT == 2) {
                        // (stereo: lanes 4 m .. 4 m + 3 are (run, half) x 2 with both channels each; the one running value per lane keeps
                        // channel lane & 1 as everywhere else — a lane and its neighbour hold the same maxima already)
                        tp_run = fmaxf(tp_run, (lane_v & 1u) ? mR : mL);
                    }
                }
            } else if (kTpPlain && (!tp_fixed || CT != 0)) {
                // (a general-count build with 4 or 16 channels: the matrix-pipe forms below)
                if (seg < kTpValuFrames) tp_exact_range(0u, seg);
                else {
                    uint32_t lane_v = lane;
                    asm volatile("" : "+v"(lane_v));
                    // scalar loads: factor 4 the three branches folded (18 taps), factor 2 its one branch of 24
                    const_f32_ptr tapp = (const_f32_ptr)(uintptr_t)(FACTOR == 4 ? &K.tp_fold[0][0] : &K.tp[0][0]);
                    asm volatile("" : "+s"(tapp));
                    constexpr int NT = Cfg::HIST;                                      // window reach: 12 or 24 frames
                    constexpr int NTAPS = FACTOR == 4 ? 18 : NT;
                    float tcf[NTAPS];
#pragma unroll
                    for (int t = 0; t < NTAPS; t++) tcf[t] = tapp[t];
                    const uint32_t nl = (seg + (uint32_t)kTpValuFrames - 1u) / (uint32_t)kTpValuFrames * C;
                    float mC = 0.0f;
                    for (uint32_t l0 = 0; l0 < nl; l0 += 64u) {
                        const uint32_t li = l0 + lane_v;
                        if (li < nl) {
                            const uint32_t run = li / C, cch = li - run * C;
                            uint32_t first = run * (uint32_t)kTpValuFrames;
                            first = first + (uint32_t)kTpValuFrames <= seg ? first : seg - (uint32_t)kTpValuFrames;
                            const float *wp = tile + ((int)first - (NT - 1)) * (int)C + (int)cch;
                            float W[kTpValuFrames + NT - 1];                           // frames first - (NT - 1) .. first + 14 of the channel
#pragma unroll
                            for (int j = 0; j < NT + 2; j++) W[j] = wp[j * (int)C];
#pragma unroll
                            for (int g = 0; g < kTpValuFrames / 3; g++) {
#if defined(__HIP_DEVICE_COMPILE__)
                                __builtin_amdgcn_sched_barrier(0);
#endif
                                if constexpr (FACTOR == 4) SS_TP_VALU_FOLD3_PLAIN(mC, W, g, tcf);
                                else {
                                    float a0, a1, a2;
                                    SS_TP_VALU_PLAIN3(a0, a1, a2, W + 12, g, tcf);              // taps 0 .. 11 over frames n - 11 .. n
                                    SS_TP_VALU_PLAIN3_ACC(a0, a1, a2, W, g, tcf + 12);          // taps 12 .. 23 over frames n - 23 .. n - 12
                                    asm("v_max3_f32 %0, %0, |%1|, |%2|\n\tv_max_f32_e64 %0, %0, |%3|" : "+v"(mC) : "v"(a0), "v"(a1), "v"(a2));
                                }
#if defined(__HIP_DEVICE_COMPILE__)
                                __builtin_amdgcn_sched_barrier(0);
#endif
                                if (g + 1 < kTpValuFrames / 3) {
#pragma unroll
                                    for (int j = NT + 2 + 3 * g; j < NT + 5 + 3 * g; j++) W[j] = wp[j * (int)C];
                                }
                            }
                            atomicMax(&tpk[cch], __float_as_uint(mC));                // (a lane's channel changes from round to round)
                            mC = 0.0f;
                        }
                    }
                }
            } else if (tp_fixed) {
                // planar f16 product for the whole groups of the tile, f32 product for what is left (and for tiles
                // whose peak, or whose predecessor's, is not finite)
                uint32_t nplanar = 0;                                      // groups (16 columns x 4 outputs) on the f16 path
                uint32_t scale_bits = 0, inv_bits = 0;
                if (kTpPlanar) {
                    const uint32_t pkb = tp_now_bits > tp_prev_bits ? tp_now_bits : tp_prev_bits;
                    const uint32_t e = pkb >> 23;                          // biased exponent of the peak (sign is 0)
                    nplanar = (seg >> 2) / tp_bpg;
                    if (e == 255u || C > 8u || p.tp_f32) nplanar = 0;      // (16 channels: round 0 would not hold the 12 history frames)
                    // scale = 2^(14 - floor(log2 peak)): the scaled peak lies in [2^14, 2^15), inside the f16 range
                    uint32_t sf = 268u - e;                                // biased exponent of the scale
                    sf = sf > 254u ? 254u : sf;
                    scale_bits = sf << 23;
                    inv_bits = (254u - sf) << 23;                          // exact reciprocal (0 when the peak is below 2^-113)
                }
                const uint32_t f0 = nplanar * tp_bpg * 4;                  // frames covered by the planar path
                if (f0 < seg) { if (kTpValu) tp_exact_range(f0, seg - f0); else tp_f32_range(f0, seg - f0); }
                if (nplanar) {
                    const float scale = __uint_as_float(scale_bits);
                    const uint32_t ps = f0 + 12;                           // converted frames: [-12, f0), even
                    const uint32_t FB = 64u / C, lb = 31u - (uint32_t)__clz((int)FB);    // frames per block (a power of two >= 4)
                    // a conversion round is two blocks: lane -> (block of the round, pair of the block) = frames 2 fpl, 2 fpl + 1 of channel cc
                    uint32_t lane_h = lane;                     // (everything lane-dependent of this path rebuilt per tile from an opaque copy:
                    asm volatile("" : "+v"(lane_h));            //  hoisted, its addresses were spilled around the tile loop in the four-waves builds)
                    const uint32_t half = lane_h >> 5, pr = lane_h & 31u, fpl = pr / C, cc = pr - fpl * C;
                    // (1) the 12 frames in front of the tile live in the halo, which (2) is about to replace
                    float s0 = 0.0f, s1 = 0.0f;
                    {
                        const uint32_t q = lane_h < 6u * C ? lane_h : 0u, qf = q / C, qc = q - qf * C;      // pair q: frames -12 + 2 qf, channel qc
                        const float *xp = tile + ((int)(2 * qf) - 12) * (int)C + (int)qc;
                        s0 = xp[0]; s1 = xp[C];
                    }
                    __builtin_amdgcn_wave_barrier();
                    // (2) the next tile's halo leaves the f32 tile before it is overwritten
                    {
                        const uint32_t hn = halo_frames * C;
                        float *dst = tile - hn;
                        const float *srcp = dst + (size_t)seg * C;
                        for (uint32_t j = lane; j < hn; j += 64u) {
                            const float v = srcp[j];
                            __builtin_amdgcn_wave_barrier();
                            dst[j] = v;
                        }
                        halo_done = true;
                    }
                    __builtin_amdgcn_wave_barrier();
                    // (3) convert in place, rounds (two blocks each: 128 floats in, 128 dwords out) from the top down, four
                    // rounds per batch: all reads of a batch, then its writes.  Lane addresses step by 512 bytes per round.
                    // The top block may run past the converted range into the slack (sized for it); nothing reads that.
                    const uint32_t nblocks = (ps + FB - 1) >> lb;
                    const int nround = (int)((nblocks + 1u) >> 1);
                    const bool top_ok = 2u * (uint32_t)(nround - 1) + half < nblocks;     // odd block count: the top round's upper block does not exist
                    const float *rbase = tile + ((int)(half * FB + 2u * fpl) - 12) * (int)C + (int)cc;    // round 0; + 128 floats per round
                    uint32_t *wbase = reinterpret_cast<uint32_t *>(tile) + half * 64u + cc * (FB >> 1) + fpl;   // hi pair; lo: + 32
                    const bool saver = half * FB + 2u * fpl < 12u;         // this lane saved its round-0 pair from the old halo (lane < 6 C)
                    // (hi, hi) = f16(s x0), f16(s x1);  (lo, lo) = f16(s x - hi): four v_fma_mix
                    auto split2 = [&](float xa, float xb, uint32_t &hh, uint32_t &ll) {
                        asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hh) : "v"(xa), "s"(scale));
                        asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hh) : "v"(xb), "s"(scale));
                        asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(ll) : "v"(xa), "s"(scale), "v"(hh));
                        asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(ll) : "v"(xb), "s"(scale), "v"(hh));
                    };
                    // The top round (its upper block may not exist) and round 0 (whose first pairs come from the saved halo)
                    // are peeled off, so the rounds in between run without predicates or selects.
                    int rd = nround - 1;
                    const float *rp = rbase + rd * 128;
                    uint32_t *wp = wbase + rd * 128;
                    if (rd > 0) {
                        uint32_t hh, ll;
                        split2(rp[0], rp[(int)C], hh, ll);
                        if (top_ok) { wp[0] = hh; wp[32] = ll; }
                        rd--; rp -= 128; wp -= 128;
                        __builtin_amdgcn_wave_barrier();
                    }
                    for (; rd >= 4; rd -= 4, rp -= 512, wp -= 512) {        // rounds rd .. rd - 3, all >= 1
                        float x0[4], x1[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) { x0[u] = rp[-128 * u]; x1[u] = rp[-128 * u + (int)C]; }
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            uint32_t hh, ll;
                            split2(x0[u], x1[u], hh, ll);
                            wp[-128 * u] = hh;
                            wp[-128 * u + 32] = ll;
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                    for (; rd >= 1; rd--, rp -= 128, wp -= 128) {           // up to three rounds left above round 0
                        uint32_t hh, ll;
                        split2(rp[0], rp[(int)C], hh, ll);
                        wp[0] = hh; wp[32] = ll;
                        __builtin_amdgcn_wave_barrier();
                    }
                    {                                                       // round 0
                        uint32_t hh, ll;
                        split2(saver ? s0 : rbase[0], saver ? s1 : rbase[(int)C], hh, ll);
                        if (nround > 1 || top_ok) { wbase[0] = hh; wbase[32] = ll; }
                        __builtin_amdgcn_wave_barrier();
                    }
                    // (4) column (channel tp_c, block of outputs b = 16/C g + mrow / C) reads halves 4 kq .. + 4 of its window
                    // [4 b, 4 b + 16) of converted frames from the hi plane and from the lo plane (aligned 8-byte pieces)
                    const char *tb = reinterpret_cast<const char *>(tile);
                    const uint32_t mrow_p = lane_h & 15u, kq_p = lane_h >> 4, tp_c_p = mrow_p % C;      // (this lane's column role, per tile)
                    auto plane_addr = [&](uint32_t j, uint32_t lo) -> const char * {
                        return tb + ((j >> lb) << 8) + (lo << 7) + ((tp_c_p * FB + (j & (FB - 1u))) << 1);
                    };
                    const uint32_t jb = 4u * (mrow_p / C);
                    auto ld4 = [](const char *q, int off) -> halfx4 { return __builtin_bit_cast(halfx4, *reinterpret_cast<const uint2 *>(q + off)); };
                    SS_PROF_MARK(5);
                    float m16 = 0.0f;
                    {
                        // three K = 16 products per group (hi and lo planes at halves 4 kq .. + 4), four groups per iteration:
                        // four independent accumulator chains, and the next iteration's operands are read before this one's MFMAs
                        const char *ph = plane_addr(jb + 4u * kq_p, 0);                  // lo plane: + 128 bytes; next group: + 256
                        auto absmax4 = [](float m, const floatx4 &a) {
                            return fmaxf(fmaxf(fmaxf(m, fabsf(a[0])), fabsf(a[1])), fmaxf(fabsf(a[2]), fabsf(a[3])));
                        };
                        // groups per iteration of this loop: 2 in the four-waves-per-SIMD build, 4 in the three-waves build
                        constexpr int NG = (WPS >= 4) ? 2 : 4;              // independent accumulator chains (2 or 4)
                        constexpr int NGS = NG == 4 ? 2 : 1;
                        const uint32_t nquad = nplanar >> NGS;
                        if (nquad) {
                            halfx4 h[NG], l[NG];
#pragma unroll
                            for (int g = 0; g < NG; g++) { h[g] = ld4(ph, 256 * g); l[g] = ld4(ph, 256 * g + 128); }
                            for (uint32_t it = 0; it < nquad; it++) {
                                ph += (it + 1 < nquad) ? 256 * NG : 0;     // the last iteration re-reads its own operands: nothing past the planes
                                halfx4 hn[NG], ln[NG];
#pragma unroll
                                for (int g = 0; g < NG; g++) { hn[g] = ld4(ph, 256 * g); ln[g] = ld4(ph, 256 * g + 128); }
                                floatx4 acc[NG];
#pragma unroll
                                for (int g = 0; g < NG; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x16f16(a16_hi, h[g], floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                                for (int g = 0; g < NG; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x16f16(a16_hi, l[g], acc[g], 0, 0, 0);
#pragma unroll
                                for (int g = 0; g < NG; g++) acc[g] = __builtin_amdgcn_mfma_f32_16x16x16f16(a16_lo, h[g], acc[g], 0, 0, 0);
                                // max |.| of the results: v_max3 with |abs| source modifiers, two instructions per group (through the
                                // fmaxf / fabsf builtins the compiler quiets every operand first: more than twice as many).  ONE asm
                                // statement naming every accumulator (so that it cannot be scheduled in front of any of the MFMAs), with
                                // the wait states a VALU read needs behind an MFMA write inside the string — inline asm hides the hazard
                                // from the compiler: twelve states between the LAST MFMA and the v_max3 that reads its result (the last
                                // accumulator is read by the last two v_max3).
                                if (NG == 4)
                                    asm volatile("s_nop 5\n\t"
                                                 "v_max3_f32 %0, %0, |%1|, |%2|\n\t"
                                                 "v_max3_f32 %0, %0, |%3|, |%4|\n\t"
                                                 "v_max3_f32 %0, %0, |%5|, |%6|\n\t"
                                                 "v_max3_f32 %0, %0, |%7|, |%8|\n\t"
                                                 "v_max3_f32 %0, %0, |%9|, |%10|\n\t"
                                                 "v_max3_f32 %0, %0, |%11|, |%12|\n\t"
                                                 "v_max3_f32 %0, %0, |%13|, |%14|\n\t"
                                                 "v_max3_f32 %0, %0, |%15|, |%16|"
                                                 : "+v"(m16)
                                                 : "v"(acc[0][0]), "v"(acc[0][1]), "v"(acc[0][2]), "v"(acc[0][3]),
                                                   "v"(acc[1][0]), "v"(acc[1][1]), "v"(acc[1][2]), "v"(acc[1][3]),
                                                   "v"(acc[NG - 2][0]), "v"(acc[NG - 2][1]), "v"(acc[NG - 2][2]), "v"(acc[NG - 2][3]),
                                                   "v"(acc[NG - 1][0]), "v"(acc[NG - 1][1]), "v"(acc[NG - 1][2]), "v"(acc[NG - 1][3]));
                                else
                                    asm volatile("s_nop 10\n\t"
                                                 "v_max3_f32 %0, %0, |%1|, |%2|\n\t"
                                                 "v_max3_f32 %0, %0, |%3|, |%4|\n\t"
                                                 "v_max3_f32 %0, %0, |%5|, |%6|\n\t"
                                                 "v_max3_f32 %0, %0, |%7|, |%8|"
                                                 : "+v"(m16)
                                                 : "v"(acc[0][0]), "v"(acc[0][1]), "v"(acc[0][2]), "v"(acc[0][3]),
                                                   "v"(acc[NG - 1][0]), "v"(acc[NG - 1][1]), "v"(acc[NG - 1][2]), "v"(acc[NG - 1][3]));
#pragma unroll
                                for (int g = 0; g < NG; g++) { h[g] = hn[g]; l[g] = ln[g]; }
                            }
                            ph += 256 * NG;
                        }
                        for (uint32_t g = nquad << NGS; g < nplanar; g++, ph += 256) {    // up to NG - 1 groups left
                            const halfx4 h0 = ld4(ph, 0), l0 = ld4(ph, 128);
                            floatx4 acc0 = {0.f, 0.f, 0.f, 0.f};
                            acc0 = __builtin_amdgcn_mfma_f32_16x16x16f16(a16_hi, h0, acc0, 0, 0, 0);
                            acc0 = __builtin_amdgcn_mfma_f32_16x16x16f16(a16_hi, l0, acc0, 0, 0, 0);
                            acc0 = __builtin_amdgcn_mfma_f32_16x16x16f16(a16_lo, h0, acc0, 0, 0, 0);
                            m16 = absmax4(m16, acc0);
                        }
                    }
                    tp_run = fmaxf(tp_run, m16 * __uint_as_float(inv_bits));
                }
            } else {
                // channel counts that do not divide 16 (5.1 = 6 channels, 3, 5, 7 ...): channel-major groups — the 16
                // columns of a group are 16 consecutive blocks of ONE channel, so a lane's running maximum belongs to
                // that channel and one LDS atomic per channel and tile closes it (it was one per group)
                const uint32_t nblk = (seg + Cfg::BLK - 1) / Cfg::BLK;
                const uint32_t gpc = (nblk + 15) >> 4;                  // groups per channel
                uint32_t lane_t = lane;                                  // (the column roles rebuilt from an opaque copy of the lane id, as in the
                asm volatile("" : "+v"(lane_t));                         //  rare paths above: nothing of them held across the tile loop)
                const int kq = (int)(lane_t >> 4), mrow = (int)(lane_t & 15u);
                for (uint32_t c = 0; c < C; c++) {
                    float m = 0.0f;
                    for (uint32_t gi = 0; gi < gpc; gi++) {
                        const uint32_t bi = gi * 16 + (uint32_t)mrow;
                        const bool col_ok = bi < nblk;
                        const float *bp = tile + ((int)(bi * Cfg::BLK) - (Cfg::HIST - 1) + kq) * (int)C + (int)c;
                        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int s = 0; s < Cfg::KSTEPS; s++)
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[s], col_ok ? bp[4 * s * (int)C] : 0.0f, acc, 0, 0, 0);
#pragma unroll
                        for (int reg = 0; reg < 4; reg++) {
                            const int row = 4 * kq + reg;
                            const bool ok = col_ok && (bi * Cfg::BLK + (uint32_t)(row % Cfg::BLK)) < seg;
                            m = fmaxf(m, ok ? fabsf(acc[reg]) : 0.0f);
                        }
                    }
                    atomicMax(&tpk[c], __float_as_uint(m));
                }
            }
        }
        SS_PROF_MARK(6);
        if (kTpPlanar) tp_prev_bits = seg >= 12u ? tp_now_bits : (tp_now_bits > tp_prev_bits ? tp_now_bits : tp_prev_bits);

        if (!SPLIT && !kTpValu && !kTpValu2 && !(kTpPlain && CT != 0)) tile_carry_out();
        if (FACTOR != 0 && !warm && (tile_nf || halo_bad)) {
            // A tile with a NaN or an infinity among its frames or within the interpolator's reach in front of it does not go
            // through the matrix pipe (nor through the packed form): a banded product multiplies the out-of-band samples of a column's
            // window by zero, and 0 x NaN (0 x Inf) would take the column's other outputs with it, where the crate loses exactly the
            // HIST outputs per phase whose taps touch the sample.  The crate's own loop instead.  Rare by definition: no speed claim.
            tp_exact_range(0u, seg);
        }
        if (!SPLIT && FACTOR != 0) halo_bad = tile_nf || (seg < (uint32_t)kTpHistMax && halo_bad);     // what the next tile's first windows reach back into
        // ---- new halo: the halo_frames frames before the tile end (a contiguous copy; when the tile
        // is shorter than the halo the source reaches into the old halo).  Ascending order is safe:
        // the source of element j sits seg*C floats above its destination, beyond anything written so far.
        if (!halo_done) {
            const uint32_t hn = halo_frames * C;
            float *dst = tile - hn;
            const float *srcp = dst + (size_t)seg * C;
            for (uint32_t j = lane; j < hn; j += 64u) {
                const float v = srcp[j];
                __builtin_amdgcn_wave_barrier();
                dst[j] = v;
            }
        }
        }                                               // (this wave's tile)
        if (sub_done) {
            sb++;
            slot = slot + 1u == p.sub_cap ? 0u : slot + 1u;
        }
        pos = npos;
        off = noff;
        toff = ntoff;
        seg = nseg_frames;
        ti++;
        SS_PROF_MARK(7);
    } while (seg != 0);
    SS_PROF_END;

    fold_results(ti);
#undef SS_TILE_FRAMES
#undef SS_PREFETCH
