// ss_fft_dev.h: device-side pieces of the spectrum kernels that more than one translation unit compiles — the packed-f32 complex
// arithmetic, the register-resident 16-point DFT, and the one-window N = 16384 transform (k_fft16k of ss_fft.hip; the tick
// kernel of ss_time_domain.hip runs it in the workgroups beside the loudness chain's).
#pragma once
#include "ss_kernels.h"

namespace ssk {

// ============================================================================
//  small complex helpers (f32)
// ============================================================================
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
// a * (c - i s)
__device__ __forceinline__ float2 cmul_cs(float2 a, float c, float s) { return make_float2(a.x * c + a.y * s, a.y * c - a.x * s); }
// a * (-i)
__device__ __forceinline__ float2 cmul_mi(float2 a) { return make_float2(a.y, -a.x); }

// ---- packed-f32 complex arithmetic -------------------------------------------------------------
// A complex number lives in an even-aligned VGPR pair (re, im) and is processed with VOP3P packed
// f32 instructions, two flops per lane per instruction.  Measured on gfx950 (tools/ubench3.hip):
// v_pk_add_f32 issues in 5.7 cycles per wave-instruction at 2 waves/SIMD against 3.9 for v_add_f32,
// i.e. 27 % fewer issue cycles per complex add.  The swizzles a radix-4 butterfly needs (multiply by
// -i / +i, complex multiply) are expressed with op_sel / neg modifiers, which the compiler's SLP
// packer does not find (it pays ~30 % v_mov to pair registers instead — hence -fno-slp-vectorize).
typedef float v2f __attribute__((ext_vector_type(2)));
// one ds_read_b64 (see kRowB): a volatile load in the LDS address space is neither merged with its neighbours nor widened
__device__ __forceinline__ v2f lds_ld64(const v2f *p)
{
    return *(const volatile __attribute__((address_space(3))) v2f *)p;
}
// a - i b = (a.x + b.y, a.y - b.x)
__device__ __forceinline__ v2f pk_sub_ib(v2f a, v2f b)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a + i b = (a.x - b.y, a.y + b.x)
__device__ __forceinline__ v2f pk_add_ib(v2f a, v2f b)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a * w (complex): m = (a.y w.y, a.y w.x); r = (a.x w.x - m.x, a.x w.y + m.y)
// (ONE asm statement for the dependent pair: behind every asm statement whose output the next VALU instruction reads, hipcc
// pads an s_nop — written as two statements a complex multiply carried two of them, eighty issue slots per window in
// k_fft4096_ms1; the hardware interlocks a VALU result read by the next VALU instruction by itself)
__device__ __forceinline__ v2f pk_cmul(v2f a, v2f w)
{
    v2f m, r;
    asm("v_pk_mul_f32 %1, %2, %3 op_sel:[1,1] op_sel_hi:[1,0]\n\t"
        "v_pk_fma_f32 %0, %2, %3, %1 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,1] neg_hi:[0,0,0]"
        : "=v"(r), "=&v"(m) : "v"(a), "v"(w));
    return r;
}
// (a.x + a.y, a.y - a.x) = a - i a      [times R gives a * W16^2]
__device__ __forceinline__ v2f pk_w2pre(v2f a) { return pk_sub_ib(a, a); }
// (a.y - a.x, -(a.x + a.y))             [times R gives a * W16^6]
__device__ __forceinline__ v2f pk_w6pre(v2f a)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[1,1]" : "=v"(r) : "v"(a));
    return r;
}
// a * w.lo (S = 0) or a * w.hi (S = 1) in both halves: one real weight out of a register pair that holds two
template <int S>
__device__ __forceinline__ v2f pk_mul_bcast(v2f a, v2f w)
{
    v2f r;
    if (S == 0) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(w));
    else asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(w));
    return r;
}
// (l + r, l - r) of one stereo frame (l, r)
__device__ __forceinline__ v2f pk_sum_diff(v2f f)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(f));
    return r;
}

// forward radix-4 butterfly on (a0,a1,a2,a3) in place: A_k = sum_j a_j (-i)^(jk)  — 8 packed adds
__device__ __forceinline__ void radix4(v2f &a0, v2f &a1, v2f &a2, v2f &a3)
{
    const v2f t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = a1 - a3;
    a0 = t0 + t2;
    a2 = t0 - t2;
    a1 = pk_sub_ib(t1, t3);   // t1 - i t3
    a3 = pk_add_ib(t1, t3);   // t1 + i t3
}

// Forward 16-point DFT in registers: 72 packed instructions, 64 of the eight radix-4 butterflies and ONE per non-trivial twiddle.
// Input a[j] natural order; output X[k] is left in a[R16(k)] with R16(k) = ((k & 3) << 2) | (k >> 2).
// The twiddles W16^(r p) between the stages are applied less their real factor, which the fmas of the stage-2 butterfly carry:
//   W^2 = R (1 - i), W^6 = -R (1 + i)     the pre-forms pk_w2pre / pk_w6pre, R = sqrt(1/2)
//   W^4 = -i                              no instruction: the butterfly's first pair is b0 -+ i b2
//   W^1 = C (1 - i T), W^3 = -i C (1 + i T), W^9 = -C (1 - i T)     C = cos(pi/8), T = tan(pi/8): one fma each, a (1 -+ i T);
//                                         the two of a column share C, which goes onto their sum and their difference
// Stage 2 of columns p = 1, 2, 3 is ONE asm statement each (ten or eleven dependent instructions: see pk_cmul on the s_nop
// the compiler puts behind a statement whose result the next instruction reads), in place, with one temporary pair.
// The constants stand in scalar register pairs ("s"): left to a "v" constraint the compiler copies them into vector registers in
// front of every use.  The modifier sets, D = the result:
#define SS_PK_SUB_IB(D, A, B) "v_pk_add_f32 " D ", " A ", " B " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]\n\t"          /* A - i B */
#define SS_PK_ADD_IB(D, A, B) "v_pk_add_f32 " D ", " A ", " B " op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]\n\t"          /* A + i B */
#define SS_PK_W6PRE(D, A) "v_pk_add_f32 " D ", " A ", " A " op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[1,1]\n\t"              /* -(1 + i) A */
#define SS_PK_ADD(D, A, B) "v_pk_add_f32 " D ", " A ", " B "\n\t"
#define SS_PK_SUB(D, A, B) "v_pk_add_f32 " D ", " A ", " B " neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define SS_PK_FMA(D, V, K, T) "v_pk_fma_f32 " D ", " V ", " K ", " T "\n\t"                                                            /* T + K V */
#define SS_PK_FNMA(D, V, K, T) "v_pk_fma_f32 " D ", " V ", " K ", " T " neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"                             /* T - K V */
#define SS_PK_FMA_SUB_IK(D, V, K, T) "v_pk_fma_f32 " D ", " V ", " K ", " T " op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[0,0,0] neg_hi:[1,0,0]\n\t"   /* T - i K V */
#define SS_PK_FMA_ADD_IK(D, V, K, T) "v_pk_fma_f32 " D ", " V ", " K ", " T " op_sel:[1,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[0,0,0]\n\t"   /* T + i K V */
#define R16(k) ((((k) & 3) << 2) | ((k) >> 2))
__device__ __forceinline__ void fft16_stage2(v2f (&a)[16])
{
    constexpr float C1 = 0.92387953251128674f, T1 = 0.41421356237309505f, R = 0.70710678118654752f;
    const v2f kc = {C1, C1}, kt = {T1, T1}, kr = {R, R};
    v2f tmp;
    // stage 2: 4-point DFTs over r of a[r + 4p] W16^(r p); result s lands in a[s + 4p] = X[p + 4s]
    radix4(a[0], a[1], a[2], a[3]);
    // p = 1: (a4, C q5, R p6, -i C q7);  t0, t1 = a4 +- R p6;  a4, a6 = t0 +- C (q5 - i q7);  a5, a7 = t1 -+ i C (q5 + i q7)
    asm(SS_PK_FMA_SUB_IK("%1", "%1", "%5", "%1")          // q5
        SS_PK_FMA_ADD_IK("%3", "%3", "%5", "%3")          // q7
        SS_PK_SUB_IB("%2", "%2", "%2")                    // p6
        SS_PK_ADD_IB("%4", "%1", "%3")
        SS_PK_SUB_IB("%3", "%1", "%3")
        SS_PK_FNMA("%1", "%2", "%7", "%0")                // t1
        SS_PK_FMA("%2", "%2", "%7", "%0")                 // t0
        SS_PK_FMA("%0", "%3", "%6", "%2")
        SS_PK_FNMA("%2", "%3", "%6", "%2")
        SS_PK_FMA_ADD_IK("%3", "%4", "%6", "%1")
        SS_PK_FMA_SUB_IK("%1", "%4", "%6", "%1")
        : "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "=&v"(tmp) : "s"(kt), "s"(kc), "s"(kr));
    // p = 2: (a8, R p9, -i a10, R p11);  t0, t1 = a8 -+ i a10;  a8, a10 = t0 +- R (p9 + p11);  a9, a11 = t1 -+ i R (p9 - p11)
    asm(SS_PK_SUB_IB("%1", "%1", "%1")                    // p9
        SS_PK_W6PRE("%3", "%3")                           // p11
        SS_PK_SUB_IB("%4", "%0", "%2")                    // t0
        SS_PK_ADD_IB("%2", "%0", "%2")                    // t1
        SS_PK_ADD("%0", "%1", "%3")
        SS_PK_SUB("%1", "%1", "%3")
        SS_PK_FNMA("%3", "%0", "%5", "%4")                // (a10, parked in a11's pair)
        SS_PK_FMA("%0", "%0", "%5", "%4")
        SS_PK_FMA_ADD_IK("%4", "%1", "%5", "%2")          // (a11, parked in the temporary)
        SS_PK_FMA_SUB_IK("%1", "%1", "%5", "%2")
        : "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), "+v"(a[11]), "=&v"(tmp) : "s"(kr));
    a[10] = a[11];
    a[11] = tmp;
    // p = 3: (a12, -i C q13, R p14, -C q15);  t0, t1 = a12 +- R p14;  a12, a14 = t0 -+ C (q15 + i q13);  a13, a15 = t1 -+ i C (q15 - i q13)
    asm(SS_PK_FMA_ADD_IK("%1", "%1", "%5", "%1")          // q13
        SS_PK_FMA_SUB_IK("%3", "%3", "%5", "%3")          // q15
        SS_PK_W6PRE("%2", "%2")                           // p14
        SS_PK_SUB_IB("%4", "%3", "%1")
        SS_PK_ADD_IB("%3", "%3", "%1")
        SS_PK_FNMA("%1", "%2", "%7", "%0")                // t1
        SS_PK_FMA("%2", "%2", "%7", "%0")                 // t0
        SS_PK_FNMA("%0", "%3", "%6", "%2")
        SS_PK_FMA("%2", "%3", "%6", "%2")
        SS_PK_FMA_ADD_IK("%3", "%4", "%6", "%1")
        SS_PK_FMA_SUB_IK("%1", "%4", "%6", "%1")
        : "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]), "=&v"(tmp) : "s"(kt), "s"(kc), "s"(kr));
}

__device__ __forceinline__ void fft16(v2f (&a)[16])
{
    // stage 1: 4-point DFTs over q of a[r + 4q]; result p lands in a[r + 4p]
    radix4(a[0], a[4], a[8], a[12]);
    radix4(a[1], a[5], a[9], a[13]);
    radix4(a[2], a[6], a[10], a[14]);
    radix4(a[3], a[7], a[11], a[15]);
    fft16_stage2(a);
}
// A stage-1 butterfly of fft16 on WINDOWED samples, the window multiply of its last two inputs inside: with m_a = s_a h_a and
// m_b = s_b h_b formed (pk_mul_bcast), t0, t1 = m_a +- s_c h_c and t2, t3 = m_b +- s_d h_d are four fmas where two products and four
// adds were six instructions.  hc, hd: the register pairs that hold the weights in half S.  In: a0 = m_a, a1 = m_b; out: the
// butterfly's four results.  One asm statement (see pk_cmul).
template <int S>
__device__ __forceinline__ void radix4_windowed(v2f &a0, v2f &a1, v2f &a2, v2f &a3, v2f sc, v2f hc, v2f sd, v2f hd)
{
#define SS_WIN_FMA(D, V, H, T, NEG) "v_pk_fma_f32 " D ", " V ", " H ", " T " op_sel:[0,%c9,0] op_sel_hi:[1,%c9,1]" NEG "\n\t"
    v2f o0, m1 = a1;
    asm(SS_WIN_FMA("%2", "%5", "%6", "%0", "")                                  // t0
        SS_WIN_FMA("%0", "%5", "%6", "%0", " neg_lo:[1,0,0] neg_hi:[1,0,0]")    // t1
        SS_WIN_FMA("%3", "%7", "%8", "%1", "")                                  // t2
        SS_WIN_FMA("%1", "%7", "%8", "%1", " neg_lo:[1,0,0] neg_hi:[1,0,0]")    // t3
        SS_PK_ADD("%4", "%2", "%3")
        SS_PK_SUB("%2", "%2", "%3")
        SS_PK_ADD_IB("%3", "%0", "%1")
        SS_PK_SUB_IB("%0", "%0", "%1")
        : "+v"(a0), "+v"(m1), "=&v"(a2), "=&v"(a3), "=&v"(o0) : "v"(sc), "v"(hc), "v"(sd), "v"(hd), "n"(S));
    a1 = a0;
    a0 = o0;
#undef SS_WIN_FMA
}

// ---- pass 1 of a 4096-point transform on radix-16 passes: the twiddles W^(t ka), W = W_4096, of thread t ----------------------
// TWN of the fifteen are resident in tw[ka]: 6 = {1, 2, 3, 4, 8, 12}, 9 adds {5, 6, 7}, 12 adds {9, 10, 11}.  The others are
// applied factored, W^(t ka) = W^(t (ka & 3)) * W^(t (ka & 12)): one more complex multiply per window, in THAT order (the order
// decides the bits).  (The product of the two factors formed off the data's dependent chain, then one multiply of the data:
// measured in round 6 in k_fft4096_ms1, six interleaved repetitions: 2.996 vs 2.995 ms — nothing.)
template <int TWN>
constexpr bool r16_resident(int ka)
{
    static_assert(TWN == 6 || TWN == 9 || TWN == 12, "resident pass-1 twiddles: 6, 9 or 12");
    return (ka & 3) == 0 || (ka & 12) == 0 || (TWN >= 9 && (ka >> 2) == 1) || (TWN >= 12 && (ka >> 2) == 2);
}
template <int TWN>
__device__ __forceinline__ void r16_load_tw1(v2f (&tw)[16], const v2f *w4096, int t)
{
#pragma unroll
    for (int ka = 1; ka < 16; ka++) if (r16_resident<TWN>(ka)) tw[ka] = w4096[ka * t];
}
// v W^(t ka), ka = 1..15.  (With six resident every resident one is a factor, which the skips below reach with one multiply
// too: taken that way because it is the text that leaves every kernel's instructions where they were.)
template <int TWN>
__device__ __forceinline__ v2f r16_pass1_tw(int ka, v2f v, const v2f (&tw)[16])
{
    if (TWN > 6 && r16_resident<TWN>(ka)) return pk_cmul(v, tw[ka]);
    if (ka & 3) v = pk_cmul(v, tw[ka & 3]);
    if (ka & 12) v = pk_cmul(v, tw[ka & 12]);
    return v;
}

// dB of a squared magnitude q with dB = 10*log10(2)*log2(q) + off; q == 0 -> -150
// (scale_to_dbfs, analyzer.rs:11-27: val == 0.0 => -150.0)
__device__ __forceinline__ float db_from_sq(float q, float off)
{
    float r = fmaf(__log2f(q), 3.01029995663981195f, off);
    return q == 0.0f ? -150.0f : r;
}


constexpr int kX1Stride = 272;   // 256 + 16 de-phases the 4 ka-groups of a wave across banks
constexpr int kRow = 18;
constexpr int kPlane = 16 * kRow;   // 288 complex per outer index; 16 planes = 4608 complex = 36864 B

// ============================================================================
//  Spectrum, N = 16384 (the reference's native window, tui.rs:1488), ONE window of one REAL channel per
//  512-thread workgroup: real FFT through an 8192-point complex FFT, split by one radix-2
//  decimation-in-frequency step into two 4096-point problems that reuse the radix-16 machinery:
//    z[i] = (xw[2i], xw[2i+1]),  y_q[i] = (z[i] + (-1)^q z[i+4096]) W_8192^(i q),  Z[2k+q] = FFT_4096(y_q)[k]
//    X[b] = (Z[b] + conj Z[8192-b])/2 - (i/2) W_16384^b (Z[b] - conj Z[8192-b])
//  Threads 0-255 run q = 0, threads 256-511 run q = 1; the mirror 8192-b has the parity of b, so each
//  half only mirrors inside its own published spectrum.  midside 0: mono buffer or channel `ch` of an interleaved one,
//  1: stereo -> mid/side (audio_player.rs:400-419).  `bid`: (stream, window, channel) index of this workgroup.
//  `lds`: kFft16kLdsBytes of workgroup memory, 16-byte aligned (k_fft16k's own static array; the tick kernel's dynamic block, which
//  its other workgroups use for the loudness call's tiles — a kernel's LDS is the largest need, not the sum).
//  The epilogue asks for the twiddles (and pink values) of eight of a thread's bins before it uses the first: a tick runs
//  TWO of these workgroups on an otherwise idle chip, and one exposed memory round trip per bin was most of its 17 us.
// ============================================================================
constexpr int kFft16kLdsBytes = (2 * 16 * kPlane + 256) * 8;                // 75776
// The body, with what varies between its users in a window source `src` (the arithmetic is one text, so every user's dB values
// are the same bits for the same windowed samples):
//   src.begin():   which window this workgroup transforms; false: none (the transform returns at once)
//   src.load(i):   the windowed real samples 2i, 2i + 1 of the window as one complex value
//   src.loaded():  called once a thread's 32 values are loaded, ahead of the transform's first barrier (a meter bank folds its
//                  non-finite flags there without a barrier of its own)
//   src.row():     called once the transform is published; returns store(idx, r, pk), which takes the dB value r (pink not
//                  added) of retained bin first_bin + idx and pk = p.pink[idx] (0 without p.pink)
//   src.done():    called behind the last store
template <class Src>
__device__ __forceinline__ void fft16k_transform(const FftBatchParams &p, Src &src, void *lds)
{
    v2f (*const xbuf2)[16 * kPlane] = reinterpret_cast<v2f (*)[16 * kPlane]>(lds);      // [2][16 * kPlane]: 2 x 36864 B
    v2f *const tw2s = reinterpret_cast<v2f *>(lds) + 2 * 16 * kPlane;                    // [256]
#define X1W(ka, tb_, ta_) ((ka) * kX1Stride + (tb_) + 16 * (ta_))
#define X2W(kb, ka_, tb_) ((kb) * kPlane + (ka_) * kRow + (tb_))
    const int q = threadIdx.x >> 8;                 // which half-problem
    const int t = threadIdx.x & 255;
    v2f *xbuf = xbuf2[q];
    if (!src.begin()) return;
    const v2f *tw16k = reinterpret_cast<const v2f *>(p.tw_n);       // W_16384^k, k < 8192
    const v2f *tw4k = reinterpret_cast<const v2f *>(p.tw_core);     // W_4096^k
    if (threadIdx.x < 256) tw2s[t] = reinterpret_cast<const v2f *>(p.tw_256)[t];

    v2f z[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint32_t i = (uint32_t)t + 256u * j;
        const v2f a = src.load(i), b = src.load(i + 4096u);
        z[j] = q ? pk_cmul(a - b, tw16k[2 * i]) : a + b;             // W_8192^i = W_16384^(2i)
    }
    const int tb = t & 15, hi = t >> 4;
    // ---- the 4096-point transform of y_q (same passes and LDS layouts as k_fft4096_ms)
    // pass-1 twiddles from six gathered ones (scattered 8-byte gathers are the expensive part of this one-window-per-workgroup kernel)
    v2f twg[16];
    r16_load_tw1<6>(twg, tw4k, t);
    fft16(z);
    xbuf[X1W(0, tb, hi)] = z[R16(0)];
#pragma unroll
    for (int ka = 1; ka < 16; ka++) xbuf[X1W(ka, tb, hi)] = r16_pass1_tw<6>(ka, z[R16(ka)], twg);
    src.loaded();
    __syncthreads();
#pragma unroll
    for (int ta = 0; ta < 16; ta++) z[ta] = xbuf[X1W(hi, tb, ta)];
    __syncthreads();
    fft16(z);
    xbuf[X2W(0, hi, tb)] = z[R16(0)];
#pragma unroll
    for (int kb = 1; kb < 16; kb++) xbuf[X2W(kb, hi, tb)] = pk_cmul(z[R16(kb)], tw2s[tb * kb]);
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < 16; qq++) z[qq] = xbuf[X2W(hi, tb, qq)];
    __syncthreads();
    fft16(z);
    // publish Z_q[k] = Z[2k + q] at position k (natural order)
#pragma unroll
    for (int kc = 0; kc < 16; kc++) xbuf[kc * 256 + t] = z[R16(kc)];
    __syncthreads();
    // ---- real-FFT recombination + dB for the retained bins; consecutive threads own consecutive bins
    const auto store = src.row();
    constexpr int kAhead = 8;
    for (uint32_t idx0 = threadIdx.x; idx0 < p.n_bins; idx0 += 512u * kAhead) {
        v2f wv[kAhead];
        float pk[kAhead];
#pragma unroll
        for (int m = 0; m < kAhead; m++) {
            const uint32_t idx = idx0 + 512u * (uint32_t)m;
            const uint32_t ic = idx < p.n_bins ? idx : p.n_bins - 1u;      // (clamped: a load, never a store)
            const uint32_t b = p.first_bin + ic;
            wv[m] = tw16k[b < 8192u ? b : 0u];
            pk[m] = p.pink ? p.pink[ic] : 0.0f;
        }
#pragma unroll
        for (int m = 0; m < kAhead; m++) {
            const uint32_t idx = idx0 + 512u * (uint32_t)m;
            if (idx >= p.n_bins) break;
            const uint32_t b = p.first_bin + idx;
            float xr, xi;
            if (b == 8192u) {                                           // Nyquist of the real signal
                const v2f z0 = xbuf2[0][0];
                xr = z0.x - z0.y; xi = 0.0f;
            } else {
                const uint32_t qb = b & 1u, k = b >> 1;
                const uint32_t km = qb ? (4095u - k) : ((4096u - k) & 4095u);   // index of Z[8192 - b] in its half
                const v2f zk = xbuf2[qb][k];
                const v2f zc = xbuf2[qb][km];
                const float sr = (zk.x + zc.x) * 0.5f, si = (zk.y - zc.y) * 0.5f;
                const float dr = (zk.x - zc.x) * 0.5f, di = (zk.y + zc.y) * 0.5f;
                const float tr = wv[m].x * dr - wv[m].y * di;
                const float ti = wv[m].x * di + wv[m].y * dr;
                xr = sr + ti;
                xi = si - tr;
            }
            const float qv = fmaf(xr, xr, xi * xi);
            float r = fmaf(__log2f(qv), 3.01029995663981195f, p.db_offset);
            r = (qv == 0.0f) ? -150.0f : r;
            store(idx, r, pk[m]);
        }
    }
    src.done();
#undef X1W
#undef X2W
}

// k_fft16k and k_tick: window w of channel ch of stream `stream` in a contiguous buffer; midside 0: mono buffer or channel `ch` of
// an interleaved one, 1: stereo -> mid/side
struct Fft16kFlat {
    const FftBatchParams &p;
    int midside;
    uint32_t fft_ch, bid;
    uint32_t ch, w, stream;
    const float *base;
    __device__ __forceinline__ bool begin()
    {
        ch = bid % fft_ch; bid /= fft_ch;
        w = bid % p.n_windows;
        stream = bid / p.n_windows;
        if (p.windows_of && w >= p.windows_of[stream]) return false;                  // ragged batches
        const size_t start = p.first_start + (size_t)w * p.hop;
        base = p.pcm + ((size_t)stream * p.frames_per_stream + start) * p.channels;
        return true;
    }
    // windowed real samples 2i, 2i+1 as one complex value
    __device__ __forceinline__ v2f load(uint32_t i) const
    {
        float x0, x1;
        if (midside) {
            const float2 va = reinterpret_cast<const float2 *>(base)[2 * (size_t)i];       // frames 2i, 2i+1: (l,r)
            const float2 vb = reinterpret_cast<const float2 *>(base)[2 * (size_t)i + 1];
            x0 = ch == 0 ? (va.x + va.y) * 0.5f : (va.x - va.y) * 0.5f;
            x1 = ch == 0 ? (vb.x + vb.y) * 0.5f : (vb.x - vb.y) * 0.5f;
        } else if (p.channels == 1) {
            const float2 v = reinterpret_cast<const float2 *>(base)[i];                     // mono buffer: samples 2i, 2i+1 in one load
            x0 = v.x; x1 = v.y;
        } else {
            x0 = base[(size_t)(2 * i) * p.channels + ch];
            x1 = base[(size_t)(2 * i + 1) * p.channels + ch];
        }
        const float2 hw = *reinterpret_cast<const float2 *>(p.window + 2 * (size_t)i);
        return v2f{x0 * hw.x, x1 * hw.y};
    }
    __device__ __forceinline__ void loaded() const {}
    __device__ __forceinline__ auto row() const
    {
        float *o = p.out + (((size_t)stream * p.n_windows + w) * fft_ch + ch) * p.bin_stride;
        return [o](uint32_t idx, float r, float pk) { o[idx] = r + pk; };
    }
    __device__ __forceinline__ void done() const
    {
        if (p.done_flag) {
            // every wave completes its own stores system-wide (a workgroup barrier alone does not wait for vector stores), then
            // one lane tells the host: whoever sees the flag sees the row
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) __hip_atomic_store(p.done_flag + ch, p.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
};

__device__ __forceinline__ void fft16k_window(const FftBatchParams &p, int midside, uint32_t fft_ch, uint32_t bid, void *lds)
{
    Fft16kFlat src{p, midside, fft_ch, bid, 0u, 0u, 0u, nullptr};
    fft16k_transform(p, src, lds);
}

}  // namespace ssk
